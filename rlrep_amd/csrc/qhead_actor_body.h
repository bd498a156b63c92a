// body of qhead_actor_kernel and of its group form (group.h): `p` is the parameter block (the group form's is already moved to the member)
    __shared__ float shp[4][2];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const float alpha = (float)exp(p.alpha_state[0]);
    float accl = 0.f, accc = 0.f;
    for (int b = blockIdx.x * 4 + w; b < p.B; b += gridDim.x * 4) {
        const size_t ro = (size_t)b * (p.ldE ? p.ldE : p.H);
        const float bc0 = p.bc[0][0], bc1 = p.bc[1][0], lp = p.logp[b];          // (out with the first operand loads: see qhead_critic_kernel)
        __builtin_amdgcn_sched_barrier(0);
        float d0 = 0.f, d1 = 0.f;                  // both dot products in one pass (see qhead_critic_kernel)
#pragma unroll 4
        for (int k = lane; k < p.H; k += 64) {
            const float e0 = p.Ec[0][ro + k], e1 = p.Ec[1][ro + k], w0 = p.wc[0][k], w1 = p.wc[1][k];
            d0 = fmaf(e0, w0, d0); d1 = fmaf(e1, w1, d1);
        }
        const float q1 = wave_sum(d0) + bc0;
        const float q2 = wave_sum(d1) + bc1;
        // d(-min(q1,q2))/dq_i : -1 to the arg-min head, ties split 1/2 (torch.min backward)
        float s1, s2;
        if (q1 < q2) { s1 = 1.f; s2 = 0.f; } else if (q2 < q1) { s1 = 0.f; s2 = 1.f; } else { s1 = s2 = 0.5f; }
        const float g1 = -s1 * p.inv_batch, g2 = -s2 * p.inv_batch;
        for (int k = lane; k < p.H; k += 64) {
            p.GE[0][ro + k] = g1 * p.wc[0][k] * elu_grad_from_out(p.Ec[0][ro + k]);
            p.GE[1][ro + k] = g2 * p.wc[1][k] * elu_grad_from_out(p.Ec[1][ro + k]);
        }
        accl += alpha * lp - fminf(q1, q2);
        accc += -lp - p.target_entropy;
    }
    if (lane == 0) { shp[w][0] = accl; shp[w][1] = accc; }
    __syncthreads();
    if (threadIdx.x == 0) {
        p.partial_loss[blockIdx.x] = ((shp[0][0] + shp[1][0]) + shp[2][0]) + shp[3][0];
        p.partial_c[blockIdx.x] = ((shp[0][1] + shp[1][1]) + shp[2][1]) + shp[3][1];
        if (blockIdx.x == 0 && p.step) bump_group(p.step);
    }
