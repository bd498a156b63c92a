// body of the sac critic head with per-sample weights: of qhead_critic_w_kernel (per.hip) and of its two group forms (per_group.hip).  `p`
// is the QHeadCritic block (a group form's is already moved to the member), pw_w / pw_td the weights read and the |TD| written, B each.
// qhead_critic_body.h with the weights worked in -- included there under a switch, the body would have to change in the kernels every
// unweighted train() runs.  #included, not called, as that body is (group.h).  With d_h = q_h - y:
//   g_h = (2 d_h inv_batch) w   (in this order: w = 1 is the identity),  loss partials w d_h^2,  td = 0.5 (|d_1| + |d_2|)
    __shared__ float shp[4][4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const float alpha = (float)exp(p.alpha_state[0]);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int b = blockIdx.x * 4 + w; b < p.B; b += gridDim.x * 4) {
        const size_t ro = (size_t)b * (p.ldE ? p.ldE : p.H);
        const float bt0 = p.bt[0][0], bt1 = p.bt[1][0], bc0 = p.bc[0][0], bc1 = p.bc[1][0], lpb = p.logp[b], Rb = p.R[b], Db = p.D[b], wb = pw_w[b];
        __builtin_amdgcn_sched_barrier(0);
        float dd0 = 0.f, dd1 = 0.f, dd2 = 0.f, dd3 = 0.f;
#pragma unroll 4
        for (int k = lane; k < p.H; k += 64) {
            const float e0 = p.Et[0][ro + k], e1 = p.Et[1][ro + k], e2 = p.Ec[0][ro + k], e3 = p.Ec[1][ro + k];
            const float w0 = p.wt[0][k], w1 = p.wt[1][k], w2 = p.wc[0][k], w3 = p.wc[1][k];
            dd0 = fmaf(e0, w0, dd0); dd1 = fmaf(e1, w1, dd1); dd2 = fmaf(e2, w2, dd2); dd3 = fmaf(e3, w3, dd3);
        }
        const float tq1 = wave_sum(dd0) + bt0;
        const float tq2 = wave_sum(dd1) + bt1;
        const float q1 = wave_sum(dd2) + bc0;
        const float q2 = wave_sum(dd3) + bc1;
        const float tv = fminf(tq1, tq2) - alpha * lpb;
        const float y = Rb + (1.f - Db) * p.gamma * tv;
        const float d1 = q1 - y, d2 = q2 - y;
        const float g1 = __fmul_rn(2.f * d1 * p.inv_batch, wb), g2 = __fmul_rn(2.f * d2 * p.inv_batch, wb);
        if (p.train) {
            for (int k = lane; k < p.H; k += 64) {
                p.GE[0][ro + k] = g1 * p.wc[0][k] * elu_grad_from_out(p.Ec[0][ro + k]);
                p.GE[1][ro + k] = g2 * p.wc[1][k] * elu_grad_from_out(p.Ec[1][ro + k]);
            }
            if (lane == 0) { p.dq[b] = g1; p.dq[p.B + b] = g2; }
        }
        if (lane == 0) pw_td[b] = __fmul_rn(0.5f, __fadd_rn(fabsf(d1), fabsf(d2)));
        // (the unweighted kernel's acc += d * d is one fused multiply-add: with w = 1 this is the same operation on the same operands)
        acc[0] = fmaf(__fmul_rn(wb, d1), d1, acc[0]); acc[1] = fmaf(__fmul_rn(wb, d2), d2, acc[1]); acc[2] += q1; acc[3] += q2;
    }
    if (lane == 0) { for (int i = 0; i < 4; ++i) shp[w][i] = acc[i]; }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int i = threadIdx.x;
        p.partial[4 * blockIdx.x + i] = ((shp[0][i] + shp[1][i]) + shp[2][i]) + shp[3][i];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && p.step) bump_group(p.step);
