// body of infonce_kernel and of its group form (group.h): `p` is the record (the group form's is already moved to the member)
    __shared__ float shp[4][2];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float accm = 0.f, accr = 0.f;
    for (int i = blockIdx.x * 4 + w; i < p.B; i += gridDim.x * 4) {
        float* row = p.S + (size_t)i * p.ldS;
        float mx = -INFINITY;
        const int NC = p.ncols, di = p.diag_off + i;
        for (int j = lane; j < NC; j += 64) mx = fmaxf(mx, row[j]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        float se = 0.f;
        for (int j = lane; j < NC; j += 64) se += expf(row[j] - mx);
        se = wave_sum(se);
        const float lse = mx + logf(se);
        const float sii = row[di];
        for (int j = lane; j < NC; j += 64) {
            const float sm = expf(row[j] - lse);
            row[j] = (sm - (j == di ? 1.f : 0.f)) * p.inv_batch;
        }
        float rh;
        if (p.Z) {
            const float* z = p.Z + (size_t)i * p.ldZ;
            float s = 0.f;
            for (int f = lane; f < p.F; f += 64) s = fmaf(z[f], p.theta_w[f], s);
            rh = wave_sum(s) + p.theta_b[0];
        } else rh = p.rhat[i];
        const float dr = rh - p.r[i];
        if (lane == 0) p.drhat[i] = dr * p.inv_batch;
        accm += lse - sii;
        accr += dr * dr;
    }
    if (lane == 0) { shp[w][0] = accm; shp[w][1] = accr; }
    __syncthreads();
    if (threadIdx.x == 0) {
        p.partial[2 * blockIdx.x] = ((shp[0][0] + shp[1][0]) + shp[2][0]) + shp[3][0];
        p.partial[2 * blockIdx.x + 1] = ((shp[0][1] + shp[1][1]) + shp[2][1]) + shp[3][1];
        if (blockIdx.x == 0 && p.step) bump_group(p.step);
    }
