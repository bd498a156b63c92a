// body of actor_tile_kernel and of its group form: `p` is the parameter block (the group form's is already moved to the member), `r0` the first
// of the 16 observation rows of this workgroup.  LDS: xa[16][LD] | xb[16][LD] | o[16][2A].
    extern __shared__ float sm[];
    const int LD = p.LD;
    float* const xa = sm; float* const xb = xa + 16 * LD; float* const o = xb + 16 * LD;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;          // 4 waves
    {   // the observation tile, zero-filled up to the next multiple of 16 columns; rows past the last one re-read the last one (never stored)
        const int S16 = (p.S + 15) & ~15;
        for (int e = threadIdx.x; e < 16 * S16; e += 256) {
            const int i = e / S16, k = e - i * S16;
            const long long row = min((long long)r0 + i, (long long)p.rows - 1);
            const float v = p.obs[row * p.ld_obs + min(k, p.S - 1)];
            xa[i * LD + k] = k < p.S ? v : 0.f;
        }
    }
    __syncthreads();
    at_layer(p.W1, p.b1, xa, LD, p.S, p.Ha, xb, LD, true, true, lane, w);
    __syncthreads();
    at_layer(p.W2, p.b2, xb, LD, p.Ha, p.Ha, xa, LD, true, true, lane, w);
    __syncthreads();
    at_layer(p.W3, p.b3, xa, LD, p.Ha, 2 * p.A, o, 2 * p.A, false, false, lane, w);
    __syncthreads();
    // the head of select_action_body.h, restated per (row, j): that file's kernels stay as they are
    for (int e = threadIdx.x; e < 16 * p.A; e += 256) {
        const int i = e / p.A, j = e - i * p.A;
        const long long row = (long long)r0 + i;
        if (row >= p.rows) continue;
        float eps = 0.f;
        if (p.explore) {                                  // element j of the normal stream (kind 0, std 1, stream 0) at offset + (row << 20)
            const unsigned long long off = p.offset + ((unsigned long long)row << 20);
            const long long q = j >> 2;
            uint32_t c[4] = {(uint32_t)q, (uint32_t)(q >> 32), (uint32_t)off, (uint32_t)(off >> 32)};
            philox4x32_10(c, (uint32_t)p.seed, (uint32_t)(p.seed >> 32));
            const int h = (j & 3) >> 1;
            const float u1 = ((float)(c[2 * h] >> 8) + 0.5f) * (1.0f / 16777216.0f);
            const float u2 = ((float)(c[2 * h + 1] >> 8) + 0.5f) * (1.0f / 16777216.0f);
            const float rad = sqrtf(-2.0f * logf(u1));
            float sn, cs;
            sincosf(6.283185307179586f * u2, &sn, &cs);
            eps = (j & 1) ? rad * sn : rad * cs;
        }
        const float mu = o[i * 2 * p.A + j];
        const float t = tanhf(o[i * 2 * p.A + p.A + j]);
        const float sg = expf(-5.f + 3.5f * (t + 1.f));
        const float y = tanhf(mu + eps * sg);
        p.act[row * p.ld_act + j] = fminf(fmaxf(y, p.lo), p.hi);
    }
