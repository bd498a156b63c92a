// body of select_action_kernel and of its group form (group.h): `p` is the parameter block (the group form's is already moved to the member)
    extern __shared__ float sm[];                        // obs[S] | h1[Ha] | h2[Ha] | o[2A]
    float* const x0 = sm; float* const h1 = x0 + p.S; float* const h2 = h1 + p.Ha; float* const o = h2 + p.Ha;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;          // 16 waves
    for (int k = threadIdx.x; k < p.S; k += 1024) x0[k] = p.obs[k];
    __syncthreads();
    // a wave takes rows w, w + 16, ...; EIGHT rows at a time with all their loads in flight together (a row after the other is one exposed
    // round trip per row: 147 us for the three layers on one workgroup, measured)
    auto layer = [&](const float* __restrict__ W, const float* __restrict__ b, const float* in, int K, int N, float* out, bool elu) {
        for (int j0 = w; j0 < N; j0 += 16 * 8) {
            float s[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) s[r] = 0.f;
            for (int k0 = 0; k0 < K; k0 += 256) {
                float wv[8][4], xv[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) { const int k = k0 + lane + 64 * i; xv[i] = k < K ? in[k] : 0.f; }
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    const int j = min(j0 + 16 * r, N - 1);
#pragma unroll
                    for (int i = 0; i < 4; ++i) wv[r][i] = W[(size_t)j * K + min(k0 + lane + 64 * i, K - 1)];
                }
#pragma unroll
                for (int r = 0; r < 8; ++r)
#pragma unroll
                    for (int i = 0; i < 4; ++i) s[r] = fmaf(wv[r][i], xv[i], s[r]);
            }
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int j = j0 + 16 * r;
                const float t = wave_sum(s[r]);
                if (lane == 0 && j < N) { const float v = t + b[j]; out[j] = elu ? elu_f(v) : v; }
            }
        }
    };
    layer(p.W1, p.b1, x0, p.S, p.Ha, h1, true);
    __syncthreads();
    layer(p.W2, p.b2, h1, p.Ha, p.Ha, h2, true);
    __syncthreads();
    layer(p.W3, p.b3, h2, p.Ha, 2 * p.A, o, false);
    __syncthreads();
    const int j = threadIdx.x;
    if (j < p.A) {
        float e = 0.f;
        if (p.explore) {                                  // element j of philox_fill_body's normal stream (kind 0, std 1, stream 0, no device counter)
            const long long q = j >> 2;
            uint32_t c[4] = {(uint32_t)q, (uint32_t)(q >> 32), (uint32_t)p.offset, (uint32_t)(p.offset >> 32)};
            philox4x32_10(c, (uint32_t)p.seed, (uint32_t)(p.seed >> 32));
            const int h = (j & 3) >> 1;
            const float u1 = ((float)(c[2 * h] >> 8) + 0.5f) * (1.0f / 16777216.0f);
            const float u2 = ((float)(c[2 * h + 1] >> 8) + 0.5f) * (1.0f / 16777216.0f);
            const float rad = sqrtf(-2.0f * logf(u1));
            float sn, cs;
            sincosf(6.283185307179586f * u2, &sn, &cs);
            e = (j & 1) ? rad * sn : rad * cs;
        }
        const float mu = o[j];
        const float t = tanhf(o[p.A + j]);
        const float sg = expf(-5.f + 3.5f * (t + 1.f));
        const float y = tanhf(mu + e * sg);
        p.act[j] = fminf(fmaxf(y, p.lo), p.hi);
    }
