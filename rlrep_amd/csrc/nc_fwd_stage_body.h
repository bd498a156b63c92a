// nc_fwd_kernel / nc_fwd_chunk_kernel (noisecritic.hip), included inside the loop over the 256-column chunks cb of a table row: every wave
// issues ALL of its row loads of the chunk back to back, then files them in the LDS tables (sigma rows as exp(clamp(log_std)), stored to
// sigma_out by the workgroups of column tile 0 on the way; columns k >= F are zeros).  CHUNK: column cb + 4 lane lands at 4 lane of the table.
            const int k = cb + 4 * lane;
            f32x4 v[SLOTS];
#pragma unroll
            for (int q = 0; q < SLOTS; ++q) {
                const int row = NW * q + w;
                v[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
                if (row < NROWS && k < F) {
                    if (row < 2 * RB) {
                        const int rr = row < RB ? row : row - RB;
                        const float* src = (row < RB ? t.mean : t.lstd) + (size_t)(b0 + rr) * t.ld_ml + k;
                        if (b0 + rr < t.B) v[q] = *reinterpret_cast<const f32x4*>(src);
                    } else {
                        v[q] = *reinterpret_cast<const f32x4*>(t.noise + (size_t)(row - 2 * RB) * F + k);
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < SLOTS; ++q) {
                const int row = NW * q + w;
                if (row >= NROWS || k >= Fp) continue;
                f32x4 x = v[q];
                if (row >= RB && row < 2 * RB) {
                    const int rr = row - RB;
                    const bool ok = (b0 + rr < t.B) && (k < F);
#pragma unroll
                    for (int s = 0; s < 4; ++s) x[s] = ok ? expf(clamp_lstd(x[s])) : 0.f;
                    if (t.sigma_out && th == 0 && ok) *reinterpret_cast<f32x4*>(t.sigma_out + (size_t)(b0 + rr) * F + k) = x;
                }
                float* dst = (row < RB ? mu_s + row * LDS_LD : row < 2 * RB ? sg_s + (row - RB) * LDS_LD : nz_s + (row - 2 * RB) * LDS_LD) + (CHUNK ? 4 * lane : k);
                *reinterpret_cast<f32x4*>(dst) = x;
            }
