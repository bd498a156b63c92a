// nc_fwd_kernel / nc_fwd_chunk_kernel (noisecritic.hip), included inside the K loop (kb in steps of 16): the W fragment of the next step is
// prefetched (bounded by the row end Fp, not by a chunk end), then 4 x G2 x 5 MFMAs on operands built from the LDS tables.  CHUNK: column k of
// the row sits at k - cb of the staged table.
        const int k0 = kb + 4 * kq;
        {   // prefetch the next W fragment
            const int k1 = k0 + 16;
            const int valid = colok ? max(0, min(4, F - k1)) : 0;
            if (kb + 16 < Fp) ld4(wrow + k1, vecW, valid, wn);
        }
        f32x4 mu4[G2], sg4[G2], nz4[NC_NF];
#pragma unroll
        for (int g = 0; g < G2; ++g) {
            mu4[g] = *reinterpret_cast<const f32x4*>(&mu_s[(4 * g + bp) * LDS_LD + (CHUNK ? k0 - cb : k0)]);
            sg4[g] = *reinterpret_cast<const f32x4*>(&sg_s[(4 * g + bp) * LDS_LD + (CHUNK ? k0 - cb : k0)]);
        }
#pragma unroll
        for (int f = 0; f < NC_NF; ++f) nz4[f] = *reinterpret_cast<const f32x4*>(&nz_s[(4 * f + nn) * LDS_LD + (CHUNK ? k0 - cb : k0)]);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int g = 0; g < G2; ++g)
#pragma unroll
                for (int f = 0; f < NC_NF; ++f)
                    acc[g][f] = __builtin_amdgcn_mfma_f32_16x16x4f32(fmaf(sg4[g][s], nz4[f][s], mu4[g][s]), wv[s], acc[g][f], 0, 0, 0);
#pragma unroll
        for (int s = 0; s < 4; ++s) wv[s] = wn[s];
