// The exploration mix behind the head of the counter-reading act kernels (actor_tile.hip actor_tile_kernel_ctl and its group form): #included
// into both, like actor_tile_body.h, so that both compile the same statements.  In scope: p (ActTile: the launch's -- a group's rebased to the
// member, p.seed the member's key), k (ActCtl), r0 (the tile's first row), tg (T) and it (ITER) as read from the record.  Defines `warm`.
    const bool warm = tg < k.start_timesteps;
    if (warm || k.eps_greedy > 0.f) {
        for (int e = threadIdx.x; e < 16 * p.A; e += 256) {
            const int i = e / p.A, j = e - i * p.A;
            const long long row = (long long)r0 + i;
            if (row >= p.rows) continue;
            uint32_t c[4] = {(uint32_t)it, (uint32_t)(it >> 32), (uint32_t)row, RL_STREAM_SIM};
            philox4x32_10(c, (uint32_t)p.seed, (uint32_t)(p.seed >> 32));
            if (!(warm || env_u01f(c[0]) < k.eps_greedy)) continue;
            const int wq = (1 + j) >> 2, ww = (1 + j) & 3;
            if (wq) {
                c[0] = (uint32_t)it; c[1] = (uint32_t)(it >> 32); c[2] = (uint32_t)row; c[3] = RL_STREAM_SIM + (uint32_t)wq;
                philox4x32_10(c, (uint32_t)p.seed, (uint32_t)(p.seed >> 32));
            }
            const uint32_t word = ww == 0 ? c[0] : ww == 1 ? c[1] : ww == 2 ? c[2] : c[3];
            const float u = mix_add(p.lo, mix_mul(mix_sub(p.hi, p.lo), env_u01f(word)));
            p.act[row * p.ld_act + j] = fminf(fmaxf(u, p.lo), p.hi);
        }
    }
