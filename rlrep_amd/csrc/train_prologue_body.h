// body of train_prologue_kernel and of its group form (group.h): `p` is the parameter block (the group form's is already moved to the member)
    __builtin_amdgcn_s_setprio(3);      // small launch on a latency-critical chain (see gemm16_kernel)
    const int bid = blockIdx.x;
    if (bid < p.nb_idx) philox_fill_body(p.idx, bid, p.nb_idx);
    else if (bid < p.nb_idx + p.nb_eps) philox_fill_body(p.eps, bid - p.nb_idx, p.nb_eps);
    else if (bid >= p.nb_idx + p.nb_eps + p.nb_fill) shadow_tile_body(p.sh, p.nsh, p.sh_base, bid - p.nb_idx - p.nb_eps - p.nb_fill, false);
    else {
        IdxGen g; g.on = 1; g.seed = p.idx.seed; g.stream_id = p.idx.stream_id;
        g.off = p.idx.offset + (unsigned long long)(*p.idx.step_dev + p.idx.step_add);
        g.hi = p.idx.hi_dev ? *p.idx.hi_dev : p.idx.hi;
        fill_slot_body(p.fill, g, bid - p.nb_idx - p.nb_eps, p.nb_fill);
    }
    // steps += 1.  Every block of this launch reads the counter -- so none of them may write what the others read: the blocks read word 2 of the
    // counter block ("the counter as the next prologue will read it", p.idx.step_dev), ONE thread writes word 0 = word 2 + 1 (what every later
    // launch reads), and the first optimizer launch behind this one in the chain brings word 2 up to word 0 (AdamTask::sync_steps).  (It used to
    // be one word, bumped by the block that drew the last of ~300 tickets from an atomic counter: 3.6 us of same-address atomics at the head of
    // every train(); timing-only build without it: 3 921 -> 3 958 train()/s.)
    if (bid == 0 && threadIdx.x == 0) *p.counter = *p.idx.step_dev + 1;
