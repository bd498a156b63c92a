"""Writes tests/golden/gemm_lds_plan.json: what rlrep_gemm_plan answers over a grid of products, per RLREP_DISABLE setting.

The fixture pins the ROUTING of the LDS-tiled GEMM engine (csrc/gemm_lds.hip rl_gemm_lds_route) for tests/test_gemm_lds_plan_cpu.py, so it must be
recorded from a library built from the commit BEFORE a change to that routing, never from the code under test:

    OBJDIR=.obj_base OUTNAME=librlrep_hip_base.so bash rlrep_amd/csrc/build.sh      # in a checkout of the base commit
    RLREP_LIB=<that checkout>/rlrep_amd/lib/librlrep_hip_base.so python tests/golden/make_gemm_lds_plan.py

rlrep_gemm_plan launches nothing and needs no GPU.  The switches are read at every library entry, so one process records every setting.
"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, 'gemm_lds_plan.json')

LD_ROW, LD_COL = 0, 1
FWD, DX, DW = (LD_ROW, LD_ROW), (LD_ROW, LD_COL), (LD_COL, LD_COL)      # the three layout pairs the engine accepts
REFUSED = (LD_COL, LD_ROW)                                              # ... and one it does not
SETTINGS = ('', 'gemm_lds', 'x3', 'x3_dw', 'x3w', 'x3s', 'x3s_unaligned', 'x3q')      # RLREP_DISABLE=

# The five agents at the BASELINE.json dimensions (ctrlsac as main.py builds it, and at the 256-wide layers of its golden case; diffsrsac also at the
# reduced nabla-mu head of tests/test_large_dims.py): alg, S, A, batch, oracle.shapes.param_shapes keywords
AGENTS = (
    ('sac', 3, 1, 64, dict(hidden_dim=256)),
    ('vlsac', 17, 6, 256, dict(hidden_dim=256, feature_dim=256)),
    ('ctrlsac', 17, 6, 256, dict(hidden_dim=1024, feature_dim=2048)),
    ('ctrlsac', 17, 6, 256, dict(hidden_dim=256, feature_dim=256)),
    ('spedersac', 111, 8, 1024, dict(phi_hidden_dim=512, phi_hidden_depth=1, mu_hidden_dim=512, mu_hidden_depth=0,
                                     critic_and_actor_hidden_dim=256, feature_dim=512, hidden_dim=256)),
    ('diffsrsac', 376, 17, 2048, dict(hidden_dim=256)),
    ('diffsrsac', 76, 8, 1024, dict(hidden_dim=256)),
)

# (layout, R, Cn, K): the default-switch routes worked out by hand from the routing code, then shapes on both sides of every threshold it has
HAND = (
    (FWD, 4096, 4096, 4096),        # 256 x 128 persistent tile
    (FWD, 2560, 3840, 1024),        # 128-wide bf16x3: 300 wide tiles fill 59 % of the second round
    (FWD, 2048, 2048, 128),         # 128-wide fp32: below 2e9 flop
    (FWD, 256, 256, 4096),          # 64-wide bf16x3, split
    (FWD, 256, 1024, 1024),         # 32 x 32
    (FWD, 64, 64, 64), (DX, 64, 64, 64), (DW, 64, 64, 64),      # 16-row engine
)
EDGES = (
    (DX, 4096, 4096, 4096), (DW, 4096, 4096, 4096), (DX, 2560, 3840, 1024), (DW, 2560, 3840, 1024),
    (FWD, 1000, 1000, 100), (FWD, 1000, 1000, 99), (FWD, 4096, 4096, 63), (FWD, 4096, 4096, 64),          # 2e8 flop; K >= 64
    (FWD, 1000, 1000, 1000), (FWD, 1000, 1000, 999), (FWD, 2048, 2048, 256), (FWD, 2048, 2048, 232),      # 2e9 flop
    (FWD, 256, 1024, 512), (FWD, 256, 1024, 496), (FWD, 256, 1024, 520), (FWD, 288, 1024, 1024),          # 32 x 32: K >= 512, K % 16, R <= 256
    (FWD, 256, 768, 1024), (FWD, 256, 736, 1024), (DX, 256, 1024, 1024), (DX, 256, 1028, 1024), (DW, 256, 1024, 1024),      # ... >= 192 tiles, Cn % 8
    (FWD, 32, 8192, 1024), (FWD, 32, 24, 262144), (DX, 16, 32, 262144),                                   # ... Cn >= 32
    (FWD, 3, 8192, 8191), (DX, 8192, 3, 8191), (FWD, 4, 8192, 8191),                                      # any-alignment loaders: R, Cn, K >= 4
    (FWD, 8192, 8192, 512), (FWD, 8192, 4096, 512), (FWD, 2304, 4096, 1024), (FWD, 2048, 4096, 1024),     # 0.85 fill rule of the wide tile
    (FWD, 1024, 1024, 8192), (DW, 512, 512, 65536), (DW, 1024, 119, 1024), (FWD, 100, 100, 100000),       # split plans
)


def _ld(layout, R, Cn, K):
    """natural leading dimensions of dense operands: a row-major operand has its inner length contiguous, a k-major one its rows"""
    la, lb = layout
    return (K if la == LD_ROW else R), (K if lb == LD_ROW else Cn), Cn


def grid():
    """rows (la, lb, R, Cn, K, lda, ldb, ldc), in a fixed order without repeats"""
    sys.path.insert(0, ROOT)
    from oracle.shapes import param_shapes
    prods = []
    for alg, S, A, B, kw in AGENTS:
        for _, shape in param_shapes(alg, S, A, **kw):
            if len(shape) != 2:
                continue
            N, K = shape                                                    # a layer Y[B, N] = X[B, K] W[N, K]^T: forward, dX, weight gradient
            prods += [(FWD, B, N, K), (DX, B, K, N), (DW, N, K, B)]
        if alg == 'ctrlsac':
            F = kw['feature_dim']                                           # the InfoNCE score matrix phi mu^T [B, B] and its two gradients
            prods += [(FWD, B, B, F), (DX, B, F, B), (DW, B, F, B)]
    prods += list(HAND) + list(EDGES)
    prods += [(REFUSED, R, Cn, K) for _, R, Cn, K in HAND]
    rows, seen = [], set()
    for layout, R, Cn, K in prods:
        lda, ldb, ldc = _ld(layout, R, Cn, K)
        # ... and leading dimensions that are no multiple of four: each sets one scalar side
        for ld in ((lda, ldb, ldc), (lda + 1, ldb, ldc), (lda, ldb + 2, ldc), (lda, ldb, ldc + 3)):
            row = (layout[0], layout[1], R, Cn, K) + ld
            if row not in seen:
                seen.add(row)
                rows.append(list(row))
    return rows


def plan(lib, row):
    out = [C.c_int32() for _ in range(5)]
    rc = lib.rlrep_gemm_plan(*row, *[C.byref(o) for o in out])
    assert rc == 0, (row, rc)
    return [o.value for o in out]                # engine, tile, splits, kchunk, scalar_sides


def record(lib, rows):
    plans = {}
    for s in SETTINGS:
        os.environ['RLREP_DISABLE'] = s
        plans[s] = [plan(lib, r) for r in rows]
    return plans


if __name__ == '__main__':
    assert os.environ.get('RLREP_LIB'), 'point RLREP_LIB at a library built from the base commit (see the module docstring)'
    os.environ.pop('RLREP_ENABLE', None)
    sys.path.insert(0, ROOT)
    from rlrep_amd import _lib
    rows = grid()
    plans = record(_lib.lib, rows)
    with open(FIXTURE, 'w') as f:
        f.write('{"library": "base commit", "columns": ["la", "lb", "R", "Cn", "K", "lda", "ldb", "ldc"],\n "grid": [\n')
        f.write(',\n'.join('  ' + json.dumps(r) for r in rows))
        f.write('\n ],\n "results": ["engine", "tile", "splits", "kchunk", "scalar_sides"],\n "plans": {\n')
        f.write(',\n'.join('  %s: %s' % (json.dumps(s), json.dumps(plans[s], separators=(',', ':'))) for s in SETTINGS))
        f.write('\n }}\n')
    pairs = sorted({(p[0], p[1]) for p in plans['']})
    print(f'{len(rows)} rows x {len(SETTINGS)} settings -> {FIXTURE} ({os.path.getsize(FIXTURE)} bytes); default (engine, tile) pairs: {pairs}')
    for layout, R, Cn, K in HAND:
        print((layout, R, Cn, K), plans[''][rows.index([layout[0], layout[1], R, Cn, K, *_ld(layout, R, Cn, K)])])
