// The tile kinds of the LDS-tiled GEMM engine (gemm_lds.hip), each described ONCE: the routing (rl_gemm_lds_route), the launcher
// (rl_launch_gemm_lds), the program builder (engine_internal.h Builder::gemm / gemm_lds_stage) and the entry points rlrep_gemm / rlrep_gemm_plan
// (engine.hip) all read this table, number their tiles through gl_number_tiles and ask the same two eligibility predicates.  Host only.
#pragma once
#include "../../include/rlrep.h"
#include "common.h"

enum GlKind { GL_GEMM16 = 0, GL_T64, GL_T128, GL_X3Q32, GL_X3S64, GL_X3_128, GL_X3W256, GL_NKINDS };
struct GlKindDesc {
    int rows, cols;         // the output tile (rows: also the tile rlrep_gemm_plan reports)
    int engine_tag;         // RLREP_ENGINE_*: what rlrep_stage_info reports for a stage of this kind
    int plan_engine;        // what rlrep_gemm_plan reports: 0 = 16-row engine, 1 = fp32 MFMA, 2 = bf16x3
    bool group_form;        // has a seed-group form (group.h)
    bool split_k;           // can write split-K slabs for the finishing blocks
    bool fin_inline;        // can finish its split-K sums inside the launch (FLAG_FIN_INLINE, opt-in)
};
static constexpr GlKindDesc GL_KINDS[GL_NKINDS] = {
    { 16,  16, RLREP_ENGINE_GEMM16, 0, true,  false, false},       // GL_GEMM16: no tile of this engine -- the task stays on the 16-row tile engine (gemm16.hip)
    { 64,  64, RLREP_ENGINE_LDS64,  1, true,  true,  false},       // GL_T64: fp32 MFMA
    {128, 128, RLREP_ENGINE_LDS128, 1, true,  true,  false},       // GL_T128: fp32 MFMA
    { 32,  32, RLREP_ENGINE_X3,     2, true,  false, false},       // GL_X3Q32: bf16 pipe (bf16x3); its four waves split K among themselves (gemm_x3q.h)
    { 64,  64, RLREP_ENGINE_X3,     2, true,  true,  true },       // GL_X3S64: bf16 pipe
    {128, 128, RLREP_ENGINE_X3,     2, true,  true,  false},       // GL_X3_128: bf16 pipe
    {256, 128, RLREP_ENGINE_X3,     2, false, true,  false},       // GL_X3W256: bf16 pipe, persistent workgroups that walk the tiles by grid stride (gemm_x3w.h)
};

// Tile numbering of one launch, from tasks whose splits / kchunk are set: every task gets its column-tile count, its tile count (splits included)
// and its first tile; a split task its first finishing block -- 0x7fffffff (no finishing block ever matches it) where its slabs are summed elsewhere
// (FLAG_FIN_IN_ADAM: by the optimizer launch; FLAG_FIN_INLINE: inside the launch).  Returns the launch's tiles and, in *fin_blocks, its finishing blocks.
static inline int gl_number_tiles(GemmTask* tasks, int ntasks, GlKind kind, int* fin_blocks) {
    const GlKindDesc& d = GL_KINDS[kind];
    int base = 0, fin = 0;
    for (int q = 0; q < ntasks; ++q) {
        GemmTask& t = tasks[q];
        t.tiles_c = (t.Cn + d.cols - 1) / d.cols;
        t.ntiles = ((t.R + d.rows - 1) / d.rows) * t.tiles_c * t.splits; t.tile_base = base; base += t.ntiles;
        if (t.splits <= 1) continue;
        if (t.flags & (FLAG_FIN_IN_ADAM | FLAG_FIN_INLINE)) { t.fin_base = 0x7fffffff; continue; }
        const bool bias = t.epi == EPI_DW && (t.flags & FLAG_BIASGRAD);
        t.fin_base = fin;
        fin += (int)(((long long)t.R * ((t.Cn + 3) / 4) + 255) / 256) + (bias ? (t.R + 255) / 256 : 0);
    }
    *fin_blocks = fin;
    return base;
}
// Can the 32 x 32 tile run this task?  Row-major A, 16-byte-regular operands (`flags`: the task's scalar-staging flags), K in whole 16-deep
// steps and at least two of them, no slabs, and whole 8-column groups of a k-major B.
static inline bool gl_x3q_can_run(const GemmTask* t, int la, int lb, int flags, int splits) {
    return la == LD_ROW && !(flags & (FLAG_SCALAR_A | FLAG_SCALAR_B)) && (t->K & 15) == 0 && t->K >= 32 && splits == 1 &&
           !(lb == LD_COL && ((t->Cn & 7) || t->Cn < 8));
}
// Can the any-alignment loaders of the 64-wide bf16x3 tile run this task?  (the pulled-back tail load needs four elements to exist)
static inline bool gl_x3s_unaligned_can_run(const GemmTask* t) { return t->R >= 4 && t->Cn >= 4 && t->K >= 4; }
