// gemm_tiles.h -- the output tiles of svdx_gemm: ONE list that the geometry table, the launch switch of gemm_entry and the rules that turn a
// `variant` argument into a tile (resolve_tile; queryable as svdx_gemm_tile) are generated from.  ops.GEMM_TILES is its Python twin, held
// to it by value (tests/test_host_logic.py).  Host code only.
#pragma once
#include "../../include/svdx.h"

// V4(id, narrower sibling or 0, NB, MB, WGM, NSTG, MSTEP): gemm_v4_kernel, (16 MB WGM) x (32 NB), NSTG stages, 2 WGM waves; MSTEP: rows the
//     tile owns when fewer than it computes.      V5(id, sibling, MF, NF): gemm_v5_kernel, (32 MF) x (64 NF), two K-tiles, eight waves.
//    6 / 7 / 8: the two-stage four-wave tiles (two workgroups per CU), the only ones with the second-operand loop
//   16 / 17 / 18, 20 / 21, 22 / 23, 24 / 25: ring-staged tiles (see the K-loop banner), one workgroup per CU.  22 / 23 at M = 8960: 47 row
//       tiles x 5 = 235 of 256 CUs where 256-row tiles give 175; 24 / 25 at M = 2240, N = 1280, short K: 240 tiles, not 180
//   26: 192x128, TWO stages, eight waves: 80 KB of LDS and 114 VGPRs, so TWO workgroups share a CU -- the tile under the GEGLU
//       epilogues, where main loop, GELU polynomial and 275-366 MB of stores run one after the other inside a workgroup
//   27 / 28: TWO stages, eight waves (64 / 72 KB of LDS: two workgroups per CU): candidates of the in-situ tuner for the short-K linears
//   32 / 34: two-role tiles (round 6), one workgroup per CU
//   36 (round 6): 144 x 160, SIX waves (3 x 2), two stages, two workgroups per CU, row tiles 140 apart -- the 64x40 level's 35840 rows are
//       256 x 140 and the 32x20 level's 8960 are 64 x 140, so N = 320 / 1280 give exactly 512 workgroups: every slot of the chip, where the
//       160-row tile of variant 6 fills 448
#define SVDX_GEMM_TILES(V4, V5)                                                                                            \
    V4( 6,  8, 5, 5, 2, 2, 0)   /* 160x160 */  V4( 7,  8, 5, 4, 2, 2, 0)   /* 128x160 */  V4( 8, 0, 4, 4, 2, 2, 0)   /* 128x128 */ \
    V4(16, 17, 5, 4, 4, 3, 0)   /* 256x160 */  V4(17,  0, 4, 4, 4, 3, 0)   /* 256x128 */  V4(18, 17, 8, 4, 4, 2, 0)  /* 256x256 */ \
    V4(20, 21, 5, 4, 2, 4, 0)   /* 128x160 */  V4(21,  0, 4, 4, 2, 4, 0)   /* 128x128 */                                          \
    V4(23, 22, 5, 3, 4, 3, 0)   /* 192x160 */  V4(22,  0, 4, 3, 4, 3, 0)   /* 192x128 */                                          \
    V4(25, 24, 5, 3, 2, 4, 0)   /*  96x160 */  V4(24,  0, 4, 3, 2, 4, 0)   /*  96x128 */                                          \
    V4(26,  0, 4, 3, 4, 2, 0)   /* 192x128 */  V4(28, 27, 5, 2, 4, 2, 0)   /* 128x160 */  V4(27,  0, 4, 2, 4, 2, 0)  /* 128x128 */ \
    V5(32, 16, 8, 4)            /* 256x256 */  V5(34, 16, 5, 5)            /* 160x320 */                                          \
    V4(36, 28, 5, 3, 3, 2, 140) /* 144x160, steps 140 */

struct GemmTile {
    int id, sibling;
    int row_step, rows, cols, stages, waves;    // rows a tile owns | computes; columns; LDS stages of the K-loop; waves per workgroup
    bool has_dual;                              // the LoRA second-operand loop is only instantiated for the two-stage four-wave tiles
    bool v5;
};
#define SVDX_TILE_ROW_V4(id, sib, NB, MB, WGM, NSTG, MSTEP) \
    {id, sib, (MSTEP) ? (MSTEP) : 16 * (MB) * (WGM), 16 * (MB) * (WGM), 32 * (NB), NSTG, 2 * (WGM), (WGM) == 2 && (NSTG) == 2, false},
#define SVDX_TILE_ROW_V5(id, sib, MF, NF) {id, sib, 32 * (MF), 32 * (MF), 64 * (NF), 2, 8, false, true},
constexpr GemmTile GEMM_TILES[] = {SVDX_GEMM_TILES(SVDX_TILE_ROW_V4, SVDX_TILE_ROW_V5)};

static inline const GemmTile* gemm_tile(int id) {
    for (const GemmTile& t : GEMM_TILES)
        if (t.id == id) return &t;
    return nullptr;
}

// The tile svdx_gemm launches for `variant`: an id of the list, 0 for the 64-bit-pointer gemm_kernel (variants 0 / 1), < 0: unknown variant.
static inline int resolve_tile(int variant, int M, int N, int split_k, int epilogue, int aux_dim) {
    if (variant < 2) return 0;
    const int n_cols = epilogue == SVDX_EPI_GEGLU_FWD ? 2 * aux_dim : N;
    // the GEGLU-forward epilogue pairs 64 value with 64 gate columns: no 160-wide tile under it
    const bool wide_ok = epilogue != SVDX_EPI_GEGLU_FWD && N % 160 == 0;
    int id = variant;
    if (variant < 16) {
        // variant 4 = heuristic; 6 / 7 / 8 force 160x160 / 128x160 / 128x128 (the host autotuner times them); the rest of 2..15 run like 7
        id = variant == 6 || variant == 8 ? variant : 7;
        // 160-row tiles when they turn a 1.1-wave grid (512 resident blocks) into a single wave, e.g. M = 35840, N = 320:
        // 280 x 2 = 560 tiles of 128 rows vs 224 x 2 = 448 tiles of 160 rows
        const long t128 = ((long)M + 127) / 128 * (((long)N + 159) / 160), t160 = ((long)M + 159) / 160 * (((long)N + 159) / 160);
        if (variant == 4 && split_k == 1 && wide_ok && ((t128 + 511) / 512 * 4 > (t160 + 511) / 512 * 5) && t160 >= 384) id = 6;
    }
    // A 160-wide request on an N that 160 does not divide (or with the GEGLU-forward epilogue) takes the 128-wide sibling; the 256-wide
    // ring tile needs whole column tiles (18 -> 17), the two-role tiles need them under a GEGLU epilogue only (32 / 34 -> 16 -> 17).
    for (;;) {
        const GemmTile* t = gemm_tile(id);
        if (!t) return -1;
        const bool fits = t->cols == 128 || (t->cols == 160 ? wide_ok : (t->v5 && epilogue == SVDX_EPI_NONE) || n_cols % t->cols == 0);
        if (fits) return id;
        id = t->sibling;
    }
}
