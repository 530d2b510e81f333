// gemm_common.h -- what more than one GEMM kernel family needs (gemm_nt.hip, gemm_tn.hip, gemm_small.hip): the launch parameters, the gathered
// A-row addressing, the inf check of the gradient stores, the LDS-staged epilogue of the 128 x 128 tiles, the K-loop stage ring and the
// host-side XCD arrangement.
#pragma once
#include <stdlib.h>
#include "common.h"

namespace {

constexpr int BM = 128, BN = 128, BK = 64, NTHREADS = 256;
constexpr int STAGE_BYTES = (BM + BN) * BK * 2;   // 32 KiB
constexpr int CS_LD = 132;                          // padded f32 row of the epilogue staging tile

struct GemmParams {
    const void* A; const void* B; void* C;
    int M, N, K, lda, ldb, ldc;
    const float* bias; const float* rowvec; int rv_ld, rv_rpg, rv_mod;
    const void* res; int ldres;
    svdx_gather g; const void* zero_page;
    int out_mode; float alpha; int split_k; int tiles_m, tiles_n; int vec_ok; long slab_stride; int a_bytes, b_bytes;
    int xcd_n, sub_m, sub_n;   // variant 4: the 8 XCDs form an (8/xcd_n) x xcd_n grid, each owning sub_m x sub_n tiles (0: balanced row-major split)
    int z_xcd;                 // variant 4, split_k in {2, 4, 8}: K slice z owns 8 / split_k XCDs, arranged (8/split_k/xcd_n) x xcd_n over the tiles (1-D grid)
    int epi; const void* aux_in; void* aux_out; int aux_dim;   // fused GEGLU epilogues (variant 4)
    float* a_colsum;                                           // TN form: += column sums of A (the bias gradient), or null
    float* found_inf;                                          // TN form, float store / += modes: *found_inf = 1 when a value written is not finite (or null)
    // variant 4, second operand pair: acc += A2 [M, K2] B2^T [N, K2] after the main reduction (the LoRA term of a projection)
    const void* A2; const void* B2; int K2, lda2, ldb2, a2_bytes, b2_bytes;
    int a2_seg;   // > 0: output columns [j * a2_seg, (j + 1) * a2_seg) read A2 columns [j * K2, (j + 1) * K2) (fused q/k/v adapters)
    // variant 4, activation output: GroupNorm statistics of the tensor this launch writes (sum, sum of squares per (sample, group) of the
    // ROUNDED values, in the fixed-point replica slots svdx_gn_apply reads) -- the norm that consumes C needs no pass of its own over it
    unsigned long long* gn_stats; int gn_rows, gn_cg; float gn_m0, gn_m1;
    // variant 4 / 5: rows a row tile OWNS (= its stride over M).  Equal to the tile height except for the 144-row tile of variant 36,
    // which steps 140 rows (35840 = 256 x 140, 8960 = 64 x 140: the grid fills every workgroup slot of the chip exactly); rows of a
    // tile beyond its step are computed and not stored (they are the next tile's).
    int m_step;
};

struct RowInfo { int a, b, base; };   // per gathered A row (meaning depends on gather mode)

// Source row (of the gathered tensor) that tap `tap` of a gathered A row reads; valid: the tap lies inside the image.  The one place the
// tap -> source map is written down: the forward / data-gradient staging (a_row_ptr) and the weight-gradient staging (gemm_tn.hip) call it.
__device__ __forceinline__ int a_row_src(const svdx_gather& g, const RowInfo& ri, int tap, bool& valid) {
    int src;
    if (g.mode == SVDX_GATHER_CONV3X3 || g.mode == SVDX_GATHER_CONV3X3_PAD0) {
        int dy = tap / 3, dx = tap - dy * 3;
        int ys = ri.a + dy, xs = ri.b + dx;
        valid = (ys >= 0) & (ys < g.hi) & (xs >= 0) & (xs < g.wi);
        int wsrc = g.wi >> g.ups;
        src = ri.base + (ys >> g.ups) * wsrc + (xs >> g.ups);
    } else if (g.mode == SVDX_GATHER_CONV3X3_DGRAD2) {
        int dy = tap / 3, dx = tap - dy * 3;
        int y2 = ri.a - dy, x2 = ri.b - dx;
        valid = (y2 >= 0) & ((y2 & 1) == 0) & ((y2 >> 1) < g.hi) & (x2 >= 0) & ((x2 & 1) == 0) & ((x2 >> 1) < g.wi);
        src = ri.base + (y2 >> 1) * g.wi + (x2 >> 1);
    } else {   // TEMPORAL3
        int ts = ri.a + tap - 1;
        valid = (ts >= 0) & (ts < g.t);
        src = ri.base + ts * g.hw;
    }
    return src;
}

template <typename T>
__device__ __forceinline__ const T* a_row_ptr(const GemmParams& p, const RowInfo& ri, int m_clamped, int k0,
                                              int tap, int ci0, bool& valid) {
    const T* A = reinterpret_cast<const T*>(p.A);
    const svdx_gather& g = p.g;
    valid = true;
    if (g.mode == SVDX_GATHER_PLAIN) return A + (size_t)m_clamped * p.lda + k0;
    const int src = a_row_src(g, ri, tap, valid);
    return A + (size_t)(valid ? src : 0) * g.lda + ci0;
}

__device__ __forceinline__ RowInfo decode_row(const svdx_gather& g, int m) {
    RowInfo ri{0, 0, 0};
    if (g.mode == SVDX_GATHER_CONV3X3 || g.mode == SVDX_GATHER_CONV3X3_PAD0) {
        int x = m % g.wo, t = m / g.wo;
        int y = t % g.ho, n = t / g.ho;
        const int pad = g.mode == SVDX_GATHER_CONV3X3 ? 1 : 0;      // PAD0: the zero row / column sit below / right of the image only
        ri.a = y * g.stride - pad;
        ri.b = x * g.stride - pad;
        ri.base = n * (g.hi >> g.ups) * (g.wi >> g.ups);
    } else if (g.mode == SVDX_GATHER_CONV3X3_DGRAD2) {
        int x = m % g.wo, t = m / g.wo;
        int y = t % g.ho, n = t / g.ho;
        ri.a = y + 1;
        ri.b = x + 1;
        ri.base = n * g.hi * g.wi;
    } else if (g.mode == SVDX_GATHER_TEMPORAL3) {
        int pp = m % g.hw, t = m / g.hw;
        int tt = t % g.t, b = t / g.t;
        ri.a = tt;
        ri.base = b * g.t * g.hw + pp;
    }
    return ri;
}

// GradScaler's inf check folded into the kernels that WRITE the gradients (round 5): a weight gradient that is stored once per step is
// tested where it is stored, and svdx_check_finite_spans covers the few slots that are accumulated -- the 1.59 GB pass of
// svdx_check_finite over the flat buffer leaves the single-rank step.  Any number of threads may raise the flag (same value, no ordering).
__device__ __forceinline__ bool not_finite(float v) { return (__builtin_bit_cast(unsigned, v) & 0x7f800000u) == 0x7f800000u; }
__device__ __forceinline__ void raise_found_inf(float* found, bool bad) {
    if (found && __any(bad) && (threadIdx.x & 63) == 0) *found = 1.f;
}

template <typename T>
__device__ __forceinline__ void gemm_epilogue(const GemmParams& p, f32x4 (&acc)[4][4], char* smem, int m0, int n0, int z, int tid,
                                              int lane, int wm, int wn) {
    // ---- epilogue: stage 64 rows at a time through LDS as f32, then vectorised fused store ----
    float* Cs = reinterpret_cast<float*>(smem);
    bool bad_any = false;
    const bool lead = (z == 0) && p.out_mode != SVDX_OUT_F32_SLAB;
    T* Ct = reinterpret_cast<T*>(p.C);
    float* Cf = reinterpret_cast<float*>(p.C) + (p.out_mode == SVDX_OUT_F32_SLAB ? (size_t)z * p.slab_stride : 0);
    const T* R = reinterpret_cast<const T*>(p.res);
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {
        if (wm == pass) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        Cs[(i * 16 + (lane >> 4) * 4 + r) * CS_LD + wn * 64 + j * 16 + (lane & 15)] = acc[i][j][r];
        }
        __syncthreads();
#pragma unroll 1
        for (int i = 0; i < 4; ++i) {
            const int id = i * 256 + tid;
            const int row = id >> 4, c8 = id & 15;
            const int m = m0 + pass * 64 + row, nc = n0 + c8 * 8;
            if (m >= p.M || nc >= p.N) continue;
            float v[8];
            const f32x4 lo = *reinterpret_cast<const f32x4*>(Cs + row * CS_LD + c8 * 8);
            const f32x4 hi = *reinterpret_cast<const f32x4*>(Cs + row * CS_LD + c8 * 8 + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) { v[j] = lo[j] * p.alpha; v[4 + j] = hi[j] * p.alpha; }
            const bool full = p.vec_ok && (nc + 8 <= p.N);
            const int nvalid = min(8, p.N - nc);
            if (lead) {
                if (p.bias) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) if (j < nvalid) v[j] += p.bias[nc + j];
                }
                if (p.rowvec) {
                    const int gi = p.rv_mod ? (m % p.rv_mod) : (m / p.rv_rpg);
                    const float* rv = p.rowvec + (size_t)gi * p.rv_ld + nc;
#pragma unroll
                    for (int j = 0; j < 8; ++j) if (j < nvalid) v[j] += rv[j];
                }
                if (R) {
                    const T* rp = R + (size_t)m * p.ldres + nc;
                    if (full) {
                        float rr[8];
                        load8<T>(rp, rr);
#pragma unroll
                        for (int j = 0; j < 8; ++j) v[j] += rr[j];
                    } else {
#pragma unroll
                        for (int j = 0; j < 8; ++j) if (j < nvalid) v[j] += to_f<T>(rp[j]);
                    }
                }
            }
            const size_t co = (size_t)m * p.ldc + nc;
            if (p.out_mode == SVDX_OUT_ACT) {
                if (full) {
                    store8<T>(Ct + co, v);
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) if (j < nvalid) Ct[co + j] = from_f<T>(v[j]);
                }
            } else if (p.out_mode == SVDX_OUT_F32 || p.out_mode == SVDX_OUT_F32_SLAB) {
                if (full) {
                    *reinterpret_cast<f32x4*>(Cf + co) = f32x4{v[0], v[1], v[2], v[3]};
                    *reinterpret_cast<f32x4*>(Cf + co + 4) = f32x4{v[4], v[5], v[6], v[7]};
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) if (j < nvalid) Cf[co + j] = v[j];
                }
                if (p.found_inf && p.out_mode == SVDX_OUT_F32) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) bad_any |= j < nvalid && not_finite(v[j]);
                }
            } else if (p.out_mode == SVDX_OUT_F32_ADD) {      // this block owns the element: plain read-modify-write
                if (full) {
                    f32x4 c0 = *reinterpret_cast<const f32x4*>(Cf + co), c1 = *reinterpret_cast<const f32x4*>(Cf + co + 4);
                    c0 += f32x4{v[0], v[1], v[2], v[3]};
                    c1 += f32x4{v[4], v[5], v[6], v[7]};
                    *reinterpret_cast<f32x4*>(Cf + co) = c0;
                    *reinterpret_cast<f32x4*>(Cf + co + 4) = c1;
                    if (p.found_inf) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) bad_any |= not_finite(c0[j]) || not_finite(c1[j]);
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) if (j < nvalid) { const float t = Cf[co + j] + v[j]; Cf[co + j] = t; bad_any |= p.found_inf && not_finite(t); }
                }
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) if (j < nvalid) atomicAdd(Cf + co + j, v[j]);
            }
        }
        __syncthreads();
    }
    raise_found_inf(p.found_inf, bad_any);
}

// ---- the K-loop stage ring of gemm_v4_kernel, gemm_tn_kernel and gemm_tn8_kernel ----
// The stages form a ring: while tile kt is computed, tiles kt+1 .. kt+NSTG-2 are in flight and the pieces of tile kt+NSTG-1 are
// issued into the stage tile kt-1 just left.  One barrier per K-step.  With more than two stages the wait in front of it is a
// COUNTED vmcnt -- it retires this wave's pieces of tile kt+1 and leaves the younger tiles in flight across the barrier, which
// must then be the raw s_barrier (__syncthreads() fences with vmcnt(0) while an LDS-DMA is pending); every wave issues the same
// number of pieces per tile, so the count is exact.  The two-stage form (wait for everything, __syncthreads) is the round-1 loop:
// right when two workgroups share a CU and hide each other's drain; the ring is for grids of <= 1 workgroup per CU (the 10x16 /
// 5x8 levels, where a drained K-step is one exposed L2 / HBM round trip) and for the eight-wave tiles.
template <int NSTG>
__device__ __forceinline__ void stage_barrier() {
    if (NSTG == 2) { __syncthreads(); return; }
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}
// The ring is a macro, not a function template over callables: inlined through a helper function the same loops reach the optimiser with
// another block order, and every kernel that uses them is scheduled differently (all 16 TN kernels were; tried with the callables taken
// by reference, by value, and with the issue step wrapped or passed through).  Expanded in place the device code is what the three
// hand-written copies gave.  Arguments (statements may use the ring's own `t`, `cur`, `nxt`, `kt` and `LA` = NSTG - 1):
//   N_TILES     K-tiles of this workgroup
//   ISSUE       prologue: stage tile t (0 .. LA - 1, counted from the workgroup's first) into stage t
//   STEADY      compute stage cur and stage tile kt + LA into stage nxt (in front of the MFMAs, or piece by piece between their rows)
//   DRAIN       compute stage cur, nothing left to stage
//   WAIT        wait_tiles(n): s_waitcnt that leaves at most the n youngest tiles of this wave in flight -- the piece counts are the kernel's
#define SVDX_STAGE_RING(NSTG, N_TILES, ISSUE, STEADY, DRAIN, WAIT)                       \
    {                                                                                    \
        constexpr int LA = (NSTG) - 1;   /* tiles staged ahead of the one being computed */ \
        static_assert(LA >= 1 && LA <= 3, "2 to 4 LDS stages");                          \
        _Pragma("unroll") for (int t = 0; t < LA; ++t)                                   \
            if (t < (N_TILES)) { ISSUE; }                                                \
        WAIT(min(LA, (N_TILES)) - 1);                                                    \
        stage_barrier<NSTG>();                                                           \
        int cur = 0, nxt = LA, kt = 0;                                                   \
        for (; kt + LA < (N_TILES); ++kt) {                                              \
            STEADY;                                                                      \
            WAIT(LA - 1);                                                                \
            stage_barrier<NSTG>();                                                       \
            cur = cur + 1 == (NSTG) ? 0 : cur + 1;                                       \
            nxt = nxt + 1 == (NSTG) ? 0 : nxt + 1;                                       \
        }                                                                                \
        for (; kt < (N_TILES); ++kt) {                                                   \
            DRAIN;                                                                       \
            if (kt + 1 < (N_TILES)) {                                                    \
                WAIT((N_TILES) - 2 - kt);                                                \
                stage_barrier<NSTG>();                                                   \
            }                                                                            \
            cur = cur + 1 == (NSTG) ? 0 : cur + 1;                                       \
        }                                                                                \
    }

// raises a kernel's dynamic-LDS limit; the launchers call it once per instantiation, through a function-local static
template <typename Kernel>
bool allow_lds(Kernel* kernel, int bytes) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    return true;
}

// XCDs as an (xcds / xn) x xn grid over tiles_m x tiles_n tiles, each owning cdiv(tiles_m, xcds / xn) x cdiv(tiles_n, xn) of them: -> the xn
// with the least operand re-fetch (`cost`: every XCD column re-fetches A, every XCD row re-fetches B) among those that keep >= 90 % of
// the best tile balance
static int xcd_arrangement(int tiles_m, int tiles_n, int xcds, double a_bytes, double b_bytes, double& best_cost) {
    int best_xn = 0;
    double best_eff = 0;
    best_cost = 0;
    for (int pass = 0; pass < 2; ++pass)
        for (int xn = 1; xn <= xcds; xn *= 2) {
            const int xm = xcds / xn, sm = cdiv(tiles_m, xm), sn = cdiv(tiles_n, xn);
            const double eff = (double)tiles_m * tiles_n / ((double)xcds * sm * sn);
            if (pass == 0) { best_eff = eff > best_eff ? eff : best_eff; continue; }
            const double cost = a_bytes * xn + b_bytes * xm;
            if (eff >= 0.9 * best_eff && (best_xn == 0 || cost < best_cost)) { best_xn = xn; best_cost = cost; }
        }
    return best_xn;
}

}  // namespace
