// gemm_nt.hip -- NT GEMM on MFMA for gfx950 with an implicit-convolution A operand.
//
//   acc[m,n] = sum_k Aeff[m,k] * B[n,k]      (f16/bf16 in, f32 accumulate, v_mfma_f32_16x16x32_*)
//
// One kernel serves every matmul-shaped op of the SVD UNet step: nn.Linear fwd /
// data-grad / weight-grad, conv2d 3x3 (stride 1/2, nearest-x2 source) and its data-grads, Conv3d (3,1,1).
// Convolutions never materialise im2col: each K-tile of 64 channels belongs to one filter tap, and the A
// rows of that tile are fetched from the tap's shifted pixel (or from a zero page outside the image).
//
// Kernels in this file (variant argument of svdx_gemm):
//   variant 0 / 1  gemm_kernel: 128x128x64, global_load_lds_dwordx4 (LDS-DMA) with 64-bit pointers, swizzle on the per-lane SOURCE
//              address -- the fallback when a buffer exceeds the 2 GiB range of variant 4's 32-bit offsets (round 1's register-staged
//              variant 0 was removed in round 4: it now runs this kernel too)
//   variant 4  gemm_v4_kernel         : production (see its banner): 128x160 tiles, lean buffer_load...lds loop, coalesced epilogue
//   variant 5 family  gemm_v5_kernel  : two-role eight-wave tiles (see its banner)
// The other GEMM families: gemm_tn.hip (weight gradients straight from row-major dY / X via ds_read_b64_tr_b16) and gemm_small.hip (skinny
// linears, outer products, split-K finalizers); what they share with this file is in gemm_common.h.
// Common: 256 threads = 4 waves (2x2); LDS rows of 128 B with the 16-byte chunk index XOR-swizzled by (row & 7) so the
// ds_read_b128 fragment reads are bank-conflict free (SQ_LDS_BANK_CONFLICT = 0 measured); XCD-aware block -> tile mapping
// (consecutive tiles of one A row-panel stay on one XCD's L2); split-K into float slabs + svdx_gemm_finalize.
#include "gemm_common.h"
#include "gemm_tiles.h"

namespace {

constexpr int GN_MAX_S = 8, GN_MAX_G = 36;               // samples / groups one output tile may touch (else the host runs svdx_gn_stats)
constexpr int GN_LDS = GN_MAX_S * GN_MAX_G * 2 * 8;

template <typename T>
__global__ __launch_bounds__(NTHREADS) void gemm_kernel(GemmParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef typename TT<T>::v8 v8;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;

    // ---- XCD-aware tile mapping (block b runs on XCD b % 8; give each XCD a contiguous run of tiles) ----
    const int nwg = p.tiles_m * p.tiles_n;
    const int bid = blockIdx.x;
    const int xcd = bid & 7, q = nwg >> 3, r8 = nwg & 7;
    const int swz = (xcd < r8 ? xcd * (q + 1) : r8 * (q + 1) + (xcd - r8) * q) + (bid >> 3);
    const int pid_m = swz / p.tiles_n, pid_n = swz - pid_m * p.tiles_n;
    const int m0 = pid_m * BM, n0 = pid_n * BN;

    // ---- split-K range ----
    const int kt_total = p.K / BK;
    const int z = blockIdx.y;
    const int kt_per = (kt_total + p.split_k - 1) / p.split_k;
    const int kt_begin = z * kt_per;
    const int kt_end = min(kt_total, kt_begin + kt_per);
    if (kt_begin >= kt_end) return;

    // ---- per-thread staging assignment: 4 A rows + 4 B rows, one 16-byte chunk each ----
    const int ld_row = tid >> 3;                 // 0..31
    const int pc = tid & 7;                      // physical chunk inside the 128-byte LDS row
    const int lc = pc ^ (ld_row & 7);            // logical chunk (k offset lc*8) that lives there
    int a_m[4];
    RowInfo a_ri[4];
    const T* b_ptr[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int m = min(m0 + i * 32 + ld_row, p.M - 1);
        a_m[i] = m;
        a_ri[i] = decode_row(p.g, m);
        int n = min(n0 + i * 32 + ld_row, p.N - 1);
        b_ptr[i] = reinterpret_cast<const T*>(p.B) + (size_t)n * p.ldb + lc * 8;
    }
    const int cin = p.g.mode == SVDX_GATHER_PLAIN ? p.K : p.g.cin;
    const T* zero = reinterpret_cast<const T*>(p.zero_page);

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    auto stage_ptrs = [&](int kt, const T* (&pa)[4], const T* (&pb)[4]) __attribute__((always_inline)) {
        const int k0 = kt * BK;
        int tap = 0, ci0 = k0;
        if (p.g.mode != SVDX_GATHER_PLAIN) { tap = k0 / cin; ci0 = k0 - tap * cin; }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            bool valid;
            const T* ptr = a_row_ptr<T>(p, a_ri[i], a_m[i], k0, tap, ci0, valid);
            pa[i] = valid ? ptr + lc * 8 : zero;
            pb[i] = b_ptr[i] + k0;
        }
    };
    auto issue_glds = [&](int kt, int stage) __attribute__((always_inline)) {
        const T* pa[4]; const T* pb[4];
        stage_ptrs(kt, pa, pb);
        char* As = smem + stage * STAGE_BYTES;
        char* Bs = As + BM * BK * 2;
        const int wave_u = __builtin_amdgcn_readfirstlane(wave);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            // LDS destination = wave-uniform base + lane*16 (chunk id = i*256 + tid)
            const int base = (i * 256 + wave_u * 64) * 16;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)pa[i],
                                             (__attribute__((address_space(3))) void*)(As + base), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)pb[i],
                                             (__attribute__((address_space(3))) void*)(Bs + base), 16, 0, 0);
        }
    };
    auto compute = [&](int stage) __attribute__((always_inline)) {
        const char* As = smem + stage * STAGE_BYTES;
        const char* Bs = As + BM * BK * 2;
        const int fr = lane & 15, fg = lane >> 4;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const int chunk = ((kk * 4 + fg) ^ (fr & 7)) * 16;
            v8 af[4], bf[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                af[i] = *reinterpret_cast<const v8*>(As + (wm * 64 + i * 16 + fr) * 128 + chunk);
                bf[i] = *reinterpret_cast<const v8*>(Bs + (wn * 64 + i * 16 + fr) * 128 + chunk);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = TT<T>::mfma(af[i], bf[j], acc[i][j]);
        }
    };

    issue_glds(kt_begin, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int cur = 0;
    for (int kt = kt_begin; kt < kt_end - 1; ++kt) {
        issue_glds(kt + 1, cur ^ 1);
        compute(cur);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        cur ^= 1;
    }
    compute(cur);
    __syncthreads();

    gemm_epilogue<T>(p, acc, smem, m0, n0, z, tid, lane, wm, wn);
}

// Which (row tile, column tile, K slice) a workgroup of the gemm_v4 / gemm_v5 kernels computes (false: none -- the grid is rounded up).
// Workgroup ids go round-robin to the 8 XCDs (id & 7), each with a private 4 MiB L2.  Every XCD re-fetches whatever operand
// rows its tiles touch, so the host picks an (8/xcd_n) x xcd_n arrangement of XCDs over the tile grid that minimises
// A_bytes * xcd_n + B_bytes * (8 / xcd_n): row bands when A dominates (the 64x40 level: A = 23 MB x taps, B < 2 MB), column
// bands when the weights dominate (10x16 / 5x8 levels: B = 30-60 MB, A = 1-6 MB; measured 8x weight re-fetch before).
// Split-K (round 4): the K slices of one tile share nothing, so a slice count of 2 / 4 / 8 gives every slice its OWN 8 / split_k XCDs
// (z_xcd): an XCD then streams half / a quarter / an eighth of K for its tiles instead of all of it -- 2240 x 1280 x 10240 in two slices
// fetched 197 MB where 72 MB are algorithmic with every XCD holding both slices of a 3 x 5 tile block; 144 MB with 2 x 2 XCDs per slice.
__device__ __forceinline__ bool v4_tile_of_block(const GemmParams& p, int& pid_m, int& pid_n, int& z) {
    const int bid = blockIdx.x;
    z = blockIdx.y;
    if (p.z_xcd) {
        const int xcd = bid & 7, l = bid >> 3, xps = 8 / p.split_k;
        z = xcd / xps;
        const int xi = xcd - z * xps;
        const int xi_m = xi / p.xcd_n, xi_n = xi - xi_m * p.xcd_n;
        const int lm = l / p.sub_n;
        pid_m = xi_m * p.sub_m + lm;
        pid_n = xi_n * p.sub_n + (l - lm * p.sub_n);
        if (lm >= p.sub_m || pid_m >= p.tiles_m || pid_n >= p.tiles_n) return false;
    } else if (p.xcd_n > 0) {
        const int xcd = bid & 7, l = bid >> 3;
        const int xi_m = xcd / p.xcd_n, xi_n = xcd - xi_m * p.xcd_n;
        const int lm = l / p.sub_n;
        pid_m = xi_m * p.sub_m + lm;
        pid_n = xi_n * p.sub_n + (l - lm * p.sub_n);
        if (lm >= p.sub_m || pid_m >= p.tiles_m || pid_n >= p.tiles_n) return false;
    } else {
        const int nwg = p.tiles_m * p.tiles_n;
        const int xcd = bid & 7, q = nwg >> 3, r8 = nwg & 7;
        const int swz = (xcd < r8 ? xcd * (q + 1) : r8 * (q + 1) + (xcd - r8) * q) + (bid >> 3);
        pid_m = swz / p.tiles_n;
        pid_n = swz - pid_m * p.tiles_n;
    }
    return true;
}

// GEGLU-forward tiles pair 16 value columns with their 16 gate columns: local n-block 2q is rows F*0 + c, block 2q+1 is rows
// F + c of the [2F, K] projection, so a lane ends up holding a value and its gate (no weight re-packing needed).
template <int BN3>
__device__ __forceinline__ int v4_brow(const GemmParams& p, int pid_n, int n0, int nl) {
    return p.epi == SVDX_EPI_GEGLU_FWD ? (((nl >> 4) & 1) ? p.aux_dim : 0) + pid_n * (BN3 / 2) + (nl >> 5) * 16 + (nl & 15)
                                       : min(n0 + nl, p.N - 1);
}

// ---- the store side shared by gemm_v4_kernel and gemm_v5_kernel.  acc[i][j] is the TRANSPOSED 16x16 block (n-block i, m-block j) of a wave that owns
// rows wm * WM4 + j * 16 .. and columns wn * WN3 + i * 16 .. of a BM4 x BN3 tile computed by NT threads: lane (fr, fg) holds row fr, columns fg * 4 .. + 3.
template <typename T, int NB, int MB, int NT, int BM4, int BN3, int WM4, int WN3>
__device__ __forceinline__ void v4_epilogue(const GemmParams& p, char* smem, f32x4 (&acc)[NB][MB], int z, int m0, int n0, int pid_m, int pid_n,
                                            int wm, int wn, int tid) {
    const int lane = tid & 63, fr = lane & 15, fg = lane >> 4;
    const int Fdim = p.aux_dim;
    const int m_lim = min(p.M, m0 + p.m_step);          // first row this tile does not own
    auto brow = [&](int nl) __attribute__((always_inline)) { return v4_brow<BN3>(p, pid_n, n0, nl); };
    // ---- epilogue A (activation output): coalesced.  Each lane adds bias / row vector to its 4-column groups, rounds to the
    //      activation dtype and parks them in LDS (the stage buffers are free now); then every thread moves 16-byte row
    //      pieces: residual add + store with full-line coalescing (20 lanes cover one 320-byte output row of the tile).
    if (p.out_mode == SVDX_OUT_ACT && p.vec_ok && (p.ldc % 8 == 0) && (!p.res || p.ldres % 8 == 0) &&
        (n0 + BN3 <= p.N || p.epi == SVDX_EPI_GEGLU_FWD)) {
        constexpr int PITCH = (BN3 + 8) * 2;              // bytes per staged row (multiple of 16)
        __syncthreads();
        if (p.gn_stats) {                                  // the statistics table sits behind the parked tile; every wave has left the K-loop
            unsigned long long* gacc = reinterpret_cast<unsigned long long*>(smem + ((BM4 * PITCH + 15) & ~15));
            for (int i = tid; i < GN_MAX_S * GN_MAX_G * 2; i += NT) gacc[i] = 0ull;
        }
        {
            const bool lead0 = (z == 0);
            const int nb0 = n0 + wn * WN3 + fg * 4;
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                float bb[4];
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    bb[e] = (lead0 && p.bias) ? p.bias[p.epi == SVDX_EPI_GEGLU_FWD ? brow(wn * WN3 + i * 16 + fg * 4 + e) : nb0 + i * 16 + e] : 0.f;
#pragma unroll
                for (int j = 0; j < MB; ++j) {
                    const int ml = wm * WM4 + j * 16 + fr;
                    const int m = min(m0 + ml, p.M - 1);
                    float v[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = acc[i][j][e] * p.alpha + bb[e];
                    if (lead0 && p.rowvec) {
                        const float* rv = p.rowvec + (size_t)(p.rv_mod ? (m % p.rv_mod) : (m / p.rv_rpg)) * p.rv_ld + nb0 + i * 16;
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] += rv[e];
                    }
                    Vec4<T> o;
#pragma unroll
                    for (int e = 0; e < 4; ++e) o.v[e] = from_f<T>(v[e]);
                    *reinterpret_cast<Vec4<T>*>(smem + ml * PITCH + (wn * WN3 + i * 16 + fg * 4) * 2) = o;
                }
            }
        }
        __syncthreads();
        if (p.epi == SVDX_EPI_GEGLU_FWD) {
            // tile = 128 rows x (BN3/32) pairs of [16 values | 16 gates]; emit pre (both halves) and h = value * gelu(gate)
            T* pre = reinterpret_cast<T*>(p.C);
            T* hh = reinterpret_cast<T*>(p.aux_out);
            constexpr int NPAIR = BN3 / 32;
            for (int id = tid; id < BM4 * NPAIR * 2; id += NT) {
                const int row = id / (NPAIR * 2), r2 = id - row * (NPAIR * 2);
                const int pr = r2 >> 1, c2 = r2 & 1;
                const int m = m0 + row;
                if (m >= m_lim) continue;
                const Vec8<T> a8 = *reinterpret_cast<const Vec8<T>*>(smem + row * PITCH + (pr * 32 + c2 * 8) * 2);
                const Vec8<T> g8 = *reinterpret_cast<const Vec8<T>*>(smem + row * PITCH + (pr * 32 + 16 + c2 * 8) * 2);
                const int fc = pid_n * (BN3 / 2) + pr * 16 + c2 * 8;
                if (fc >= Fdim) continue;
                Vec8<T> h8;
#pragma unroll
                for (int e = 0; e < 8; ++e) h8.v[e] = from_f<T>(to_f<T>(a8.v[e]) * gelu_erf(to_f<T>(g8.v[e])));
                // `pre` is not read again before the backward sweep: streaming (non-temporal) stores keep it out of the L2 / Infinity
                // Cache lines the next kernels want
                typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
                __builtin_nontemporal_store(__builtin_bit_cast(u32x4, a8), reinterpret_cast<u32x4*>(pre + (size_t)m * p.ldc + fc));
                __builtin_nontemporal_store(__builtin_bit_cast(u32x4, g8), reinterpret_cast<u32x4*>(pre + (size_t)m * p.ldc + Fdim + fc));
                *reinterpret_cast<Vec8<T>*>(hh + (size_t)m * Fdim + fc) = h8;
            }
            return;
        }
        constexpr int CPR = BN3 / 8;                      // 16-byte chunks per row
        if (p.epi == SVDX_EPI_GEGLU_BWD) {
            // the tile holds d(h) for columns n0..; read (value, gate) from pre and emit d(pre) = [dh*gelu(g) | dh*a*gelu'(g)]
            const T* pre = reinterpret_cast<const T*>(p.aux_in);
            T* dpre = reinterpret_cast<T*>(p.C);
            for (int id = tid; id < BM4 * CPR; id += NT) {
                const int row = id / CPR, c = id - row * CPR;
                const int m = m0 + row;
                if (m >= m_lim) continue;
                const Vec8<T> d8 = *reinterpret_cast<const Vec8<T>*>(smem + row * PITCH + c * 16);
                const size_t po = (size_t)m * (2 * Fdim) + n0 + c * 8;
                // `pre` was written a whole forward sweep ago and is dead after this read: streaming loads, so that its 183 MB (64x40 level) do not
                // push the d(pre) lines this launch writes -- the A operand of the next GEMM -- out of the Infinity Cache
                typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
                const Vec8<T> a8 = __builtin_bit_cast(Vec8<T>, __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(pre + po)));
                const Vec8<T> g8 = __builtin_bit_cast(Vec8<T>, __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(pre + po + Fdim)));
                Vec8<T> da, dg;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float d = to_f<T>(d8.v[e]), gv = to_f<T>(g8.v[e]);
                    const GeluParts gp = gelu_parts(gv);
                    da.v[e] = from_f<T>(d * gv * gp.cdf);
                    dg.v[e] = from_f<T>(d * to_f<T>(a8.v[e]) * (gp.cdf + gp.pdf_x));
                }
                *reinterpret_cast<Vec8<T>*>(dpre + po) = da;
                *reinterpret_cast<Vec8<T>*>(dpre + po + Fdim) = dg;
            }
            return;
        }
        T* Ct2 = reinterpret_cast<T*>(p.C);
        const T* R2 = (z == 0) ? reinterpret_cast<const T*>(p.res) : nullptr;
        if (p.gn_stats) {
            // Same stores, with every thread on ONE fixed 16-byte column chunk (threads beyond the last whole row of a pass idle) so that the
            // statistics of its 8 channels stay in registers while it walks down the tile's rows.  Rows ascend, so the GroupNorm sample
            // (frame or clip) of a thread changes monotonically: on a change, and at the end, the 8 channel sums are merged into their
            // groups and added to the tile's [sample][group] table in LDS as 64-bit fixed-point integers (integer addition is
            // associative: the statistics do not depend on the order of the atomics -- run-to-run identical, like svdx_gn_stats);
            // the table's nonzero entries then go to the replica slots in HBM, one atomic each.
            constexpr int RPS = NT / CPR;
            unsigned long long* gacc = reinterpret_cast<unsigned long long*>(smem + ((BM4 * PITCH + 15) & ~15));
            const int c = tid % CPR;
            const int s_first = m0 / p.gn_rows, g_first = n0 / p.gn_cg;
            float a0[8], a1[8];
            int cur_s = -1;
            auto flush = [&](int sl) __attribute__((always_inline)) {
                int cur = (n0 + c * 8) / p.gn_cg;
                float s0 = 0.f, s1 = 0.f;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int g = (n0 + c * 8 + e) / p.gn_cg;
                    if (g != cur) {
                        atomicAdd(&gacc[(sl * GN_MAX_G + cur - g_first) * 2], (unsigned long long)__float2ll_rn(s0 * p.gn_m0));
                        atomicAdd(&gacc[(sl * GN_MAX_G + cur - g_first) * 2 + 1], (unsigned long long)__float2ll_rn(s1 * p.gn_m1));
                        cur = g; s0 = 0.f; s1 = 0.f;
                    }
                    s0 += a0[e]; s1 += a1[e];
                }
                atomicAdd(&gacc[(sl * GN_MAX_G + cur - g_first) * 2], (unsigned long long)__float2ll_rn(s0 * p.gn_m0));
                atomicAdd(&gacc[(sl * GN_MAX_G + cur - g_first) * 2 + 1], (unsigned long long)__float2ll_rn(s1 * p.gn_m1));
            };
            if (tid < RPS * CPR) {
                for (int row = tid / CPR; row < BM4; row += RPS) {
                    const int m = m0 + row;
                    if (m >= m_lim) break;
                    Vec8<T> o8 = *reinterpret_cast<const Vec8<T>*>(smem + row * PITCH + c * 16);
                    const size_t co = (size_t)m * p.ldc + n0 + c * 8;
                    if (R2) {
                        const Vec8<T> r8 = *reinterpret_cast<const Vec8<T>*>(R2 + (size_t)m * p.ldres + n0 + c * 8);
#pragma unroll
                        for (int e = 0; e < 8; ++e) o8.v[e] = from_f<T>(to_f<T>(o8.v[e]) + to_f<T>(r8.v[e]));
                    }
                    *reinterpret_cast<Vec8<T>*>(Ct2 + co) = o8;
                    const int sl = m / p.gn_rows - s_first;
                    if (sl != cur_s) {
                        if (cur_s >= 0) flush(cur_s);
                        cur_s = sl;
#pragma unroll
                        for (int e = 0; e < 8; ++e) a0[e] = a1[e] = 0.f;
                    }
#pragma unroll
                        for (int e = 0; e < 8; ++e) { const float v = to_f<T>(o8.v[e]); a0[e] += v; a1[e] += v * v; }
                }
                if (cur_s >= 0) flush(cur_s);
            }
            __syncthreads();
            const int ns_t = (m_lim - 1) / p.gn_rows - s_first + 1, ng_t = (min(n0 + BN3, p.N) - 1) / p.gn_cg - g_first + 1;
            const int n_s = p.M / p.gn_rows, G = p.N / p.gn_cg;
            unsigned long long* out = p.gn_stats + (size_t)((pid_m + pid_n) % SVDX_GN_REPLICAS) * n_s * G * 2;
            for (int i = tid; i < ns_t * ng_t * 2; i += NT) {
                const int w = i & 1, gl = (i >> 1) % ng_t, sl = (i >> 1) / ng_t;
                const unsigned long long v = gacc[(sl * GN_MAX_G + gl) * 2 + w];
                if (v) atomicAdd(out + ((size_t)(s_first + sl) * G + g_first + gl) * 2 + w, v);
            }
            return;
        }
#pragma unroll 2
        for (int id = tid; id < BM4 * CPR; id += NT) {
            const int row = id / CPR, c = id - row * CPR;
            const int m = m0 + row;
            if (m >= m_lim) continue;
            const Vec8<T> t8 = *reinterpret_cast<const Vec8<T>*>(smem + row * PITCH + c * 16);
            const size_t co = (size_t)m * p.ldc + n0 + c * 8;
            if (R2) {
                const Vec8<T> r8 = *reinterpret_cast<const Vec8<T>*>(R2 + (size_t)m * p.ldres + n0 + c * 8);
                Vec8<T> o8;
#pragma unroll
                for (int e = 0; e < 8; ++e) o8.v[e] = from_f<T>(to_f<T>(t8.v[e]) + to_f<T>(r8.v[e]));
                *reinterpret_cast<Vec8<T>*>(Ct2 + co) = o8;
            } else {
                *reinterpret_cast<Vec8<T>*>(Ct2 + co) = t8;
            }
        }
        return;
    }
    // ---- direct epilogue: lane (fr, fg) owns row m = .. + fr and columns n = .. + fg*4 + {0..3} of every 16x16 block ----
    const bool lead = (z == 0) && p.out_mode != SVDX_OUT_F32_SLAB;
    T* Ct = reinterpret_cast<T*>(p.C);
    float* Cf = reinterpret_cast<float*>(p.C) + (p.out_mode == SVDX_OUT_F32_SLAB ? (size_t)z * p.slab_stride : 0);
    const T* R = reinterpret_cast<const T*>(p.res);
    const int nbase = n0 + wn * WN3 + fg * 4;
    float bv[NB][4];
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int n = nbase + i * 16 + e;
            bv[i][e] = (lead && p.bias && n < p.N) ? p.bias[n] : 0.f;
        }
#pragma unroll
    for (int j = 0; j < MB; ++j) {
        const int m = m0 + wm * WM4 + j * 16 + fr;
        if (m >= m_lim) continue;
        const float* rv = nullptr;
        if (lead && p.rowvec) rv = p.rowvec + (size_t)(p.rv_mod ? (m % p.rv_mod) : (m / p.rv_rpg)) * p.rv_ld;
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int n = nbase + i * 16;
            if (n >= p.N) continue;
            const int nvalid = min(4, p.N - n);
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = acc[i][j][e] * p.alpha + bv[i][e];
            if (rv) {
#pragma unroll
                for (int e = 0; e < 4; ++e) if (e < nvalid) v[e] += rv[n + e];
            }
            const bool full = p.vec_ok && nvalid == 4;
            if (lead && R) {
                const T* rp = R + (size_t)m * p.ldres + n;
                if (full) {
                    const Vec4<T> r4 = *reinterpret_cast<const Vec4<T>*>(rp);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] += to_f<T>(r4.v[e]);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) if (e < nvalid) v[e] += to_f<T>(rp[e]);
                }
            }
            const size_t co = (size_t)m * p.ldc + n;
            if (p.out_mode == SVDX_OUT_ACT) {
                if (full) {
                    Vec4<T> o;
#pragma unroll
                    for (int e = 0; e < 4; ++e) o.v[e] = from_f<T>(v[e]);
                    *reinterpret_cast<Vec4<T>*>(Ct + co) = o;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) if (e < nvalid) Ct[co + e] = from_f<T>(v[e]);
                }
            } else if (p.out_mode == SVDX_OUT_F32 || p.out_mode == SVDX_OUT_F32_SLAB) {
                if (full) *reinterpret_cast<f32x4*>(Cf + co) = f32x4{v[0], v[1], v[2], v[3]};
                else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) if (e < nvalid) Cf[co + e] = v[e];
                }
            } else if (p.out_mode == SVDX_OUT_F32_ADD) {
                if (full) {
                    f32x4 c = *reinterpret_cast<const f32x4*>(Cf + co);
                    c += f32x4{v[0], v[1], v[2], v[3]};
                    *reinterpret_cast<f32x4*>(Cf + co) = c;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) if (e < nvalid) Cf[co + e] += v[e];
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) if (e < nvalid) atomicAdd(Cf + co + e, v[e]);
            }
        }
    }
}

// ================================================================================================================
// variant 4 (production): 128 x (32*NB) x 64 tile, NB = 4 or 5, lean K-loop.
//  * All channel counts of the SVD UNet are multiples of 320, so BN = 160 tiles N exactly (BN = 128 wastes 17 % of the MFMA
//    work at N = 320) and raises the MFMA : ds_read ratio (40 : 18 per wave per K-tile).
//  * Accumulators are kept TRANSPOSED (acc = mfma(B_frag, A_frag)): a lane owns 4 consecutive output columns of one row.
//    Activation outputs are rounded, parked in LDS and written with full-line coalesced 16-byte stores (bias / row vector /
//    residual / GEGLU forward+backward fused there); float outputs (slabs, += for weight-grad style uses) go straight from
//    registers with 16-byte stores.
//  * Staging: buffer_load_dwordx4 ... lds with per-lane 32-bit byte offsets computed once per filter tap, the K position as a
//    single scalar soffset, and zero padding from the buffer bounds check (offset >= num_records reads 0) -- no zero page,
//    no select, no 64-bit pointer arithmetic in the loop.  PMC counters that motivated this (profiles/r1_gemm_pmc.txt): the
//    pointer-arithmetic loop issued 2.4 VALU + 2.9 SALU instructions per MFMA (issue bound, MFMA busy ~33 %); this loop issues
//    0.3 VALU + 0.95 SALU.
//  * Tried and dropped: a 5-stage / 4-stage LDS ring with counted vmcnt + raw s_barrier (no gain in
//    situ, slower in isolation: the loop is not latency bound), direct 8-byte epilogue stores (worse DRAM efficiency).
// ================================================================================================================
template <typename T, int NB, int MB, bool DUAL, int WGM, int NSTG>
__global__ __launch_bounds__(128 * WGM, 2) void gemm_v4_kernel(GemmParams p) {     // (two waves per SIMD: the four-wave tiles share a CU in pairs -- 256 registers, whatever the allocator would like)
#if defined(__HIP_DEVICE_COMPILE__)   // the buffer-resource type and LDS-DMA builtin only exist in the device pass
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef typename TT<T>::v8 v8;
    constexpr int NT = 128 * WGM;                     // threads: WGM x 2 waves (WGM = 2: four waves, WGM = 4: eight = two per SIMD)
    constexpr int BM4 = 16 * MB * WGM;                // tile rows: 128 / 160 (four waves) or 256 / 320 (eight waves)
    constexpr int WM4 = 16 * MB;                      // rows per wave
    constexpr int BN3 = 32 * NB;                      // 2 waves along N, NB/2... each wave owns NB*16 columns
    constexpr int WN3 = 16 * NB;                      // columns per wave
    constexpr int KT = BK;                             // K extent of one stage
    constexpr int STAGE3 = (BM4 + BN3) * KT * 2;
    constexpr int CPRW = KT / 8;                       // 16-byte chunks per staged row (8 | 4)
    constexpr int RPP = NT / CPRW;                     // rows covered by one load pass (32 | 64)
    constexpr int NLA = BM4 / RPP;                      // A loads per thread per stage (4 | 2)
    constexpr int NLB = (BN3 + RPP - 1) / RPP;         // B loads per thread per stage (NB | 3 or 2)
    constexpr int ROWB = KT * 2;                       // bytes per staged row (128 | 64)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    int pid_m, pid_n, z;
    if (!v4_tile_of_block(p, pid_m, pid_n, z)) return;
    const int m0 = pid_m * p.m_step, n0 = pid_n * BN3;
    const int kt_total = p.K / KT;
    const int kt_per = (kt_total + p.split_k - 1) / p.split_k;
    const int kt_begin = z * kt_per;
    const int kt_end = min(kt_total, kt_begin + kt_per);
    if (kt_begin >= kt_end) return;

    // ---- lean staging: buffer_load ... lds with per-lane byte offsets (fixed per filter tap) + one scalar K offset ----
    const int ld_row = tid / CPRW, pc = tid % CPRW;
    const int lc = pc ^ (ld_row & 7);
    RowInfo a_ri[NLA];
    int a_m[NLA], voa[NLA], vob[NLB];
#pragma unroll
    for (int i = 0; i < NLA; ++i) {
        a_m[i] = min(m0 + i * RPP + ld_row, p.M - 1);
        a_ri[i] = decode_row(p.g, a_m[i]);
    }
    // GEGLU-forward tiles pair 16 value columns with their 16 gate columns: local n-block 2q is rows F*0 + c, block 2q+1 is rows
    // F + c of the [2F, K] projection, so a lane ends up holding a value and its gate (no weight re-packing needed).
    const int Fdim = p.aux_dim;
    auto brow = [&](int nl) __attribute__((always_inline)) {
        return p.epi == SVDX_EPI_GEGLU_FWD ? (((nl >> 4) & 1) ? Fdim : 0) + pid_n * (BN3 / 2) + (nl >> 5) * 16 + (nl & 15)
                                           : min(n0 + nl, p.N - 1);
    };
#pragma unroll
    for (int i = 0; i < NLB; ++i) {
        const int nl = i * RPP + ld_row;               // tile-local B row; rows >= BN3 (ring, NB = 5) are dummy loads that keep vmcnt uniform
        vob[i] = nl < BN3 ? (brow(nl) * p.ldb + lc * 8) * 2 : (int)0x80000000;
    }
    const bool plain = p.g.mode == SVDX_GATHER_PLAIN;
    const int cin = plain ? p.K : p.g.cin;
    __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.A), 0, p.a_bytes, 0x00020000);
    __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.B), 0, p.b_bytes, 0x00020000);
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    // DUAL: after the K-tiles of (A, B) the same pipeline runs the K2 / KT tiles of the plain pair (A2, B2) into the same
    // accumulators -- y = x W^T + (s x A^T) B^T in one launch instead of a second GEMM that re-reads and re-writes y
    bool seg2 = false;
    int tap = plain ? 0 : (kt_begin * KT) / cin;
    int ci0 = kt_begin * KT - tap * cin;                // channel offset inside the tap (plain: k offset)
    auto set_tap = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < NLA; ++i) {
            bool valid;
            const T* ptr = a_row_ptr<T>(p, a_ri[i], a_m[i], 0, tap, 0, valid);
            // invalid (zero-padding) rows: an offset beyond num_records makes the buffer load return zeros
            voa[i] = valid ? (int)((ptr - reinterpret_cast<const T*>(p.A)) + lc * 8) * 2 : (int)0x80000000;
        }
    };
    set_tap();
    // One staging piece = one buffer_load ... lds per wave (1 KiB).  Issuing an LDS-DMA piece costs the wave ~60-180 issue cycles
    // (MI355X_MICROARCH.md), so the pieces of the NEXT stage are spread between the MFMA rows of the current one instead of being
    // issued as a burst in front of them (which left the wave's MFMA pipe idle for ~1000 cycles per K-step).
    constexpr int NPIECE = NLA + NLB;
    // Eight waves cover 64 tile rows per pass, so a 160-row B tile ends in the middle of its third pass: the waves whose 8 rows lie
    // beyond the tile have nothing to fetch there and skip that piece (their vmcnt arithmetic below counts one piece less per tile).
    constexpr bool B_PARTIAL = NLB * RPP > BN3;
    const bool skip_last = B_PARTIAL && (NLB - 1) * RPP + wave_u * (64 / CPRW) >= BN3;
    auto issue_piece = [&](int stage, int pi) __attribute__((always_inline)) {
        char* As = smem + stage * STAGE3;
        char* Bs = As + BM4 * KT * 2;
        if (pi < NLA) {
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (__attribute__((address_space(3))) void*)(As + (pi * NT + wave_u * 64) * 16), 16,
                                                     voa[pi], ci0 * 2, 0, 0);
        } else {
            const int i = pi - NLA;
            if (B_PARTIAL && i == NLB - 1 && skip_last) return;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (__attribute__((address_space(3))) void*)(Bs + (i * NT + wave_u * 64) * 16), 16, vob[i],
                                                     (tap * cin + ci0) * 2, 0, 0);
        }
    };
    const int n_main = kt_end - kt_begin;                          // K-tiles of the main pair handled by this block
    const int n_tiles = n_main + (DUAL ? p.K2 / KT : 0);
    int issued = 0;
    // called after a tile was issued: make the addressing state describe the next one
    auto advance_k = [&]() __attribute__((always_inline)) {
        ++issued;
        if (DUAL && issued == n_main) {                            // next tile is the first one of (A2, B2): plain addressing
            seg2 = true;
            ci0 = 0;
            tap = 0;                                                   // B offset (tap * cin + ci0) becomes ci0
            rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.A2), 0, p.a2_bytes, 0x00020000);
            rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.B2), 0, p.b2_bytes, 0x00020000);
            const int a2_col = p.a2_seg > 0 ? (n0 / p.a2_seg) * p.K2 : 0;
#pragma unroll
            for (int i = 0; i < NLA; ++i) voa[i] = (min(m0 + i * RPP + ld_row, p.M - 1) * p.lda2 + a2_col + lc * 8) * 2;
#pragma unroll
            for (int i = 0; i < NLB; ++i) {
                const int nl = i * RPP + ld_row;
                vob[i] = nl < BN3 ? (brow(nl) * p.ldb2 + lc * 8) * 2 : (int)0x80000000;
            }
            return;
        }
        ci0 += KT;
        if (!plain && !(DUAL && seg2) && ci0 == cin) { ci0 = 0; ++tap; set_tap(); }
    };
    f32x4 acc[NB][MB];                                   // [n-block][m-block], transposed: rows = n, cols = m
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int j = 0; j < MB; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int fr = lane & 15, fg = lane >> 4;
    // compute stage `stage`; when ISSUE, stage a later K-tile into `nstage` piece by piece between the MFMA rows
#define SVDX_V4_COMPUTE(stage, nstage, ISSUE)                                                                                \
    {                                                                                                                        \
        const char* As_ = smem + (stage) * STAGE3;                                                                           \
        const char* Bs_ = As_ + BM4 * KT * 2;                                                                                \
        _Pragma("unroll") for (int kk = 0; kk < KT / 32; ++kk) {                                                             \
            const int chunk = ((kk * 4 + fg) ^ (fr & 7)) * 16;                                                               \
            v8 af[MB], bf[NB];                                                                                               \
            _Pragma("unroll") for (int i = 0; i < MB; ++i)                                                                   \
                af[i] = *reinterpret_cast<const v8*>(As_ + (wm * WM4 + i * 16 + fr) * ROWB + chunk);                         \
            _Pragma("unroll") for (int i = 0; i < NB; ++i)                                                                   \
                bf[i] = *reinterpret_cast<const v8*>(Bs_ + (wn * WN3 + i * 16 + fr) * ROWB + chunk);                         \
            _Pragma("unroll") for (int i = 0; i < NB; ++i) {                                                                 \
                __builtin_amdgcn_s_setprio(1);  /* the MFMA row outranks the other waves' loads and LDS reads */            \
                _Pragma("unroll") for (int j = 0; j < MB; ++j) acc[i][j] = TT<T>::mfma(bf[i], af[j], acc[i][j]);             \
                __builtin_amdgcn_s_setprio(0);                                                                               \
                if (ISSUE && kk * NB + i < NPIECE) {                                                                         \
                    __builtin_amdgcn_sched_barrier(0);                                                                       \
                    issue_piece((nstage), kk * NB + i);                                                                      \
                    __builtin_amdgcn_sched_barrier(0);                                                                       \
                }                                                                                                            \
            }                                                                                                                \
        }                                                                                                                    \
    }
    static_assert(NPIECE <= (KT / 32) * NB, "not enough MFMA rows to hide the staging pieces");
    // the stage ring (gemm_common.h: SVDX_STAGE_RING), the next tile's pieces issued between the MFMA rows
    auto wait_tiles = [&](int t) __attribute__((always_inline)) {          // leave at most the t youngest tiles in flight (wave-uniform)
        if (NSTG == 2 || t <= 0) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); return; }
        if (B_PARTIAL && skip_last) {
            if (t == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NPIECE - 1) : "memory");
            else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * (NPIECE - 1)) : "memory");
        } else {
            if (t == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NPIECE) : "memory");
            else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NPIECE) : "memory");
        }
    };
    SVDX_STAGE_RING(NSTG, n_tiles,
                    {
                        _Pragma("unroll") for (int pi = 0; pi < NPIECE; ++pi) issue_piece(t, pi);
                        advance_k();
                    },
                    { SVDX_V4_COMPUTE(cur, nxt, true); advance_k(); }, SVDX_V4_COMPUTE(cur, nxt, false), wait_tiles)
#undef SVDX_V4_COMPUTE

    v4_epilogue<T, NB, MB, NT, BM4, BN3, WM4, WN3>(p, smem, acc, z, m0, n0, pid_m, pid_n, wm, wn, tid);
#endif
}

// ================================================================================================================
// variant 5 family (round 6): two-role eight-wave tiles, (32 MF) x (64 NF) x 64, ONE workgroup per CU.
//
// Why: gemm_v4_kernel runs all waves of a workgroup through the same sequence -- fragment reads, then MFMA rows -- so the two waves that
// share a SIMD's matrix pipe read LDS together and multiply together; counters (profiles/r5_stall_counters.txt) show its waves parked at
// waits / barriers 35-55 % of their cycles.  Here the eight waves are 2 (M) x 4 (N); waves 0-3 (one per SIMD) and waves 4-7 (their SIMD
// partners) run the SAME program ONE BARRIER APART: while one group is in the MFMA segment of a phase its partners are in the load
// segment of theirs (ds_read_b128 of the next fragment group + their share of the staging DMA), and they swap at every barrier -- the
// matrix pipe of each SIMD always has exactly one wave feeding it (cdna_hip_programming.md, "256^2 8-phase template").
//
// One K-tile (64) = four phases, one quadrant of the wave's (16 MF) x (16 NF) output each:
//     phase     fragments read                 MFMA quadrant      staging issued (LDS-DMA pieces of 64 rows x 128 B by all 512 threads)
//     0         A sub 0, B sub 0               (m0, n0)           A rows that hold sub 1, K-tile t+1   (last read: phase 2 of t-1)
//     1         B sub 1                        (m0, n1)           --                                    [wait A]
//     2         A sub 1                        (m1, n1)           A rows of sub 0 only + B rows that hold sub 0, K-tile t+2   (last read: phase 0 of t)
//     3         -- (B sub 0 stays in registers) (m1, n0)          B rows of sub 1 only, K-tile t+2     (last read: phase 1 of t)   [wait B]
// LDS holds TWO K-tiles; inside a tile the rows are grouped by sub-tile ([sub 0: wave row 0, wave row 1][sub 1: ...]), so that a region is
// free for K-tile t+2 as soon as its last phase of K-tile t is over.  A region is re-staged two phases after its last read (the partner
// group is one barrier behind: its reads of that phase retire one barrier interval later).  Two counted waits per K-tile, each leaving ONE
// WHOLE K-TILE of pieces in flight across the barriers: [wait B] in phase 3 retires what phases 0 and 1 of K-tile t+1 read (issued in
// phases 2 and 3 of t-1), [wait A] in phase 1 retires the sub-1 rows of A that phase 2 reads (issued in phase 0 of t-1) -- every piece
// flies for four to five phases, and the first read of a region comes a barrier after its wait (both groups), as the LDS-DMA ordering
// rule demands.  (The first cut of this kernel re-read B sub 0 in phase 3, which held its region until then: the weights' last pieces had
// two phases to land.  Isolated, L2-warm runs did not care; inside the step, where every weight tile comes from HBM, the tile lost 5-13 %
// to the two-per-CU four-wave tiles -- profiles/r6d_tune_dump.txt.)  Beyond the last K-tile the pieces are issued with an out-of-range
// offset (no memory access, zeros into a free region): every wave's vmcnt arithmetic stays the same to the end.
// Epilogues: v4_epilogue (same accumulator layout: a wave owns rows wr * 16 MF .. and columns wc * 16 NF ..).
// ================================================================================================================
template <typename T, int MF, int NF>
__global__ __launch_bounds__(512) void gemm_v5_kernel(GemmParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef typename TT<T>::v8 v8;
    constexpr int NT = 512;
    constexpr int BM5 = 32 * MF, BN5 = 64 * NF, WM5 = 16 * MF, WN5 = 16 * NF;
    constexpr int MF0 = (MF + 1) / 2, MF1 = MF - MF0, NF0 = (NF + 1) / 2, NF1 = NF - NF0;
    constexpr int A0R = 2 * MF0 * 16, B0R = 4 * NF0 * 16;          // LDS rows of sub-tile 0 of A / B (all wave rows / wave columns)
    constexpr int KT = BK, ROWB = KT * 2;
    constexpr int BUFB = (BM5 + BN5) * ROWB;                         // one K-tile: A rows, then B rows
    constexpr int PA = (BM5 + 63) / 64, PB = BN5 / 64;               // staging passes (64 LDS rows each) per operand and K-tile
    static_assert(BM5 % 32 == 0 && BN5 % 64 == 0 && 2 * BUFB <= 160 * 1024, "tile does not fit");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const int wr = wave_u >> 2, wc = wave_u & 3;
    int pid_m, pid_n, z;
    if (!v4_tile_of_block(p, pid_m, pid_n, z)) return;
    const int m0 = pid_m * p.m_step, n0 = pid_n * BN5;
    const int kt_total = p.K / KT;
    const int kt_per = (kt_total + p.split_k - 1) / p.split_k;
    const int kt_begin = z * kt_per;
    const int kt_end = min(kt_total, kt_begin + kt_per);
    if (kt_begin >= kt_end) return;
    const int n_tiles = kt_end - kt_begin;

    // ---- staging addresses: pass i moves LDS rows 64 i + tid / 8, 16-byte chunk tid % 8 (XOR-swizzled by the row, as in gemm_v4_kernel)
    const int ld_row = tid >> 3, pc = tid & 7;
    const int lc = pc ^ (ld_row & 7);
    RowInfo a_ri[PA];
    int a_m[PA], voa[PA], vob[PB];
    constexpr int OOB = (int)0x80000000;
#pragma unroll
    for (int i = 0; i < PA; ++i) {
        const int r = 64 * i + ld_row;                                // LDS row -> row of the tile
        const int s = r >= A0R, q = s ? r - A0R : r, per = (s ? MF1 : MF0) * 16;
        const int tr = (q / per) * WM5 + (s ? MF0 * 16 : 0) + q % per;
        a_m[i] = min(m0 + tr, p.M - 1);
        a_ri[i] = decode_row(p.g, a_m[i]);
    }
#pragma unroll
    for (int i = 0; i < PB; ++i) {
        const int r = 64 * i + ld_row;
        const int s = r >= B0R, q = s ? r - B0R : r, per = (s ? NF1 : NF0) * 16;
        const int nl = (q / per) * WN5 + (s ? NF0 * 16 : 0) + q % per;
        vob[i] = (v4_brow<BN5>(p, pid_n, n0, nl) * p.ldb + lc * 8) * 2;
    }
    const bool plain = p.g.mode == SVDX_GATHER_PLAIN;
    const int cin = plain ? p.K : p.g.cin;
    const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.A), 0, p.a_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.B), 0, p.b_bytes, 0x00020000);
    // the A cursor (K-tile a_t: filter tap + channel offset inside it) and the B cursor (K-tile b_t) advance independently: an operand's
    // pieces are issued in K-tile order, but A's and B's pieces of one K-tile are two phases apart
    int a_t = 0, b_t = 0;
    int tap = plain ? 0 : (kt_begin * KT) / cin;
    int ci0 = kt_begin * KT - tap * cin;
    int kb = kt_begin * KT * 2;                                      // byte offset of B's K-tile
    auto set_tap = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < PA; ++i) {
            bool valid;
            const T* ptr = a_row_ptr<T>(p, a_ri[i], a_m[i], 0, tap, 0, valid);
            voa[i] = valid ? (int)((ptr - reinterpret_cast<const T*>(p.A)) + lc * 8) * 2 : OOB;
        }
    };
    set_tap();
    auto advance_a = [&]() __attribute__((always_inline)) {
        ++a_t;
        ci0 += KT;
        if (a_t >= n_tiles) {
#pragma unroll
            for (int i = 0; i < PA; ++i) voa[i] = OOB;
        } else if (!plain && ci0 == cin) { ci0 = 0; ++tap; set_tap(); }
    };
    auto advance_b = [&]() __attribute__((always_inline)) {
        ++b_t;
        kb += KT * 2;
        if (b_t >= n_tiles) {
#pragma unroll
            for (int i = 0; i < PB; ++i) vob[i] = OOB;
        }
    };
    // pieces of one slot.  SLOT 0: A passes that touch sub 1; 2: A passes inside sub 0 and B passes that touch sub 0; 3: B passes inside sub 1.
    // An A pass whose rows lie beyond the tile for this wave (160-row tiles: pass 2, waves 4-7) is skipped: that wave's counts are one lower.
#define SVDX_V5_ISSUE(SLOT, buf)                                                                                                            \
    {                                                                                                                                       \
        char* base_ = smem + (buf) * BUFB + wave_u * 1024;                                                                                  \
        if ((SLOT) == 0 || (SLOT) == 2) {                                                                                                   \
            _Pragma("unroll") for (int i = 0; i < PA; ++i) {          /* ascending: a pass that straddles sub 0 / sub 1 leads slot 0 */       \
                const bool in0 = 64 * i + 64 <= A0R;                                                                                        \
                if (((SLOT) == 2) != in0) continue;                                                                                         \
                if (64 * i + 64 > BM5 && 64 * i + wave_u * 8 >= BM5) continue;                                                              \
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (__attribute__((address_space(3))) void*)(base_ + i * 8192), 16, voa[i],      \
                                                         ci0 * 2, 0, 0);                                                                    \
            }                                                                                                                               \
        }                                                                                                                                   \
        if ((SLOT) == 2 || (SLOT) == 3) {                                                                                                   \
            _Pragma("unroll") for (int i = 0; i < PB; ++i) {                                                                                \
                const bool in1 = 64 * i >= B0R;                                                                                             \
                if (((SLOT) == 3) != in1) continue;                                                                                         \
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (__attribute__((address_space(3))) void*)(base_ + BM5 * ROWB + i * 8192), 16, \
                                                         vob[i], kb, 0, 0);                                                                 \
            }                                                                                                                               \
        }                                                                                                                                   \
    }
    // [wait A] leaves one K-tile's worth of this wave's pieces in flight.  [wait B] must also retire the A pass that straddles the two
    // sub-tiles (160-row tiles: rows 64-127 of 96 + 64) -- it holds sub-0 rows that phase 0 reads, but could only be issued with the sub-1
    // group in phase 0; it is the OLDEST piece of that group (ascending pass order), so [wait B] simply leaves one piece fewer in flight.
    static_assert(B0R % 64 == 0, "a B pass must not straddle the sub-tiles (it would be restaged one phase after its sub-1 rows were read)");
    constexpr int N_STRADDLE = (A0R % 64) ? 1 : 0;
    constexpr bool A_PARTIAL = 64 * PA > BM5;
    const bool skips_one = A_PARTIAL && 64 * (PA - 1) + wave_u * 8 >= BM5;
#define SVDX_V5_WAIT(LESS)                                                                                                                  \
    {                                                                                                                                       \
        if (A_PARTIAL && skips_one) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PA + PB - 1 - (LESS)) : "memory");                             \
        else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PA + PB - (LESS)) : "memory");                                                        \
    }

    f32x4 acc[NF][MF];                                                // [n-block][m-block], transposed like gemm_v4_kernel's
#pragma unroll
    for (int i = 0; i < NF; ++i)
#pragma unroll
        for (int j = 0; j < MF; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int fr = lane & 15, fg = lane >> 4;
    const int frag0 = fr * ROWB + ((fg ^ (fr & 7)) * 16), frag1 = fr * ROWB + (((4 + fg) ^ (fr & 7)) * 16);     // k-halves 0 / 1 of a fragment row
    const int a_lds0 = wr * (MF0 * 16) * ROWB, a_lds1 = (A0R + wr * (MF1 * 16)) * ROWB;
    const int b_lds0 = (BM5 + wc * (NF0 * 16)) * ROWB, b_lds1 = (BM5 + B0R + wc * (NF1 * 16)) * ROWB;
    v8 a0f[MF0][2], a1f[MF1 > 0 ? MF1 : 1][2], b0f[NF0][2], b1f[NF1 > 0 ? NF1 : 1][2];
#define SVDX_V5_READ(dst, n, ldsoff, buf)                                                                                                   \
    _Pragma("unroll") for (int i_ = 0; i_ < (n); ++i_) {                                                                                    \
        dst[i_][0] = *reinterpret_cast<const v8*>(smem + (buf) * BUFB + (ldsoff) + i_ * 16 * ROWB + frag0);                                 \
        dst[i_][1] = *reinterpret_cast<const v8*>(smem + (buf) * BUFB + (ldsoff) + i_ * 16 * ROWB + frag1);                                 \
    }
#define SVDX_V5_MMA(bf_, nb_, ioff, af_, mb_, joff)                                                                                         \
    {                                                                                                                                       \
        __builtin_amdgcn_s_setprio(1);                                                                                                      \
        _Pragma("unroll") for (int kk_ = 0; kk_ < 2; ++kk_)                                                                                 \
            _Pragma("unroll") for (int i_ = 0; i_ < (nb_); ++i_)                                                                           \
                _Pragma("unroll") for (int j_ = 0; j_ < (mb_); ++j_)                                                                       \
                    acc[(ioff) + i_][(joff) + j_] = TT<T>::mfma(bf_[i_][kk_], af_[j_][kk_], acc[(ioff) + i_][(joff) + j_]);                 \
        __builtin_amdgcn_s_setprio(0);                                                                                                      \
    }
#define SVDX_V5_BARRIER()                                                                                                                   \
    {                                                                                                                                       \
        __builtin_amdgcn_sched_barrier(0);                                                                                                  \
        __builtin_amdgcn_s_barrier();                                                                                                       \
        asm volatile("" ::: "memory");                                                                                                      \
        __builtin_amdgcn_sched_barrier(0);                                                                                                  \
    }
    // one K-tile out of buffer `buf`; its slot-0 pieces go to the other buffer (K-tile t+1), slots 2 / 3 into this one (K-tile t+2)
#define SVDX_V5_TILE(buf)                                                                                                                   \
    {                                                                                                                                       \
        SVDX_V5_READ(b0f, NF0, b_lds0, buf);                                                                                                \
        __builtin_amdgcn_sched_barrier(0);                                                                                                  \
        SVDX_V5_READ(a0f, MF0, a_lds0, buf);                                                                                                \
        __builtin_amdgcn_sched_barrier(0);                                                                                                  \
        SVDX_V5_ISSUE(0, (buf) ^ 1);                                                                                                        \
        advance_a();                                                                                                                        \
        SVDX_V5_BARRIER();                                                                                                                  \
        SVDX_V5_MMA(b0f, NF0, 0, a0f, MF0, 0);                                                                                              \
        SVDX_V5_BARRIER();                                                                                                                  \
        if (NF1 > 0) {                                                                                                                      \
            SVDX_V5_READ(b1f, NF1, b_lds1, buf);                                                                                            \
            __builtin_amdgcn_sched_barrier(0);                                                                                              \
        }                                                                                                                                   \
        SVDX_V5_WAIT(0);                                                                                                                    \
        SVDX_V5_BARRIER();                                                                                                                  \
        if (NF1 > 0) SVDX_V5_MMA(b1f, NF1, NF0, a0f, MF0, 0);                                                                               \
        SVDX_V5_BARRIER();                                                                                                                  \
        if (MF1 > 0) {                                                                                                                      \
            SVDX_V5_READ(a1f, MF1, a_lds1, buf);                                                                                            \
            __builtin_amdgcn_sched_barrier(0);                                                                                              \
        }                                                                                                                                   \
        SVDX_V5_ISSUE(2, buf);                                                                                                              \
        SVDX_V5_BARRIER();                                                                                                                  \
        if (MF1 > 0 && NF1 > 0) SVDX_V5_MMA(b1f, NF1, NF0, a1f, MF1, MF0);                                                                  \
        SVDX_V5_BARRIER();                                                                                                                  \
        SVDX_V5_ISSUE(3, buf);                                                                                                              \
        advance_b();                                                                                                                        \
        SVDX_V5_WAIT(N_STRADDLE);                                                                                                                   \
        SVDX_V5_BARRIER();                                                                                                                  \
        if (MF1 > 0) SVDX_V5_MMA(b0f, NF0, 0, a1f, MF1, MF0);                                                                               \
        SVDX_V5_BARRIER();                                                                                                                  \
    }
    // ---- prologue: what the steady state would have issued before K-tile 0 (phases 2, 3 of "tile -2"; 0, 2, 3 of "tile -1") ----
    SVDX_V5_ISSUE(2, 0);
    SVDX_V5_ISSUE(3, 0);
    advance_b();
    SVDX_V5_ISSUE(0, 0);
    advance_a();
    SVDX_V5_ISSUE(2, 1);
    SVDX_V5_ISSUE(3, 1);
    advance_b();
    SVDX_V5_WAIT(N_STRADDLE);
    SVDX_V5_BARRIER();
    if (wr == 1) SVDX_V5_BARRIER();                                  // waves 4-7 run one barrier behind their SIMD partners from here on
    for (int t = 0; t < n_tiles; t += 2) {
        SVDX_V5_TILE(0);
        if (t + 1 < n_tiles) SVDX_V5_TILE(1);
    }
    if (wr == 0) SVDX_V5_BARRIER();                                  // ... and meet them again
#undef SVDX_V5_TILE
#undef SVDX_V5_WAIT
#undef SVDX_V5_BARRIER
#undef SVDX_V5_MMA
#undef SVDX_V5_READ
#undef SVDX_V5_ISSUE
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");               // the out-of-range tail pieces: the epilogue parks its tile in these buffers
    __syncthreads();
    v4_epilogue<T, NF, MF, NT, BM5, BN5, WM5, WN5>(p, smem, acc, z, m0, n0, pid_m, pid_n, wr, wc, tid);
#endif
}

template <typename T>
int launch_gemm(const GemmParams& p, hipStream_t st) {
    [[maybe_unused]] static const bool lds_ok = allow_lds(&gemm_kernel<T>, 2 * STAGE_BYTES);
    dim3 grid(p.tiles_m * p.tiles_n, p.split_k);
    hipLaunchKernelGGL((gemm_kernel<T>), grid, dim3(NTHREADS), 2 * STAGE_BYTES, st, p);
    SVDX_LAUNCH_CHECK("svdx_gemm");
    return 0;
}

// Tile counts, vector-store eligibility and the XCD arrangement of a BMT x BNT tile grid (see v4_tile_of_block): the arrangement with the
// least operand re-fetch among those that keep >= 90 % of the best tile balance; -> the launch grid.  Shared by the v4 and v5 launchers.
static int arrange_nt_grid(GemmParams& p, int BMT, int BNT, dim3& grid, int rows_computed = 0) {      // BMT: rows a tile owns; rows_computed: its height when larger
    if (p.gn_stats) {
        // the statistics are taken in the coalesced store loop, which handles whole column tiles of 16-byte-aligned rows only
        const bool ok = p.N % BNT == 0 && p.ldc % 8 == 0 && ((uintptr_t)p.C & 15) == 0 && (!p.res || (p.ldres % 8 == 0 && ((uintptr_t)p.res & 15) == 0)) &&
                        ((rows_computed ? rows_computed : BMT) - 1) / p.gn_rows + 2 <= GN_MAX_S && (BNT - 1) / p.gn_cg + 2 <= GN_MAX_G;
        if (!ok) { svdx_set_error("svdx_gemm_gn: N=%d / ldc=%d / rows=%d / cg=%d do not fit the %dx%d tile's statistics path", p.N, p.ldc, p.gn_rows, p.gn_cg, BMT, BNT); return -2; }
    }
    p.tiles_m = cdiv(p.M, BMT);
    p.tiles_n = p.epi == SVDX_EPI_GEGLU_FWD ? cdiv(p.aux_dim, BNT / 2) : cdiv(p.N, BNT);
    p.vec_ok = (p.ldc % 4 == 0) && (((uintptr_t)p.C & 15) == 0) && (!p.res || (p.ldres % 4 == 0 && ((uintptr_t)p.res & 15) == 0));
    const double a_bytes = 2.0 * p.M * (p.g.mode == SVDX_GATHER_PLAIN ? p.K : 2 * p.g.cin);   // conv: unique rows + halo
    const double b_bytes = 2.0 * (p.epi == SVDX_EPI_GEGLU_FWD ? 2 * p.aux_dim : p.N) * p.K;
    double best_cost, zb_cost;
    const int best_xn = xcd_arrangement(p.tiles_m, p.tiles_n, 8, a_bytes, b_bytes, best_cost);
    p.xcd_n = best_xn;
    p.z_xcd = 0;
    int gx = p.tiles_m * p.tiles_n, gy = p.split_k;
    if (best_xn > 0) {
        p.sub_m = cdiv(p.tiles_m, 8 / best_xn);
        p.sub_n = cdiv(p.tiles_n, best_xn);
        gx = 8 * p.sub_m * p.sub_n;
    }
    // K slices on XCDs of their own (see v4_tile_of_block): among the arrangements of the 8 / split_k XCDs of a slice, the least re-fetch that keeps
    // >= 90 % of the best balance; taken when it fetches less than the slice-agnostic arrangement and leaves no more workgroup slots empty
    if (best_xn > 0 && (p.split_k == 2 || p.split_k == 4 || p.split_k == 8)) {
        const int xps = 8 / p.split_k, zb_xn = xcd_arrangement(p.tiles_m, p.tiles_n, xps, a_bytes, b_bytes, zb_cost);
        const int zsm = cdiv(p.tiles_m, xps / zb_xn), zsn = cdiv(p.tiles_n, zb_xn);
        if (zb_cost < best_cost && zsm * zsn <= p.sub_m * p.sub_n * p.split_k) {
            p.z_xcd = 1; p.xcd_n = zb_xn; p.sub_m = zsm; p.sub_n = zsn;
            gx = 8 * zsm * zsn; gy = 1;
        }
    }
    grid = dim3(gx, gy);
    return 0;
}

template <typename T, int NB, int MB, int WGM = 2, int NSTG = 2, int MSTEP = 0>
int launch_gemm_v4(GemmParams p, hipStream_t st) {
    constexpr int BMT = 16 * MB * WGM, BNT = 32 * NB;
    constexpr int STEP = MSTEP ? MSTEP : BMT;                    // rows a tile owns (variant 36: 140 of its 144)
    static_assert(STEP <= BMT && STEP > 0, "a tile cannot own more rows than it computes");
    constexpr int LDS_STG = NSTG * (BMT + BNT) * BK * 2, LDS_EPI = ((BMT * (BNT + 8) * 2 + 15) & ~15) + GN_LDS;      // K-loop stages | the rounded output tile parked for the coalesced stores (+ the GroupNorm statistics table behind it)
    constexpr int LDS = LDS_STG > LDS_EPI ? LDS_STG : LDS_EPI;
    static_assert(LDS <= 160 * 1024, "stages (and the epilogue tile parked in them) must fit the 160 KiB LDS");
    constexpr bool HAS_DUAL = WGM == 2 && NSTG == 2;            // the LoRA second-operand loop is only instantiated for the round-1 tiles (gemm_entry refuses K2 > 0 on the others)
    [[maybe_unused]] static const bool lds_ok = allow_lds(&gemm_v4_kernel<T, NB, MB, false, WGM, NSTG>, LDS) && (!HAS_DUAL || allow_lds(&gemm_v4_kernel<T, NB, MB, HAS_DUAL, WGM, NSTG>, LDS));
    dim3 grid;
    p.m_step = STEP;
    if (int rc = arrange_nt_grid(p, STEP, BNT, grid, BMT)) return rc;
    if (p.K2 > 0) hipLaunchKernelGGL((gemm_v4_kernel<T, NB, MB, HAS_DUAL, WGM, NSTG>), grid, dim3(128 * WGM), LDS, st, p);
    else hipLaunchKernelGGL((gemm_v4_kernel<T, NB, MB, false, WGM, NSTG>), grid, dim3(128 * WGM), LDS, st, p);
    SVDX_LAUNCH_CHECK("svdx_gemm");
    return 0;
}

// the two-role eight-wave tiles (gemm_v5_kernel): (32 MF) x (64 NF), two K-tiles of LDS
template <typename T, int MF, int NF>
int launch_gemm_v5(GemmParams p, hipStream_t st) {
    constexpr int BMT = 32 * MF, BNT = 64 * NF;
    constexpr int LDS_STG = 2 * (BMT + BNT) * BK * 2, LDS_EPI = ((BMT * (BNT + 8) * 2 + 15) & ~15) + GN_LDS;
    constexpr int LDS = LDS_STG > LDS_EPI ? LDS_STG : LDS_EPI;
    static_assert(LDS <= 160 * 1024, "K-tiles (and the epilogue tile parked in them) must fit the 160 KiB LDS");
    [[maybe_unused]] static const bool lds_ok = allow_lds(&gemm_v5_kernel<T, MF, NF>, LDS);
    dim3 grid;
    p.m_step = BMT;
    if (int rc = arrange_nt_grid(p, BMT, BNT, grid)) return rc;
    hipLaunchKernelGGL((gemm_v5_kernel<T, MF, NF>), grid, dim3(512), LDS, st, p);
    SVDX_LAUNCH_CHECK("svdx_gemm");
    return 0;
}

}  // namespace

extern "C" int svdx_gemm_tile(int variant, int M, int N, int split_k, int epilogue, int aux_dim, int* geom) {
    const int id = resolve_tile(variant, M, N, split_k, epilogue, aux_dim);
    const GemmTile* t = gemm_tile(id);
    if (geom && t) {
        geom[0] = t->row_step; geom[1] = t->rows; geom[2] = t->cols; geom[3] = t->stages; geom[4] = t->waves; geom[5] = t->has_dual;
    }
    return id;
}

// the launch of one row of SVDX_GEMM_TILES, as a case of gemm_entry's switch over the resolved tile
#define SVDX_LAUNCH_V4(id, sib, NB, MB, WGM, NSTG, MSTEP) case id: return launch_gemm_v4<T, NB, MB, WGM, NSTG, MSTEP>(p, st);
#define SVDX_LAUNCH_V5(id, sib, MF, NF) case id: return launch_gemm_v5<T, MF, NF>(p, st);

static int gemm_entry(const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc,
                      const float* bias, const float* rowvec, int rv_ld, int rv_rows_per_group, int rv_mod,
                      const void* res, int ldres, const svdx_gather* gather, const void* zero_page,
                      int out_mode, float alpha, int split_k, int variant, int epilogue, const void* aux_in, void* aux_out,
                      int aux_dim, const void* A2, const void* B2, int K2, int lda2, int ldb2, int a2_seg, float* gn_stats, int gn_rows,
                      int gn_cg, int dtype, void* stream) {
    SVDX_CHECK_ARG(A && B && C, "svdx_gemm: null operand");
    const int tile_id = resolve_tile(variant, M, N, split_k, epilogue, aux_dim);
    const GemmTile* tile = gemm_tile(tile_id);                   // null: the 64-bit-pointer kernel (variants 0 / 1) or an unknown variant
    if (gn_stats) {
        SVDX_CHECK_ARG(variant >= 2 && out_mode == SVDX_OUT_ACT && split_k == 1 && epilogue == SVDX_EPI_NONE && K2 <= 0,
                       "svdx_gemm_gn: statistics ride on an unsplit variant-4 launch with activation output and no fused epilogue");
        SVDX_CHECK_ARG(gn_rows > 0 && gn_cg > 0 && M % gn_rows == 0 && N % gn_cg == 0 && ((uintptr_t)gn_stats & 7) == 0,
                       "svdx_gemm_gn: M=%d must be whole samples of %d rows, N=%d whole groups of %d channels", M, gn_rows, N, gn_cg);
    }
    if (K2 > 0) {
        SVDX_CHECK_ARG(A2 && B2 && K2 % BK == 0 && lda2 % 8 == 0 && ldb2 % 8 == 0 && lda2 >= K2 && ldb2 >= K2 &&
                           (((uintptr_t)A2 | (uintptr_t)B2) & 15) == 0, "svdx_gemm_dual: second operand pair misaligned (K2=%d)", K2);
        SVDX_CHECK_ARG(variant >= 2 && split_k == 1, "svdx_gemm_dual: needs variant 4 and split_k == 1");
        SVDX_CHECK_ARG(!tile || tile->has_dual, "svdx_gemm_dual: this tile variant has no second-operand loop");
        SVDX_CHECK_ARG(!tile || a2_seg == 0 || (a2_seg > 0 && N % a2_seg == 0 && a2_seg % tile->cols == 0 && lda2 >= (N / a2_seg) * K2),
                       "svdx_gemm_dual: a2_seg_n=%d must divide N=%d, be a multiple of the %d-column tile, and fit lda2", a2_seg, N, tile ? tile->cols : 0);
    }
    if (epilogue != SVDX_EPI_NONE) {
        SVDX_CHECK_ARG(variant >= 2 && out_mode == SVDX_OUT_ACT && split_k == 1 && !res && !rowvec && aux_dim > 0 && aux_dim % 64 == 0 &&
                           (!gather || gather->mode == SVDX_GATHER_PLAIN), "svdx_gemm: fused GEGLU epilogue needs variant 4, plain A, no split-K");
        SVDX_CHECK_ARG(((uintptr_t)C & 15) == 0, "svdx_gemm: fused epilogue output must be 16-byte aligned");
        if (epilogue == SVDX_EPI_GEGLU_FWD)
            SVDX_CHECK_ARG(N == 2 * aux_dim && ldc == N && aux_out && ((uintptr_t)aux_out & 15) == 0, "svdx_gemm: GEGLU fwd wants C=[M,2F], aux_out=[M,F]");
        else
            SVDX_CHECK_ARG(epilogue == SVDX_EPI_GEGLU_BWD && N == aux_dim && ldc == 2 * aux_dim && aux_in && ((uintptr_t)aux_in & 15) == 0 &&
                               (N % 160 == 0 || N % 128 == 0), "svdx_gemm: GEGLU bwd wants N=F (multiple of 128 or 160), C=dpre [M,2F], aux_in=pre [M,2F]");
    }
    SVDX_CHECK_ARG(M > 0 && N > 0 && K > 0, "svdx_gemm: bad sizes M=%d N=%d K=%d", M, N, K);
    SVDX_CHECK_ARG(K % BK == 0, "svdx_gemm: K=%d must be a multiple of %d", K, BK);
    SVDX_CHECK_ARG(ldb % 8 == 0 && ((uintptr_t)B & 15) == 0, "svdx_gemm: B must be 16-byte aligned (ldb=%d)", ldb);
    SVDX_CHECK_ARG(split_k >= 1 && (split_k == 1 || out_mode == SVDX_OUT_F32_ATOMIC || out_mode == SVDX_OUT_F32_SLAB),
                   "svdx_gemm: split_k=%d needs atomic or slab output", split_k);
    SVDX_CHECK_ARG(!rowvec || rv_mod > 0 || rv_rows_per_group > 0, "svdx_gemm: rowvec needs a grouping");
    // a slice without K-tiles would leave its slab unwritten (found by tests/sim/fuzz.py with NaN-filled slabs; ops.choose_cfg never asks for one)
    SVDX_CHECK_ARG(out_mode != SVDX_OUT_F32_SLAB || (split_k - 1) * cdiv(K / BK, split_k) < K / BK,
                   "svdx_gemm: split_k=%d leaves slices without K-tiles (K=%d): their slabs would stay unwritten", split_k, K);
    GemmParams p{};                   // whatever a path below leaves alone is zero / null in the kernel arguments (and in a recorded launch plan)
    p.A = A; p.B = B; p.C = C; p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldb = ldb; p.ldc = ldc;
    p.bias = bias; p.rowvec = rowvec; p.rv_ld = rv_ld; p.rv_rpg = rv_rows_per_group; p.rv_mod = rv_mod;
    p.res = res; p.ldres = ldres; p.zero_page = zero_page;
    p.out_mode = out_mode; p.alpha = alpha; p.split_k = split_k; p.slab_stride = (long)M * ldc;
    p.epi = epilogue; p.aux_in = aux_in; p.aux_out = aux_out; p.aux_dim = aux_dim;
    p.A2 = A2; p.B2 = B2; p.K2 = K2 > 0 ? K2 : 0; p.lda2 = lda2; p.ldb2 = ldb2; p.a2_seg = K2 > 0 ? a2_seg : 0;
    p.gn_stats = reinterpret_cast<unsigned long long*>(gn_stats); p.gn_rows = gn_rows; p.gn_cg = gn_cg;
    if (gn_stats) {
        int k0, k1;
        gn_fixed_scales((long)gn_rows * gn_cg, 0, k0, k1);
        p.gn_m0 = exp2f((float)k0); p.gn_m1 = exp2f((float)k1);
    }
    if (gather && gather->mode != SVDX_GATHER_PLAIN) {
        p.g = *gather;
        SVDX_CHECK_ARG(p.g.cin % BK == 0, "svdx_gemm: gather cin=%d must be a multiple of %d", p.g.cin, BK);
        SVDX_CHECK_ARG(p.g.lda % 8 == 0 && ((uintptr_t)A & 15) == 0, "svdx_gemm: gather source misaligned");
        SVDX_CHECK_ARG(zero_page && ((uintptr_t)zero_page & 15) == 0, "svdx_gemm: gather needs an aligned zero page");
        const int taps = p.g.mode == SVDX_GATHER_TEMPORAL3 ? 3 : 9;
        SVDX_CHECK_ARG(K == taps * p.g.cin, "svdx_gemm: K=%d != taps*cin=%d", K, taps * p.g.cin);
        if (p.g.mode == SVDX_GATHER_CONV3X3 || p.g.mode == SVDX_GATHER_CONV3X3_PAD0) {
            SVDX_CHECK_ARG(M == p.g.n_img * p.g.ho * p.g.wo, "svdx_gemm: conv rows mismatch");
            SVDX_CHECK_ARG(p.g.mode == SVDX_GATHER_CONV3X3 || (p.g.stride == 2 && !p.g.ups), "svdx_gemm: the pad-0 gather is the stride-2 downsample");
            SVDX_CHECK_ARG(p.g.stride == 1 || p.g.stride == 2, "svdx_gemm: conv stride");
            SVDX_CHECK_ARG(!p.g.ups || (p.g.hi % 2 == 0 && p.g.wi % 2 == 0), "svdx_gemm: upsampled dims must be even");
        } else if (p.g.mode == SVDX_GATHER_CONV3X3_DGRAD2) {
            SVDX_CHECK_ARG(M == p.g.n_img * p.g.ho * p.g.wo, "svdx_gemm: dgrad rows mismatch");
        } else if (p.g.mode == SVDX_GATHER_TEMPORAL3) {
            SVDX_CHECK_ARG(M == p.g.n_img * p.g.t * p.g.hw, "svdx_gemm: temporal rows mismatch");
        } else {
            svdx_set_error("svdx_gemm: unknown gather mode %d", p.g.mode);
            return -2;
        }
    } else {
        p.g = svdx_gather{};
        p.g.mode = SVDX_GATHER_PLAIN;
        SVDX_CHECK_ARG(lda % 8 == 0 && ((uintptr_t)A & 15) == 0, "svdx_gemm: A must be 16-byte aligned (lda=%d)", lda);
    }
    p.tiles_m = cdiv(M, BM);
    p.tiles_n = cdiv(N, BN);
    const int esz = out_mode == SVDX_OUT_ACT ? 2 : 4;
    p.vec_ok = (ldc % 8 == 0) && (((uintptr_t)C % (esz == 2 ? 16 : 4)) == 0) &&
               (!res || (ldres % 8 == 0 && ((uintptr_t)res & 15) == 0));
    hipStream_t st = (hipStream_t)stream;
    // extents of the A / B buffers for the bounds-checked buffer loads of variant 4 (must stay below 2 GiB)
    long a_rows = M;
    if (p.g.mode == SVDX_GATHER_CONV3X3 || p.g.mode == SVDX_GATHER_CONV3X3_PAD0) a_rows = (long)p.g.n_img * (p.g.hi >> p.g.ups) * (p.g.wi >> p.g.ups);
    else if (p.g.mode == SVDX_GATHER_CONV3X3_DGRAD2) a_rows = (long)p.g.n_img * p.g.hi * p.g.wi;
    else if (p.g.mode == SVDX_GATHER_TEMPORAL3) a_rows = (long)p.g.n_img * p.g.t * p.g.hw;
    const int a_ld = p.g.mode == SVDX_GATHER_PLAIN ? lda : p.g.lda;
    const int a_w = p.g.mode == SVDX_GATHER_PLAIN ? K : p.g.cin;
    long a_bytes = ((a_rows - 1) * a_ld + a_w) * 2, b_bytes = ((long)(N - 1) * ldb + K) * 2;
    if (a_bytes >= (1L << 31) || b_bytes >= (1L << 31)) { a_bytes = 0; b_bytes = 0; }   // falls back to variant 1 (64-bit pointers)
    if (p.K2 > 0) {
        const long b_rows = epilogue == SVDX_EPI_GEGLU_FWD ? 2L * aux_dim : N;
        const long a2 = ((long)(M - 1) * lda2 + (long)(a2_seg > 0 ? N / a2_seg : 1) * K2) * 2, b2 = ((b_rows - 1) * ldb2 + K2) * 2;
        if (a_bytes == 0 || a2 >= (1L << 31) || b2 >= (1L << 31)) { svdx_set_error("svdx_gemm_dual: operands too large for the buffer-addressed kernel"); return -2; }
        p.a2_bytes = (int)a2; p.b2_bytes = (int)b2;
    }
    DISPATCH_DTYPE(dtype, {
        if (variant >= 2 && a_bytes > 0 && b_bytes > 0) {
            p.a_bytes = (int)a_bytes; p.b_bytes = (int)b_bytes;
            if (!tile) { svdx_set_error("svdx_gemm: unknown variant %d", variant); return -2; }
            // the GEGLU-backward epilogue only exists in the coalesced store path, which takes whole column tiles: d(pre) of a partial last
            // tile would be written as plain d(h) (found by tests/sim/fuzz.py; F = 4C of the UNet is always a multiple of 128)
            SVDX_CHECK_ARG(epilogue != SVDX_EPI_GEGLU_BWD || N % tile->cols == 0,
                           "svdx_gemm: GEGLU bwd with tile variant %d needs N=%d to be a multiple of its %d-column tile", variant, N, tile->cols);
            switch (tile_id) { SVDX_GEMM_TILES(SVDX_LAUNCH_V4, SVDX_LAUNCH_V5) }
        }
        if (epilogue != SVDX_EPI_NONE) { svdx_set_error("svdx_gemm: fused epilogue unavailable (buffer too large for variant 4)"); return -2; }
        if (gn_stats) { svdx_set_error("svdx_gemm_gn: statistics unavailable (buffer too large for variant 4)"); return -2; }
        return launch_gemm<T>(p, st);
    });
}

extern "C" int svdx_gemm(const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc,
                         const float* bias, const float* rowvec, int rv_ld, int rv_rows_per_group, int rv_mod,
                         const void* res, int ldres, const svdx_gather* gather, const void* zero_page,
                         int out_mode, float alpha, int split_k, int variant, int epilogue, const void* aux_in, void* aux_out,
                         int aux_dim, int dtype, void* stream) {
    return gemm_entry(A, B, C, M, N, K, lda, ldb, ldc, bias, rowvec, rv_ld, rv_rows_per_group, rv_mod, res, ldres, gather, zero_page,
                      out_mode, alpha, split_k, variant, epilogue, aux_in, aux_out, aux_dim, nullptr, nullptr, 0, 0, 0, 0, nullptr, 0, 0, dtype, stream);
}

extern "C" int svdx_gemm_gn(const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc,
                            const float* bias, const float* rowvec, int rv_ld, int rv_rows_per_group, int rv_mod,
                            const void* res, int ldres, const svdx_gather* gather, const void* zero_page,
                            float alpha, int variant, float* gn_stats, int gn_rows, int gn_cg, int dtype, void* stream) {
    SVDX_CHECK_ARG(gn_stats, "svdx_gemm_gn: gn_stats must not be NULL");
    return gemm_entry(A, B, C, M, N, K, lda, ldb, ldc, bias, rowvec, rv_ld, rv_rows_per_group, rv_mod, res, ldres, gather, zero_page,
                      SVDX_OUT_ACT, alpha, 1, variant, SVDX_EPI_NONE, nullptr, nullptr, 0, nullptr, nullptr, 0, 0, 0, 0, gn_stats, gn_rows, gn_cg, dtype, stream);
}

extern "C" int svdx_gemm_dual(const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc,
                              const float* bias, const float* rowvec, int rv_ld, int rv_rows_per_group, int rv_mod,
                              const void* res, int ldres, const svdx_gather* gather, const void* zero_page,
                              int out_mode, float alpha, int variant, const void* A2, const void* B2, int K2, int lda2, int ldb2,
                              int a2_seg_n, int dtype, void* stream) {
    SVDX_CHECK_ARG(K2 > 0, "svdx_gemm_dual: K2 must be positive");
    return gemm_entry(A, B, C, M, N, K, lda, ldb, ldc, bias, rowvec, rv_ld, rv_rows_per_group, rv_mod, res, ldres, gather, zero_page,
                      out_mode, alpha, 1, variant, SVDX_EPI_NONE, nullptr, nullptr, 0, A2, B2, K2, lda2, ldb2, a2_seg_n, nullptr, 0, 0, dtype, stream);
}
