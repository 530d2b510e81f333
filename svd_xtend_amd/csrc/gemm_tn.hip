// gemm_tn.hip -- the TN weight-gradient kernels (svdx_gemm_tn).
//
// ================================================================================================================
// TN form for weight gradients:  C[n,k] (+)= sum_r A[r,n] * B[r,k]   (A = dY [R, lda], B = X [R, ldb]; float output)
// Both operands are stored with the reduction index r as the ROW, so tiles are staged row-major ([64 r][128 cols],
// 256-byte rows, coalesced 16-byte loads along the columns) and the MFMA fragments -- 8 consecutive r for one column --
// are fetched with ds_read_b64_tr_b16, gfx950's transposing LDS read: within a 16-lane group lane i supplies the
// address of row (i>>2), column piece (i&3)*4, and receives column i of the 4x16 block (probed on hardware, see
// tools/probes/tr_probe.hip).  No transposed copies of dY / X are ever materialised and every output element has
// one owner, so no atomics either.  8-byte units of a row are XOR-swizzled with a 3-bit row id so the 32 lanes of
// a half-wave hit 32 distinct bank pairs.
// ================================================================================================================
#include "gemm_common.h"

namespace {

// ---- LDS-DMA that the compiler does not see (the TN kernels, round 5) ----------------------------------------------------------------------
// hipcc (ROCm 7.2) orders every ds_read_b64_tr_b16 INTRINSIC behind all pending LDS-DMA with an `s_waitcnt vmcnt(0)` -- for the plain
// ds_read_b128 of gemm_v4_kernel it proves the stage being read distinct from the stage being filled, for the intrinsic it has no alias
// information -- so in every TN kernel of rounds 1-4 the next tile's loads and this tile's MFMAs ran strictly one after the other
// (profiles/r5_tn_isa_waits.txt: the wait sits between the staging pieces and the first fragment read of every K-step; standalone counters:
// waves parked 57-63 % of their cycles, MFMA busy 0.18 in the step).  Issued from an `asm` statement the DMA is invisible to that pass; the
// kernels count their vmcnt themselves (they always did: counted waits + s_barrier).  No VGPR destination, so nothing for the register
// allocator to mis-track (cdna_hip_programming.md 5.7); M0 -- the LDS base of the instruction -- is saved and restored inside the statement.
typedef int desc4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ desc4 hidden_desc(const void* p, unsigned bytes) {      // raw buffer descriptor: base, stride 0, num_records, gfx950 flags
    const unsigned long a = (unsigned long)p;
    return desc4{(int)(unsigned)a, (int)((unsigned)(a >> 32) & 0xffffu), (int)bytes, 0x00020000};
}
template <int SIZE, bool STREAM = false>
__device__ __forceinline__ void hidden_dma(desc4 d, char* lds, unsigned voff) {     // lane l: SIZE bytes from d.base + voff -> lds + l * SIZE (0 beyond num_records)
    static_assert(SIZE == 16 || SIZE == 4, "dwordx4 or dword");
    /*SIM-BEGIN*/
    const unsigned la = __builtin_amdgcn_readfirstlane((unsigned)(unsigned long)(__attribute__((address_space(3))) char*)lds);
    unsigned keep;
    if (SIZE == 16 && STREAM)          // nt (streaming policy).  Round 6 tried it on the X operand of the weight-gradient kernels (a saved activation, dead after the
                                       // launch): +0.3 ms / step -- the tiles of a row slice share those lines through the L2 (profiles/r6q_ab_tn_nt_operand.txt); unused
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %3, 0 offen nt lds\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "s"(la), "v"(voff), "s"(d) : "memory");
    else if (SIZE == 16)
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %3, 0 offen lds\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "s"(la), "v"(voff), "s"(d) : "memory");
    else
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tbuffer_load_dword %2, %3, 0 offen lds\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "s"(la), "v"(voff), "s"(d) : "memory");
    /*SIM-END sim_hidden_dma<SIZE>(d, lds, voff); */
}

__device__ __forceinline__ int tn_rid(int row) { return (row & 3) | (((row >> 3) & 1) << 2); }

template <typename T>
__device__ __forceinline__ typename TT<T>::v8 tn_frag(const char* tile, int colblk16, int ks, int fr, int fg) {
    typedef short v4s __attribute__((ext_vector_type(4)));
    const int r0 = ks * 32 + fg * 8 + (fr >> 2);
    const int unit = colblk16 * 4 + (fr & 3);
    const int a0 = r0 * 256 + ((unit ^ (tn_rid(r0) << 2)) * 8);
    const int a1 = (r0 + 4) * 256 + ((unit ^ (tn_rid(r0 + 4) << 2)) * 8);
    const v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((v4s __attribute__((address_space(3)))*)(tile + a0));
    const v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((v4s __attribute__((address_space(3)))*)(tile + a1));
    typedef short v8s __attribute__((ext_vector_type(8)));
    const v8s r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(typename TT<T>::v8, r);
}

// ---- which (row slice z, output tile) a TN workgroup computes.  Workgroup ids go round-robin to the 8 XCDs (id & 7), each with a private
// 4 MiB L2, and a TN workgroup streams ROWS of dY / X: everything that shares rows wants to sit on one XCD at the same time.
//   * split_k a multiple of 8 (the 64x40-level gradients: 16-32 slices of 35840 rows): XCD x runs slices x, x + 8, ... -- ALL output
//     tiles of a slice side by side, walking the slice's rows in step, so each row of dY and X comes over the fabric once (round 3 put
//     the slices of one TILE on an XCD: they share nothing, and every operand row was fetched by up to 8 XCDs -- 344 MB where 115 MB are
//     algorithmic on the 320 x 1280 gradient, profiles/r4_pmc_traffic_by_shape.txt);
//   * split_k in {1, 2, 4}: each slice owns 8 / split_k XCDs, arranged xm x xn over its tile grid so that the cheaper operand is the one
//     re-fetched (host: tn_arrange -- the rule of launch_gemm_v4).
// Grid: 8 * zsets * sub_m * sub_n workgroups in x; out-of-range ids exit.
struct TnWho { int pid_m, pid_n, z; bool live; };
__device__ __forceinline__ TnWho tn_who(const GemmParams& p) {
    const int bid = blockIdx.x, xcd = bid & 7, l = bid >> 3;
    const int per = p.sub_m * p.sub_n;
    const int zs = l / per, r = l - zs * per;
    TnWho w;
    int xi_m = 0, xi_n = 0;
    if (p.split_k >= 8 || 8 % p.split_k) {           // (a slice count that neither divides 8 nor is a multiple of it leaves XCDs idle: legal, slow)
        w.z = zs * 8 + xcd;
    } else {
        const int xps = 8 / p.split_k, xi = xcd % xps;
        w.z = xcd / xps;
        xi_m = xi / p.xcd_n;
        xi_n = xi - xi_m * p.xcd_n;
    }
    const int lm = r / p.sub_n;
    w.pid_m = xi_m * p.sub_m + lm;
    w.pid_n = xi_n * p.sub_n + (r - lm * p.sub_n);
    w.live = w.z < p.split_k && w.pid_m < p.tiles_m && w.pid_n < p.tiles_n;
    return w;
}

// ---- what gemm_tn_kernel and gemm_tn8_kernel share beyond tn_who and the stage ring (gemm_common.h) ----
// (The empty-slice exit, the column-sum store and the flat-path pieces are spelled out in both kernels: moved into a helper -- by reference,
// by value, per 16-row block, pointer only -- each changed the schedule of every TN kernel; profiles/gemm_split_isa_identity.md.)
// BUF staging: byte offset of a 16-byte piece at (row, col) of K-tile 0; a column beyond the operand gets an offset beyond num_records, so
// the piece reads zeros like a row beyond R does (the descriptor checks voffset, not soffset)
constexpr unsigned TN_OOB = 0x7ffffff0u;
__device__ __forceinline__ unsigned tn_voff(int row, int ld, int col, int ncols) { return col < ncols ? (unsigned)(row * ld + col) * 2u : TN_OOB; }

// The K-tiles [begin, end) of row slice z (p.K: the reduction length, rows of A and B)
struct TnSlice { int begin, end; };
__device__ __forceinline__ TnSlice tn_k_slice(const GemmParams& p, int z) {
    const int kt_total = (p.K + BK - 1) / BK;
    const int kt_per = (kt_total + p.split_k - 1) / p.split_k;
    const int kt_begin = z * kt_per;
    return TnSlice{kt_begin, min(kt_total, kt_begin + kt_per)};
}

// GATHER (svdx_gemm_tn_gather, the convolution weight gradients; the template value is the gather mode, SVDX_GATHER_CONV3X3 or
// SVDX_GATHER_TEMPORAL3, 0 = the plain kernel): byte offset into the gathered tensor p.B of the 16-byte piece that holds columns
// k .. k + 7 (k = tap * cin + ci; a piece never straddles taps, cin % 8 == 0) of row r of Aeff -- the operand svdx_gemm's forward sees for
// the same p.g.  The row -> source row map IS the forward's (decode_row / a_row_src of gemm_common.h).  A row >= R, a tap outside the
// image and a column beyond taps * cin (tap < 0) get the offset beyond num_records, so the piece reads zeros.  Branch-free: the mode is
// a compile-time constant here (a_row_src's mode tests fold away), the rest are selects.
template <int MODE>
__device__ __forceinline__ unsigned tn_gather_voff(const GemmParams& p, const RowInfo& ri, int r, int tap, int ci) {
    svdx_gather g = p.g;
    g.mode = MODE;
    bool valid;
    const int src = a_row_src(g, ri, tap, valid);
    return (valid & (r < p.K) & (tap >= 0)) ? (unsigned)(src * g.lda + ci) * 2u : TN_OOB;
}
// decode_row costs two integer divisions, and a thread stages four rows of EVERY K-tile: decoded per tile, the address arithmetic outweighed
// the tile's MFMAs (profiles/conv_wgrad.md).  So each thread decodes its four rows once, for its first K-tile, and WALKS them from tile to
// tile: BK rows further on is a fixed step in (x, y, image) -- or (pixel, frame, clip) -- with at most one carry per coordinate.  Every
// constant of the walk comes out of decode_row itself (rows 0, BK and one image), so the walk cannot drift from the forward's map; the
// simulator runs it against the float64 convolutions at widths from 2 to 16 and clips of 1 to 14 frames.
// In the temporal mode RowInfo::b (unused by that map) carries the pixel index, which decode_row folds into `base`.
struct TnWalk { int db, b_wrap, b_size, da, a_carry, a_wrap, a_size, dbase, unit; };
template <int MODE>
__device__ __forceinline__ TnWalk tn_walk(const svdx_gather& g0) {
    svdx_gather g = g0;
    g.mode = MODE;
    const RowInfo z = decode_row(g, 0), d = decode_row(g, BK);
    TnWalk w;
    if (MODE == SVDX_GATHER_TEMPORAL3) {
        w.db = BK % g.hw; w.b_size = g.hw; w.b_wrap = g.hw;                                   // pixel
        w.da = d.a - z.a; w.a_carry = 1; w.a_size = g.t; w.a_wrap = g.t;                      // frame
        w.unit = decode_row(g, g.t * g.hw).base - z.base;                                     // one clip
        w.dbase = d.base - z.base - w.db;                                                     // whole clips in BK rows
    } else {
        w.db = d.b - z.b; w.b_size = g.wo * g.stride; w.b_wrap = w.b_size + z.b;              // x (RowInfo::b = x * stride - 1)
        w.da = d.a - z.a; w.a_carry = g.stride; w.a_size = g.ho * g.stride; w.a_wrap = w.a_size + z.a;
        w.unit = decode_row(g, g.wo * g.ho).base - z.base;                                    // one image
        w.dbase = d.base - z.base;
    }
    return w;
}
template <int MODE>
__device__ __forceinline__ RowInfo tn_walk_first(const svdx_gather& g0, int r) {
    svdx_gather g = g0;
    g.mode = MODE;
    RowInfo ri = decode_row(g, r);
    if (MODE == SVDX_GATHER_TEMPORAL3) ri.b = r % g.hw;
    return ri;
}
template <int MODE>
__device__ __forceinline__ void tn_walk_step(const TnWalk& w, RowInfo& ri) {
    ri.b += w.db;
    const bool cb = ri.b >= w.b_wrap;
    ri.b -= cb ? w.b_size : 0;
    if (MODE == SVDX_GATHER_TEMPORAL3) ri.base += w.db - (cb ? w.b_size : 0);
    ri.a += w.da + (cb ? w.a_carry : 0);
    const bool ca = ri.a >= w.a_wrap;
    ri.a -= ca ? w.a_size : 0;
    ri.base += w.dbase + (ca ? w.unit : 0);
}

// BUF (round 5): the staging as buffer_load ... lds through two raw descriptors (operands below 2 GiB), issued by hidden_dma above: per-thread
// byte offsets computed once, the row bound from num_records instead of a zero page (a column beyond the operand gets an offset beyond it), and
// -- the point -- no compiler-inserted vmcnt(0) between the staging pieces and the fragment reads: loads and MFMAs overlap at last.
// GATHER (needs BUF): B is the source tensor of p.g and the B tile is gathered from it, row by row of every K-tile (tn_gather_voff).
template <typename T, int NSTG, bool BUF = false, int GATHER = 0>
__global__ __launch_bounds__(NTHREADS) void gemm_tn_kernel(GemmParams p) {
    static_assert(BUF || !GATHER, "the gathered B operand is staged through its buffer descriptor");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef typename TT<T>::v8 v8;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const TnWho who = tn_who(p);
    if (!who.live) return;
    const int pid_m = who.pid_m, pid_n = who.pid_n;
    const int m0 = pid_m * BM, n0 = pid_n * BN;          // m0: first output row (a column of A), n0: first output col (a column of B)
    const int R = p.K;                                   // reduction length (rows of A and B)
    const int z = who.z;
    const TnSlice ks = tn_k_slice(p, z);
    const int kt_begin = ks.begin, kt_end = ks.end;
    if (kt_begin >= kt_end) {               // a slice without rows (the host never asks for one): its column-sum row is all zeros
        if (p.a_colsum && p.out_mode == SVDX_OUT_F32_SLAB && pid_n == 0 && tid < BM && m0 + tid < p.M) p.a_colsum[(size_t)z * p.M + m0 + tid] = 0.f;
        return;
    }

    // staging: tile = 64 rows x 16 chunks (16 B); thread handles 4 rows, one fixed physical chunk
    const int pc = tid & 15, ld_row = tid >> 4;          // ld_row 0..15; rows ld_row + 16*i
    const T* zero = reinterpret_cast<const T*>(p.zero_page);
    const T* A = reinterpret_cast<const T*>(p.A);
    const T* B = reinterpret_cast<const T*>(p.B);
    // BUF: byte offsets of this thread's four pieces inside K-tile 0 (tn_voff; the K-tile adds kt * BK rows)
    const desc4 rsA = hidden_desc(p.A, BUF ? (unsigned)p.a_bytes : 0u), rsB = hidden_desc(p.B, BUF ? (unsigned)p.b_bytes : 0u);
    unsigned voa[4], vob[4];
    int gtap[4], gci[4];                                 // GATHER: tap (-1: a column beyond the operand) and channel of this thread's four pieces
    RowInfo gri[4];                                      // GATHER: this thread's four rows of the K-tile staged next (issue() walks them on)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = i * 16 + ld_row;
        const int lc = pc ^ (tn_rid(row) << 1);
        voa[i] = tn_voff(row, p.lda, m0 + lc * 8, p.M);
        vob[i] = tn_voff(row, p.ldb, n0 + lc * 8, p.N);
        if (GATHER) {
            const int k = n0 + lc * 8;
            gtap[i] = k < p.N ? k / p.g.cin : -1;
            gci[i] = k - gtap[i] * p.g.cin;
            gri[i] = tn_walk_first<GATHER>(p.g, kt_begin * BK + row);
        }
    }
    const TnWalk walk = GATHER ? tn_walk<GATHER>(p.g) : TnWalk{};
    auto issue = [&](int kt, int stage) __attribute__((always_inline)) {
        char* As = smem + stage * STAGE_BYTES;
        char* Bs = As + BM * BK * 2;
        const int wave_u = __builtin_amdgcn_readfirstlane(wave);
        if (BUF) {
            const unsigned ka = (unsigned)kt * (unsigned)(BK * 2) * (unsigned)p.lda, kb = (unsigned)kt * (unsigned)(BK * 2) * (unsigned)p.ldb;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int base = (i * 256 + wave_u * 64) * 16;
                hidden_dma<16>(rsA, As + base, voa[i] + ka);
                hidden_dma<16>(rsB, Bs + base, GATHER ? tn_gather_voff<GATHER>(p, gri[i], kt * BK + i * 16 + ld_row, gtap[i], gci[i]) : vob[i] + kb);
                if (GATHER) tn_walk_step<GATHER>(walk, gri[i]);          // issue() is called for consecutive K-tiles
            }
            return;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = i * 16 + ld_row;
            const int lc = pc ^ (tn_rid(row) << 1);       // logical 16-byte chunk stored at physical chunk pc
            const int r = kt * BK + row;
            const int ca = m0 + lc * 8, cb = n0 + lc * 8;
            const T* pa = (r < R && ca < p.M) ? A + (size_t)r * p.lda + ca : zero;
            const T* pb = (r < R && cb < p.N) ? B + (size_t)r * p.ldb + cb : zero;
            const int base = (i * 256 + wave_u * 64) * 16;      // chunk id = i*256 + tid = row*16 + pc
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)pa,
                                             (__attribute__((address_space(3))) void*)(As + base), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)pb,
                                             (__attribute__((address_space(3))) void*)(Bs + base), 16, 0, 0);
        }
    };
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // bias gradient = column sums of A = A^T * ones: the first column tile's wn == 0 waves spend 4 extra MFMAs per k-half on an
    // all-ones B fragment (no LDS traffic, float accumulation) instead of a separate pass over dY
    const bool do_cs = p.a_colsum != nullptr && pid_n == 0 && wn == 0;
    f32x4 accb[4];
    v8 ones;
#pragma unroll
    for (int e = 0; e < 8; ++e) ones[e] = (T)1.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) accb[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    // a 320-wide output ends in the middle of its third 128-wide tile: the waves whose 64 x 64 quadrant lies entirely outside the
    // output (wave-uniform) skip their fragment reads and MFMAs and only take part in the staging and the barriers
    const bool quad_live = m0 + wm * 64 < p.M && n0 + wn * 64 < p.N;
    auto compute = [&](int stage) __attribute__((always_inline)) {
        if (!quad_live) return;
        const char* As = smem + stage * STAGE_BYTES;
        const char* Bs = As + BM * BK * 2;
        const int fr = lane & 15, fg = lane >> 4;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            v8 af[4], bf[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                af[i] = tn_frag<T>(As, wm * 4 + i, ks, fr, fg);
                bf[i] = tn_frag<T>(Bs, wn * 4 + i, ks, fr, fg);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = TT<T>::mfma(af[i], bf[j], acc[i][j]);
            if (do_cs) {
#pragma unroll
                for (int i = 0; i < 4; ++i) accb[i] = TT<T>::mfma(af[i], ones, accb[i]);
            }
        }
    };
    // the stage ring (gemm_common.h: SVDX_STAGE_RING).  Every wave issues 8 pieces (4 of A, 4 of B) per tile.
    auto wait_tiles = [&](int t) __attribute__((always_inline)) {
        if (NSTG == 2 || t <= 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        else if (t == 1) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    };
    const int n_tiles = kt_end - kt_begin;
    SVDX_STAGE_RING(NSTG, n_tiles, issue(kt_begin + t, t),
                    { issue(kt_begin + kt + LA, nxt); __builtin_amdgcn_sched_barrier(0); compute(cur); }, compute(cur), wait_tiles)
    __syncthreads();
    if (do_cs && (lane & 15) == 0) {        // every column of the 16x16 result holds the sums: lanes 0/16/32/48 own rows 4*(lane>>4)..+3
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int n = m0 + wm * 64 + i * 16 + (lane >> 4) * 4 + e;
                if (n >= p.M) continue;
                // one owner per (row slice z, column n): a split reduction leaves its partial in slab z of a_colsum (summed in a fixed
                // order by svdx_gemm_finalize), an unsplit one adds to the running bias gradient -- no atomics, reproducible bits
                if (p.out_mode == SVDX_OUT_F32_SLAB) p.a_colsum[(size_t)z * p.M + n] = accb[i][e];
                else p.a_colsum[n] += accb[i][e];
            }
    }
    gemm_epilogue<T>(p, acc, smem, m0, n0, z, tid, lane, wm, wn);
}


// ----------------------------------------------------------------------------------------------------------------
// Eight-wave TN tiles: 128*PA output rows x 128*PB output columns (instantiated: 256 x 256), one workgroup per CU.
// The weight gradients of the step are [2560..10240] x [320..1280] outputs over 560..35840 rows: with 128 x 128 tiles the grids are
// 60-800 tiles that need up to 32 row slices to fill the chip; the larger tiles stage 2/3 (256 x 128) or 1/2 (256 x 256) of the
// operand bytes per flop and need a quarter of the slices.  Same operand layout as gemm_tn_kernel: an operand tile is PA (PB)
// panels of [64 r][128 cols] with that kernel's 8-byte-unit swizzle, fragments by ds_read_b64_tr_b16; accumulators are kept
// transposed (acc = mfma(B_frag, A_frag)) so that a lane owns 4 consecutive output columns: results leave as 16-byte stores
// straight from the registers.  Stage ring: SVDX_STAGE_RING (gemm_common.h).
// ----------------------------------------------------------------------------------------------------------------
template <typename T, int PA, int PB, int NSTG, bool BUF = false>
__global__ __launch_bounds__(512) void gemm_tn8_kernel(GemmParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef typename TT<T>::v8 v8;
    constexpr int NT = 512;
    constexpr int TM = 128 * PA, TK = 128 * PB;                    // output tile
    constexpr int WMN = 2 * PA, WNN = 8 / WMN;                     // waves along the output rows / columns (64 rows each)
    constexpr int NJ = TK / WNN / 16;                              // 16-column blocks per wave (4 | 8)
    constexpr int PANEL = 64 * 256;                                // bytes of one [64 r][128 cols] panel
    constexpr int STAGE = (PA + PB) * PANEL;
    constexpr int NPIECE = 2 * (PA + PB);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WNN, wn = wave % WNN;
    const TnWho who = tn_who(p);
    if (!who.live) return;
    const int pid_m = who.pid_m, pid_n = who.pid_n;
    const int m0 = pid_m * TM, n0 = pid_n * TK;
    const int R = p.K;
    const int z = who.z;
    const TnSlice ks = tn_k_slice(p, z);
    const int kt_begin = ks.begin, kt_end = ks.end;
    if (kt_begin >= kt_end) {
        if (p.a_colsum && p.out_mode == SVDX_OUT_F32_SLAB && pid_n == 0 && tid < TM && m0 + tid < p.M) p.a_colsum[(size_t)z * p.M + m0 + tid] = 0.f;
        return;
    }
    const int pc = tid & 15, ld_row = tid >> 4;                   // ld_row 0..31; rows ld_row + 32 * i of a panel
    const T* zero = reinterpret_cast<const T*>(p.zero_page);
    const T* A = reinterpret_cast<const T*>(p.A);
    const T* B = reinterpret_cast<const T*>(p.B);
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    // BUF: see gemm_tn_kernel -- buffer_load ... lds through descriptors; per-thread byte offsets of its pieces inside K-tile 0
    const desc4 rsA = hidden_desc(p.A, BUF ? (unsigned)p.a_bytes : 0u), rsB = hidden_desc(p.B, BUF ? (unsigned)p.b_bytes : 0u);
    unsigned voa[2][PA], vob[2][PB];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = i * 32 + ld_row;
        const int lc = pc ^ (tn_rid(row) << 1);
#pragma unroll
        for (int pa = 0; pa < PA; ++pa) voa[i][pa] = tn_voff(row, p.lda, m0 + pa * 128 + lc * 8, p.M);
#pragma unroll
        for (int pb = 0; pb < PB; ++pb) vob[i][pb] = tn_voff(row, p.ldb, n0 + pb * 128 + lc * 8, p.N);
    }
    auto issue = [&](int kt, int stage) __attribute__((always_inline)) {
        char* As = smem + stage * STAGE;
        char* Bs = As + PA * PANEL;
        if (BUF) {
            const unsigned ka = (unsigned)kt * (unsigned)(BK * 2) * (unsigned)p.lda, kb = (unsigned)kt * (unsigned)(BK * 2) * (unsigned)p.ldb;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int base = (i * NT + wave_u * 64) * 16;
#pragma unroll
                for (int pa = 0; pa < PA; ++pa)
                    hidden_dma<16>(rsA, As + pa * PANEL + base, voa[i][pa] + ka);
#pragma unroll
                for (int pb = 0; pb < PB; ++pb)
                    hidden_dma<16>(rsB, Bs + pb * PANEL + base, vob[i][pb] + kb);
            }
            return;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row = i * 32 + ld_row;
            const int lc = pc ^ (tn_rid(row) << 1);
            const int r = kt * BK + row;
            const int base = (i * NT + wave_u * 64) * 16;            // chunk id inside the panel = i * 512 + tid = row * 16 + pc
#pragma unroll
            for (int pa = 0; pa < PA; ++pa) {
                const int ca = m0 + pa * 128 + lc * 8;
                const T* src = (r < R && ca < p.M) ? A + (size_t)r * p.lda + ca : zero;
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                                 (__attribute__((address_space(3))) void*)(As + pa * PANEL + base), 16, 0, 0);
            }
#pragma unroll
            for (int pb = 0; pb < PB; ++pb) {
                const int cb = n0 + pb * 128 + lc * 8;
                const T* src = (r < R && cb < p.N) ? B + (size_t)r * p.ldb + cb : zero;
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                                 (__attribute__((address_space(3))) void*)(Bs + pb * PANEL + base), 16, 0, 0);
            }
        }
    };
    f32x4 acc[4][NJ];                                             // [16-row block i][16-column block j], transposed inside a block
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const bool do_cs = p.a_colsum != nullptr && pid_n == 0 && wn == 0;      // bias gradient = A^T * ones (see gemm_tn_kernel)
    f32x4 accb[4];
    v8 ones;
#pragma unroll
    for (int e = 0; e < 8; ++e) ones[e] = (T)1.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) accb[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int fr = lane & 15, fg = lane >> 4;
    auto compute = [&](int stage) __attribute__((always_inline)) {
        const char* As = smem + stage * STAGE;
        const char* Bs = As + PA * PANEL;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            v8 af[4], bf[NJ];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int blk = wm * 4 + i;
                af[i] = tn_frag<T>(As + (blk >> 3) * PANEL, blk & 7, ks, fr, fg);
            }
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int blk = wn * NJ + j;
                bf[j] = tn_frag<T>(Bs + (blk >> 3) * PANEL, blk & 7, ks, fr, fg);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < NJ; ++j) acc[i][j] = TT<T>::mfma(bf[j], af[i], acc[i][j]);
            if (do_cs) {
#pragma unroll
                for (int i = 0; i < 4; ++i) accb[i] = TT<T>::mfma(af[i], ones, accb[i]);
            }
        }
    };
    static_assert(NSTG >= 2 && NSTG <= 3, "2 or 3 LDS stages");
    auto wait_tiles = [&](int t) __attribute__((always_inline)) {
        if (NSTG == 2 || t <= 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NPIECE) : "memory");
    };
    const int n_tiles = kt_end - kt_begin;
    SVDX_STAGE_RING(NSTG, n_tiles, issue(kt_begin + t, t),
                    { issue(kt_begin + kt + LA, nxt); __builtin_amdgcn_sched_barrier(0); compute(cur); }, compute(cur), wait_tiles)
    if (do_cs && fr == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int n = m0 + wm * 64 + i * 16 + fg * 4 + e;
                if (n >= p.M) continue;
                if (p.out_mode == SVDX_OUT_F32_SLAB) p.a_colsum[(size_t)z * p.M + n] = accb[i][e];
                else p.a_colsum[n] += accb[i][e];
            }
    }
    float* Cf = reinterpret_cast<float*>(p.C) + (p.out_mode == SVDX_OUT_F32_SLAB ? (size_t)z * p.slab_stride : 0);
    bool bad_any = false;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int n = m0 + wm * 64 + i * 16 + fr;
        if (n >= p.M) continue;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int k = n0 + wn * (16 * NJ) + j * 16 + fg * 4;
            if (k >= p.N) continue;
            float* o = Cf + (size_t)n * p.ldc + k;
            const f32x4 v = acc[i][j] * p.alpha;
            if (p.vec_ok && k + 4 <= p.N) {
                if (p.out_mode == SVDX_OUT_F32) {
                    __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(o));      // a weight gradient: read next by the optimizer
                    if (p.found_inf) bad_any |= not_finite(v[0]) || not_finite(v[1]) || not_finite(v[2]) || not_finite(v[3]);
                } else if (p.out_mode == SVDX_OUT_F32_SLAB) *reinterpret_cast<f32x4*>(o) = v;
                else if (p.out_mode == SVDX_OUT_F32_ADD) {
                    const f32x4 t = *reinterpret_cast<const f32x4*>(o) + v;
                    *reinterpret_cast<f32x4*>(o) = t;
                    if (p.found_inf) bad_any |= not_finite(t[0]) || not_finite(t[1]) || not_finite(t[2]) || not_finite(t[3]);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) atomicAdd(o + e, v[e]);
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (k + e >= p.N) continue;
                    if (p.out_mode == SVDX_OUT_F32 || p.out_mode == SVDX_OUT_F32_SLAB) {
                        o[e] = v[e];
                        bad_any |= p.found_inf && p.out_mode == SVDX_OUT_F32 && not_finite(v[e]);
                    } else if (p.out_mode == SVDX_OUT_F32_ADD) {
                        const float t = o[e] + v[e];
                        o[e] = t;
                        bad_any |= p.found_inf && not_finite(t);
                    } else atomicAdd(o + e, v[e]);
                }
            }
        }
    }
    raise_found_inf(p.found_inf, bad_any);
}

// grid of the TN kernels (tn_who): fills p.xcd_n / sub_m / sub_n, returns the number of workgroups.  The host side asks for 1, 2, 4 or a
// multiple of 8 row slices (ops._tn_formula); any other count runs with some XCDs idle.
static long tn_arrange(GemmParams& p) {
    if (p.split_k >= 8 || 8 % p.split_k) {
        p.xcd_n = 1; p.sub_m = p.tiles_m; p.sub_n = p.tiles_n;
        return 8L * cdiv(p.split_k, 8) * p.sub_m * p.sub_n;
    }
    const int xps = 8 / p.split_k;
    const double a_bytes = 2.0 * p.K * p.M, b_bytes = 2.0 * p.K * p.N;          // dY [R, N_out] and X [R, K_out] of one call (p.M / p.N = output rows / columns)
    double cost;                                                                // every XCD column re-fetches dY, every XCD row re-fetches X
    int best_xn = xcd_arrangement(p.tiles_m, p.tiles_n, xps, a_bytes, b_bytes, cost);
    if (best_xn == 0) best_xn = 1;
    p.xcd_n = best_xn;
    p.sub_m = cdiv(p.tiles_m, xps / best_xn);
    p.sub_n = cdiv(p.tiles_n, best_xn);
    return 8L * p.sub_m * p.sub_n;
}

template <typename T, int NSTG, bool BUF = false, int GATHER = 0>
int launch_gemm_tn(GemmParams p, hipStream_t st) {
    constexpr int LDS = NSTG * STAGE_BYTES;
    [[maybe_unused]] static const bool lds_ok = allow_lds(&gemm_tn_kernel<T, NSTG, BUF, GATHER>, LDS);
    dim3 grid((unsigned)tn_arrange(p));
    hipLaunchKernelGGL((gemm_tn_kernel<T, NSTG, BUF, GATHER>), grid, dim3(NTHREADS), LDS, st, p);
    SVDX_LAUNCH_CHECK(GATHER ? "svdx_gemm_tn_gather" : "svdx_gemm_tn");
    return 0;
}

template <typename T, int PA, int PB, int NSTG, bool BUF = false>
int launch_gemm_tn8(GemmParams p, hipStream_t st) {
    constexpr int LDS = NSTG * (PA + PB) * 64 * 256;
    static_assert(LDS <= 160 * 1024, "stages must fit the 160 KiB LDS");
    [[maybe_unused]] static const bool lds_ok = allow_lds(&gemm_tn8_kernel<T, PA, PB, NSTG, BUF>, LDS);
    p.tiles_m = cdiv(p.M, 128 * PA);
    p.tiles_n = cdiv(p.N, 128 * PB);
    dim3 grid((unsigned)tn_arrange(p));
    hipLaunchKernelGGL((gemm_tn8_kernel<T, PA, PB, NSTG, BUF>), grid, dim3(512), LDS, st, p);
    SVDX_LAUNCH_CHECK("svdx_gemm_tn");
    return 0;
}

}  // namespace

extern "C" int svdx_gemm_tn(const void* A, const void* B, float* C, int R, int N, int K, int lda, int ldb, int ldc,
                            float* a_colsum, const void* zero_page, int out_mode, int split_k, int stages, float* found_inf, int dtype,
                            void* stream) {
    SVDX_CHECK_ARG(A && B && C && zero_page && R > 0 && N > 0 && K > 0, "svdx_gemm_tn: bad args");
    SVDX_CHECK_ARG(!found_inf || out_mode == SVDX_OUT_F32 || out_mode == SVDX_OUT_F32_ADD, "svdx_gemm_tn: found_inf goes with the store / += modes");
    // operands below 2 GiB are staged through buffer descriptors (SVDX_TN_FLAT: a test asks for the large-operand path on a small operand)
    const long a_span = ((long)(R - 1) * lda + N) * 2, b_span = ((long)(R - 1) * ldb + K) * 2;
    // (the kernels mark columns beyond the operand with the offset 0x7ffffff0, which must itself lie beyond num_records: spans up to that value only)
    const bool buf = a_span <= 0x7ffffff0L && b_span <= 0x7ffffff0L && !(stages & SVDX_TN_FLAT);
    stages &= ~SVDX_TN_FLAT;
    SVDX_CHECK_ARG(stages == 0 || (stages >= 2 && stages <= 4) || stages == 18,
                   "svdx_gemm_tn: stages=%d (0 = default, 2..4 stages of the 128x128 tile, 18 = the 256x256 eight-wave tile)", stages);
    // the unsplit / ADD modes read-modify-write a_colsum from every z slice: one slice only (SVDX_OUT_F32_SLAB keeps a row per slice)
    SVDX_CHECK_ARG(!a_colsum || split_k == 1 || out_mode == SVDX_OUT_F32_SLAB, "svdx_gemm_tn: a_colsum with split_k > 1 needs slab output");
    SVDX_CHECK_ARG(N % 8 == 0 && K % 8 == 0 && lda % 8 == 0 && ldb % 8 == 0 && ((uintptr_t)A & 15) == 0 && ((uintptr_t)B & 15) == 0 &&
                       ((uintptr_t)zero_page & 15) == 0, "svdx_gemm_tn: operands must be 16-byte aligned, N/K multiples of 8");
    SVDX_CHECK_ARG(out_mode == SVDX_OUT_F32 || out_mode == SVDX_OUT_F32_ADD || out_mode == SVDX_OUT_F32_SLAB ||
                       out_mode == SVDX_OUT_F32_ATOMIC, "svdx_gemm_tn: float output modes only");
    SVDX_CHECK_ARG(split_k >= 1 && (split_k == 1 || out_mode == SVDX_OUT_F32_SLAB || out_mode == SVDX_OUT_F32_ATOMIC),
                   "svdx_gemm_tn: split_k needs slab or atomic output");
    SVDX_CHECK_ARG(out_mode != SVDX_OUT_F32_SLAB || (split_k - 1) * cdiv(cdiv(R, BK), split_k) < cdiv(R, BK),
                   "svdx_gemm_tn: split_k=%d leaves slices without rows (R=%d): their slabs would stay unwritten", split_k, R);
    GemmParams p{};                   // every field the TN kernels do not use is zero / null in the kernel arguments (and in a recorded launch plan)
    p.A = A; p.B = B; p.C = C; p.M = N; p.N = K; p.K = R; p.lda = lda; p.ldb = ldb; p.ldc = ldc;
    p.zero_page = zero_page; p.out_mode = out_mode; p.alpha = 1.f; p.split_k = split_k;
    p.a_colsum = a_colsum; p.found_inf = found_inf;
    p.a_bytes = buf ? (int)a_span : 0; p.b_bytes = buf ? (int)b_span : 0;
    p.tiles_m = cdiv(N, BM); p.tiles_n = cdiv(K, BN);
    p.vec_ok = (ldc % 4 == 0) && (((uintptr_t)C & 15) == 0) && (K % 8 == 0);
    p.slab_stride = (long)N * ldc;
    DISPATCH_DTYPE(dtype, {
        hipStream_t st = (hipStream_t)stream;
        if (stages == 18) return buf ? launch_gemm_tn8<T, 2, 2, 2, true>(p, st) : launch_gemm_tn8<T, 2, 2, 2>(p, st);
        if (stages == 3) return buf ? launch_gemm_tn<T, 3, true>(p, st) : launch_gemm_tn<T, 3>(p, st);
        if (stages == 4) return buf ? launch_gemm_tn<T, 4, true>(p, st) : launch_gemm_tn<T, 4>(p, st);
        return buf ? launch_gemm_tn<T, 2, true>(p, st) : launch_gemm_tn<T, 2>(p, st);
    });
}

extern "C" int svdx_gemm_tn_gather(const void* A, const void* X, float* C, int R, int N, int lda, int ldc, const svdx_gather* gather,
                                   float* a_colsum, int out_mode, int split_k, int stages, float* found_inf, int dtype, void* stream) {
    SVDX_CHECK_ARG(A && X && C && gather && R > 0 && N > 0, "svdx_gemm_tn_gather: bad args");
    const svdx_gather& g = *gather;
    SVDX_CHECK_ARG(g.mode == SVDX_GATHER_CONV3X3 || g.mode == SVDX_GATHER_TEMPORAL3,
                   "svdx_gemm_tn_gather: gather mode %d (the 3x3 convolution and the temporal convolution only)", g.mode);
    SVDX_CHECK_ARG(g.cin > 0 && g.cin % 8 == 0 && g.lda >= g.cin && g.lda % 8 == 0 && g.n_img > 0, "svdx_gemm_tn_gather: cin=%d lda=%d must be multiples of 8", g.cin, g.lda);
    long src_rows;
    if (g.mode == SVDX_GATHER_CONV3X3) {
        SVDX_CHECK_ARG(g.stride == 1 || g.stride == 2, "svdx_gemm_tn_gather: conv stride");
        SVDX_CHECK_ARG(g.ups == 0 || (g.ups == 1 && g.hi % 2 == 0 && g.wi % 2 == 0), "svdx_gemm_tn_gather: upsampled dims must be even");
        SVDX_CHECK_ARG(g.hi > 0 && g.wi > 0 && g.ho > 0 && g.wo > 0 && (long)R == (long)g.n_img * g.ho * g.wo, "svdx_gemm_tn_gather: conv rows mismatch");
        src_rows = (long)g.n_img * (g.hi >> g.ups) * (g.wi >> g.ups);
    } else {
        SVDX_CHECK_ARG(g.t > 0 && g.hw > 0 && (long)R == (long)g.n_img * g.t * g.hw, "svdx_gemm_tn_gather: temporal rows mismatch");
        src_rows = R;
    }
    const int K = (g.mode == SVDX_GATHER_TEMPORAL3 ? 3 : 9) * g.cin;
    SVDX_CHECK_ARG(!found_inf || out_mode == SVDX_OUT_F32 || out_mode == SVDX_OUT_F32_ADD, "svdx_gemm_tn_gather: found_inf goes with the store / += modes");
    SVDX_CHECK_ARG(stages == 0 || (stages >= 2 && stages <= 4), "svdx_gemm_tn_gather: stages=%d (0 = default, 2..4 stages of the 128x128 tile)", stages);
    SVDX_CHECK_ARG(out_mode == SVDX_OUT_F32 || out_mode == SVDX_OUT_F32_ADD || out_mode == SVDX_OUT_F32_SLAB, "svdx_gemm_tn_gather: F32, F32_ADD or F32_SLAB output");
    SVDX_CHECK_ARG(split_k >= 1 && (split_k == 1 || out_mode == SVDX_OUT_F32_SLAB), "svdx_gemm_tn_gather: split_k needs slab output");
    SVDX_CHECK_ARG(out_mode != SVDX_OUT_F32_SLAB || (split_k - 1) * cdiv(cdiv(R, BK), split_k) < cdiv(R, BK),
                   "svdx_gemm_tn_gather: split_k=%d leaves slices without rows (R=%d): their slabs would stay unwritten", split_k, R);
    SVDX_CHECK_ARG(N % 8 == 0 && lda >= N && lda % 8 == 0 && ldc >= K && ((uintptr_t)A & 15) == 0 && ((uintptr_t)X & 15) == 0,
                   "svdx_gemm_tn_gather: operands must be 16-byte aligned, N and lda multiples of 8, ldc >= taps * cin");
    // both operands go through buffer descriptors (the flat staging of svdx_gemm_tn has no gathered form): below 2 GiB only
    const long a_span = ((long)(R - 1) * lda + N) * 2, x_span = ((src_rows - 1) * g.lda + g.cin) * 2;
    SVDX_CHECK_ARG(a_span <= 0x7ffffff0L && x_span <= 0x7ffffff0L, "svdx_gemm_tn_gather: operands of 2 GiB and more are not supported");
    GemmParams p{};
    p.A = A; p.B = X; p.C = C; p.M = N; p.N = K; p.K = R; p.lda = lda; p.ldb = g.lda; p.ldc = ldc;
    p.g = g; p.out_mode = out_mode; p.alpha = 1.f; p.split_k = split_k;
    p.a_colsum = a_colsum; p.found_inf = found_inf;
    p.a_bytes = (int)a_span; p.b_bytes = (int)x_span;
    p.tiles_m = cdiv(N, BM); p.tiles_n = cdiv(K, BN);
    p.vec_ok = (ldc % 4 == 0) && (((uintptr_t)C & 15) == 0);
    p.slab_stride = (long)N * ldc;
    DISPATCH_DTYPE(dtype, {
        hipStream_t st = (hipStream_t)stream;
        if (g.mode == SVDX_GATHER_TEMPORAL3) {
            if (stages == 3) return launch_gemm_tn<T, 3, true, SVDX_GATHER_TEMPORAL3>(p, st);
            if (stages == 4) return launch_gemm_tn<T, 4, true, SVDX_GATHER_TEMPORAL3>(p, st);
            return launch_gemm_tn<T, 2, true, SVDX_GATHER_TEMPORAL3>(p, st);
        }
        if (stages == 3) return launch_gemm_tn<T, 3, true, SVDX_GATHER_CONV3X3>(p, st);
        if (stages == 4) return launch_gemm_tn<T, 4, true, SVDX_GATHER_CONV3X3>(p, st);
        return launch_gemm_tn<T, 2, true, SVDX_GATHER_CONV3X3>(p, st);
    });
}
