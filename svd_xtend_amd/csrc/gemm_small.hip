// gemm_small.hip -- the matmul-shaped launches that are not MFMA tiles: skinny linears and outer products (single and table-driven), the
// split-K finalizers and the timestep embedding.
#include "gemm_common.h"

namespace {

// ---- skinny linear: one wave per output column, lanes split K (trans = 0); MT rows of X per pass ------------------
template <typename T, int MT>
__device__ __forceinline__ void small_linear_nt_body(const float* __restrict__ X, const T* __restrict__ W, const float* __restrict__ bias,
                                                     float* Y, int M, int N, int K, int ldw, int silu_in, int accumulate, int blk) {
    const int lane = threadIdx.x & 63;
    const int n = blk * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    const T* w = W + (size_t)n * ldw;
    for (int mb = 0; mb < M; mb += MT) {
        float acc[MT];
#pragma unroll
        for (int mi = 0; mi < MT; ++mi) acc[mi] = 0.f;
        for (int k8 = lane; k8 * 8 < K; k8 += 64) {
            float wv[8];
            load8<T>(w + k8 * 8, wv);
#pragma unroll
            for (int mi = 0; mi < MT; ++mi) {
                if (mb + mi < M) {
                    const f32x4 x0 = *reinterpret_cast<const f32x4*>(X + (size_t)(mb + mi) * K + k8 * 8);
                    const f32x4 x1 = *reinterpret_cast<const f32x4*>(X + (size_t)(mb + mi) * K + k8 * 8 + 4);
                    float xv[8] = {x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
                    float s = 0.f;
#pragma unroll
                    for (int j = 0; j < 8; ++j) s += (silu_in ? siluf_(xv[j]) : xv[j]) * wv[j];
                    acc[mi] += s;
                }
            }
        }
#pragma unroll
        for (int mi = 0; mi < MT; ++mi) {
            const float s = wave_sum(acc[mi]);
            if (lane == 0 && mb + mi < M) {
                float* y = Y + (size_t)(mb + mi) * N + n;
                const float r = s + (bias ? bias[n] : 0.f);
                *y = accumulate ? *y + r : r;
            }
        }
    }
}

template <typename T, int MT>
__global__ __launch_bounds__(256) void small_linear_nt(const float* __restrict__ X, const T* __restrict__ W, const float* __restrict__ bias,
                                                       float* Y, int M, int N, int K, int ldw, int silu_in, int accumulate) {
    small_linear_nt_body<T, MT>(X, W, bias, Y, M, N, K, ldw, silu_in, accumulate, blockIdx.x);
}

// trans = 1: Y[m,k] (+)= sum_n X[m,n] W[n,k].  The op is a GEMV over a matrix of a few MB: latency-shaped.  A block owns 64
// output columns (8 chunks of 8) x 32 row lanes; a thread walks the rows n = nl, nl + 32, ... with four 16-byte loads in flight and
// the 32 partial sums of a column are then added in a fixed order -- no atomics, so the result is run-to-run identical (the
// gradient of the cross-attention value path depends on it).
template <typename T>
__device__ __forceinline__ void small_linear_nn_body(const float* X, const T* W, float* Y, int M, int N, int K, int ldw, int accumulate,
                                                     int blk, float (*part)[65]) {
    const int kc = threadIdx.x & 7, nl = threadIdx.x >> 3;
    const int k8 = blk * 8 + kc;
    const int m = blockIdx.y;
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (k8 * 8 < K) {
        const float* x = X + (size_t)m * N;
        const T* wp = W + k8 * 8;
        int n = nl;
        for (; n + 96 < N; n += 128) {
            const Vec8<T> w0 = *reinterpret_cast<const Vec8<T>*>(wp + (size_t)n * ldw);
            const Vec8<T> w1 = *reinterpret_cast<const Vec8<T>*>(wp + (size_t)(n + 32) * ldw);
            const Vec8<T> w2 = *reinterpret_cast<const Vec8<T>*>(wp + (size_t)(n + 64) * ldw);
            const Vec8<T> w3 = *reinterpret_cast<const Vec8<T>*>(wp + (size_t)(n + 96) * ldw);
            const float x0 = x[n], x1 = x[n + 32], x2 = x[n + 64], x3 = x[n + 96];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                acc[j] += x0 * to_f<T>(w0.v[j]);
                acc[j] += x1 * to_f<T>(w1.v[j]);
                acc[j] += x2 * to_f<T>(w2.v[j]);
                acc[j] += x3 * to_f<T>(w3.v[j]);
            }
        }
        for (; n < N; n += 32) {
            const Vec8<T> w0 = *reinterpret_cast<const Vec8<T>*>(wp + (size_t)n * ldw);
            const float x0 = x[n];
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] += x0 * to_f<T>(w0.v[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) part[nl][kc * 8 + j] = acc[j];
    __syncthreads();
    if (threadIdx.x < 64) {
        const int k = blk * 64 + threadIdx.x;
        float sum = 0.f;
#pragma unroll
        for (int r = 0; r < 32; ++r) sum += part[r][threadIdx.x];
        if (k < K) {
            float* y = Y + (size_t)m * K + k;
            *y = accumulate ? *y + sum : sum;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void small_linear_nn(const float* X, const T* W, float* Y, int M, int N, int K, int ldw, int accumulate) {
    __shared__ float part[32][65];
    small_linear_nn_body<T>(X, W, Y, M, N, K, ldw, accumulate, blockIdx.x, part);
}

// ---- the same two kernels over a PACK of jobs in one launch: the per-clip vector chain of the KV-length-1 cross-attention is ~5 us of
// launch latency per linear and there are 64 of them per forward sweep (v and out of 32 blocks).  The job table travels in the kernel
// arguments (graph-capturable, no device-side table to keep alive); a workgroup finds its job by scanning the block prefix.
struct LinPack {
    svdx_lin_job job[SVDX_BATCH_MAX_JOBS];
    int start[SVDX_BATCH_MAX_JOBS + 1];        // first workgroup of job j; start[n_jobs] = grid size
    int n_jobs;
};

__device__ __forceinline__ int pack_find(const int* start, int n_jobs, int blk) {
    int j = 0;
    while (j + 1 < n_jobs && blk >= start[j + 1]) ++j;
    return j;
}

template <typename T, int MT>
__global__ __launch_bounds__(256) void small_linear_nt_batch(const LinPack pk, int M) {
    const int j = pack_find(pk.start, pk.n_jobs, blockIdx.x);
    const svdx_lin_job& q = pk.job[j];
    small_linear_nt_body<T, MT>(q.X, (const T*)q.W, q.bias, q.Y, M, q.N, q.K, q.ldw, q.flags & 1, (q.flags >> 1) & 1, blockIdx.x - pk.start[j]);
}

template <typename T>
__global__ __launch_bounds__(256) void small_linear_nn_batch(const LinPack pk, int M) {
    __shared__ float part[32][65];
    const int j = pack_find(pk.start, pk.n_jobs, blockIdx.x);
    const svdx_lin_job& q = pk.job[j];
    small_linear_nn_body<T>(q.X, (const T*)q.W, q.Y, M, q.N, q.K, q.ldw, (q.flags >> 1) & 1, blockIdx.x - pk.start[j], part);
}

// split-K epilogue: v = sum over `nsplit` float slabs (+ bias + rowvec + res);  C = (dtype)v, or Cf += v (weight grads)
// GN: also the GroupNorm statistics of the activation tensor it writes (see svdx_gemm_gn): a block's 256 pieces of 4 consecutive
// channels are 1024 consecutive elements of C -- at most two samples -- whose (sample, group) sums meet in a small LDS table of 64-bit
// fixed-point integers before they go to the replica slots, one atomic per touched entry.
struct FinGn { unsigned long long* stats; int rows, cg; float m0, m1; };
constexpr int FIN_GN_G = 64;
template <typename T, bool GN>
__global__ __launch_bounds__(256) void gemm_finalize_kernel(const float* __restrict__ acc, int nsplit, long slab_stride, T* __restrict__ C,
                                                            float* __restrict__ Cf, int f32_store, int M, int N, int ldc,
                                                            const float* __restrict__ bias, const float* __restrict__ rowvec,
                                                            int rv_ld, int rv_rpg, int rv_mod, const T* __restrict__ res, int ldres,
                                                            const float* __restrict__ cs_slabs, float* cs_out, int cs_n, FinGn gn) {
    __shared__ unsigned long long gacc[GN ? 2 * FIN_GN_G * 2 : 1];
    if (cs_slabs) {                            // bias gradient: the row slices' column sums, added in slice order (spread over the grid)
        for (int n = blockIdx.x * blockDim.x + threadIdx.x; n < cs_n; n += gridDim.x * blockDim.x) {
            float t = 0.f;
            for (int z = 0; z < nsplit; ++z) t += cs_slabs[(size_t)z * cs_n + n];
            cs_out[n] += t;
        }
    }
    const long total4 = (long)M * N / 4;       // N % 4 == 0
    for (long b4 = (long)blockIdx.x * blockDim.x; b4 < total4; b4 += (long)gridDim.x * blockDim.x) {
        const long i4 = b4 + threadIdx.x;
        if (GN) {
            for (int t = threadIdx.x; t < 2 * FIN_GN_G * 2; t += 256) gacc[t] = 0ull;
            __syncthreads();
        }
        if (i4 < total4) {
            const long i = i4 * 4;
            const int m = (int)(i / N), n = (int)(i - (long)m * N);
            f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(acc + i));       // slabs: written once, read once
            for (int z = 1; z < nsplit; ++z) v += __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(acc + (size_t)z * slab_stride + i));
            if (bias) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] += bias[n + e];
            }
            if (rowvec) {
                const float* rv = rowvec + (size_t)(rv_mod ? m % rv_mod : m / rv_rpg) * rv_ld + n;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] += rv[e];
            }
            if (res) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] += to_f<T>(res[(size_t)m * ldres + n + e]);
            }
            if (Cf) {
                float* o = Cf + (size_t)m * ldc + n;
                if (f32_store) {             // a weight gradient: next read by the optimizer, a whole backward sweep later
                    __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(o));
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] += v[e];
                }
            } else {
                Vec4<T> o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o.v[e] = from_f<T>(v[e]);
                *reinterpret_cast<Vec4<T>*>(C + (size_t)m * ldc + n) = o;
                if (GN) {
                    const int sl = m / gn.rows - (int)((b4 * 4) / N) / gn.rows;      // 0 or 1 (host: N * rows >= 1024)
                    int cur = n / gn.cg;
                    float s0 = 0.f, s1 = 0.f;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int g = (n + e) / gn.cg;
                        if (g != cur) {
                            atomicAdd(&gacc[(sl * FIN_GN_G + cur) * 2], (unsigned long long)__float2ll_rn(s0 * gn.m0));
                            atomicAdd(&gacc[(sl * FIN_GN_G + cur) * 2 + 1], (unsigned long long)__float2ll_rn(s1 * gn.m1));
                            cur = g; s0 = 0.f; s1 = 0.f;
                        }
                        const float x = to_f<T>(o.v[e]);
                        s0 += x; s1 += x * x;
                    }
                    atomicAdd(&gacc[(sl * FIN_GN_G + cur) * 2], (unsigned long long)__float2ll_rn(s0 * gn.m0));
                    atomicAdd(&gacc[(sl * FIN_GN_G + cur) * 2 + 1], (unsigned long long)__float2ll_rn(s1 * gn.m1));
                }
            }
        }
        if (GN) {
            __syncthreads();
            const int G = N / gn.cg, n_s = M / gn.rows;
            const int s_first = (int)((b4 * 4) / N) / gn.rows;              // sample of the block's first element
            unsigned long long* out = gn.stats + (size_t)(blockIdx.x % SVDX_GN_REPLICAS) * n_s * G * 2;
            for (int t = threadIdx.x; t < 2 * G * 2; t += 256) {
                const int w = t & 1, g = (t >> 1) % G, s2 = (t >> 1) / G;
                const unsigned long long a = gacc[(s2 * FIN_GN_G + g) * 2 + w];
                if (a && s_first + s2 < n_s) atomicAdd(out + ((size_t)(s_first + s2) * G + g) * 2 + w, a);
            }
            __syncthreads();
        }
    }
}

// ---- the float form of that epilogue over a PACK of jobs: the weight gradients of a backward sweep are not read before the optimizer,
// so the reducing launches of their row-sliced TN GEMMs (96 per step at c2, a few us of launch latency each for a few hundred KB) wait
// and run as one launch per 48 -- the same arithmetic in the same order per element (slice 0 first), so the bits do not change.
struct GradFinPack {
    svdx_gradfin_job job[SVDX_BATCH_MAX_JOBS];
    int start[SVDX_BATCH_MAX_JOBS + 1];
    int n_jobs;
};
__global__ __launch_bounds__(256) void grad_finalize_batch_kernel(const GradFinPack pk) {
    const int j = pack_find(pk.start, pk.n_jobs, blockIdx.x);
    const svdx_gradfin_job& q = pk.job[j];
    const int blk = blockIdx.x - pk.start[j], nblk = pk.start[j + 1] - pk.start[j];
    if (q.colsum_slabs) {                      // bias gradient: the row slices' column sums, added in slice order
        for (int n = blk * 256 + threadIdx.x; n < q.colsum_n; n += nblk * 256) {
            float t = 0.f;
            for (int z = 0; z < q.nsplit; ++z) t += q.colsum_slabs[(size_t)z * q.colsum_n + n];
            q.colsum_out[n] += t;
        }
    }
    const long total4 = q.count / 4;
    bool bad_any = false;
    for (long i4 = (long)blk * 256 + threadIdx.x; i4 < total4; i4 += (long)nblk * 256) {
        const long i = i4 * 4;
        f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(q.acc + i));
        for (int z = 1; z < q.nsplit; ++z) v += __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(q.acc + (size_t)z * q.slab_stride + i));
        f32x4* o = reinterpret_cast<f32x4*>(q.dst + i);
        if (q.store) __builtin_nontemporal_store(v, o);
        else { v = *o + v; *o = v; }
        bad_any |= not_finite(v[0]) || not_finite(v[1]) || not_finite(v[2]) || not_finite(v[3]);
    }
    raise_found_inf(q.found_inf, bad_any);
}

// X == nullptr: a column of ones (the bias gradient, K = 1)
__device__ __forceinline__ void outer_acc_body(const float* dY, const float* X, float* dW, int M, int N, int K, float scale, size_t blk) {
    const size_t idx = blk * blockDim.x + threadIdx.x;
    if (idx >= (size_t)N * K) return;
    const int n = (int)(idx / K), k = (int)(idx - (size_t)n * K);
    float s = 0.f;
    for (int m = 0; m < M; ++m) s += dY[(size_t)m * N + n] * (X ? X[(size_t)m * K + k] : 1.f);
    dW[idx] += scale * s;
}

__global__ void outer_acc_kernel(const float* dY, const float* X, float* dW, int M, int N, int K, float scale) {
    outer_acc_body(dY, X, dW, M, N, K, scale, blockIdx.x);
}

struct OuterPack {
    svdx_outer_job job[SVDX_BATCH_MAX_JOBS];
    int start[SVDX_BATCH_MAX_JOBS + 1];
    int n_jobs;
};

__global__ void outer_acc_batch_kernel(const OuterPack pk, int M) {
    const int j = pack_find(pk.start, pk.n_jobs, blockIdx.x);
    const svdx_outer_job& q = pk.job[j];
    outer_acc_body(q.dY, q.X, q.dW, M, q.N, q.K, q.scale, (size_t)(blockIdx.x - pk.start[j]));
}

__global__ void timestep_embed_kernel(const float* t, float* out, int n, int dim) {
    const int half = dim / 2;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * half) return;
    const int i = idx / half, j = idx - i * half;
    const float f = expf(-9.210340371976184f * (float)j / (float)half);   // ln(10000)
    const float a = t[i] * f;
    out[(size_t)i * dim + j] = cosf(a);
    out[(size_t)i * dim + half + j] = sinf(a);
}

}  // namespace

extern "C" int svdx_small_linear(const float* X, const void* W, const float* bias, float* Y, int M, int N, int K,
                                 int ldw, int trans, int silu_in, int accumulate, int dtype, void* stream) {
    SVDX_CHECK_ARG(X && W && Y && M > 0 && N > 0 && K > 0, "svdx_small_linear: bad args");
    SVDX_CHECK_ARG(K % 8 == 0 && ldw % 8 == 0 && ((uintptr_t)W & 15) == 0, "svdx_small_linear: K/ldw must be multiples of 8");
    hipStream_t st = (hipStream_t)stream;
    DISPATCH_DTYPE(dtype, {
        if (trans == 0) {
            SVDX_CHECK_ARG(((uintptr_t)X & 15) == 0 && K % 4 == 0, "svdx_small_linear: X must be 16-byte aligned");
            if (M == 1)
                hipLaunchKernelGGL((small_linear_nt<T, 1>), dim3(cdiv(N, 4)), dim3(256), 0, st, X, (const T*)W, bias, Y, M, N, K, ldw,
                                   silu_in, accumulate);
            else if (M <= 4)
                hipLaunchKernelGGL((small_linear_nt<T, 4>), dim3(cdiv(N, 4)), dim3(256), 0, st, X, (const T*)W, bias, Y, M, N, K, ldw,
                                   silu_in, accumulate);
            else
                hipLaunchKernelGGL((small_linear_nt<T, 8>), dim3(cdiv(N, 4)), dim3(256), 0, st, X, (const T*)W, bias, Y, M, N, K, ldw,
                                   silu_in, accumulate);
        } else {
            SVDX_CHECK_ARG(!bias && !silu_in, "svdx_small_linear: trans=1 takes no bias/activation");
            hipLaunchKernelGGL((small_linear_nn<T>), dim3(cdiv(K / 8, 8), M), dim3(256), 0, st, X, (const T*)W, Y, M, N, K, ldw, accumulate);
        }
    });
    SVDX_LAUNCH_CHECK("svdx_small_linear");
    return 0;
}

extern "C" int svdx_gemm_finalize(const float* acc, int nsplit, int64_t slab_stride, void* C, int c_is_f32_accumulate, int M, int N,
                                  int ldc, const float* bias, const float* rowvec, int rv_ld, int rv_rows_per_group, int rv_mod,
                                  const void* res, int ldres, const float* colsum_slabs, float* colsum_out, int colsum_n, int dtype,
                                  void* stream) {
    SVDX_CHECK_ARG(!colsum_slabs || (colsum_out && colsum_n > 0), "svdx_gemm_finalize: colsum_slabs needs colsum_out / colsum_n");
    SVDX_CHECK_ARG(acc && C && M > 0 && N > 0 && nsplit >= 1, "svdx_gemm_finalize: bad args");
    SVDX_CHECK_ARG(N % 4 == 0 && ldc % 4 == 0 && slab_stride % 4 == 0 && (!res || ldres % 4 == 0) && (!rowvec || rv_ld % 4 == 0),
                   "svdx_gemm_finalize: N/ld must be multiples of 4");
    SVDX_CHECK_ARG(!rowvec || rv_mod > 0 || rv_rows_per_group > 0, "svdx_gemm_finalize: rowvec needs a grouping");
    const int blocks = (int)std::min<long>(((long)M * N / 4 + 255) / 256, 4096);
    DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((gemm_finalize_kernel<T, false>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, acc, nsplit,
                                             (long)slab_stride, c_is_f32_accumulate ? (T*)nullptr : (T*)C,
                                             c_is_f32_accumulate ? (float*)C : (float*)nullptr, c_is_f32_accumulate == 2, M, N, ldc, bias, rowvec, rv_ld,
                                             rv_rows_per_group, rv_mod, (const T*)res, ldres, colsum_slabs, colsum_out, colsum_n, FinGn{}));
    SVDX_LAUNCH_CHECK("svdx_gemm_finalize");
    return 0;
}

extern "C" int svdx_gemm_finalize_gn(const float* acc, int nsplit, int64_t slab_stride, void* C, int M, int N, int ldc, const float* bias,
                                     const float* rowvec, int rv_ld, int rv_rows_per_group, int rv_mod, const void* res, int ldres,
                                     float* gn_stats, int gn_rows, int gn_cg, int dtype, void* stream) {
    SVDX_CHECK_ARG(acc && C && gn_stats && M > 0 && N > 0 && nsplit >= 1, "svdx_gemm_finalize_gn: bad args");
    SVDX_CHECK_ARG(N % 4 == 0 && ldc % 4 == 0 && slab_stride % 4 == 0 && (!res || ldres % 4 == 0) && (!rowvec || rv_ld % 4 == 0),
                   "svdx_gemm_finalize_gn: N/ld must be multiples of 4");
    SVDX_CHECK_ARG(!rowvec || rv_mod > 0 || rv_rows_per_group > 0, "svdx_gemm_finalize_gn: rowvec needs a grouping");
    SVDX_CHECK_ARG(gn_rows > 0 && gn_cg > 0 && M % gn_rows == 0 && N % gn_cg == 0 && N / gn_cg <= FIN_GN_G && (long)N * gn_rows >= 1024 &&
                       ((uintptr_t)gn_stats & 7) == 0,
                   "svdx_gemm_finalize_gn: M=%d whole samples of %d rows (N x rows >= 1024), N=%d whole groups of %d channels (<= %d groups)", M, gn_rows, N, gn_cg, FIN_GN_G);
    FinGn gn;
    gn.stats = reinterpret_cast<unsigned long long*>(gn_stats); gn.rows = gn_rows; gn.cg = gn_cg;
    int k0, k1;
    gn_fixed_scales((long)gn_rows * gn_cg, 0, k0, k1);
    gn.m0 = exp2f((float)k0); gn.m1 = exp2f((float)k1);
    const int blocks = (int)std::min<long>(((long)M * N / 4 + 255) / 256, 4096);
    DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((gemm_finalize_kernel<T, true>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, acc, nsplit,
                                             (long)slab_stride, (T*)C, (float*)nullptr, 0, M, N, ldc, bias, rowvec, rv_ld,
                                             rv_rows_per_group, rv_mod, (const T*)res, ldres, (const float*)nullptr, (float*)nullptr, 0, gn));
    SVDX_LAUNCH_CHECK("svdx_gemm_finalize_gn");
    return 0;
}

extern "C" int svdx_outer_acc(const float* dY, const float* X, float* dW, int M, int N, int K, float scale, void* stream) {
    SVDX_CHECK_ARG(dY && X && dW && M > 0 && N > 0 && K > 0, "svdx_outer_acc: bad args");
    const size_t n = (size_t)N * K;
    hipLaunchKernelGGL(outer_acc_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, dY, X, dW, M, N, K, scale);
    SVDX_LAUNCH_CHECK("svdx_outer_acc");
    return 0;
}

extern "C" int svdx_small_linear_batch(const svdx_lin_job* jobs, int n_jobs, int M, int trans, int dtype, void* stream) {
    SVDX_CHECK_ARG(jobs && n_jobs > 0 && M > 0, "svdx_small_linear_batch: bad args");
    hipStream_t st = (hipStream_t)stream;
    for (int j0 = 0; j0 < n_jobs; j0 += SVDX_BATCH_MAX_JOBS) {
        LinPack pk;
        pk.n_jobs = std::min(n_jobs - j0, SVDX_BATCH_MAX_JOBS);
        int blocks = 0;
        for (int j = 0; j < pk.n_jobs; ++j) {
            const svdx_lin_job& q = jobs[j0 + j];
            SVDX_CHECK_ARG(q.X && q.W && q.Y && q.N > 0 && q.K > 0, "svdx_small_linear_batch: job %d: bad args", j0 + j);
            SVDX_CHECK_ARG(q.K % 8 == 0 && q.ldw % 8 == 0 && ((uintptr_t)q.W & 15) == 0,
                           "svdx_small_linear_batch: job %d: K/ldw must be multiples of 8", j0 + j);
            if (trans == 0)
                SVDX_CHECK_ARG(((uintptr_t)q.X & 15) == 0, "svdx_small_linear_batch: job %d: X must be 16-byte aligned", j0 + j);
            else
                SVDX_CHECK_ARG(!q.bias && !(q.flags & 1), "svdx_small_linear_batch: trans=1 takes no bias/activation");
            pk.job[j] = q;
            pk.start[j] = blocks;
            blocks += trans == 0 ? cdiv(q.N, 4) : cdiv(q.K / 8, 8);
        }
        for (int j = pk.n_jobs; j <= SVDX_BATCH_MAX_JOBS; ++j) pk.start[j] = blocks;
        DISPATCH_DTYPE(dtype, {
            if (trans == 0) {
                if (M == 1) hipLaunchKernelGGL((small_linear_nt_batch<T, 1>), dim3(blocks), dim3(256), 0, st, pk, M);
                else if (M <= 4) hipLaunchKernelGGL((small_linear_nt_batch<T, 4>), dim3(blocks), dim3(256), 0, st, pk, M);
                else hipLaunchKernelGGL((small_linear_nt_batch<T, 8>), dim3(blocks), dim3(256), 0, st, pk, M);
            } else {
                hipLaunchKernelGGL((small_linear_nn_batch<T>), dim3(blocks, M), dim3(256), 0, st, pk, M);
            }
        });
        SVDX_LAUNCH_CHECK("svdx_small_linear_batch");
    }
    return 0;
}

extern "C" int svdx_outer_acc_batch(const svdx_outer_job* jobs, int n_jobs, int M, void* stream) {
    SVDX_CHECK_ARG(jobs && n_jobs > 0 && M > 0, "svdx_outer_acc_batch: bad args");
    for (int j0 = 0; j0 < n_jobs; j0 += SVDX_BATCH_MAX_JOBS) {
        OuterPack pk;
        pk.n_jobs = std::min(n_jobs - j0, SVDX_BATCH_MAX_JOBS);
        long blocks = 0;
        for (int j = 0; j < pk.n_jobs; ++j) {
            const svdx_outer_job& q = jobs[j0 + j];
            SVDX_CHECK_ARG(q.dY && q.dW && q.N > 0 && q.K > 0 && (q.X || q.K == 1), "svdx_outer_acc_batch: job %d: bad args", j0 + j);
            pk.job[j] = q;
            pk.start[j] = (int)blocks;
            blocks += cdiv((size_t)q.N * q.K, 256);
            SVDX_CHECK_ARG(blocks < (1l << 31), "svdx_outer_acc_batch: too many workgroups");
        }
        for (int j = pk.n_jobs; j <= SVDX_BATCH_MAX_JOBS; ++j) pk.start[j] = (int)blocks;
        hipLaunchKernelGGL(outer_acc_batch_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, pk, M);
        SVDX_LAUNCH_CHECK("svdx_outer_acc_batch");
    }
    return 0;
}

extern "C" int svdx_grad_finalize_batch(const svdx_gradfin_job* jobs, int n_jobs, void* stream) {
    SVDX_CHECK_ARG(jobs && n_jobs > 0, "svdx_grad_finalize_batch: bad args");
    for (int j0 = 0; j0 < n_jobs; j0 += SVDX_BATCH_MAX_JOBS) {
        GradFinPack pk;
        pk.n_jobs = std::min(n_jobs - j0, SVDX_BATCH_MAX_JOBS);
        long blocks = 0;
        for (int j = 0; j < pk.n_jobs; ++j) {
            const svdx_gradfin_job& q = jobs[j0 + j];
            SVDX_CHECK_ARG(q.acc && q.dst && q.nsplit >= 1 && q.count > 0 && q.count % 4 == 0 && q.slab_stride % 4 == 0 &&
                               (((uintptr_t)q.acc | (uintptr_t)q.dst) & 15) == 0 && (!q.colsum_slabs || (q.colsum_out && q.colsum_n > 0)),
                           "svdx_grad_finalize_batch: job %d: bad args", j0 + j);
            pk.job[j] = q;
            pk.start[j] = (int)blocks;
            blocks += std::min<long>(cdiv(q.count / 4, 256), 1024);
        }
        for (int j = pk.n_jobs; j <= SVDX_BATCH_MAX_JOBS; ++j) pk.start[j] = (int)blocks;
        hipLaunchKernelGGL(grad_finalize_batch_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, pk);
        SVDX_LAUNCH_CHECK("svdx_grad_finalize_batch");
    }
    return 0;
}

extern "C" int svdx_timestep_embed(const float* t, float* out, int n, int dim, void* stream) {
    SVDX_CHECK_ARG(t && out && n > 0 && dim > 0 && dim % 2 == 0, "svdx_timestep_embed: bad args");
    hipLaunchKernelGGL(timestep_embed_kernel, dim3(cdiv((long)n * dim / 2, 256)), dim3(256), 0, (hipStream_t)stream, t, out,
                       n, dim);
    SVDX_LAUNCH_CHECK("svdx_timestep_embed");
    return 0;
}
