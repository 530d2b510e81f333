// conv_wgrad.hip -- the two layout kernels either side of a trainable convolution (svdx_conv_wgrad_finalize, svdx_conv_pack).
//
// The GEMMs see a convolution weight as [cout][tap][cin_p] (forward, k = tap * cin_p + ci: the order svdx_gather walks) and as
// [cin][tap][cout_p] (data gradient); the parameter, its gradient and the optimizer state are diffusers' [cout][cin][tap]
// (nn.Conv2d [cout, cin, 3, 3], nn.Conv3d [cout, cin, 3, 1, 1]).  Both kernels move between the two through an LDS tile, so that the reads
// and the writes both run along the contiguous index of their side.
#include "gemm_common.h"

namespace {

constexpr int CW_CI = 64;          // channels of one finalize workgroup
constexpr int CW_MAX_TAPS = 9;

// One workgroup: output channel n, input channels ci0 .. ci0 + 63, every tap.  Reads run along ci (contiguous in a slab row), writes
// along (ci, tap) (contiguous in the parameter); the LDS rows are `taps` floats apart -- 3 or 9, odd: no bank conflicts either way.
// The workgroups behind the last (n, ci block) reduce the column-sum slabs into the bias gradient.
__global__ __launch_bounds__(256) void conv_wgrad_finalize_kernel(const float* __restrict__ acc, int nsplit, long slab_stride, int ld_acc, float* __restrict__ wg,
                                                                  int cout, int cin, int cin_p, int taps, float alpha, int store,
                                                                  const float* __restrict__ cs, int cs_ld, float* __restrict__ bg, float* found_inf) {
    __shared__ float tile[CW_CI * CW_MAX_TAPS];
    const int tid = threadIdx.x;
    const int chunks = (cin + CW_CI - 1) / CW_CI;
    int blk = blockIdx.x;
    bool bad = false;
    if (blk >= cout * chunks) {                          // bias gradient: alpha * (sum of the slices' column sums), slice 0 first
        const int n = (blk - cout * chunks) * 256 + tid;
        if (n < cout) {
            float s = 0.f;
            for (int z = 0; z < nsplit; ++z) s += cs[(size_t)z * cs_ld + n];
            s *= alpha;
            if (!store) s += bg[n];
            bg[n] = s;
            bad = not_finite(s);
        }
        raise_found_inf(found_inf, bad);
        return;
    }
    const int n = blk / chunks, ci0 = (blk - n * chunks) * CW_CI;
    const int nci = min(CW_CI, cin - ci0);
    const float* row = acc + (size_t)n * ld_acc + ci0;
    for (int i = tid; i < taps * CW_CI; i += 256) {
        const int tap = i / CW_CI, c = i - tap * CW_CI;
        if (c >= nci) continue;
        float s = 0.f;
        for (int z = 0; z < nsplit; ++z) s += row[(size_t)z * slab_stride + tap * cin_p + c];
        tile[c * taps + tap] = s * alpha;
    }
    __syncthreads();
    float* dst = wg + ((size_t)n * cin + ci0) * taps;
    for (int i = tid; i < nci * taps; i += 256) {
        float v = tile[i];
        if (!store) v += dst[i];
        dst[i] = v;
        bad |= not_finite(v);
    }
    raise_found_inf(found_inf, bad);
}

constexpr int CP_T = 32;           // a pack workgroup owns 32 output x 32 input channels, every tap

// master [cout][cin][taps] (float) -> w [cout][taps][cin_p] and, when wd != null, wd [cin][taps][cout_p] (tap order reversed under `flip`),
// each element fl(master * out_scale) rounded ONCE to T; the padded channels of both forms are written as zeros.  bias_out (float, may be
// null) = bias * out_scale: the bias the forward adds, kept beside the scaled weights.
template <typename T>
__global__ __launch_bounds__(256) void conv_pack_kernel(const float* __restrict__ master, float out_scale, T* __restrict__ w, T* __restrict__ wd,
                                                        int cout, int cin, int taps, int cin_p, int cout_p, int flip,
                                                        const float* __restrict__ bias, float* __restrict__ bias_out) {
    __shared__ float tile[CP_T][CP_T * CW_MAX_TAPS + 1];
    const int tid = threadIdx.x;
    const int co0 = blockIdx.y * CP_T, ci0 = blockIdx.x * CP_T;
    const int run = CP_T * taps;                          // floats of one output channel's 32 input channels: contiguous in the master
    if (bias_out != nullptr && blockIdx.x == 0 && tid < CP_T && co0 + tid < cout) bias_out[co0 + tid] = bias[co0 + tid] * out_scale;
    for (int i = tid; i < CP_T * run; i += 256) {
        const int r = i / run, j = i - r * run;           // j = c * taps + tap
        const int co = co0 + r, ci = ci0 + j / taps;
        tile[r][j] = (co < cout && ci < cin) ? master[((size_t)co * cin + ci0) * taps + j] * out_scale : 0.f;
    }
    __syncthreads();
    for (int i = tid; i < CP_T * run; i += 256) {        // w: runs of 32 input channels
        const int c = i % CP_T, t = i / CP_T, tap = t % taps, r = t / taps;
        const int co = co0 + r, ci = ci0 + c;
        if (co < cout && ci < cin_p) w[((size_t)co * taps + tap) * cin_p + ci] = from_f<T>(tile[r][c * taps + tap]);
    }
    if (wd == nullptr) return;
    for (int i = tid; i < CP_T * run; i += 256) {        // wd: runs of 32 output channels
        const int r = i % CP_T, t = i / CP_T, tap = t % taps, c = t / taps;
        const int co = co0 + r, ci = ci0 + c;
        if (ci < cin && co < cout_p) wd[((size_t)ci * taps + tap) * cout_p + co] = from_f<T>(tile[r][c * taps + (flip ? taps - 1 - tap : tap)]);
    }
}

}  // namespace

extern "C" int svdx_conv_wgrad_finalize(const float* acc, int nsplit, int64_t slab_stride, int ld_acc, float* w_grad, int cout, int cin, int cin_p,
                                        int taps, float alpha, int store, const float* colsum_slabs, int colsum_ld, float* b_grad,
                                        float* found_inf, void* stream) {
    SVDX_CHECK_ARG(acc && w_grad && nsplit >= 1 && cout > 0 && cin > 0, "svdx_conv_wgrad_finalize: bad args");
    SVDX_CHECK_ARG(taps == 3 || taps == 9, "svdx_conv_wgrad_finalize: taps=%d (3: temporal, 9: 3x3)", taps);
    SVDX_CHECK_ARG(cin_p >= cin && ld_acc >= taps * cin_p && (nsplit == 1 || slab_stride >= (int64_t)cout * ld_acc),
                   "svdx_conv_wgrad_finalize: cin_p=%d ld_acc=%d slab_stride=%ld do not hold [cout=%d][%d * cin_p]", cin_p, ld_acc, (long)slab_stride, cout, taps);
    SVDX_CHECK_ARG((colsum_slabs == nullptr) == (b_grad == nullptr) && (!b_grad || colsum_ld >= cout), "svdx_conv_wgrad_finalize: colsum_slabs and b_grad go together, colsum_ld >= cout");
    const long blocks = (long)cout * cdiv(cin, CW_CI) + (b_grad ? cdiv(cout, 256) : 0);
    SVDX_CHECK_ARG(blocks <= 0x7fffffffL, "svdx_conv_wgrad_finalize: too many workgroups");
    hipLaunchKernelGGL(conv_wgrad_finalize_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, acc, nsplit, (long)slab_stride, ld_acc, w_grad,
                       cout, cin, cin_p, taps, alpha, store, colsum_slabs, colsum_ld, b_grad, found_inf);
    SVDX_LAUNCH_CHECK("svdx_conv_wgrad_finalize");
    return 0;
}

extern "C" int svdx_conv_pack(const float* master, float out_scale, void* w, void* wd, int cout, int cin, int taps, int cin_p, int cout_p,
                              int flip, const float* bias, float* bias_out, int dtype, void* stream) {
    SVDX_CHECK_ARG(master && w && cout > 0 && cin > 0, "svdx_conv_pack: bad args");
    SVDX_CHECK_ARG(taps == 1 || taps == 3 || taps == 9, "svdx_conv_pack: taps=%d (1, 3 or 9)", taps);
    SVDX_CHECK_ARG(cin_p >= cin && (!wd || cout_p >= cout), "svdx_conv_pack: padded channel counts below the real ones");
    SVDX_CHECK_ARG(!bias_out || (bias && bias != bias_out), "svdx_conv_pack: bias_out needs a bias of its own to scale");
    dim3 grid((unsigned)cdiv(cin_p, CP_T), (unsigned)cdiv(wd ? cout_p : cout, CP_T));      // the tiles cover the padded channels of both forms
    SVDX_CHECK_ARG(grid.y <= 65535u, "svdx_conv_pack: too many output channels");
    DISPATCH_DTYPE(dtype, {
        hipLaunchKernelGGL(conv_pack_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, master, out_scale, reinterpret_cast<T*>(w),
                           reinterpret_cast<T*>(wd), cout, cin, taps, cin_p, cout_p, flip, bias, bias_out);
        SVDX_LAUNCH_CHECK("svdx_conv_pack");
        return 0;
    });
}
