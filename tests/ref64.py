"""Float64 references of the libsvdx entry families, written from torch's own operators and autograd (not from tests/emul.py).

Every function takes LOGICAL tensors (the caller has already resolved pointers, pitches and aliasing), works in float64 on whatever
device they are on, rounds nothing, and -- for the sum-shaped entries -- also returns the magnitude sum S (the same expression with
every term replaced by its absolute value) that the error model of tests/census.py needs.  Backward passes are `torch.autograd.grad`
of the float64 forward.
"""
import math

import torch
import torch.nn.functional as F

from svd_xtend_amd import kernels as K


def d(t):
    return None if t is None else t.to(torch.float64)


# ---- implicit-GEMM gathers as convolutions ------------------------------------------------------------------------------------------
def gather_matmul(src, W, g: K.Gather, M):
    """[M, N] = gathered(src) @ W^T for the addressing modes of svdx_gather.  src: [source rows, cin]; W: [N, taps * cin] with the
    reduction index k = tap * cin + c, tap = dy * 3 + dx (frames before / same / after for the temporal mode)."""
    src, W = d(src), d(W)
    N, cin = W.shape[0], g.cin
    if g.mode == K.GATHER_TEMPORAL3:
        x = src.view(g.n_img, g.t, g.hw, cin).permute(0, 2, 3, 1).reshape(g.n_img * g.hw, cin, g.t)
        y = F.conv1d(x, W.view(N, 3, cin).permute(0, 2, 1).contiguous(), padding=1)                    # [B*hw, N, T]
        return y.view(g.n_img, g.hw, N, g.t).permute(0, 3, 1, 2).reshape(M, N)
    w4 = W.view(N, 3, 3, cin).permute(0, 3, 1, 2).contiguous()                                          # [N, cin, 3, 3]
    if g.mode == K.GATHER_CONV3X3_DGRAD2:            # data gradient of the stride-2 convolution: (hi, wi) is the SMALL grid here
        x = src.view(g.n_img, g.hi, g.wi, cin).permute(0, 3, 1, 2)
        op = (g.ho - (2 * g.hi - 1), g.wo - (2 * g.wi - 1))
        y = F.conv_transpose2d(x, w4.permute(1, 0, 2, 3).contiguous(), stride=2, padding=1, output_padding=op)
        return y.permute(0, 2, 3, 1).reshape(M, N)
    assert g.mode in (K.GATHER_CONV3X3, K.GATHER_CONV3X3_PAD0)
    pad = 1 if g.mode == K.GATHER_CONV3X3 else 0
    if g.ups:
        x = src.view(g.n_img, g.hi // 2, g.wi // 2, cin).permute(0, 3, 1, 2)
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    else:
        x = src.view(g.n_img, g.hi, g.wi, cin).permute(0, 3, 1, 2)
    # zero border of `pad` at the top / left; as much at the bottom / right as the (ho, wo) outputs reach
    pb, pr = (g.ho - 1) * g.stride + 3 - g.hi - pad, (g.wo - 1) * g.stride + 3 - g.wi - pad
    x = F.pad(x, (pad, pr, pad, pb))
    y = F.conv2d(x, w4, stride=g.stride)
    assert y.shape[2:] == (g.ho, g.wo), (y.shape, g)
    return y.permute(0, 2, 3, 1).reshape(M, N)


def group_index(M, rpg, mod, dev):
    m = torch.arange(M, device=dev)
    return (m % mod) if mod else torch.div(m, rpg, rounding_mode="floor")


def gemm_nt(A, B, M, alpha=1.0, gather=None, dual=None, bias=None, rowvec=None, rv_rpg=0, rv_mod=0, res=None, c0=None):
    """alpha (A B^T + A2 B2^T) + bias + rowvec[group of the row] + res (+ c0, the accumulate forms).  dual = (A2 [M, K2 or nseg*K2],
    B2 [N, K2], seg): with seg, column block j of the output takes columns j*K2..(j+1)*K2 of A2.  Returns (value, S, number of
    accumulated products, number of epilogue terms)."""
    def prod(a, b, a2, b2):
        v = gather_matmul(a, b, gather, M) if gather is not None and gather.mode != K.GATHER_PLAIN else a @ b.t()
        if a2 is not None:
            seg, K2 = dual[2], b2.shape[1]
            if seg:
                v = v + torch.cat([a2[:, j * K2:(j + 1) * K2] @ b2[j * seg:(j + 1) * seg].t() for j in range(b2.shape[0] // seg)], 1)
            else:
                v = v + a2 @ b2.t()
        return v
    A, B = d(A), d(B)
    A2, B2 = (d(dual[0]), d(dual[1])) if dual is not None else (None, None)
    v = alpha * prod(A, B, A2, B2)
    S = abs(alpha) * prod(A.abs(), B.abs(), None if A2 is None else A2.abs(), None if B2 is None else B2.abs())
    k_acc, e = B.shape[1] + (B2.shape[1] if B2 is not None else 0), 1
    terms = [None if bias is None else d(bias)[None],
             None if rowvec is None else d(rowvec)[group_index(M, rv_rpg, rv_mod, A.device)], d(res), d(c0)]
    for t in terms:
        if t is not None:
            v, S, e = v + t, S + t.abs(), e + 1
    return v, S, k_acc, e


def gemm_tn(A, B):
    """A^T B over the rows: ([N, K] value, S, rows)."""
    A, B = d(A), d(B)
    return A.t() @ B, A.abs().t() @ B.abs(), A.shape[0]


def slab_sum(slabs, extra=()):
    """sum of float slabs [nsplit, ...] plus further terms: (value, S, terms)."""
    v, S = d(slabs).sum(0), d(slabs).abs().sum(0)
    n = slabs.shape[0]
    for t in extra:
        if t is not None:
            v, S, n = v + d(t), S + d(t).abs(), n + 1
    return v, S, n


def geglu(pre, Fd):
    p = d(pre)
    return p[:, :Fd] * F.gelu(p[:, Fd:])


@torch.enable_grad()
def geglu_bwd(dh, pre, Fd):
    """d(pre) of h = a * gelu(g) for the upstream gradient dh: autograd of the float64 forward."""
    p = d(pre).clone().requires_grad_(True)
    (gp,) = torch.autograd.grad(geglu(p, Fd), p, d(dh))
    return gp


# ---- norms ---------------------------------------------------------------------------------------------------------------------------
def _gn_layout(x, n_s, rows, C):
    return d(x).view(n_s, rows, C).permute(0, 2, 1)                     # [n_s, C, rows]: channels second, as F.group_norm wants


def gn_sums(x, n_s, rows, C, G):
    xf = d(x).view(n_s, rows, G, C // G)
    return xf.sum((1, 3)), (xf * xf).sum((1, 3))


def gn_fwd(x, gamma, beta, n_s, rows, C, G, eps, silu):
    y = F.group_norm(_gn_layout(x, n_s, rows, C), G, d(gamma), d(beta), eps)
    if silu:
        y = F.silu(y)
    return y.permute(0, 2, 1).reshape(n_s * rows, C)


def gn_fwd_S(x, gamma, beta, n_s, rows, C, G, eps):
    """(magnitude sum of the normalisation (|x| + |mean|) rstd |gamma| + |beta|, cond = E[x^2] / var of the element's group)"""
    xf = d(x).view(n_s, rows, G, C // G)
    mean = xf.mean((1, 3), keepdim=True)
    var = xf.var((1, 3), unbiased=False, keepdim=True)
    rstd = torch.rsqrt(var + eps)
    S = (((xf.abs() + mean.abs()) * rstd).reshape(n_s, rows, C) * d(gamma).abs() + d(beta).abs()).reshape(n_s * rows, C)
    cond = ((xf * xf).mean((1, 3), keepdim=True) / var.clamp(min=1e-300)).expand_as(xf).reshape(n_s * rows, C)
    return S, cond


@torch.enable_grad()
def gn_bwd(dy, x, gamma, beta, n_s, rows, C, G, eps, silu):
    """(dx, sum dz*gamma, sum dz*gamma*xhat per (sample, group)) -- the two sums are what svdx_gn_bwd_stats leaves."""
    x64 = d(x).clone().requires_grad_(True)
    y = gn_fwd(x64, gamma, beta, n_s, rows, C, G, eps, silu)
    (dx,) = torch.autograd.grad(y, x64, d(dy))
    # the statistics of the backward pass, through autograd as well: dz = d(loss)/d(pre-activation)
    xf = d(x).view(n_s, rows, G, C // G)
    mean = xf.mean((1, 3), keepdim=True)
    xhat = ((xf - mean) * torch.rsqrt(xf.var((1, 3), unbiased=False, keepdim=True) + eps)).reshape(n_s * rows, C)
    z = (xhat * d(gamma) + d(beta)).requires_grad_(True)
    (dz,) = torch.autograd.grad(F.silu(z) if silu else z * 1.0, z, d(dy))
    dzg = (dz * d(gamma)).view(n_s, rows, G, C // G)
    return dx, dzg.sum((1, 3)), (dzg * xhat.view(n_s, rows, G, C // G)).sum((1, 3))


def gn_bwd_magnitudes(dy, x, gamma, beta, n_s, rows, C, G, eps, silu):
    """What the derived bound of dx = rstd (dz gamma - (s1 + xhat s2) / count) needs, [n_s * rows, C] each:
    S    = rstd (|dz gamma| + (|s1| + |xhat| |s2|) / count), the magnitude sum;
    amp  = what one relative fp32 rounding of (|x| + |mean|) rstd -- the cancellation inside xhat -- moves dx by: through xhat s2 / count
           and, with SiLU, through silu'(z) (|silu''| <= 1/2, dz / dxhat = gamma);
    cond = E[x^2] / var of the element's group: the variance comes from the two sums, one rounding of E[x^2] is cond roundings of var."""
    _, s1, s2 = gn_bwd(dy, x, gamma, beta, n_s, rows, C, G, eps, silu)
    cnt = rows * (C // G)
    xf = d(x).view(n_s, rows, G, C // G)
    mean = xf.mean((1, 3), keepdim=True)
    var = xf.var((1, 3), unbiased=False, keepdim=True)
    rstd = torch.rsqrt(var + eps)
    xhat = (xf - mean) * rstd
    g4 = d(gamma).view(1, 1, G, C // G)
    with torch.enable_grad():
        z = (xhat * g4 + d(beta).view(1, 1, G, C // G)).requires_grad_(True)
        (dz,) = torch.autograd.grad(F.silu(z) if silu else z * 1.0, z, d(dy).view(n_s, rows, G, C // G))
    a1, a2 = s1.abs()[:, None, :, None], s2.abs()[:, None, :, None]
    S = rstd * ((dz * g4).abs() + (a1 + xhat.abs() * a2) / cnt)
    dxh = (xf.abs() + mean.abs()) * rstd
    amp = dxh * rstd * (a2 / cnt + (0.5 * d(dy).view(n_s, rows, G, C // G).abs() * g4 * g4 if silu else 0.0))
    cond = ((xf * xf).mean((1, 3), keepdim=True) / var.clamp(min=1e-300)).expand_as(S)
    return S.reshape(n_s * rows, C), amp.reshape(n_s * rows, C), cond.reshape(n_s * rows, C)


def ln_fwd(x, gamma, beta, eps):
    x = d(x)
    y = F.layer_norm(x, (x.shape[1],), d(gamma), d(beta), eps)
    mean = x.mean(1)
    rstd = torch.rsqrt(x.var(1, unbiased=False) + eps)
    S = (x.abs() + mean.abs()[:, None]) * rstd[:, None] * d(gamma).abs() + d(beta).abs()
    return y, mean, rstd, S


@torch.enable_grad()
def ln_bwd(dy, x, gamma, eps):
    """(dx, dgamma, dbeta, S_dgamma, S_dbeta) through autograd of F.layer_norm in float64"""
    x64 = d(x).clone().requires_grad_(True)
    g64 = d(gamma).clone().requires_grad_(True)
    b64 = torch.zeros_like(g64, requires_grad=True)
    y = F.layer_norm(x64, (x64.shape[1],), g64, b64, eps)
    dx, dg, db = torch.autograd.grad(y, (x64, g64, b64), d(dy))
    xhat = F.layer_norm(d(x), (x64.shape[1],), None, None, eps)
    return dx, dg, db, (d(dy) * xhat).abs().sum(0), d(dy).abs().sum(0)


def ln_bwd_magnitudes(dy, x, gamma, eps):
    """For the derived bound of dx = rstd (g - mean(g) - xhat mean(g xhat)), g = dy gamma, [rows, C] each:
    S = rstd (|g| + mean|g| + |xhat| mean|g xhat|); red = the part of S that comes out of the two row reductions;
    amp = what one relative fp32 rounding of (|x| + |mean|) rstd (the cancellation inside xhat) moves dx by."""
    x, g = d(x), d(dy) * d(gamma)
    mean = x.mean(1, keepdim=True)
    rstd = torch.rsqrt(x.var(1, unbiased=False, keepdim=True) + eps)
    xhat = (x - mean) * rstd
    dxh = (x.abs() + mean.abs()) * rstd
    red = rstd * (g.abs().mean(1, keepdim=True) + xhat.abs() * (g * xhat).abs().mean(1, keepdim=True))
    amp = rstd * (dxh * (g * xhat).abs().mean(1, keepdim=True) + xhat.abs() * (g.abs() * dxh).mean(1, keepdim=True))
    return rstd * g.abs() + red, red, amp


# ---- attention -----------------------------------------------------------------------------------------------------------------------
def attention(q, k, v, scale):
    """softmax(q k^T scale) v over the second-last axis of [..., S, 64] operands: (o, lse, P|V|, max_j scale |q|.|k_j|)"""
    q, k, v = d(q), d(k), d(v)
    s = (q @ k.transpose(-1, -2)) * scale
    lse = torch.logsumexp(s, -1)
    p = torch.softmax(s, -1)
    return p @ v, lse, p @ v.abs(), ((q.abs() @ k.abs().transpose(-1, -2)) * scale).amax(-1)


@torch.enable_grad()
def attention_bwd(q, k, v, d_o, scale):
    """(dq, dk, dv, o) through autograd of F.scaled_dot_product_attention's definition in float64"""
    q, k, v = (d(t).clone().requires_grad_(True) for t in (q, k, v))
    o = torch.softmax((q @ k.transpose(-1, -2)) * scale, -1) @ v
    dq, dk, dv = torch.autograd.grad(o, (q, k, v), d(d_o))
    return dq, dk, dv, o.detach()


# ---- loss / optimizer ----------------------------------------------------------------------------------------------------------------
@torch.enable_grad()
def edm_loss(pred, noisy, target, sigma, loss_scale):
    """EDM-weighted mean squared error of the denoised prediction and the gradient of (loss_scale * loss) w.r.t. pred.
    pred / noisy / target: [B, T, C, HW]; sigma [B].  Returns (loss, dpred, S_loss, S_dpred)."""
    p = d(pred).clone().requires_grad_(True)
    s = d(sigma)[:, None, None, None]
    c_out, c_skip, wgt = -s / torch.sqrt(s * s + 1), 1 / (s * s + 1), (1 + s * s) / (s * s)
    den = c_out * p + c_skip * d(noisy)
    loss = (wgt * (den - d(target)) ** 2).mean()
    (dp,) = torch.autograd.grad(loss * loss_scale, p)
    mag = (c_out * p).abs() + (c_skip * d(noisy)).abs() + d(target).abs()
    S_dp = (2 * wgt * c_out.abs() * loss_scale / p.numel()) * mag
    return loss.detach(), dp, (wgt * mag * mag).mean().detach(), S_dp.detach()


@torch.enable_grad()
def adamw_step(p, g, m, v, lr, beta1, beta2, eps, wd, step):
    """One torch.optim.AdamW step on float64 tensors whose state says `step - 1` steps were taken: (p, m, v) afterwards."""
    par = torch.nn.Parameter(d(p).clone())
    par.grad = d(g).clone()
    opt = torch.optim.AdamW([par], lr=lr, betas=(beta1, beta2), eps=eps, weight_decay=wd, foreach=False)
    opt.state[par] = dict(step=torch.tensor(float(step - 1)), exp_avg=d(m).clone(), exp_avg_sq=d(v).clone())
    opt.step()
    st = opt.state[par]
    return par.detach(), st["exp_avg"], st["exp_avg_sq"]


def timestep_embed(t, dim):
    half = dim // 2
    f = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float64, device=t.device) / half)
    arg = d(t)[:, None] * f[None]
    return torch.cat([torch.cos(arg), torch.sin(arg)], 1), torch.cat([arg, arg], 1).abs()


# ---- the conditioners' kernels ----------------------------------------------------------------------------------------------------------
def patch_rows(x, kh, kw, stride, pad, ldk, mul):
    """im2col rows [n*ho*wo, ldk] of x [n, C, H, W]: F.unfold's order k = (c*kh + dy)*kw + dx, zero padding, times `mul` as the float the
    binding passes; the columns C*kh*kw .. ldk are zero."""
    n, C = x.shape[:2]
    m = float(torch.tensor(mul, dtype=torch.float32))
    cols = F.unfold(d(x) * m, (kh, kw), padding=pad, stride=stride)                    # [n, C*kh*kw, ho*wo]
    out = torch.zeros(n * cols.shape[2], ldk, dtype=torch.float64, device=x.device)
    out[:, :C * kh * kw] = cols.permute(0, 2, 1).reshape(-1, C * kh * kw)
    return out


def act(x, kind):
    """0: exact-erf GELU, 1: x sigmoid(1.702 x) (CLIP's quick_gelu)"""
    x = d(x)
    return F.gelu(x) if kind == 0 else x * torch.sigmoid(1.702 * x)


def ema_lerp(s, p, omd):
    """(shadow - omd (shadow - p), its magnitude sum)"""
    s, p = d(s), d(p)
    return s - omd * (s - p), s.abs() + abs(omd) * (s.abs() + p.abs())


def blur_axis(x, taps, axis):
    """x [planes, H, W]; odd tap count, reflect padding; axis 0 = along W, 1 = along H: (value, magnitude sum)"""
    half = (taps.numel() - 1) // 2
    x4, t = d(x)[:, None], d(taps)
    if axis == 0:
        f = lambda v, w: F.conv2d(F.pad(v, (half, half, 0, 0), mode="reflect"), w.view(1, 1, 1, -1))
    else:
        f = lambda v, w: F.conv2d(F.pad(v, (0, 0, half, half), mode="reflect"), w.view(1, 1, -1, 1))
    return f(x4, t)[:, 0], f(x4.abs(), t.abs())[:, 0]


def bicubic_affine(x, ho, wo, scale, shift):
    """torch's bicubic (A = -0.75) with align_corners=True, then the per-channel affine; x [n, C, H, W]"""
    C = x.shape[1]
    return F.interpolate(d(x), size=(ho, wo), mode="bicubic", align_corners=True) * d(scale).view(1, C, 1, 1) + d(shift).view(1, C, 1, 1)


def _cubic(t, A=-0.75):
    """(|weights|, |d weight / dt|) of the four taps at fraction t, [len, 4]"""
    x0, x1, x2, x3 = t + 1, t, 1 - t, 2 - t
    outer = lambda x: ((A * x - 5 * A) * x + 8 * A) * x - 4 * A
    inner = lambda x: ((A + 2) * x - (A + 3)) * x * x + 1
    douter = lambda x: (3 * A * x - 10 * A) * x + 8 * A
    dinner = lambda x: (3 * (A + 2) * x - 2 * (A + 3)) * x
    w = torch.stack([outer(x0), inner(x1), inner(x2), outer(x3)], 1)
    dw = torch.stack([douter(x0), dinner(x1), dinner(x2), douter(x3)], 1)
    return w.abs(), dw.abs()


def bicubic_magnitudes(x, ho, wo):
    """What the bound of the bicubic resize needs beside the value, [n, C, ho, wo] each: S = sum |wy| |wx| |x| over the 4 x 4 taps;
    pos = the same sum with one axis' weights replaced by |dw/dt| times the source coordinate (an error of 2^-23 of the coordinate in t);
    wgt = with one axis' weights replaced by the largest partial sum of its Horner evaluation (36 outer taps, 4.5 inner)."""
    n, C, H, W = x.shape
    ax = d(x).abs()
    dev = x.device

    def axis(size, out):
        r = (size - 1) / (out - 1) if out > 1 else 0.0
        f = torch.arange(out, dtype=torch.float64, device=dev) * r
        i = torch.floor(f)
        w, dw = _cubic(f - i)
        idx = (i.to(torch.int64)[:, None] + torch.arange(-1, 3, device=dev)[None]).clamp(0, size - 1)
        # a coordinate that fp32 puts on the other side of an integer: the weights are continuous there, the bound holds either way
        return idx, w, dw * f[:, None], torch.tensor([36.0, 4.5, 4.5, 36.0], dtype=torch.float64, device=dev).expand(out, 4)
    iy, wy, py, ey = axis(H, ho)
    ix, wx, px, ex = axis(W, wo)
    g = ax[:, :, iy][:, :, :, :, ix]                      # [n, C, ho, 4, wo, 4]
    comb = lambda a, b: torch.einsum("ncyaxb,ya,xb->ncyx", g, a, b)
    return comb(wy, wx), comb(py, wx) + comb(wy, px), comb(ey, wx) + comb(wy, ex)
