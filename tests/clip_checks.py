"""Gradient-norm clipping (Trainer(max_grad_norm=...), include/svdx.h svdx_grad_sumsq_spans / svdx_grad_clip_coef): the pieces the CPU
tests (test_clip_grad_norm.py) and the GPU tests (test_clip_grad_norm_gpu.py) share -- span tables, seeded inputs, the torch reference of
the reference-dtype LoRA recipe, and the emulation of the two entries for host-logic tests."""
import math

import torch

import emul
from svd_xtend_amd import kernels as K

FLT_MIN = 2.0 ** -126


def span_rows(sizes, offsets=None, chunk=K.CLIP_SPAN_FLOATS):
    """(offset, count, tensor) rows for tensors of `sizes` floats at `offsets` (default: packed at 64-float alignment), chunked as the
    Trainer chunks them.  Returns (rows, offsets, total floats)."""
    rows, offs, pos = [], [], 0
    for i, n in enumerate(sizes):
        off = offsets[i] if offsets is not None else pos
        offs.append(off)
        rows += [(off + c, min(chunk, n - c), i) for c in range(0, n, chunk)]
        pos = max(pos, -(-(off + n) // 64) * 64)
    return rows, offs, pos


def rb16_f64(x: float) -> float:
    """x >= 0 correctly rounded to bf16 from float64 (ties to even), as the kernel's rb16_f64."""
    if not math.isfinite(x) or x == 0.0:
        return x
    e = max(math.frexp(x)[1] - 1, -126)
    q = 2.0 ** (e - 7)
    return torch.tensor(round(x / q) * q, dtype=torch.float64).float().item()


def rb16(x: float) -> float:
    return torch.tensor(x, dtype=torch.float32).to(torch.bfloat16).float().item()


def f32(x: float) -> float:
    return torch.tensor(x, dtype=torch.float64).float().item()


def coef_from_sums(tensor_sums, max_norm, unscale, ref):
    """(total_norm, coef) from per-tensor float64 sums of squares, the arithmetic svdx_grad_clip_coef documents."""
    if ref:
        tot = sum(rb16_f64(math.sqrt(s) * unscale) ** 2 for s in tensor_sums)
        norm = rb16_f64(math.sqrt(tot))
        coef = rb16(rb16(f32(1.0 / rb16(f32(norm + rb16_f64(1e-6))))) * f32(max_norm))
    else:
        norm = f32(math.sqrt(sum(tensor_sums)) * unscale)
        coef = f32(max_norm / (norm + 1e-6))
    return norm, (1.0 if coef > 1.0 else coef)


class ClipEmuBackend(emul.EmuBackend):
    """tests/emul.py's emulation plus the two clipping entries (float64 on the host, the kernels' arithmetic), counting their calls."""

    def __init__(self):
        super().__init__()
        self.clip_calls = []

    def grad_sumsq_spans(self, g, spans, n_spans, partial):
        self.clip_calls.append("svdx_grad_sumsq_spans")
        flat = g.reshape(-1)
        for s, (off, cnt, _) in enumerate(spans[:n_spans].view(-1, 3).tolist()):
            partial[s] = flat[off:off + cnt].double().pow(2).sum()

    def grad_clip_coef(self, partial, spans, n_spans, n_tensors, max_norm, grad_mul, opt_state, out, param_mode=K.PARAMS_F32):
        self.clip_calls.append("svdx_grad_clip_coef")
        sums = [0.0] * n_tensors
        for s, (_, _, t) in enumerate(spans[:n_spans].view(-1, 3).tolist()):
            sums[t] += float(partial[s])
        norm, coef = coef_from_sums(sums, max_norm, float(opt_state[4]) * grad_mul, param_mode == K.PARAMS_BF16_REFERENCE)
        out[0], out[1] = norm, coef
        if not float(opt_state[7]) > 0:
            opt_state[4] = opt_state[4] * torch.tensor(coef, dtype=torch.float32)


# ---- the reference-dtype LoRA pin: torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW on bf16 tensors -----------------------------------
PIN_SEED = 0
PIN_LR, PIN_BETAS, PIN_WD, PIN_EPS = 1e-3, (0.9, 0.999), 1e-2, 1e-8


def pin_grads(shapes, seed=PIN_SEED):
    """Seeded bf16 gradients of the given shapes, with per-tensor magnitudes spread over three decades."""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for i, s in enumerate(shapes):
        scale = 10.0 ** (-3 + 3 * torch.rand((), generator=gen).item())
        out.append((torch.randn(s, generator=gen) * scale).to(torch.bfloat16))
    return out


def foreach_norm_mismatches(grads):
    """The pin's precondition: indices where torch's bf16 per-tensor norm differs from the correctly rounded one."""
    got = torch._foreach_norm(list(grads), 2.0)
    return [i for i, (g, n) in enumerate(zip(grads, got))
            if float(n) != rb16_f64(math.sqrt(float(g.double().pow(2).sum())))]


def torch_clip_adamw(params, grads, max_norm):
    """One step of the reference's recipe on bf16 tensors: clip_grad_norm_(params, max_norm), then torch.optim.AdamW.  Returns
    (params, exp_avg, exp_avg_sq, total_norm) as float tensors / a float."""
    ps = [torch.nn.Parameter(p.clone().to(torch.bfloat16)) for p in params]
    for p, g in zip(ps, grads):
        p.grad = g.clone()
    opt = torch.optim.AdamW(ps, lr=PIN_LR, betas=PIN_BETAS, weight_decay=PIN_WD, eps=PIN_EPS)
    total = torch.nn.utils.clip_grad_norm_(ps, max_norm)
    opt.step()
    return ([p.detach().float() for p in ps], [opt.state[p]["exp_avg"].float() for p in ps],
            [opt.state[p]["exp_avg_sq"].float() for p in ps], float(total))
