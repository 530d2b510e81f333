"""Gradient-norm clipping (Trainer(max_grad_norm=...), include/svdx.h svdx_grad_sumsq_spans / svdx_grad_clip_coef): the pieces the CPU
tests (test_clip_grad_norm.py) and the GPU tests (test_clip_grad_norm_gpu.py) share -- span tables, seeded inputs, the torch reference of
the reference-dtype LoRA recipe.  The emulation of the two entries is emul.EmuBackend's, and its arithmetic (coef_from_sums and the
roundings) is imported back from there."""
import math

import torch

from emul import coef_from_sums, f32, rb16, rb16_f64  # noqa: F401
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
