"""Gradient-norm clipping on the MI355X (`-m gpu`): svdx_grad_sumsq_spans / svdx_grad_clip_coef at the size of config 2's trainable buffer,
Trainer(max_grad_norm=...) on the tiny topology in fp16 and bf16, the reference-dtype LoRA recipe pinned to torch, and the captured step
(GraphedStep, its launch plan, grad_accum = 2) against eager steps.  The bars are those derived in test_clip_grad_norm.py."""
import math
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import clip_checks as cc  # noqa: E402
from svd_xtend_amd import kernels as K  # noqa: E402

SUM_REL = 1e-11
COEF_REL = 2.0 ** -22
M_REL = 2.0 ** -21
C2_TRAINABLE_FLOATS = 397_620_480          # config 2's flat gradient buffer
DEV = torch.device("cuda")


def _state(inv_scale=1.0):
    st = torch.zeros(K.OPT_STATE_ALLOC, device=DEV)
    st[1], st[4], st[5], st[6], st[8] = 1.0, inv_scale, 1.0, 1.0, 1.0
    return st


@pytest.mark.gpu
def test_kernels_at_the_c2_size():
    """397,620,480 floats over a wide exponent range (tensors of 13.1 M floats, the remainder, small odd sizes) against torch's float64
    sums on the device; the same bits on a second run."""
    be = K.backend()
    sizes = [13_107_200] * 30 + [C2_TRAINABLE_FLOATS - 30 * 13_107_200, 5, 7, 130, 1, 3001, 65_536 + 3]
    rows, offs, n = cc.span_rows(sizes)
    gen = torch.Generator(device=DEV).manual_seed(5)
    g = torch.zeros(n + 64, device=DEV)
    for i, (o, s) in enumerate(zip(offs, sizes)):
        seg = g[o:o + s]
        seg.normal_(generator=gen)
        seg.mul_(torch.exp2(torch.empty(s, device=DEV).uniform_(-24, 24, generator=gen) + (i % 7 - 3) * 8))
    spans = torch.tensor(rows, dtype=torch.int32, device=DEV)
    part = torch.empty(len(rows), dtype=torch.float64, device=DEV)
    be.grad_sumsq_spans(g, spans, len(rows), part)
    # the reference: torch's float64 sum of each span on the device
    ref = torch.empty_like(part)
    for s, (o, c, _) in enumerate(rows):
        if c != K.CLIP_SPAN_FLOATS:
            ref[s] = g[o:o + c].double().square().sum()
    full = [s for s, r in enumerate(rows) if r[1] == K.CLIP_SPAN_FLOATS]
    starts = torch.tensor([rows[s][0] for s in full], device=DEV)
    for lo in range(0, len(full), 512):
        idx = starts[lo:lo + 512, None] + torch.arange(K.CLIP_SPAN_FLOATS, device=DEV)[None]
        ref[full[lo:lo + 512]] = g[idx].double().square().sum(1)
    rel = ((part - ref).abs() / ref.clamp_min(1e-300)).max().item()
    print(f"{len(rows)} spans: max relative error of a span sum {rel:.3e}")
    assert rel <= SUM_REL
    tid = torch.tensor([r[2] for r in rows], device=DEV)
    tsum = torch.zeros(len(sizes), dtype=torch.float64, device=DEV).index_add_(0, tid, part)
    tref = torch.zeros_like(tsum).index_add_(0, tid, ref)
    trel = ((tsum - tref).abs() / tref).max().item()
    print(f"max relative error of a tensor sum {trel:.3e}")
    assert trel <= SUM_REL
    again = torch.full_like(part, float("nan"))
    be.grad_sumsq_spans(g, spans, len(rows), again)
    assert torch.equal(again, part)

    inv, grad_mul = 2.0 ** -16, 0.125
    exact_norm = math.sqrt(tref.sum().item()) * inv * grad_mul
    outs = []
    for _ in range(2):
        st, out = _state(inv), torch.zeros(2, device=DEV)
        be.grad_clip_coef(part, spans, len(rows), len(sizes), 0.25 * exact_norm, grad_mul, st, out)
        outs.append((out.clone(), st[4].clone()))
    norm, coef = outs[0][0].tolist()
    exact = 0.25 * exact_norm / (exact_norm + 1e-6)
    print(f"norm {norm!r} vs {exact_norm!r}, coef {coef!r} vs {exact!r}")
    assert abs(norm - exact_norm) <= COEF_REL * exact_norm and abs(coef - exact) <= COEF_REL * exact
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def _batch(seed=77, T=3):
    from oracle.step import edm_inputs, make_synthetic_batch
    b = make_synthetic_batch(1, T, 16, 16, seed, cross_dim=64)
    unet_in, ts, ehs, ids, noisy, _ = edm_inputs(b)
    return {k: v.to(DEV) for k, v in dict(unet_in=unet_in, timesteps=ts, ehs=ehs, added_time_ids=ids, noisy_latents=noisy,
                                           target=b["latents"], sigmas=b["sigmas"]).items()}


_SD = {}


def _trainer(dtype, max_grad_norm, grad_accum=1, lora_r=0, lora_param_dtype=None):
    import e2e_checks
    from oracle.unet import TINY_CONFIG
    from svd_xtend_amd.train import Trainer
    if "sd" not in _SD:
        _SD["sd"] = e2e_checks.seeded_weights(TINY_CONFIG, 5)
    m = e2e_checks.UNetSpatioTemporalConditionModel(**TINY_CONFIG)
    m.load_state_dict(_SD["sd"], strict=True)
    if lora_r:
        from svd_xtend_amd.lora import LoraConfig
        torch.manual_seed(11)
        m.add_adapter(LoraConfig(r=lora_r, lora_alpha=lora_r, init_lora_weights="gaussian"))
    m.to(DEV)
    return Trainer(m, dtype=dtype, lr=1e-3, grad_accum=grad_accum, max_grad_norm=max_grad_norm, lora_param_dtype=lora_param_dtype)


def _snap(tr):
    torch.cuda.synchronize()
    return dict(p=tr.p_flat.clone(), m=tr.m_flat.clone(), v=tr.v_flat.clone(), g=tr.g_flat[:tr.n_flat].clone(), w16=tr.rt.w16_flat.clone(),
                wt16=tr.rt.wt16_flat[:tr.rt.wt_pos].clone(), st=tr.opt_state.clone(),
                clip=tr.clip_out.clone() if tr.clip_out is not None else None)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_trainer_clipping_on_the_tiny_topology(dtype):
    b = _batch()
    runs = {}
    for key, mgn in (("none", None), ("huge", 1e30)):
        tr = _trainer(dtype, mgn)
        tr.zero_grad()
        tr.forward_backward(**b)
        scale = float(tr.opt_state[1])
        # the product's own unscaled gradients, as e2e_checks.product_step extracts them
        grads = {n: p.grad.detach().double() / scale for n, p in tr.model.named_parameters() if p.requires_grad}
        tr.optimizer_step()
        runs[key] = _snap(tr)
        assert float(tr.opt_state[0]) == 1.0
    for k in ("p", "m", "v", "w16", "wt16", "g"):
        assert torch.equal(runs["none"][k], runs["huge"][k]), k
    want = math.sqrt(sum(float(g.square().sum()) for g in grads.values()))
    norm = float(runs["huge"]["clip"][0])
    print(f"{dtype}: grad_norm {norm!r} vs {want!r}")
    assert float(runs["huge"]["clip"][1]) == 1.0 and abs(norm - want) <= COEF_REL * want
    tr = _trainer(dtype, 0.25 * norm)
    tr.step(b)
    clip = _snap(tr)
    coef = float(tr.clip_coef)
    assert torch.equal(clip["g"], runs["none"]["g"]) and float(tr.grad_norm) == norm and coef < 1.0
    normal = (runs["none"]["m"].abs() >= cc.FLT_MIN) & (clip["m"].abs() >= cc.FLT_MIN)
    assert int(normal.sum()) > 0.5 * tr.n_flat
    dev_ = (clip["m"][normal].double() / runs["none"]["m"][normal].double() / coef - 1).abs().max().item()
    print(f"{dtype}: coef {coef!r}, first moments off the ratio by {dev_:.3e}")
    assert dev_ <= M_REL


@pytest.mark.gpu
def test_reference_dtype_lora_pin_on_device():
    """LoRA r = 8 under bf16, lora_param_dtype="reference": test_clip_grad_norm's seeded bf16 gradients written into g_flat, one optimizer
    step, against clip_grad_norm_ + torch.optim.AdamW on bf16 tensors -- adapters and both moments bit for bit."""
    probe = _trainer(torch.bfloat16, 1.0, lora_r=8, lora_param_dtype="reference")
    shapes = [tuple(p.shape) for p in probe.params]
    grads = cc.pin_grads(shapes)
    assert cc.foreach_norm_mismatches(grads) == []                       # the precondition of the pin
    max_norm = 0.25 * float(torch.nn.utils.get_total_norm(grads))
    del probe
    tr = _trainer(torch.bfloat16, max_grad_norm=max_norm, lora_r=8, lora_param_dtype="reference")
    params = [p.detach().float().cpu().to(torch.bfloat16) for p in tr.params]
    tr.zero_grad()
    tr.g_flat.zero_()
    for p, o, gr in zip(tr.params, tr.offsets, grads):
        tr.g_flat[o:o + p.numel()] = gr.float().flatten().to(DEV)
    tr.optimizer_step()
    torch.cuda.synchronize()
    ref_p, ref_m, ref_v, ref_norm = cc.torch_clip_adamw(params, grads, max_norm)
    print(f"total norm {float(tr.grad_norm)!r} (torch {ref_norm!r}), coef {float(tr.clip_coef)!r}")
    assert float(tr.grad_norm) == ref_norm and float(tr.clip_coef) < 1.0
    P, M, V = tr.p_flat.cpu(), tr.m_flat.cpu(), tr.v_flat.cpu()
    for i, (p, o) in enumerate(zip(tr.params, tr.offsets)):
        k = p.numel()
        assert torch.equal(P[o:o + k], ref_p[i].flatten()), (i, float((P[o:o + k] - ref_p[i].flatten()).abs().max()))
        assert torch.equal(M[o:o + k], ref_m[i].flatten()), i
        assert torch.equal(V[o:o + k], ref_v[i].flatten()), i


@pytest.mark.gpu
@pytest.mark.parametrize("grad_accum", [1, 2])
def test_captured_step_with_clipping_equals_eager(grad_accum):
    """GraphedStep replays (the clip's two launches inside the optimizer graph) against eager steps, bit for bit; with one micro-batch also
    the launch plan recorded during the capture against the graph replays.  max_grad_norm 1e-3 clips every step here."""
    from svd_xtend_amd.train import GraphedStep
    batches = [_batch(77 + j) for j in range(grad_accum)]
    arg = batches[0] if grad_accum == 1 else batches
    steps, out = 3, {}
    for mode in ("eager", "graph") + (("plan",) if grad_accum == 1 else ()):
        tr = _trainer(torch.float16, 1e-3, grad_accum=grad_accum)
        if mode == "eager":
            for _ in range(steps):
                tr.step(arg)
        else:
            gs = GraphedStep(tr, arg, record_plan=(mode == "plan"))      # its warm-up pass is step 1
            for _ in range(steps - 1):
                gs.replay_plan() if mode == "plan" else gs()
        out[mode] = _snap(tr)
        print(f"grad_accum {grad_accum} {mode}: norm, coef {out[mode]['clip'].tolist()}, steps {float(out[mode]['st'][0])}")
        assert float(out[mode]["st"][0]) == steps and float(out[mode]["clip"][1]) < 1.0
    for mode in out:
        for k in ("p", "m", "v", "w16", "wt16", "clip", "st"):
            assert torch.equal(out[mode][k], out["eager"][k]), (mode, k)
    # the norm is that of the gradient averaged over the micro-batches
    g = out["eager"]["g"].double() / float(out["eager"]["st"][1]) / grad_accum
    want = math.sqrt(float(g.square().sum()))
    assert abs(float(out["eager"]["clip"][0]) - want) <= COEF_REL * want
