"""Gradient-norm clipping on the CPU (`-m "not gpu"`): the two HIP entries (svdx_grad_sumsq_spans, svdx_grad_clip_coef) from their unmodified
source on the wave64 simulator of tests/sim, the Trainer's orchestration through the emulation, the coefficient of two gloo ranks, and the
reference-dtype LoRA recipe pinned to torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW on bf16 tensors.

Bars (derived, not measured):
  * a sum of squares: every product of two floats is exact in fp64 and each sum is a chain of at most 2^16 + 16 fp64 additions, so the
    relative error is at most (2^16 + 16) * 2^-53 ~ 7.3e-12 < 1e-11;
  * the coefficient: at most four fp32 roundings of half an ulp each after that, 4 * 2^-24 = 2^-22 relative;
  * the first moment after one step is (1 - beta1) * g * gmul with gmul = opt_state[4] * coef: against the unclipped run two more fp32
    roundings, 2^-21 relative."""
import math
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE, os.path.join(HERE, "sim")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import clip_checks as cc  # noqa: E402
import emul  # noqa: E402
from svd_xtend_amd import kernels as K  # noqa: E402

SUM_REL = 1e-11
COEF_REL = 2.0 ** -22
M_REL = 2.0 ** -21


@pytest.fixture(scope="module")
def sim():
    from backend import SimBackend
    return SimBackend()


def _state(inv_scale=1.0):
    st = torch.zeros(K.OPT_STATE_ALLOC)
    st[1], st[4], st[5], st[6], st[8] = 1.0, inv_scale, 1.0, 1.0, 1.0
    return st


def _wide_buffer(sizes, seed=0):
    """Tensors of `sizes` packed as the Trainer packs them, every tensor at its own magnitude (2^-40 .. 2^40) and the elements of each
    spread over a further 2^+-8."""
    rows, offs, n = cc.span_rows(sizes)
    g = torch.zeros(n + 64)
    gen = torch.Generator().manual_seed(seed)
    for i, (o, s) in enumerate(zip(offs, sizes)):
        e = -40 + 80 * i / max(1, len(sizes) - 1)
        g[o:o + s] = torch.randn(s, generator=gen) * 2.0 ** e * torch.exp2(torch.empty(s).uniform_(-8, 8, generator=gen))
    return g, rows, offs


# spans with tails that are not a multiple of 4, tensors split over several spans (one of three, one ending in a 3-float span), an
# all-zero tensor, one-float tensors
SIZES = [5, K.CLIP_SPAN_FLOATS + 7, 130, 1, 3001, 2 * K.CLIP_SPAN_FLOATS + 3, 64, 6]
ZERO = 2


def test_sums_of_squares_and_coefficient_on_simulator(sim):
    g, rows, offs = _wide_buffer(SIZES)
    g[offs[ZERO]:offs[ZERO] + SIZES[ZERO]] = 0
    spans = torch.tensor(rows, dtype=torch.int32)
    assert any(c % 4 for _, c, _ in rows) and len(rows) > len(SIZES)
    part = torch.full((len(rows),), float("nan"), dtype=torch.float64)
    sim.grad_sumsq_spans(g, spans, len(rows), part)
    host = [g[o:o + c].double().pow(2).sum().item() for o, c, _ in rows]
    for s, (want, got) in enumerate(zip(host, part.tolist())):
        print(f"span {s} ({rows[s][1]} floats): {got!r} vs {want!r}")
        assert abs(got - want) <= SUM_REL * want, (s, got, want)
    assert part[[s for s, r in enumerate(rows) if r[2] == ZERO]].eq(0).all()
    tsum = [0.0] * len(SIZES)
    for s, (_, _, t) in enumerate(rows):
        tsum[t] += part[s].item()
    for t, (o, n) in enumerate(zip(offs, SIZES)):
        want = g[o:o + n].double().pow(2).sum().item()
        print(f"tensor {t}: {tsum[t]!r} vs {want!r}")
        assert abs(tsum[t] - want) <= SUM_REL * want, (t, tsum[t], want)
    again = torch.zeros_like(part)
    sim.grad_sumsq_spans(g, spans, len(rows), again)
    assert torch.equal(again, part)                                            # fixed order: the same bits

    inv, grad_mul = 2.0 ** -16, 0.25                                           # a loss scale and a mean over four ranks / micro-batches
    exact_norm = math.sqrt(g.double().pow(2).sum().item()) * inv * grad_mul
    for max_norm in (0.25 * exact_norm, 1e30):
        st, out = _state(inv), torch.zeros(2)
        sim.grad_clip_coef(part, spans, len(rows), len(SIZES), max_norm, grad_mul, st, out)
        exact = min(1.0, max_norm / (exact_norm + 1e-6))
        norm, coef = out.tolist()
        print(f"max_norm {max_norm:.6e}: norm {norm!r} vs {exact_norm!r}, coef {coef!r} vs {exact!r}")
        assert abs(norm - exact_norm) <= COEF_REL * exact_norm
        assert abs(coef - exact) <= COEF_REL * exact
        assert float(st[4]) == cc.f32(inv * coef)                              # folded into AdamW's gradient factor
        if max_norm == 1e30:
            assert coef == 1.0 and float(st[4]) == inv                         # nothing to clip: the factor keeps its bits


def test_non_finite_gradients_give_a_non_finite_norm_on_simulator(sim):
    g, rows, offs = _wide_buffer(SIZES, seed=1)
    spans = torch.tensor(rows, dtype=torch.int32)
    part = torch.zeros(len(rows), dtype=torch.float64)
    for bad in ({1: float("inf")}, {5: float("nan")}, {1: float("inf"), 5: float("nan")}):
        gb = g.clone()
        for t, val in bad.items():
            gb[offs[t] + SIZES[t] - 1] = val                                   # the last float of the tensor: a tail span
        sim.grad_sumsq_spans(gb, spans, len(rows), part)
        st, out = _state(), torch.zeros(2)
        st[7] = 1.0                                                            # the inf check's verdict: skip this step
        sim.grad_clip_coef(part, spans, len(rows), len(SIZES), 1.0, 1.0, st, out)
        print(bad, out.tolist())
        assert not math.isfinite(float(out[0]))
        if 5 not in bad:
            assert float(out[0]) == float("inf")
        assert float(st[4]) == 1.0                                             # a skipped step leaves the factor alone


def test_reference_dtype_lora_pin_on_simulator(sim):
    """param_mode 1 (Trainer(lora_param_dtype="reference")): clip_grad_norm_ followed by torch.optim.AdamW on bf16 tensors, bit for bit --
    the tiny topology's rank-8 adapters as shapes, seeded bf16 parameters and gradients.  Precondition (asserted): torch's per-tensor bf16
    norm is the correctly rounded one for every tensor."""
    shapes = lora_shapes()
    grads = cc.pin_grads(shapes)
    assert cc.foreach_norm_mismatches(grads) == []
    gen = torch.Generator().manual_seed(cc.PIN_SEED + 1)
    # the A factors seeded, the B factors zero as peft creates them: their first update is -lr * m / (sqrt(v) / sqrt(bc2) + eps) itself
    params = [(torch.randn(s, generator=gen) * 0.05 * (i % 2 == 0)).to(torch.bfloat16) for i, s in enumerate(shapes)]
    max_norm = 0.25 * float(torch.nn.utils.get_total_norm(grads))
    ref_p, ref_m, ref_v, ref_norm = cc.torch_clip_adamw(params, grads, max_norm)
    rows, offs, n = cc.span_rows([math.prod(s) for s in shapes])
    p, g, m, v = (torch.zeros(n) for _ in range(4))
    for o, pp, gg in zip(offs, params, grads):
        p[o:o + pp.numel()] = pp.float().flatten()
        g[o:o + gg.numel()] = gg.float().flatten()
    spans = torch.tensor(rows, dtype=torch.int32)
    part, out, st, pa = torch.zeros(len(rows), dtype=torch.float64), torch.zeros(2), _state(), torch.zeros(n, dtype=torch.bfloat16)
    sim.optim_prep(st, cc.PIN_BETAS[0], cc.PIN_BETAS[1], 2.0, 0.5, 2000, 0)
    sim.grad_sumsq_spans(g, spans, len(rows), part)
    sim.grad_clip_coef(part, spans, len(rows), len(shapes), max_norm, 1.0, st, out, param_mode=K.PARAMS_BF16_REFERENCE)
    sim.adamw(p, g, m, v, n, cc.PIN_LR, cc.PIN_BETAS[0], cc.PIN_BETAS[1], cc.PIN_EPS, cc.PIN_WD, 1.0, st, pa, param_mode=K.PARAMS_BF16_REFERENCE)
    print(f"total norm {float(out[0])!r} (torch {ref_norm!r}), coef {float(out[1])!r}")
    assert float(out[0]) == ref_norm and float(out[1]) < 1.0
    for i, o in enumerate(offs):
        k = ref_p[i].numel()
        assert torch.equal(p[o:o + k], ref_p[i].flatten()), (i, float((p[o:o + k] - ref_p[i].flatten()).abs().max()))
        assert torch.equal(m[o:o + k], ref_m[i].flatten()), i
        assert torch.equal(v[o:o + k], ref_v[i].flatten()), i


def lora_shapes():
    """Shapes of the tiny topology's rank-8 adapters, in the Trainer's tensor order."""
    from oracle.unet import TINY_CONFIG
    from svd_xtend_amd.lora import LoraConfig
    from svd_xtend_amd.train import select_trainable
    from svd_xtend_amd.unet import UNetSpatioTemporalConditionModel
    m = UNetSpatioTemporalConditionModel(**TINY_CONFIG)
    m.add_adapter(LoraConfig(r=8, lora_alpha=8, init_lora_weights="gaussian"))
    named = dict(m.named_parameters())
    return [tuple(named[nm].shape) for nm in select_trainable(m)]


# ---- the Trainer through the emulation ---------------------------------------------------------------------------------------------------
def _model(seed=0):
    from oracle.unet import TINY_CONFIG, UNetSpatioTemporalConditionOracle, scaled_init_
    from svd_xtend_amd.unet import UNetSpatioTemporalConditionModel
    orc = UNetSpatioTemporalConditionOracle(**TINY_CONFIG)
    scaled_init_(orc, seed)
    m = UNetSpatioTemporalConditionModel(**TINY_CONFIG)
    m.load_state_dict(orc.state_dict(), strict=True)
    return m


def _batch(seed, T=3):
    from oracle.step import edm_inputs, make_synthetic_batch
    b = make_synthetic_batch(1, T, 16, 16, seed, cross_dim=64)
    unet_in, ts, ehs, ids, noisy, _ = edm_inputs(b)
    return dict(unet_in=unet_in, timesteps=ts, ehs=ehs, added_time_ids=ids, noisy_latents=noisy, target=b["latents"], sigmas=b["sigmas"])


def _one_step(max_grad_norm, batch, dtype=torch.float16):
    from svd_xtend_amd.train import Trainer
    tr = Trainer(_model(0), dtype=dtype, lr=1e-3, max_grad_norm=max_grad_norm)
    tr.step(batch)
    assert float(tr.opt_state[0]) == 1.0                                      # the step was taken
    n = tr.n_flat
    return tr, dict(p=tr.p_flat.clone(), m=tr.m_flat.clone(), v=tr.v_flat.clone(), g=tr.g_flat[:n].clone(),
                    w16=tr.rt.w16_flat.clone(), wt16=tr.rt.wt16_flat[:tr.rt.wt_pos].clone() if tr.rt.wt16_flat is not None else None)   # (the arena beyond wt_pos is unused)


def test_trainer_clipping_is_opt_in_and_scales_the_update(emu_backend):
    rec = emul.record(K._backend)
    clip_calls = lambda: [e for e in rec.names(depth=0) if e in ("svdx_grad_sumsq_spans", "svdx_grad_clip_coef")]   # noqa: E731
    b = _batch(7)
    tr0, none = _one_step(None, b)
    assert clip_calls() == [] and tr0.grad_norm is None and tr0.clip_coef is None
    tr1, huge = _one_step(1e30, b)
    assert clip_calls() == ["svdx_grad_sumsq_spans", "svdx_grad_clip_coef"]
    assert float(tr1.clip_coef) == 1.0 and tr1.grad_norm.dim() == 0
    for k in none:
        assert (none[k] is None and huge[k] is None) or torch.equal(none[k], huge[k]), k
    norm = float(tr1.grad_norm)
    # the norm is that of the unscaled gradient: g_flat still carries the loss scale the backward pass used
    want = math.sqrt(none["g"].double().pow(2).sum().item()) / float(tr0.opt_state[1])
    assert abs(norm - want) <= COEF_REL * want, (norm, want)
    tr2, clip = _one_step(0.25 * norm, b)
    coef = float(tr2.clip_coef)
    print(f"norm {norm!r}, coef {coef!r}")
    assert torch.equal(clip["g"], none["g"]) and float(tr2.grad_norm) == norm
    assert abs(coef - 0.25 * norm / (norm + 1e-6)) <= COEF_REL * 0.25
    normal = (none["m"].abs() >= cc.FLT_MIN) & (clip["m"].abs() >= cc.FLT_MIN)
    assert int(normal.sum()) > 0.5 * tr2.n_flat
    ratio = clip["m"][normal].double() / none["m"][normal].double()
    assert float((ratio / coef - 1).abs().max()) <= M_REL, float((ratio / coef - 1).abs().max())


def _rank_worker(rank, world, port, out, max_grad_norm):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(2)
    for p in (ROOT, HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    import emul
    from svd_xtend_amd import kernels
    kernels._set_backend_for_tests(emul.EmuBackend())
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from svd_xtend_amd.train import Trainer
    tr = Trainer(_model(0), dtype=torch.float32, lr=1e-3, max_grad_norm=max_grad_norm)
    tr.zero_grad()
    tr.forward_backward(**_batch(300 + rank, T=2))                             # rank-distinct data
    local = tr.g_flat[:tr.n_flat].double().clone()
    tr.finish_grads()
    tr.optimizer_step()
    torch.save(dict(local=local, coef=tr.clip_coef.clone(), norm=tr.grad_norm.clone(), st=tr.opt_state.clone()), os.path.join(out, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_ranks_clip_the_mean_gradient(tmp_path):
    """Two gloo ranks with different data: one coefficient, bit-equal on both, that of the MEAN gradient (float64 on the host) -- and more
    than 1 % away from what either rank's own gradient would give (a norm taken before the sum would fail here)."""
    max_norm = 1e-3
    port = 29500 + (os.getpid() + 977) % 2000
    mp.spawn(_rank_worker, args=(2, port, str(tmp_path), max_norm), nprocs=2, join=True)
    r = [torch.load(tmp_path / f"r{q}.pt") for q in range(2)]
    assert torch.equal(r[0]["coef"], r[1]["coef"]) and torch.equal(r[0]["norm"], r[1]["norm"])
    mean_norm = math.sqrt(((r[0]["local"] + r[1]["local"]) / 2).pow(2).sum().item())
    exact = min(1.0, max_norm / (mean_norm + 1e-6))
    coef = float(r[0]["coef"])
    print(f"mean-gradient norm {mean_norm!r}: coef {coef!r} vs {exact!r}")
    assert exact < 1.0 and abs(coef - exact) <= COEF_REL * exact
    for q in range(2):
        local = min(1.0, max_norm / (math.sqrt(r[q]["local"].pow(2).sum().item()) / 2 + 1e-6))
        print(f"rank {q}: the local coefficient would be {local!r}")
        assert abs(local - coef) > 0.01 * coef
