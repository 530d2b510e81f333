"""CPU (`-m "not gpu"`): the convolution weight gradient -- svdx_gemm_tn_gather + svdx_conv_wgrad_finalize and svdx_conv_pack -- with the
kernel sources executed by the simulator of tests/sim/ and with the emulation of tests/emul.py, against the float64
reference (autograd through the float64 convolutions of tests/ref64.py) under the census' svdx_gemm_tn bound."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "sim"))

import conv_wgrad_checks as cw  # noqa: E402
import emul  # noqa: E402
import selection_checks as sc  # noqa: E402
from svd_xtend_amd import kernels as K  # noqa: E402


@pytest.fixture(scope="module")
def sim():
    from backend import SimBackend
    return SimBackend()


@pytest.fixture
def sim_installed(sim):
    prev = K._backend
    K._set_backend_for_tests(sim)
    yield sim
    K._set_backend_for_tests(prev)


def test_case_table_covers_what_it_claims():
    """SELF-CHECK of the case table (no library code runs): every split_k of {1, 2, 4, 8} and alpha != 1 occur, R stays within the significance rule's reach (every case runs at full size
    on the simulator: the largest takes under a second)"""
    assert len({c.name for c in cw.CASES}) == len(cw.CASES) == 16
    assert {s for c in cw.CASES for s in cw.splits_of(c)} == {1, 2, 4, 8}
    assert sum(c.alpha != 1.0 for c in cw.CASES) >= 2
    assert all(cw.rows_of(c) <= 1024 for c in cw.CASES)
    assert cw.rows_of(cw.BY_NAME["3x3_s1_5x3_borders"]) == 45 and cw.splits_of(cw.BY_NAME["3x3_s1_16x16_split8"]) == [1, 2, 4, 8]


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("name", [c.name for c in cw.CASES])
def test_kernel_case_on_simulator(sim, name, dt):
    cw.sweep_case(sim, "cpu", cw.BY_NAME[name], cw.DT[dt])


@pytest.mark.parametrize("name", [c.name for c in cw.CASES])
def test_emulation_meets_the_same_reference(name):
    """SELF-CHECK of the test double, not of the feature (it passes without the library's new entries): the emulation subclass the step
    tests run on meets the float64 reference under the same bound, so a step that passes on it says something about the host code."""
    cw.sweep_case(emul.EmuBackend(), "cpu", cw.BY_NAME[name], torch.float16)


def test_a_dropped_tap_or_a_zero_result_cannot_pass():
    """SELF-CHECK of the bound (no library code runs): the significance rule at work -- the reference with one tap zeroed, and all zeros, both miss the bound almost everywhere"""
    c = cw.BY_NAME["3x3_s1_5x3_borders"]
    x, dy, _, _, ref = cw.case_reference(c, torch.float16)
    vw, bw, vb, bb = cw.bounds(c, ref, 1)
    drop = vw.clone()
    drop[:, :, 4] = 0
    assert float((cw._ratio(drop.float(), vw, bw)[:, :, 4] > 1).double().mean()) >= 0.95
    assert float((cw._ratio(torch.zeros_like(vw).float(), vw, bw) > 1).double().mean()) >= 0.95
    assert float((cw._ratio(torch.zeros_like(vb).float(), vb, bb) > 1).double().mean()) >= 0.95


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("out_scale", [1.0, 0.37])
@pytest.mark.parametrize("shape", cw.PACK_SHAPES, ids=lambda s: "{}_s{}_{}x{}_p{}_{}".format(*s))
def test_conv_pack_equals_convop_pack_on_simulator(sim_installed, shape, out_scale, dt):
    cw.run_pack("cpu", cw.DT[dt], shape, out_scale)


def test_conv_pack_without_data_gradient_form(sim_installed):
    cw.run_pack("cpu", torch.float16, cw.PACK_SHAPES[3], 0.37, need_dx=False)


def test_argument_errors(sim):
    """the gather modes the weight gradient has no use for, operands of 2 GiB and more, and a split that leaves slices without rows are
    refused before any launch"""
    c = cw.BY_NAME["3x3_s2_8x8"]
    x, dy, _, _, _ = cw.case_reference(c, torch.float16)
    R, N, Kd = cw.rows_of(c), c.cout_p, 9 * c.cin_p
    out = torch.zeros(8, N, Kd)
    g = cw.gather_of(c, c.cin_p, c.cin_p)
    for mode in (K.GATHER_CONV3X3_DGRAD2, K.GATHER_CONV3X3_PAD0, K.GATHER_PLAIN):
        bad = K.Gather(mode, n_img=g.n_img, hi=g.hi, wi=g.wi, ho=g.ho, wo=g.wo, cin=g.cin, stride=g.stride, lda=g.lda)
        with pytest.raises(K.SvdxError, match="gather mode"):
            sim.gemm_tn_gather(dy, x, out, R, N, c.cout_p, Kd, bad, split_k=1)
    with pytest.raises(K.SvdxError, match="2 GiB"):
        sim.gemm_tn_gather(dy, x, out, R, N, 1 << 26, Kd, g, split_k=1)
    huge = K.Gather(g.mode, n_img=g.n_img, hi=g.hi, wi=g.wi, ho=g.ho, wo=g.wo, cin=g.cin, stride=g.stride, lda=1 << 24)
    with pytest.raises(K.SvdxError, match="2 GiB"):
        sim.gemm_tn_gather(dy, x, out, R, N, c.cout_p, Kd, huge, split_k=1)
    with pytest.raises(K.SvdxError, match="slices without rows"):
        sim.gemm_tn_gather(dy, x, out, R, N, c.cout_p, Kd, g, split_k=8)
    with pytest.raises(K.SvdxError, match="rows mismatch"):
        sim.gemm_tn_gather(dy, x, out, R + 1, N, c.cout_p, Kd, g, split_k=1)
    with pytest.raises(K.SvdxError, match="stages"):
        sim.gemm_tn_gather(dy, x, out, R, N, c.cout_p, Kd, g, split_k=1, stages=18)
    assert not out.any()


# ---- ConvOp.bwd_dw / refresh: the host side of one convolution, on the emulation ----------------------------------------------------
def _trainable_op(c, dev, seed=0):
    from svd_xtend_amd import ops
    g = torch.Generator().manual_seed(seed)
    shape = (c.cout, c.cin, 3, 1, 1) if c.kind == "t3" else (c.cout, c.cin, 3, 3)
    weight = torch.nn.Parameter(torch.randn(*shape, generator=g).to(dev))
    bias = torch.nn.Parameter(torch.randn(c.cout, generator=g).to(dev))
    weight.grad, bias.grad = torch.full_like(weight, float("nan")), torch.full_like(bias, float("nan"))
    return ops.ConvOp(weight, bias, c.kind, stride=c.stride, ups=bool(c.ups), cin_pad=c.cin_p, cout_pad=c.cout_p)


@pytest.mark.parametrize("name", ["3x3_s2_8x8", "3x3_ups_4x4", "3x3_conv_out_cout4", "3x3_conv_in_cin8", "t3_T3_c64", "3x3_s1_16x16_split8"])
def test_convop_bwd_dw_on_emulation(emu_backend, name):
    """ConvOp.bwd_dw (store on the first micro-batch, += on the second) against the float64 reference, the alpha of the case folded in as
    the packed out_scale; conv_out runs at N = cout_p and keeps its 4 rows"""
    from svd_xtend_amd import ops
    c = cw.BY_NAME[name]
    x, dy, _, _, ref = cw.case_reference(c, torch.float16)
    rt = ops.Runtime(torch.float16, torch.device("cpu"))
    rt.found_inf = torch.zeros(1)
    op = _trainable_op(c, "cpu")
    assert op.trainable
    op.pack(rt, out_scale=c.alpha)
    assert {id(op.weight), id(op.bias)} <= rt.write_once          # (3x3 / temporal: the reducing launch stores both)
    rt.grad_overwrite = True
    op.bwd_dw(rt, dy, x, c.n_img, c.h, c.w, T=c.T)
    N = c.cout if c.cout % 8 == 0 else 8
    sk = ops._tn_formula(cw.rows_of(c), N, cw.taps_of(c) * c.cin_p)[0]           # the slabs bwd_dw's formula asks for
    vw, bw, vb, bb = cw.bounds(c, ref, sk)
    assert float(cw._ratio(op.weight.grad.reshape(vw.shape), vw, bw).max()) <= 1.0
    assert float(cw._ratio(op.bias.grad, vb, bb).max()) <= 1.0
    rt.grad_overwrite = False
    first_w, first_b = op.weight.grad.clone(), op.bias.grad.clone()
    op.bwd_dw(rt, dy, x, c.n_img, c.h, c.w, T=c.T)
    vw2, bw2, vb2, bb2 = cw.bounds(c, ref, sk, first_w.reshape(vw.shape), first_b)
    assert float(cw._ratio(op.weight.grad.reshape(vw.shape), vw2, bw2).max()) <= 1.0
    assert float(cw._ratio(op.bias.grad, vb2, bb2).max()) <= 1.0
    assert float(rt.found_inf) == 0.0
    op.bwd_dw(rt, torch.full_like(dy, float("inf")), x, c.n_img, c.h, c.w, T=c.T)
    assert float(rt.found_inf) == 1.0


def test_convop_refresh_follows_the_master(emu_backend):
    """after the master moved, refresh leaves exactly what a fresh pack of the new master gives"""
    from svd_xtend_amd import ops
    c = cw.BY_NAME["t3_T3_c64"]
    rt = ops.Runtime(torch.bfloat16, torch.device("cpu"))
    op, fresh = _trainable_op(c, "cpu"), _trainable_op(c, "cpu")
    op.pack(rt, out_scale=0.37)
    with torch.no_grad():
        op.weight.mul_(1.5).add_(0.01)
        op.bias.add_(0.25)
        fresh.weight.copy_(op.weight)
        fresh.bias.copy_(op.bias)
    fresh.pack(rt, out_scale=0.37)
    assert not torch.equal(op.w, fresh.w)
    op.refresh(rt)
    assert torch.equal(op.w, fresh.w) and torch.equal(op.wd, fresh.wd) and torch.equal(op.b, fresh.b)


# ---- the step: Trainer(trainable=...) on the emulation against the CPU oracle --------------------------------------------------------------
def test_step_with_convolutions_and_temporal_blocks_matches_oracle(emu_backend):
    ref = sc.oracle_step(cw.CONV_AND_TEMPORAL)
    got = sc.product_step(ref, cw.CONV_AND_TEMPORAL, torch.float16, torch.device("cpu"))
    r = cw.assert_step_parity("emulation conv+temporal float16", ref, got)
    print(r)
    tr = got["trainer"]
    # conv tensors are not 2-D: elementwise optimizer tiles, no transposed twin, 16-byte offsets; their gradients sit outside the per-block
    # buckets, in the spans the data-parallel sum reduces as "the rest"
    conv = {id(p): n for n, p in tr.model.named_parameters() if p.requires_grad and p.ndim > 2}
    assert len(conv) > 20
    for p, off in zip(tr.params, tr.offsets):
        if id(p) in conv:
            assert off % 4 == 0 and p.numel() % 4 == 0 and id(p) not in tr.rt.wt_map, conv[id(p)]
            assert any(lo <= off and off + p.numel() <= hi for lo, hi in tr._rest), conv[id(p)]
            assert not any(lo < off + p.numel() and off < hi for lo, hi in tr._buckets.values()), conv[id(p)]


def test_a_second_sweep_after_zero_grad_gives_the_same_gradients(emu_backend):
    """zero_grad(); forward_backward(batch) twice on one batch, no optimizer step between: every gradient comes out bit-equal.  A slot
    that is neither stored by its producer nor zeroed would double -- the 1x1 shortcuts' bias gradients did (their column sums go through
    gemm_tn_acc, which accumulates), so their biases must stay out of Runtime.write_once while the 3x3 / temporal ones are in it."""
    ref = sc.oracle_step(cw.CONV_AND_TEMPORAL)
    tr = sc.make_trainer(ref, cw.CONV_AND_TEMPORAL, torch.float16, torch.device("cpu"))
    batch = sc.step_batch(ref, "cpu")
    sweeps = []
    for _ in range(2):
        tr.zero_grad()
        tr.forward_backward(**batch)
        tr.micro = 0
        sweeps.append({n: p.grad.detach().clone() for n, p in tr.model.named_parameters() if p.requires_grad})
    assert sum("conv_shortcut.bias" in n for n in sweeps[0]) >= 10
    differ = [n for n in sweeps[0] if not torch.equal(sweeps[0][n], sweeps[1][n])]
    assert not differ, differ[:8]
    ops_ = tr.model._conv_ops
    assert all((id(op.bias) in tr.rt.write_once) == (op.kind != "1x1") for op in ops_ if op.trainable and op.bias is not None)
    assert any(op.kind == "1x1" for op in ops_) and all(id(op.weight) in tr.rt.write_once for op in ops_ if op.trainable)


def test_two_optimizer_steps_match_the_oracle(emu_backend):
    """the second step starts from gradients the first one left behind: after two steps on one batch every trainable tensor has moved as
    the oracle's (torch.optim.AdamW), the shortcut biases included"""
    ref = sc.oracle_step(cw.CONV_AND_TEMPORAL, steps=2)
    tr = sc.make_trainer(ref, cw.CONV_AND_TEMPORAL, torch.float32, torch.device("cpu"))
    batch = sc.step_batch(ref, "cpu")
    for _ in range(2):
        tr.step(batch)
    lr = ref["lr"]
    for n, p in tr.model.named_parameters():
        if p.requires_grad:
            d = (p.detach() - ref["params_after2"][n]).abs()
            assert float(d.max()) <= 2.5 * lr and float(d.mean()) <= 0.05 * lr, (n, float(d.max()), float(d.mean()))
    short = [n for n in ref["names"] if "conv_shortcut.bias" in n]
    moved = [float((ref["params_after2"][n] - ref["sd0"][n]).abs().mean()) for n in short]
    assert short and min(moved) > 0.5 * lr                   # (they do move: a doubled gradient would show in the update's direction only)


def test_step_with_convolutions_alone(emu_backend):
    """trainable="@conv": no attention block trains, every module behind conv_in still needs its input gradient, the skips carry
    gradients, and the gradients match the oracle"""
    ref = sc.oracle_step("@conv")
    got = sc.product_step(ref, "@conv", torch.float16, torch.device("cpu"))
    cw.assert_step_parity("emulation conv float16", ref, got)
    m = got["trainer"].model
    assert not any(mod.has_trainable() for kind, mod in m.steps if kind == "attn")
    assert all(mod.need_dx for kind, mod in m.steps if kind in ("res", "attn", "down", "up"))
    assert all(m._skip_needs_grad) and m._any_trainable


def test_trainable_tail_only_skips_the_data_gradients_it_does_not_need(emu_backend):
    """only the LAST resnet's convolutions train: nothing upstream needs a gradient, so that block runs its weight gradients with
    need_dx == False and the sweep stops there"""
    which = "up_blocks.3.resnets.2.spatial_res_block.conv"
    ref = sc.oracle_step(which)
    assert len(ref["names"]) == 6                                    # conv1, conv2, conv_shortcut: weight and bias
    got = sc.product_step(ref, which, torch.float16, torch.device("cpu"))
    import e2e_checks
    for n in ref["names"]:
        assert e2e_checks.cosine(got["grads"][n], ref["grads"][n]) >= 0.9995, n
    m = got["trainer"].model
    blk = m.up_blocks[3].resnets[2]
    upto = [mod for kind, mod in m.steps if kind in ("res", "attn", "down", "up")]
    upto = upto[:upto.index(blk) + 1]
    assert blk.has_trainable() and not any(mod.need_dx for mod in upto) and not any(m._skip_needs_grad)


def test_conv_out_alone_computes_no_data_gradient(emu_backend, monkeypatch):
    """only conv_out trains: its weight gradient matches the oracle and the sweep stops there (no data-gradient GEMM, no norm backward)"""
    import e2e_checks
    from svd_xtend_amd import ops
    ref = sc.oracle_step("conv_out")
    assert ref["names"] == ["conv_out.bias", "conv_out.weight"]

    def never(*a, **k):
        raise AssertionError("a data gradient nobody needs was computed")
    monkeypatch.setattr(ops.ConvOp, "bwd_dx", never)
    monkeypatch.setattr(ops.GroupNormOp, "bwd", never)
    got = sc.product_step(ref, "conv_out", torch.float16, torch.device("cpu"))
    for n in ref["names"]:
        assert e2e_checks.cosine(got["grads"][n], ref["grads"][n]) >= 0.9995, n
    m = got["trainer"].model
    assert m._any_trainable and not m._sweep_needed
    assert all(mod.sv is None for kind, blk in m.steps if kind == "res" for mod in (blk.spatial_res_block, blk.temporal_res_block))


def test_planted_nonfinite_conv_gradient_skips_the_step(emu_backend, monkeypatch):
    """one inf in the gradient that reaches a convolution's weight-gradient launch: the step is skipped -- masters, moments and the packed
    16-bit weights keep every bit (the re-pack of an unchanged master gives the same bits)"""
    from svd_xtend_amd import ops
    ref = sc.oracle_step(cw.CONV_AND_TEMPORAL)
    tr = sc.make_trainer(ref, cw.CONV_AND_TEMPORAL, torch.float16, torch.device("cpu"))
    target = tr.model.mid_block.resnets[0].temporal_res_block.c2
    packed = [op for op in tr.model._conv_ops if op.trainable]
    before = dict(p=tr.p_flat.clone(), m=tr.m_flat.clone(), v=tr.v_flat.clone(), w=[op.w.clone() for op in packed], wd=[op.wd.clone() for op in packed if op.wd is not None])
    bwd_dw, hit = ops.ConvOp.bwd_dw, []

    def planted(self, rt, dy, x, *a, **k):
        if self is target:
            dy = dy.clone()
            dy[3, 5] = float("inf")
            hit.append(1)
        return bwd_dw(self, rt, dy, x, *a, **k)
    monkeypatch.setattr(ops.ConvOp, "bwd_dw", planted)
    tr.step(sc.step_batch(ref, "cpu"))
    assert hit and float(tr.opt_state[7]) == 1.0 and float(tr.opt_state[0]) == 0.0
    assert torch.equal(tr.p_flat, before["p"]) and torch.equal(tr.m_flat, before["m"]) and torch.equal(tr.v_flat, before["v"])
    assert all(torch.equal(op.w, w) for op, w in zip(packed, before["w"]))
    assert all(torch.equal(op.wd, w) for op, w in zip([op for op in packed if op.wd is not None], before["wd"]))
    monkeypatch.setattr(ops.ConvOp, "bwd_dw", bwd_dw)
    tr.step(sc.step_batch(ref, "cpu"))                                      # the next, clean step is taken (at the halved loss scale)
    assert float(tr.opt_state[7]) == 0.0 and float(tr.opt_state[0]) == 1.0 and not torch.equal(tr.p_flat, before["p"])


def test_default_selection_is_unchanged_and_other_selections_are_refused(emu_backend):
    from oracle.unet import TINY_CONFIG
    from svd_xtend_amd.lora import LoraConfig
    from svd_xtend_amd.train import Trainer, select_trainable
    from svd_xtend_amd.unet import UNetSpatioTemporalConditionModel
    ref = sc.oracle_step(cw.CONV_AND_TEMPORAL)

    def model():
        m = UNetSpatioTemporalConditionModel(**TINY_CONFIG)
        m.load_state_dict(ref["sd0"], strict=True)
        return m
    m = model()
    tr = Trainer(m, dtype=torch.float16)
    want = [n for n, _ in m.named_parameters() if "temporal_transformer_block" in n]
    assert tr.names == want and [n for n, p in m.named_parameters() if p.requires_grad] == want
    assert not any(op.trainable for op in m._conv_ops)
    # "@conv" is the convolutions and nothing else: not conv_norm_out, which the substring "conv" would catch
    names = select_trainable(model(), "@conv")
    assert names and all(n.rsplit(".", 1)[0].split(".")[-1] in ("conv", "conv1", "conv2", "conv_shortcut", "conv_in", "conv_out") for n in names)
    assert not any("conv_norm_out" in n for n in names) and any("conv_norm_out" in n for n in select_trainable(model(), "conv"))
    assert select_trainable(model(), ["@conv", "temporal_transformer_block"]) == ref["names"] or \
        sorted(select_trainable(model(), ["@conv", "temporal_transformer_block"])) == ref["names"]
    with pytest.raises(ValueError):
        select_trainable(model(), [])
    lm = model()
    lm.add_adapter(LoraConfig(r=4, lora_alpha=4, init_lora_weights="gaussian"))
    with pytest.raises(ValueError, match="LoRA"):
        Trainer(lm, dtype=torch.float16, trainable="@conv")
    with pytest.raises(NotImplementedError, match=r"norm1\.(weight|bias)"):
        Trainer(model(), dtype=torch.float16, trainable="norm1")
