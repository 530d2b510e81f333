"""`-m gpu`: the convolution weight gradient on the device -- every kernel case of tests/conv_wgrad_checks.py in fp16 and bf16 against the
float64 reference (computed on the CPU, shared with the simulator's run of the same case), svdx_conv_pack against ConvOp.pack bit for
bit, and ConvOp.bwd_dw / refresh through the real library."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

import conv_wgrad_checks as cw  # noqa: E402
import selection_checks as sc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from svd_xtend_amd import kernels
    return kernels.backend()


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("name", [c.name for c in cw.CASES])
def test_kernel_case_on_device(hip, name, dt):
    cw.sweep_case(hip, "cuda", cw.BY_NAME[name], cw.DT[dt], verbose=True)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("out_scale", [1.0, 0.37])
@pytest.mark.parametrize("shape", cw.PACK_SHAPES, ids=lambda s: "{}_s{}_{}x{}_p{}_{}".format(*s))
def test_conv_pack_equals_convop_pack_on_device(hip, shape, out_scale, dt):
    cw.run_pack("cuda", cw.DT[dt], shape, out_scale)
    if shape == cw.PACK_SHAPES[3]:
        cw.run_pack("cuda", cw.DT[dt], shape, out_scale, need_dx=False)


@pytest.mark.parametrize("name", ["3x3_s2_8x8", "3x3_conv_out_cout4", "t3_T14_c320"])
def test_convop_bwd_dw_on_device(hip, name):
    """ConvOp.bwd_dw through the library: the first micro-batch stores, the second adds, a non-finite incoming gradient raises the flag"""
    from svd_xtend_amd import ops
    c = cw.BY_NAME[name]
    x, dy, _, _, ref = cw.case_reference(c, torch.float16)
    rt = ops.Runtime(torch.float16, torch.device("cuda"))
    rt.found_inf = torch.zeros(1, device="cuda")
    g = torch.Generator().manual_seed(1)
    shape = (c.cout, c.cin, 3, 1, 1) if c.kind == "t3" else (c.cout, c.cin, 3, 3)
    weight = torch.nn.Parameter(torch.randn(*shape, generator=g).cuda())
    bias = torch.nn.Parameter(torch.randn(c.cout, generator=g).cuda())
    weight.grad, bias.grad = torch.full_like(weight, float("nan")), torch.full_like(bias, float("nan"))
    op = ops.ConvOp(weight, bias, c.kind, stride=c.stride, ups=bool(c.ups), cin_pad=c.cin_p, cout_pad=c.cout_p)
    op.pack(rt, out_scale=c.alpha)
    xd, dyd = x.cuda(), dy.cuda()
    rt.grad_overwrite = True
    op.bwd_dw(rt, dyd, xd, c.n_img, c.h, c.w, T=c.T)
    N = c.cout if c.cout % 8 == 0 else 8
    sk = ops._tn_formula(cw.rows_of(c), N, cw.taps_of(c) * c.cin_p)[0]
    vw, bw, vb, bb = cw.bounds(c, ref, sk)
    first_w, first_b = weight.grad.cpu().reshape(vw.shape), bias.grad.cpu()
    assert float(cw._ratio(first_w, vw, bw).max()) <= 1.0 and float(cw._ratio(first_b, vb, bb).max()) <= 1.0
    rt.grad_overwrite = False
    op.bwd_dw(rt, dyd, xd, c.n_img, c.h, c.w, T=c.T)
    vw2, bw2, vb2, bb2 = cw.bounds(c, ref, sk, first_w, first_b)
    assert float(cw._ratio(weight.grad.cpu().reshape(vw.shape), vw2, bw2).max()) <= 1.0
    assert float(cw._ratio(bias.grad.cpu(), vb2, bb2).max()) <= 1.0
    assert float(rt.found_inf) == 0.0
    op.bwd_dw(rt, torch.full_like(dyd, float("inf")), xd, c.n_img, c.h, c.w, T=c.T)
    assert float(rt.found_inf) == 1.0


# ---- the step on the device ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_step_with_convolutions_and_temporal_blocks_matches_oracle(hip, dt):
    ref = sc.oracle_step(cw.CONV_AND_TEMPORAL)
    got = sc.product_step(ref, cw.CONV_AND_TEMPORAL, cw.DT[dt], torch.device("cuda"))
    print(cw.assert_step_parity(f"device conv+temporal {dt}", ref, got, bf16=dt == "bf16"))


def test_step_with_convolutions_alone_matches_oracle(hip):
    ref = sc.oracle_step("@conv")
    got = sc.product_step(ref, "@conv", torch.float16, torch.device("cuda"))
    print(cw.assert_step_parity("device conv f16", ref, got))
    m = got["trainer"].model
    assert not any(mod.has_trainable() for kind, mod in m.steps if kind == "attn")
    assert all(mod.need_dx for kind, mod in m.steps if kind in ("res", "attn", "down", "up")) and all(m._skip_needs_grad)


def test_a_second_sweep_after_zero_grad_gives_the_same_gradients_on_device(hip):
    """zero_grad(); forward_backward(batch) twice, no optimizer step between: every gradient bit-equal (no slot is left to accumulate
    across steps -- the 1x1 shortcuts' bias gradients are zeroed, the others stored)"""
    ref = sc.oracle_step(cw.CONV_AND_TEMPORAL)
    tr = sc.make_trainer(ref, cw.CONV_AND_TEMPORAL, torch.float16, "cuda")
    batch = sc.step_batch(ref, "cuda")
    sweeps = []
    for _ in range(2):
        tr.zero_grad()
        tr.forward_backward(**batch)
        tr.micro = 0
        torch.cuda.synchronize()
        sweeps.append(tr.g_flat[:tr.n_flat].clone())
    assert torch.equal(sweeps[0], sweeps[1]), int((sweeps[0] != sweeps[1]).sum())


def test_captured_step_equals_eager_and_plan_replay_equals_graph_replay(hip):
    """three optimizer steps with trainable convolutions: the captured step walks the eager trajectory bit for bit (the weight-gradient
    launches, the reducing launches and the re-pack are all inside the capture), and the recorded launch plan replays to the same bits"""
    ref = sc.oracle_step(cw.CONV_AND_TEMPORAL)
    eager = sc.run_mode(ref, cw.CONV_AND_TEMPORAL, "eager")
    graph = sc.run_mode(ref, cw.CONV_AND_TEMPORAL, "graph")
    plan = sc.run_mode(ref, cw.CONV_AND_TEMPORAL, "plan")
    assert eager["state"][0] == 3.0
    sc.assert_same_bits(eager, graph, "captured vs eager", min_packed=21)
    sc.assert_same_bits(graph, plan, "plan vs graph", min_packed=21)


def test_planted_nonfinite_conv_gradient_skips_the_step_on_device(hip, monkeypatch):
    from svd_xtend_amd import ops
    ref = sc.oracle_step(cw.CONV_AND_TEMPORAL)
    tr = sc.make_trainer(ref, cw.CONV_AND_TEMPORAL, torch.float16, "cuda")
    target = tr.model.mid_block.resnets[0].temporal_res_block.c2
    packed = [op for op in tr.model._conv_ops if op.trainable]
    before = dict(p=tr.p_flat.clone(), m=tr.m_flat.clone(), v=tr.v_flat.clone(), w=[op.w.clone() for op in packed],
                  wd=[op.wd.clone() for op in packed if op.wd is not None])
    bwd_dw, hit = ops.ConvOp.bwd_dw, []

    def planted(self, rt, dy, x, *a, **k):
        if self is target:
            dy = dy.clone()
            dy[3, 5] = float("inf")
            hit.append(1)
        return bwd_dw(self, rt, dy, x, *a, **k)
    monkeypatch.setattr(ops.ConvOp, "bwd_dw", planted)
    tr.step(sc.step_batch(ref, "cuda"))
    torch.cuda.synchronize()
    assert hit and float(tr.opt_state[7]) == 1.0 and float(tr.opt_state[0]) == 0.0
    assert torch.equal(tr.p_flat, before["p"]) and torch.equal(tr.m_flat, before["m"]) and torch.equal(tr.v_flat, before["v"])
    assert all(torch.equal(op.w, w) for op, w in zip(packed, before["w"]))
    assert all(torch.equal(op.wd, w) for op, w in zip([op for op in packed if op.wd is not None], before["wd"]))


def test_example_trains_convolutions_checkpoints_and_resumes(tmp_path):
    """examples/train_svd_amd.py --trainable_modules temporal_transformer_block,@conv: steps from the captured graph, `checkpoint-2`, a
    resumed run, and the captured loop on the eager loop's loss bit for bit"""
    import train_svd_amd as ex
    common = ["--tiny", "--seed", "7", "--width", "128", "--height", "128", "--num_frames", "3", "--learning_rate", "1e-3",
              "--trainable_modules", "temporal_transformer_block,@conv", "--validation_steps", "100"]
    out = str(tmp_path / "run")
    r = ex.main(common + ["--output_dir", out, "--max_train_steps", "3", "--checkpointing_steps", "2"])
    assert r["global_step"] == 3 and r["train_loss"] == r["train_loss"] and r["train_loss"] > 0
    assert os.path.isdir(os.path.join(out, "checkpoint-2", "unet")) and os.path.isdir(os.path.join(out, "unet"))
    r2 = ex.main(common + ["--output_dir", out, "--max_train_steps", "4", "--checkpointing_steps", "100", "--resume_from_checkpoint", "latest"])
    assert r2["global_step"] == 4 and r2["train_loss"] == r2["train_loss"] and r2["train_loss"] > 0
    b = ex.main(common + ["--output_dir", str(tmp_path / "eager"), "--max_train_steps", "3", "--checkpointing_steps", "100", "--no_graph"])
    assert r["train_loss"] == b["train_loss"], (r, b)
    assert ex.trainable_rules("temporal_transformer_block") == "temporal_transformer_block"
