"""`-m gpu`: the GroupNorm affine gradients on the device -- every kernel case of tests/gn_affine_checks.py in fp16 and bf16 against the
float64 reference (computed on the CPU, shared with the simulator's run of the same case), and the step with "@norm" through the real
library: against the oracle, sweep == sweep, captured == eager == plan replay, the planted non-finite gradient, the example end to end."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

import gn_affine_checks as ga  # noqa: E402
import selection_checks as sc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from svd_xtend_amd import kernels
    return kernels.backend()


def test_block_count_matches_the_library(hip):
    from svd_xtend_amd import kernels as K
    for n_s, rows, C in [tuple(c) for c in ga.CASES] + [(14, 2560, 320), (14, 40, 1280), (1, 35840, 320), (14, 640, 2560)]:
        assert K.gn_bwd_blocks(n_s, rows, C, 32) == hip.lib.svdx_gn_bwd_blocks(n_s, rows, C, 32) > 0


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("name", [c.name for c in ga.CASES])
def test_kernel_case_on_device(hip, name, dt):
    ga.sweep_case(hip, "cuda", ga.BY_NAME[name], ga.DT[dt], verbose=True)


# ---- the step on the device ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("which", [ga.TEMPORAL_NORM, ga.ALL_THREE], ids=["temporal+norm", "temporal+conv+norm"])
def test_step_matches_oracle(hip, which, dt):
    ref = sc.oracle_step(which)
    got = sc.product_step(ref, which, ga.DT[dt], torch.device("cuda"))
    print(ga.assert_step_parity(f"device {which} {dt}", ref, got, bf16=dt == "bf16"))


def test_conv_norm_out_alone_matches_oracle(hip):
    ref = sc.oracle_step("conv_norm_out")
    got = sc.product_step(ref, "conv_norm_out", torch.float16, torch.device("cuda"))
    print(ga.assert_step_parity("device conv_norm_out f16", ref, got))
    m = got["trainer"].model
    assert m._any_trainable and not m._sweep_needed


def test_a_second_sweep_after_zero_grad_gives_the_same_gradients_on_device(hip):
    ref = sc.oracle_step(ga.ALL_THREE)
    tr = sc.make_trainer(ref, ga.ALL_THREE, torch.float16, "cuda")
    batch = sc.step_batch(ref, "cuda")
    sweeps = []
    for _ in range(2):
        tr.zero_grad()
        tr.forward_backward(**batch)
        tr.micro = 0
        torch.cuda.synchronize()
        sweeps.append(tr.g_flat[:tr.n_flat].clone())
    assert torch.equal(sweeps[0], sweeps[1]), int((sweeps[0] != sweeps[1]).sum())
    gn = set(sc.gn_names(tr.model))
    assert all(float(p.grad.abs().max()) > 0 for n, p in tr.model.named_parameters() if n in gn)


def test_captured_step_equals_eager_and_plan_replay_equals_graph_replay(hip):
    """three optimizer steps with trainable norms (and convolutions, whose re-made inputs read the updated affines): the captured step
    walks the eager trajectory bit for bit -- masters, moments, loss, optimizer state -- and the recorded launch plan replays to the same"""
    ref = sc.oracle_step(ga.ALL_THREE)
    eager = sc.run_mode(ref, ga.ALL_THREE, "eager")
    graph = sc.run_mode(ref, ga.ALL_THREE, "graph")
    plan = sc.run_mode(ref, ga.ALL_THREE, "plan")
    assert eager["state"][0] == 3.0
    sc.assert_same_bits(eager, graph, "captured vs eager")
    sc.assert_same_bits(graph, plan, "plan vs graph")


def test_planted_nonfinite_norm_gradient_skips_the_step_on_device(hip, monkeypatch):
    from svd_xtend_amd import ops
    ref = sc.oracle_step(ga.TEMPORAL_NORM)
    tr = sc.make_trainer(ref, ga.TEMPORAL_NORM, torch.float16, "cuda")
    target = tr.model.mid_block.resnets[0].temporal_res_block.gn2
    before = dict(p=tr.p_flat.clone(), m=tr.m_flat.clone(), v=tr.v_flat.clone())
    bwd, hit = ops.GroupNormOp.bwd, []

    def planted(self, rt, dy, x, *a, **k):
        if self is target:
            dy = dy.clone()
            dy[3, 5] = float("inf")
            hit.append(1)
        return bwd(self, rt, dy, x, *a, **k)
    monkeypatch.setattr(ops.GroupNormOp, "bwd", planted)
    tr.step(sc.step_batch(ref, "cuda"))
    torch.cuda.synchronize()
    assert hit and float(tr.opt_state[7]) == 1.0 and float(tr.opt_state[0]) == 0.0
    assert torch.equal(tr.p_flat, before["p"]) and torch.equal(tr.m_flat, before["m"]) and torch.equal(tr.v_flat, before["v"])


def test_example_trains_norms_checkpoints_and_resumes(tmp_path):
    """examples/train_svd_amd.py --trainable_modules temporal_transformer_block,@norm: steps from the captured graph, `checkpoint-2`, a
    resumed run, and the captured loop on the eager loop's loss bit for bit"""
    import train_svd_amd as ex
    common = ["--tiny", "--seed", "7", "--width", "128", "--height", "128", "--num_frames", "3", "--learning_rate", "1e-3",
              "--trainable_modules", "temporal_transformer_block,@norm", "--validation_steps", "100"]
    out = str(tmp_path / "run")
    r = ex.main(common + ["--output_dir", out, "--max_train_steps", "3", "--checkpointing_steps", "2"])
    assert r["global_step"] == 3 and r["train_loss"] == r["train_loss"] and r["train_loss"] > 0
    assert os.path.isdir(os.path.join(out, "checkpoint-2", "unet")) and os.path.isdir(os.path.join(out, "unet"))
    r2 = ex.main(common + ["--output_dir", out, "--max_train_steps", "4", "--checkpointing_steps", "100", "--resume_from_checkpoint", "latest"])
    assert r2["global_step"] == 4 and r2["train_loss"] == r2["train_loss"] and r2["train_loss"] > 0
    b = ex.main(common + ["--output_dir", str(tmp_path / "eager"), "--max_train_steps", "3", "--checkpointing_steps", "100", "--no_graph"])
    assert r["train_loss"] == b["train_loss"], (r, b)
    assert ex.trainable_rules("temporal_transformer_block,@norm") == ("temporal_transformer_block", "@norm")
