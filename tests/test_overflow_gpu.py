"""A non-finite gradient anywhere skips the step, on the MI355X (`-m gpu`): the checks of tests/overflow_checks.py through HipBackend.

  1. one planted non-finite output element per svdx_gemm_tn launch: the full position list (corners, both sides of every tile seam,
     a walk that visits every output row and column) at every `stages` code, buffer-descriptor and flat staging, f16 and bf16, += and store;
     finite operands inside NaN surroundings; svdx_grad_finalize_batch, svdx_check_finite_spans, svdx_check_finite
  3. every one of the 96 flagged weight-gradient launches of the fp16 tiny step poisoned in turn, every launch of the bf16 rank-8 LoRA step
     (none flagged: a padded rank takes the full pass), one launch per distinct shape of the rank-64 LoRA step, with grad_accum = 2 (second
     micro-batch), with clipping and with the fold switched off; the row-sliced routes at op level; every accumulated slot
  4. svdx_optim_prep over the 64-step sequences, the optimizer kernels in a skipped step
Every test is one part of a few seconds; the launch counts are printed (profiles/overflow_gpu.txt)."""
import pytest
import torch

import overflow_checks as oc
from svd_xtend_amd import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def hip():
    return K.HipBackend()


def _ok(bad):
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad[:20])


@pytest.mark.parametrize("flat", (0, K.TN_FLAT))
@pytest.mark.parametrize("stages", oc.TN_STAGES)
def test_gemm_tn_raises_the_flag_from_every_output_position(hip, stages, flat):
    bad, n = oc.tn_sweeps(hip, DEV, stages | flat, quick=False)
    print(f"stages={stages} flat={bool(flat)}: {n} launches")
    for dt in (torch.float16, torch.bfloat16):
        bad += oc.tn_flag_scope(hip, DEV, dt, stages | flat)
    _ok(bad)


def test_finalize_pack_and_finite_checks_see_every_planted_value(hip):
    bad = []
    for fn in (oc.gradfin_sweep, oc.finite_spans_sweep, oc.finite_flat_sweep):
        b, n = fn(hip, DEV)
        print(f"{fn.__name__}: {n} launches")
        bad += b
    _ok(bad)


@pytest.mark.parametrize("part", range(6))
def test_every_flagged_launch_of_the_fp16_step_skips_it(hip, part):
    bad, n, ran = oc.poisoned_steps(hip, DEV, torch.float16, pick="all", part=(part, 6))
    print(f"part {part}: {ran} of {n} flagged gemm_tn launches poisoned")
    assert n == 96 and ran == 16
    _ok(bad)


@pytest.mark.parametrize("part", range(8))
def test_every_weight_gradient_launch_of_the_bf16_rank8_lora_step_skips_it(hip, part):
    bad, n, ran = oc.poisoned_steps(hip, DEV, torch.bfloat16, lora_r=8, pick="all", part=(part, 8))
    print(f"part {part}: {ran} gemm_tn launches poisoned, {n} of the step's carry the flag (padded rank: the full pass)")
    assert n == 0 and ran == 32
    _ok(bad)


@pytest.mark.parametrize("case", ("lora rank 64", "grad_accum=2", "max_grad_norm=1.0", "fold_finite=False"))
def test_one_poisoned_launch_per_distinct_shape_skips_the_step_in_the_other_modes(hip, case):
    kw = dict(grad_accum=2) if case == "grad_accum=2" else dict(max_grad_norm=1.0) if case == "max_grad_norm=1.0" else {}
    lora = case == "lora rank 64"
    bad, n, ran = oc.poisoned_steps(hip, DEV, torch.bfloat16 if lora else torch.float16, lora_r=64 if lora else 0,
                                    rt_attrs=dict(fold_finite=False) if case == "fold_finite=False" else None, **kw)
    print(f"{case}: {n} flagged gemm_tn launches per step, {ran} poisoned steps")
    assert (n > 0) == (case != "fold_finite=False")
    _ok(bad)


def test_row_sliced_weight_gradients_raise_the_flag_on_both_routes(hip):
    bad = []
    for shape in ((128, 128), (320, 64)):
        for dt in (torch.float16, torch.bfloat16):
            for overwrite in (True, False):
                for defer in (True, False):
                    bad += oc.op_level_row_sliced(hip, DEV, dt, shape, overwrite, defer)
    _ok(bad)


def test_a_non_finite_accumulated_slot_skips_and_the_loss_slot_does_not(hip):
    with oc.backend(hip):
        tr, batch = oc.tiny_trainer(DEV, torch.float16)
        bad, n = oc.accumulated_slots(tr, batch)
    print(f"{len(tr.finite_spans)} finite_spans rows, {n} optimizer steps")
    _ok(bad)


def test_optim_prep_follows_grad_scaler_over_sequences(hip):
    bad, n = [], 0
    for interval in oc.INTERVALS:
        for dynamic in (True, False):
            for name, seq in oc.prep_sequences(interval).items():
                bad += oc.prep_sequence_check(hip, DEV, seq, interval, dynamic, f"{name}, interval {interval}, dynamic {dynamic}")
                n += len(seq)
    print(f"{n} launches")
    _ok(bad)


def test_optimizer_kernels_change_nothing_in_a_skipped_step(hip):
    bad = []
    for dt in (torch.float16, torch.bfloat16):
        bad += oc.skipped_adamw(hip, DEV, dt)
    _ok(bad + oc.skipped_adamw(hip, DEV, torch.float16, skip=False) + oc.skipped_clip_coef(hip, DEV))
