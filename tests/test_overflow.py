"""A non-finite gradient anywhere skips the step, on the CPU (`-m "not gpu"`): the emulation (tests/emul.py), the HIP sources on the
wave64 simulator (tests/sim) and the host rules on the recording backend (tests/census.py).  tests/overflow_checks.py holds the helpers,
tests/test_overflow_gpu.py runs the same checks on the MI355X.

  1. detector sweeps: one planted non-finite output element per launch of svdx_gemm_tn (every `stages` code, buffer-descriptor and flat
     staging, both dtypes), svdx_grad_finalize_batch, svdx_check_finite_spans, svdx_check_finite; false positives inside NaN surroundings
  2. coverage: flagged destinations + finite_spans cover [0, n_flat) at the real geometries, or the full pass runs
  3. one poisoned weight-gradient launch in a whole Trainer step skips it and changes nothing; the row-sliced routes at op level
  4. svdx_optim_prep over 64-step sequences against GradScaler's rule, the optimizer kernels in a skipped step, two gloo ranks
  6. four planted faults, each of which must fail the named check

Shares on the CPU (launch counts are printed by the tests): the emulation runs the full position lists at stages 0 and 18 (it has one
code path per output mode) and one poisoned step per distinct (R, N, K, out_mode) of the tiny step; the simulator runs corners and tile
seams at every `stages` code, the full walk at the default tile, and the first and the last launch of the fp16 tiny step.
What f16 operands cannot isolate: one output ELEMENT in store mode (no product of two halves overflows fp32) -- rows and columns there."""
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

import emul  # noqa: E402
import overflow_checks as oc  # noqa: E402
from svd_xtend_amd import kernels as K  # noqa: E402
from svd_xtend_amd import ops  # noqa: E402

CPU = "cpu"
DTS = (torch.float16, torch.bfloat16)


@pytest.fixture(scope="module")
def sim():
    from backend import SimBackend
    return SimBackend()


@pytest.fixture
def emu():
    return emul.EmuBackend()


def _ok(bad):
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad[:20])


# ---- 1. detector sweeps ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stages", (0, 18))
def test_gemm_tn_raises_the_flag_from_every_output_position_on_emulation(emu, stages):
    bad, n = oc.tn_sweeps(emu, CPU, stages, quick=False)
    print(f"stages={stages}: {n} launches")
    _ok(bad + oc.tn_flag_scope(emu, CPU, torch.float16, stages, refuses=False))


@pytest.mark.parametrize("flat", (0, K.TN_FLAT))
@pytest.mark.parametrize("stages", oc.TN_STAGES)
def test_gemm_tn_raises_the_flag_at_corners_and_seams_on_simulator(sim, stages, flat):
    bad, n = oc.tn_sweeps(sim, CPU, stages | flat, quick=True)
    print(f"stages={stages} flat={bool(flat)}: {n} launches")
    for dt in DTS:
        bad += oc.tn_flag_scope(sim, CPU, dt, stages | flat)
    _ok(bad)


def test_gemm_tn_raises_the_flag_from_every_row_and_column_on_simulator(sim):
    """the full walk at the default 128 x 128 tile, partial-tile shape: += (f16), the bf16 store form, the f16 rows and columns"""
    shape = oc.tn_shapes(0)[0]
    bad, n = oc.tn_plant_add(sim, CPU, torch.float16, 0, shape)
    for fn in (oc.tn_plant_store_bf16, oc.tn_plant_store_f16):
        b, k = fn(sim, CPU, 0, shape)
        bad, n = bad + b, n + k
    print(f"{n} launches")
    _ok(bad)


@pytest.mark.parametrize("which", ("emulation", "simulator"))
def test_finalize_pack_and_finite_checks_see_every_planted_value(which, emu, request):
    be = emu if which == "emulation" else request.getfixturevalue("sim")
    bad = []
    for fn in (oc.gradfin_sweep, oc.finite_spans_sweep, oc.finite_flat_sweep):
        b, n = fn(be, CPU)
        print(f"{fn.__name__}: {n} launches")
        bad += b
    _ok(bad)


# ---- 2. coverage ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", oc.COVERAGE_CONFIGS)
def test_every_gradient_float_has_a_detector(name):
    cov = oc.coverage_step(name)
    mb = cov["micro"][0]
    print(f"{name}: n_flat {cov['n_flat']}, {len(mb['tn'])} flagged gemm_tn launches, {len(mb['fin'])} flagged reducing jobs, "
          f"{len(cov['finite_spans'])} finite_spans rows, finite checks run: {[e for e in cov['tail'] if 'finite' in e]}")
    assert cov["found_inf"] and "check_finite" not in cov["tail"], "a single-rank step with write-once gradients folds the check"
    if name == "c4":
        assert len(cov["micro"]) == 2 and cov["micro"][1]["tn"] and all(mode == K.OUT_F32_ADD for _, mode in cov["micro"][1]["tn"])
        assert all(not store for _, store in cov["micro"][1]["fin"])
    if name in ("c2", "c4", "c5"):
        assert mb["fin"], "the benchmark geometries row-slice"
    _ok(oc.coverage_verdict(cov, name))


def test_a_single_launch_reduction_sends_the_step_to_the_full_pass():
    """rt.defer_grad_finalize = False on a geometry that row-slices: svdx_gemm_finalize writes write-once gradients without a flag, so the
    optimizer runs svdx_check_finite over n_flat"""
    cov = oc.coverage_step("c2", dict(defer_grad_finalize=False))
    assert cov["micro"][0]["single"] and not cov["micro"][0]["fin"]
    assert "check_finite" in cov["tail"] and "check_finite_spans" not in cov["tail"], cov["tail"]
    _ok(oc.coverage_verdict(cov, "c2, immediate finalize"))


# ---- 3. one poisoned launch, whole step -------------------------------------------------------------------------------------------------------
def test_one_poisoned_launch_skips_the_fp16_step_on_emulation(emu):
    bad, n, ran = oc.poisoned_steps(emu, CPU, torch.float16)
    print(f"{n} flagged gemm_tn launches, {ran} poisoned steps (one per distinct (R, N, K, out_mode))")
    assert n == 96
    _ok(bad)


@pytest.mark.parametrize("rank", (8, 64))
def test_one_poisoned_launch_skips_the_bf16_lora_step_on_emulation(emu, rank):
    """rank 8 is padded to the K granule of 64: its gradients pass through a float scratch and a torch add, nothing is write-once and the
    step takes the full pass (no launch carries the flag).  Rank 64 is the folded route of configuration 5."""
    bad, n, ran = oc.poisoned_steps(emu, CPU, torch.bfloat16, lora_r=rank)
    print(f"rank {rank}: {n} flagged gemm_tn launches, {ran} poisoned steps")
    assert (n > 0) == (rank == 64)
    _ok(bad)


@pytest.mark.parametrize("case", ("grad_accum=2", "max_grad_norm=1.0", "fold_finite=False"))
def test_one_poisoned_launch_skips_the_step_in_the_other_modes_on_emulation(emu, case):
    kw = dict(grad_accum=2) if case == "grad_accum=2" else dict(max_grad_norm=1.0) if case == "max_grad_norm=1.0" else {}
    bad, n, ran = oc.poisoned_steps(emu, CPU, torch.float16, pick="three", rt_attrs=dict(fold_finite=False) if case == "fold_finite=False" else None, **kw)
    print(f"{case}: {n} gemm_tn launches per step, {ran} poisoned steps")
    _ok(bad)


def test_one_poisoned_launch_skips_the_fp16_step_on_simulator(sim):
    bad, _, ran = oc.poisoned_steps(sim, CPU, torch.float16, pick=(0, 95))
    print(f"{ran} poisoned steps (the first and the last of the 96 launches; the clean step after them runs on the emulation and the GPU)")
    _ok(bad)


@pytest.mark.parametrize("which", ("emulation", "simulator"))
def test_row_sliced_weight_gradients_raise_the_flag_on_both_routes(which, emu, request):
    be = emu if which == "emulation" else request.getfixturevalue("sim")
    bad = []
    for shape in ((128, 128), (320, 64)):
        for overwrite in (True, False):
            for defer in (True, False):
                if which == "simulator" and (overwrite, defer) not in ((True, True), (False, False)):
                    continue                                       # the kernels are the same four; the host routes all run on the emulation
                bad += oc.op_level_row_sliced(be, CPU, torch.float16 if shape[1] == 128 else torch.bfloat16, shape, overwrite, defer)
    _ok(bad)


def test_a_non_finite_accumulated_slot_skips_and_the_loss_slot_does_not_on_emulation(emu):
    with oc.backend(emu):
        tr, batch = oc.tiny_trainer(CPU, torch.float16)
        bad, n = oc.accumulated_slots(tr, batch)
    print(f"{len(tr.finite_spans)} finite_spans rows, {n} optimizer steps")
    assert len(tr.finite_spans) == len([1 for c, _ in tr.zero_spans.tolist() if c < tr.n_flat])
    _ok(bad)


# ---- 4. state machine and the skipped optimizer ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ("emulation", "simulator"))
def test_optim_prep_follows_grad_scaler_over_sequences(which, emu, request):
    be = emu if which == "emulation" else request.getfixturevalue("sim")
    bad = []
    for interval in oc.INTERVALS:
        for dynamic in (True, False):
            for name, seq in oc.prep_sequences(interval).items():
                bad += oc.prep_sequence_check(be, CPU, seq, interval, dynamic, f"{name}, interval {interval}, dynamic {dynamic}")
    _ok(bad)


def test_restated_rule_equals_torch_grad_scaler():
    """the few lines of overflow_checks.grad_scaler_rule against torch.amp.GradScaler itself on the CPU, where this torch runs it there"""
    ran = 0
    for interval in oc.INTERVALS:
        for name, seq in oc.prep_sequences(interval).items():
            trace = oc.torch_grad_scaler_trace(seq, interval)
            if trace is None:
                continue
            ran += 1
            scale, tracker, steps = 65536.0, 0.0, 0
            for i, found in enumerate(seq):
                scale, tracker = oc.grad_scaler_rule(scale, tracker, found, interval, True)
                steps += 0 if found else 1
                assert trace[i] == (scale, tracker, steps), (name, interval, i, trace[i], (scale, tracker, steps))
    print(f"{ran} sequences compared with torch.amp.GradScaler")


@pytest.mark.parametrize("which", ("emulation", "simulator"))
def test_optimizer_kernels_change_nothing_in_a_skipped_step(which, emu, request):
    be = emu if which == "emulation" else request.getfixturevalue("sim")
    bad = []
    for dt in DTS:
        bad += oc.skipped_adamw(be, CPU, dt)
    _ok(bad + oc.skipped_adamw(be, CPU, torch.float16, skip=False) + oc.skipped_clip_coef(be, CPU))


def _rank_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(2)
    for p in (ROOT, HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    import emul as emul_
    import overflow_checks as oc_
    from svd_xtend_amd import kernels
    be = emul_.EmuBackend()
    kernels._set_backend_for_tests(be)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    tr, batch = oc_.tiny_trainer("cpu", torch.float16)
    assert tr.world == world and tr.rt.found_inf is None              # the SUM over ranks is what has to be tested: the full pass
    before = oc_.snapshot(tr)
    with oc_.PoisonTN(be, 40 if rank == 1 else None) as p:           # rank 1 alone holds one inf in one write-once gradient
        tr.step(batch)
    assert len(p.log) == 96 and not any(e["flagged"] for e in p.log)
    skipped = oc_.snapshot(tr)
    tr.step(batch)
    torch.save(dict(before=before, skipped=skipped, after=oc_.snapshot(tr)), os.path.join(out, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_ranks_skip_together_when_one_rank_overflows(tmp_path):
    port = 29500 + (os.getpid() + 1331) % 2000
    mp.spawn(_rank_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r = [torch.load(tmp_path / f"r{q}.pt") for q in range(2)]
    for q in range(2):
        b, s, a = r[q]["before"], r[q]["skipped"], r[q]["after"]
        assert s["st"].tolist()[:4] == [0.0, 0.5 * float(b["st"][1]), 0.0, 0.0] and float(s["st"][7]) == 1.0, (q, s["st"][:8].tolist())
        for k_ in ("p", "m", "v", "w16", "wt16"):
            assert oc.same_bits(b[k_], s[k_]), (q, k_)
        assert float(a["st"][0]) == 1.0 and float(a["st"][7]) == 0.0 and not oc.same_bits(a["p"], s["p"])
    for phase in ("skipped", "after"):
        for k_ in ("st", "p"):
            assert oc.same_bits(r[0][phase][k_], r[1][phase][k_]), (phase, k_)


# ---- 6. the tests bite: four planted faults ---------------------------------------------------------------------------------------------------
class BlindLastColumns(emul.EmuBackend):
    """the emulated gemm_tn ignores the last 8 columns of C for the flag"""

    def gemm_tn(self, A, B, C, R, N, Kd, lda, ldb, ldc, out_mode=K.OUT_F32_ADD, split_k=1, a_colsum=None, stages=0, found_inf=None):
        super().gemm_tn(A, B, C, R, N, Kd, lda, ldb, ldc, out_mode, split_k, a_colsum, stages, None)
        if found_inf is not None and out_mode != K.OUT_F32_SLAB and not torch.isfinite(emul.V(C, N, Kd - 8, ldc)).all():
            found_inf[0] = 1.0


class TwinIgnoresSkip(emul.EmuBackend):
    """adamw_tiled ignores opt_state[7] for the transposed twin"""

    def adamw_tiled(self, p, g, m, v, tiles, n_tiles, lr, beta1, beta2, eps, wd, grad_mul, st, p_act, pt_act, param_mode=0):
        super().adamw_tiled(p, g, m, v, tiles, n_tiles, lr, beta1, beta2, eps, wd, grad_mul, st, p_act, pt_act, param_mode)
        if float(st[7]) > 0:
            for off, ld, rows, cols, wt_off, ldwt in tiles[:n_tiles].view(-1, 6).tolist():
                if wt_off >= 0:
                    P = torch.as_strided(p, (rows, cols), (ld, 1), p.storage_offset() + off) * (1 - lr * wd)
                    torch.as_strided(pt_act, (cols, rows), (ldwt, 1), pt_act.storage_offset() + wt_off).copy_(P.t().to(pt_act.dtype))


def test_planted_fault_flag_blind_to_the_last_columns_fails_the_detector_sweep():
    be = BlindLastColumns()
    for stages in (0, 18):
        shape = oc.tn_shapes(stages)[0]
        for bad, _ in (oc.tn_plant_add(be, CPU, torch.float16, stages, shape), oc.tn_plant_store_bf16(be, CPU, stages, shape),
                       oc.tn_plant_store_f16(be, CPU, stages, shape)):
            assert bad and all("not raised" in b for b in bad), bad[:3]
            print(f"stages={stages}: {len(bad)} launches reported, e.g. {bad[0]}")
    assert not oc.tn_plant_add(emul.EmuBackend(), CPU, torch.float16, 0, oc.tn_shapes(0)[0])[0]


def test_planted_fault_dropped_finite_spans_row_fails_coverage_and_the_slot_test(monkeypatch, emu):
    from svd_xtend_amd.train import Trainer
    build = Trainer._build_runtime

    def dropped(self):
        build(self)
        if self.finite_spans is not None:
            self.finite_spans = torch.cat([self.finite_spans[:3], self.finite_spans[4:]]).contiguous()
    monkeypatch.setattr(Trainer, "_build_runtime", dropped)
    bad = oc.coverage_verdict(oc.coverage_step("tiny_fp16"), "tiny_fp16")
    print(bad)
    assert any("without a detector" in b for b in bad)
    with oc.backend(emu):
        tr, batch = oc.tiny_trainer(CPU, torch.float16)
        bad, _ = oc.accumulated_slots(tr, batch, rows=[3])
    print(bad)
    assert any("not skipped" in b for b in bad)


def test_planted_fault_no_flag_in_accumulate_mode_fails_c4_coverage_and_the_grad_accum_step(monkeypatch, emu):
    real = ops.gemm_tn_acc

    def faulty(rt, dy, x, dst, M, N, Kd, lda, ldb, a_colsum=None, write_once=False):
        if write_once and not rt.grad_overwrite:                    # the += form: found = None
            keep, rt.found_inf = rt.found_inf, None
            try:
                return real(rt, dy, x, dst, M, N, Kd, lda, ldb, a_colsum, write_once)
            finally:
                rt.found_inf = keep
        return real(rt, dy, x, dst, M, N, Kd, lda, ldb, a_colsum, write_once)
    for mod in [m for n, m in list(sys.modules.items()) if n.startswith("svd_xtend_amd") and vars(m).get("gemm_tn_acc") is real]:
        monkeypatch.setattr(mod, "gemm_tn_acc", faulty)
    bad = oc.coverage_verdict(oc.coverage_step("c4"), "c4")
    print(bad[:3])
    assert any("micro-batch 1" in b for b in bad)
    with oc.backend(emu):
        tr, batch = oc.tiny_trainer(CPU, torch.float16, grad_accum=2)
        log = oc.tn_launches(tr, batch)
        assert not any(e["flagged"] for e in log[len(log) // 2:])
        # (a launch without column sums riding on it: those land in an accumulated slot, which the span check would still see)
        target = [i for i, e in enumerate(log) if i >= len(log) // 2 and not e["colsum"]][0]
        bad = oc.skipped_step(tr, batch, target, then_clean=False)
    print(bad[:3])
    assert any("not skipped" in b for b in bad)


def test_planted_fault_transposed_twin_written_in_a_skipped_step_fails_the_optimizer_check():
    bad = oc.skipped_adamw(TwinIgnoresSkip(), CPU, torch.float16)
    print(bad)
    assert bad and all("pt_act changed" in b for b in bad)
