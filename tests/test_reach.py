"""How far an operand reaches in memory, on the CPU (`-m "not gpu"`): the pitched cases of tests/reach_checks.py through the HIP sources on
the wave64 simulator (tests/sim).  A CPU `torch.zeros` of 4 GiB is mapped lazily and only the rows a case touches are committed.  The
simulator's buffer resources enforce num_records: an access beyond it reads zero or is dropped, as on the device, and shows through the
values (the float64 reference, the NaN prefill) -- the kernels rely on that rule for their ragged edges, so it is no error by itself; an
access whose range check depends on the scalar offset is counted by the simulator (SimBackend.range_reports) and fails the case.  tests/test_reach_gpu.py runs the same list on the device, where the spatial attention takes the census shape
(S >= 160) instead of the largest smaller S that runs here.

The quick pass keeps one signature per reach_checks.coarse_key; SVDX_SIM_FULL=1 runs one per feature combination."""
import os
import sys

import pytest
import torch

import census
import kernel_checks as kc
import reach_checks as rc
from svd_xtend_amd import kernels as K

FULL = os.environ.get("SVDX_SIM_FULL") == "1"


@pytest.fixture(scope="module")
def sim():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "sim"))
    from backend import SimBackend
    return SimBackend()


def _report(cases, worst):
    print(f"{len(cases)} cases: " + ", ".join(f"{c.level}:{c.operand}={census.reach(c.sig)[c.operand]}" + (" refused" if (c.verdict or "").startswith("refused") else "")
                                             for c in cases[:12]) + (" ..." if len(cases) > 12 else ""))
    for k, w in sorted(worst.items()):
        print(f"{w:8.3f}  {k[0]} at ({k[1]})")


def test_the_pitch_solver_lands_on_the_line():
    """(i) is the last admissible pitch below 2^31 bytes, (ii) the first at or beyond it, (iii) the first at or beyond 2^32; the forms
    the library refuses at (ii) are the dual, GroupNorm-statistics and fused-GEGLU launches, each with its accepted neighbour at (i)"""
    n, refused = 0, set()
    for entry, args in rc.PITCHES.items():
        for arg in args:
            cases = rc.pitched_cases(entry, arg)
            assert cases, (entry, arg)
            assert {c.level for c in cases} == set(rc.LEVELS), (entry, arg)
            for c in cases:
                ext = census.reach(c.sig)[c.operand]
                assert census.reach_class(ext) == list(rc.LEVELS).index(c.level), (c.entry, c.arg, c.level, ext)
                if c.verdict is not None and c.verdict.startswith("refused"):
                    a = census.sig_args(c.sig)
                    refused.add("dual" if a["dual"] is not None else "gn" if a["gn"] is not None else "epilogue")
                    assert c.level != "i" and any(d.base == c.base and d.arg == c.arg and d.level == "i" and not (d.verdict or "").startswith("refused") for d in cases)
                n += 1
    print(f"{n} pitched cases over {len(rc.PITCH_IDS)} pitch arguments; refused forms: {sorted(refused)}")
    assert refused == {"dual", "gn", "epilogue"}


@pytest.mark.parametrize("which", rc.PITCH_IDS)
def test_hip_sources_meet_float64_reference_on_both_sides_of_the_line(sim, which):
    entry, arg = which.split("-", 1)
    reports = sim.range_reports()
    cases = rc.pitched_cases(entry, arg, sim=True, full=FULL)
    if entry == "gemm_tn":
        cases = cases + rc.flat_staging(cases)
    worst = {}
    bad = rc.run_pitched(sim, "cpu", cases, worst)
    _report(cases, worst)
    assert sim.range_reports() == reports, "buffer accesses whose range check depends on the scalar offset"
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("shape", rc.T_LIMIT_CASES, ids=lambda s: "x".join(map(str, s)))
def test_temporal_attention_at_its_stated_limit_on_the_simulator(sim, shape):
    for dt in ("f16", "bf16"):
        for sig in rc.tattn_signatures(*shape, dt=dt):
            res = census.run_case(sim, sig, "cpu")
            for label, e, idx in res:
                print(f"{e:8.3f}  {sig[0]} {dt} {label}")
            assert all(e <= 1.0 for _, e, _ in res), (res, census.sig_str(sig))


def test_temporal_attention_beyond_its_limit_is_refused(sim):
    B, T, HW, heads = 1, rc.T_REFUSED, 4, 1
    for sig in rc.tattn_signatures(B, T, HW, heads):
        ops = []
        with pytest.raises(K.SvdxError, match="T<=32"):
            census.run_case(sim, sig, "cpu", operands_out=ops)
        outs = [n for n, d in ops[0].decls.items() if d[2]]
        assert outs and all(bool(torch.isnan(ops[0].t[n].float()).all()) for n in outs)
    # (and one step below: T_LIMIT_CASES[0], T = 32)
    assert rc.T_LIMIT_CASES[0][1] == rc.T_REFUSED - 1


def test_temporal_attention_limit_shapes_are_in_the_kernel_checks():
    import inspect
    src = inspect.getsource(kc.check_temporal_attention)
    assert all(repr(s) in src for s in rc.T_LIMIT_CASES)


# ---- the windowed judging of the 4 GiB cases (tests/test_reach_gpu.py), at a size the simulator runs ----------------------------------------
SMALL_LINES = (1 << 22, 1 << 23)            # byte offsets the windows straddle here, in place of 2^31 and 2^32


@pytest.mark.parametrize("entry", list(rc.WINDOWED))
def test_windowed_judging_passes_the_hip_sources_at_small_lines(sim, entry):
    """one launch over operands of 8 MiB, the entry's runner on the first units, the last and those that straddle 4 MiB and 8 MiB"""
    base = rc.base_4g(entry, list(rc.WINDOWED).index(entry))
    res, found, starts = rc.run_windowed(sim, "cpu", base, lines=SMALL_LINES, W=min(rc.WINDOWED[entry][1], 1 << 10))
    print(f"{entry}: windows at units {starts}, worst excess {max(e for _, e, _ in res):.3f}")
    assert len(starts) >= 2 and not found and all(e <= 1.0 for _, e, _ in res), (found, [r for r in res if not r[1] <= 1.0])


class _Wrapping:
    """svdx_add whose count wraps at `line` elements: the elements beyond are never written, the first ones are written twice"""

    def __init__(self, be, line):
        self.be, self.line = be, line

    def add(self, a, b, out, n):
        self.be.add(a, b, out, min(n, self.line))
        if n > self.line:
            self.be.add(a[self.line:], b[self.line:], out, n - self.line)


def test_windowed_judging_notices_a_count_that_wraps(sim):
    base = rc.base_4g("add", 0)
    line = SMALL_LINES[1] // 2                                # the element at byte offset SMALL_LINES[1]
    res, found, starts = rc.run_windowed(_Wrapping(sim, line), "cpu", base, lines=SMALL_LINES, W=1 << 10)
    flagged = [label for label, e, _ in res if not e <= 1.0]
    print(flagged, found)
    assert any("is nan after the launch" in f for f in found), found                         # the scan: elements left unwritten
    assert any(label.startswith(f"units {starts[-1]}") for label in flagged)               # the last window holds the prefill
    assert any(label.startswith("units 0..") for label in flagged)                          # the first was written twice


@pytest.mark.parametrize("dt", (torch.float16, torch.bfloat16), ids=("f16", "bf16"))
def test_gemm_tn_gather_is_served_one_step_below_its_span_limit_and_refused_at_it(sim, dt):
    c, R, N, served, refused = rc.gather_limit()
    worst = rc.run_gather_limit(sim, "cpu", dt)
    print(f"{c.name}: dY pitch {served} served (span {((R - 1) * served + N) * 2} bytes, worst error / bound {worst}), {refused} refused")


def test_tsa_fwd_windows_of_pixels_and_the_refusal_at_its_limit(sim):
    """the windowed judging the device applies to svdx_tsa_fwd one step below its limit, here over 640 pixels of 3 frames (C = 128), and the
    refusal itself, which launches nothing: M 3C 2 >= 2^31 bytes through rows that are never touched"""
    res, found, starts = rc.run_windowed(sim, "cpu", rc.tsa_signature(1, 3, 64, C=128), lines=(1 << 19, 1 << 20), W=16, units=640)
    print(f"windows at pixels {starts}, worst excess {max(e for _, e, _ in res):.3f}")
    assert len(starts) >= 3 and not found and all(e <= 1.0 for _, e, _ in res), (found, [r for r in res if not r[1] <= 1.0])
    refused = rc.tsa_signature(*rc.TSA_REFUSED)
    assert census.gemm_kernel_taken(rc.tsa_signature(*rc.TSA_SERVED)) == "tsa_fwd kernel"
    o = census._DeclaredOperands(refused, "cpu")
    a = census.sig_args(refused)
    try:
        census.RUNNERS["tsa_fwd"](None, o, a)
    except census._Declared:
        pass
    t = {n: torch.zeros(ext, dtype=census.DT_OF[o.desc[n][1]]) for n, (ext, _, _) in o.decls.items()}          # lazily mapped: nothing is touched
    outs = [n for n, d in o.decls.items() if d[2]]
    for n in outs:
        t[n][:4096] = float("nan")
    kw = {k: census._rebuild(v, t, k) for k, v in refused[1]}
    with pytest.raises(K.SvdxError, match="activation too large for 32-bit buffer offsets"):
        sim.tsa_fwd(*kw.values())
    assert all(bool(torch.isnan(t[n][:4096]).all()) for n in outs)
