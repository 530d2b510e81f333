"""How far an operand reaches in memory, on the MI355X (`-m gpu`): tests/reach_checks.py through HipBackend.

* the pitched cases of tests/test_reach.py (every entry that takes a pitch, its operand's extent just below 2^31 bytes, at 2^31 and at
  2^32), the spatial attention at the census shape (S >= 160) the simulator does not run; the refusals at the line, each beside its
  accepted neighbour one step below;
* svdx_tsa_fwd at M 3C 2 = 2^31 - 128 bytes (served, judged on windows of pixels) and beyond 2^31 (refused);
* svdx_gemm_tn_gather with dY's span at its limit (served, judged) and 16 bytes beyond (refused);
* the pitchless entries at 4 GiB plus one unit, one launch each, the entry's census runner on windows of it (reach_checks.run_windowed);
* svdx_tattn_fwd / svdx_tattn_bwd at T = 32, 31 and 24, and the refusal of T = 33.

One case is alive at a time; every test frees its buffers.  profiles/reach_gpu.txt has the times, the peak memory and the worst excess per
entry that the last test prints."""
import collections
import time

import pytest
import torch

import census
import reach_checks as rc
from svd_xtend_amd import kernels as K

pytestmark = pytest.mark.gpu

# pitch argument -> pieces (the base signatures dealt round-robin): about a hundred cases of ~40 ms a piece
PIECES = {"gemm-lda": 2, "gemm-gather.lda": 3, "gemm-ldb": 5, "gemm-ldc": 5, "gemm-ldres": 2}
PITCH_CASES = [(w, i, PIECES.get(w, 1)) for w in rc.PITCH_IDS for i in range(PIECES.get(w, 1))]
_WORST, _STATS = {}, collections.OrderedDict()


@pytest.fixture(scope="module")
def hip():
    return K.HipBackend()


@pytest.fixture(autouse=True)
def measured(request):
    rc.release("cuda")
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    yield
    torch.cuda.synchronize()
    _STATS[request.node.name] = (time.time() - t0, torch.cuda.max_memory_reserved())
    rc.release("cuda")


def _check(res, tag, key):
    bad = []
    for label, excess, idx in res:
        if "rounding" not in label:
            _WORST[key] = max(_WORST.get(key, 0.0), excess)
        if not excess <= 1.0:
            bad.append(f"excess {excess:.4g} at {idx}: {label}: {tag}")
    return bad


@pytest.mark.parametrize("which,piece,pieces", PITCH_CASES, ids=[f"{w}-{i + 1}of{k}" for w, i, k in PITCH_CASES])
def test_kernels_meet_float64_reference_on_both_sides_of_the_line(hip, which, piece, pieces):
    entry, arg = which.split("-", 1)
    cases = rc.pitched_cases(entry, arg)
    bases = list(collections.OrderedDict.fromkeys(c.base for c in cases))[piece::pieces]
    cases = [c for c in cases if c.base in bases]
    assert cases
    if entry == "gemm_tn":
        cases = cases + rc.flat_staging(cases)
    bad = rc.run_pitched(hip, "cuda", cases, _WORST)
    print(f"\n{which} piece {piece + 1} of {pieces}: {len(cases)} cases, {sum((c.verdict or '').startswith('refused') for c in cases)} of them refusals")
    assert not bad, f"{len(bad)} outputs beyond their bound:\n" + "\n".join(bad[:25])


def test_tsa_fwd_is_served_one_step_below_its_limit_and_refused_at_it(hip):
    """M 3C 2 bytes of q/k/v against 2^31 at C = 320: M = 1118481 = 3 x 372827 rows is 128 bytes below, M = 1118482 = 2 x 559241 is 1792 beyond.
    The served launch is judged on windows of pixels (reach_checks.run_windowed): its whole-tensor float64 reference took 109 GiB."""
    served, refused = rc.tsa_signature(*rc.TSA_SERVED), rc.tsa_signature(*rc.TSA_REFUSED)
    assert census.gemm_kernel_taken(served) == "tsa_fwd kernel" and census.reach(served)["qkv"] == census.REACH_2G - 128
    assert census.gemm_kernel_taken(refused).startswith("refused") and census.reach(refused)["qkv"] >= census.REACH_2G
    rc.assert_refused(hip, refused, "cuda", census.gemm_kernel_taken(refused))
    rc.release("cuda")
    res, found, starts = rc.run_windowed(hip, "cuda", rc.tsa_signature(1, rc.TSA_SERVED[1], 64), lines=rc.TSA_LINES, units=rc.TSA_SERVED[2])
    print(f"\nwindows at pixels {starts}")
    bad = _check(res, census.sig_str(served, 300), ("tsa_fwd", "below its limit")) + found
    assert len(starts) >= 3 and not bad, "\n".join(bad)


@pytest.mark.parametrize("entry", list(rc.WINDOWED))
def test_pitchless_entry_at_4_gib_plus_one_unit(hip, entry):
    base = rc.base_4g(entry, list(rc.WINDOWED).index(entry))
    res, found, starts = rc.run_windowed(hip, "cuda", base)
    big = rc._resized(base, rc.units_4g(base))
    print(f"\n{entry}: {census.sig_str(big, 300)}\n  operands {({k: v for k, v in census.reach(big).items() if v >= 1 << 20})}, windows at units {starts}")
    assert max(census.reach(big).values()) > census.REACH_4G and len(starts) >= 2
    bad = _check(res, census.sig_str(big, 300), (entry, "4 GiB")) + found
    assert not bad, "\n".join(bad[:25])


@pytest.mark.parametrize("entry", rc.WHOLE)
def test_counted_entry_beyond_2_to_the_31_elements(hip, entry):
    sig = rc.whole_signature(entry)
    assert max(census.reach(sig).values()) > census.REACH_4G
    bad = _check(rc.run_whole(hip, "cuda", entry), census.sig_str(sig, 300), (entry, "4 GiB"))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("dt", (torch.float16, torch.bfloat16), ids=("f16", "bf16"))
def test_gemm_tn_gather_is_served_one_step_below_its_span_limit_and_refused_at_it(hip, dt):
    worst = rc.run_gather_limit(hip, "cuda", dt)
    _WORST[("gemm_tn_gather", "below its limit")] = max(_WORST.get(("gemm_tn_gather", "below its limit"), 0.0), *worst)


@pytest.mark.parametrize("shape", rc.T_LIMIT_CASES, ids=lambda s: "x".join(map(str, s)))
def test_temporal_attention_at_its_stated_limit(hip, shape):
    bad = []
    for dt in ("f16", "bf16"):
        for sig in rc.tattn_signatures(*shape, dt=dt):
            bad += _check(census.run_case(hip, sig, "cuda"), census.sig_str(sig, 300), (sig[0], f"T = {shape[1]}"))
    assert not bad, "\n".join(bad)


def test_temporal_attention_beyond_its_limit_is_refused(hip):
    for sig in rc.tattn_signatures(1, rc.T_REFUSED, 4, 1):
        ops = []
        with pytest.raises(K.SvdxError, match="T<=32"):
            census.run_case(hip, sig, "cuda", operands_out=ops)
        outs = [n for n, d in ops[0].decls.items() if d[2]]
        assert outs and all(bool(torch.isnan(ops[0].t[n].float()).all()) for n in outs)


def test_zz_report():
    """(what profiles/reach_gpu.txt keeps: run last)"""
    print("\nwall time (s) and peak torch.cuda.max_memory_reserved() (GiB) per test:")
    for name, (t, m) in _STATS.items():
        print(f"{t:8.2f} {m / 2 ** 30:8.2f}  {name}")
    print("worst excess (error / bound) per entry:")
    for k, w in sorted(_WORST.items(), key=repr):
        print(f"{w:10.4f}  {k[0]} at ({k[1]})")
    assert _STATS
