"""The launch census of the train step and the per-launch checker (tests/census.py, tests/ref64.py) on the CPU (`-m "not gpu"`):
the census itself, the emulation's fused paths against torch's own float64 operators at every signature of the tiny step, the HIP
sources on the simulator at one signature per feature combination, and the checker against planted faults."""
import collections
import os

import pytest
import torch

import census
import emul
import kernel_checks as kc
from svd_xtend_amd import kernels as K

FULL = os.environ.get("SVDX_SIM_FULL") == "1"
BIG = ("c2", "c2_clip", "c5", "c5_ref", "c4")


def _run_all(be, sigs):
    bad, worst = [], collections.defaultdict(float)
    for sig in sigs:
        for label, excess, idx in census.run_case(be, sig):
            fam = census.family(sig, label)
            worst[fam] = max(worst[fam], excess)
            if not excess <= 1.0:
                bad.append(f"excess {excess:.3g} at {idx}: {label}: {census.sig_str(sig)}")
    return bad, worst


def test_census_is_deterministic_and_covers_the_step():
    c2 = census.census("c2")
    census._CACHE.pop("c2")
    assert census.census("c2") == c2, "two censuses of the same configuration differ"
    per = census.summary(c2)
    assert sum(c2.values()) >= 1400, sum(c2.values())
    assert sum(1 for s in c2 if s[0] == "gemm") >= 100
    assert {560, 2240, 8960, 35840} <= {census.sig_args(s)["M"] for s in c2 if s[0] == "gemm"}
    assert 230400 in {census.sig_args(s)["M"] for s in census.census("c4") if s[0] == "gemm"}
    assert any(s[0] == "gemm" and census.sig_args(s)["dual"] is not None for s in census.census("c5")), "config 5 without a dual-operand GEMM"
    clip = census.summary(census.census("c2_clip"))
    assert clip["grad_sumsq_spans"] == 1 and clip["grad_clip_coef"] == 1 and "grad_sumsq_spans" not in per
    # the accumulate forms of the second micro-batch are in config 4's census
    assert any(s[0] == "gemm_tn" and census.sig_args(s)["out_mode"] == K.OUT_F32_ADD for s in census.census("c4"))


@pytest.mark.parametrize("name", BIG + ("tiny_fp16", "tiny_bf16"))
def test_every_census_entry_has_a_runner_or_is_allow_listed(name):
    launches, distinct, checked, allowed, missing = census.coverage(census.census(name))
    print(f"{name}: {launches} launches, {distinct} distinct signatures, {checked} checked, allow-listed launches {dict(allowed)}")
    assert not missing, f"{name}: entries with neither a runner nor an allow-list entry: {missing}"
    assert sum(allowed.values()) <= census.ALLOW_FRACTION * launches, (dict(allowed), launches)


def test_no_c4_operand_reaches_the_64_bit_pointer_kernel():
    """svdx_gemm takes its 64-bit-pointer kernel (and refuses fused epilogues) when the extent of A or B reaches 2 GiB: the extents as
    csrc/gemm_nt.hip's entry computes them -- A over the gather's source rows with the gather's pitch, B = (N - 1) ldb + K -- from the
    signatures of config 4.  (Every signature runs on the GPU whichever kernel it takes; this says which.)"""
    worst = 0
    for s in census.census("c4"):
        if s[0] != "gemm":
            continue
        a = census.sig_args(s)
        g = a["gather"]
        if g is None or g.mode == K.GATHER_PLAIN:
            a_bytes = ((a["M"] - 1) * a["lda"] + a["K"]) * 2
        else:
            a_bytes = ((census._gather_src_rows(g) - 1) * g.lda + g.cin) * 2
        worst = max(worst, a_bytes, ((a["N"] - 1) * a["ldb"] + a["K"]) * 2)
    print(f"largest GEMM operand extent of config 4: {worst / 2 ** 30:.3f} GiB")
    assert worst < 2 ** 31, "a config-4 GEMM operand reaches 2 GiB: that launch takes the 64-bit-pointer kernel"


@pytest.mark.parametrize("name", ("tiny_fp16", "tiny_bf16"))
def test_emulation_meets_float64_reference_at_every_tiny_signature(name):
    """pins the emulation's fused paths (row-vector grouping, rv_mod, dual / segmented operand, split-K slabs, statistics encode, tsa_fwd,
    small_linear, edm_loss' gradient, ...) to torch's own operators in float64, within the derived bounds"""
    sigs = [s for s in census.census(name) if s[0] in census.RUNNERS]
    assert len(sigs) >= 250
    bad, worst = _run_all(emul.EmuBackend(), sigs)
    for fam, w in sorted(worst.items()):
        print(f"{w:8.3f}  {fam}")
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("name", ("tiny_fp16", "tiny_bf16"))
def test_hip_sources_meet_float64_reference_on_simulator(name):
    """the HIP sources themselves (tests/sim): one signature of the tiny census per (entry, feature combination); all of it under SVDX_SIM_FULL=1"""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "sim"))
    from backend import SimBackend
    sigs = [s for s in census.census(name) if s[0] in census.RUNNERS]
    if not FULL:
        first = {}
        for s in sorted(sigs, key=repr):
            first.setdefault(census.feature_key(s), s)
        sigs = list(first.values())
    print(f"{name}: {len(sigs)} signatures on the simulator")
    bad, worst = _run_all(SimBackend(), sigs)
    for fam, w in sorted(worst.items()):
        print(f"{w:8.3f}  {fam}")
    assert not bad, "\n".join(bad[:20])


# ---- planted faults --------------------------------------------------------------------------------------------------------------------
def _toward_zero(v32, dt):
    """fp32 -> dt by truncation"""
    h = v32.to(dt)
    away = h.float().abs() > v32.abs()
    return torch.where(away, (h.view(torch.int16) - 1).view(dt), h)


class Faulty(emul.EmuBackend):
    """The emulation with one planted fault in its NT GEMM: the fp32 result is perturbed before it is rounded and stored."""

    def __init__(self, fault):
        self.fault = fault

    def gemm(self, A, B, C, M, N, Kd, lda, ldb, ldc, bias=None, rowvec=None, rv_ld=0, rv_rpg=0, rv_mod=0, res=None, ldres=0, gather=None,
             out_mode=K.OUT_ACT, alpha=1.0, *rest):
        assert out_mode == K.OUT_ACT
        wide = torch.zeros(C.numel(), dtype=torch.float32)
        super().gemm(A, B, wide, M, N, Kd, lda, ldb, ldc, bias, rowvec, rv_ld, rv_rpg, rv_mod, res, ldres, gather, K.OUT_F32, alpha, *rest)
        v, out = emul.V(wide, M, N, ldc), emul.V(C, M, N, ldc)
        m = torch.arange(M)
        if self.fault == "truncated":
            out.copy_(_toward_zero(v, C.dtype))
            return
        if self.fault == "K tile dropped":             # one 64-wide K tile missing from one 16 x 16 block of the last row tile
            r0, c0, k0 = (M - 1) // 16 * 16, 32, Kd - 64
            a, b = emul.V(A, M, Kd, lda).float(), emul.V(B, N, Kd, ldb).float()
            v[r0:r0 + 16, c0:c0 + 16] -= alpha * (a[r0:r0 + 16, k0:k0 + 64] @ b[c0:c0 + 16, k0:k0 + 64].t())
        elif self.fault == "row vector of the neighbouring group":
            gi = (m % rv_mod) if rv_mod else (m // rv_rpg)
            rv = emul.V(rowvec, int(gi.max()) + 1, N, rv_ld)
            v += rv[(gi + 1) % (int(gi.max()) + 1)] - rv[gi]
        elif self.fault == "residual of row m - 1":
            r = emul.V(res, M, N, ldres).float()
            v += torch.roll(r, 1, 0) - r
        out.copy_(v.to(C.dtype))
        if self.fault == "one element unwritten":
            out[M // 2, N // 3] = float("nan")

    def ln_bwd(self, dy, x, stats, gamma, add, dx, dgamma, dbeta, rows, C, *rest):
        assert self.fault == "truncated (norm backward)"
        wide = torch.zeros(dx.numel(), dtype=torch.float32)
        super().ln_bwd(dy, x, stats, gamma, add, wide, dgamma, dbeta, rows, C, *rest)
        emul.V(dx, rows, C, C).copy_(_toward_zero(emul.V(wide, rows, C, C), dx.dtype))

    def small_linear(self, X, W, bias, Y, M, N, Kd, ldw, trans=0, silu_in=0, accumulate=0):
        assert self.fault == "stored instead of added" and accumulate
        super().small_linear(X, W, bias, Y, M, N, Kd, ldw, trans, silu_in, 0)


def _pick(name, pred, entry="gemm"):
    sigs = sorted((s for s in census.census(name) if s[0] == entry and pred(census.sig_args(s))), key=repr)
    assert sigs, "no such signature in the census"
    return sigs[0]


def _plain(a):
    return a["out_mode"] == K.OUT_ACT and a["epilogue"] == K.EPI_NONE and a["gather"] is None and a["dual"] is None and a["gn"] is None and a["split_k"] == 1


FAULTS = {
    # fault -> (configuration, predicate on the signature's arguments)
    "truncated": ("c2", lambda a: _plain(a) and (a["M"], a["N"], a["K"]) == (2240, 1280, 1280)),
    "K tile dropped": ("c2", lambda a: _plain(a) and (a["M"], a["N"], a["K"]) == (2240, 1280, 1280)),
    "row vector of the neighbouring group": ("tiny_fp16", lambda a: _plain(a) and a["rowvec"] is not None and a["M"] % 4 == 0),
    "residual of row m - 1": ("tiny_fp16", lambda a: _plain(a) and a["res"] is not None),
    "one element unwritten": ("tiny_fp16", lambda a: _plain(a)),
    "truncated (norm backward)": ("c2", lambda a: a["rows"] * a["C"] >= 10 ** 6 and a["dgamma"] is None),     # (entry: ln_bwd, a multi-stage output)
    "stored instead of added": ("tiny_fp16", lambda a: a["accumulate"] == 1 and a["trans"] == 0),          # (entry: small_linear)
}
PASSES_TODAYS_BAR = {"truncated"}       # the faults tests/kernel_checks.py's relerr / tol_for comparison with the emulation lets through


def _relerr_bar(sig, fault):
    """today's check on the same operands: relerr(faulty, emulation) against tol_for"""
    outs = []
    for be in (Faulty(fault), emul.EmuBackend()):
        ops = []
        census.run_case(be, sig, operands_out=ops)
        outs.append(ops[0]["C"])
    a = census.sig_args(sig)
    view = lambda t: emul.V(t, a["M"], a["N"], a["ldc"])
    return kc.relerr(view(outs[0]), view(outs[1])), kc.tol_for(census.DT_OF[a["A"][1]])


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_checker_notices_planted_fault(fault):
    """numeric perturbations of a correct CPU result (nothing runs on a GPU): each must be flagged by the census checker; which of them
    today's relerr / tol_for bar lets through is recorded (the truncating cast is one)."""
    cfg, pred = FAULTS[fault]
    sig = _pick(cfg, pred, {"stored instead of added": "small_linear", "truncated (norm backward)": "ln_bwd"}.get(fault, "gemm"))
    if fault == "row vector of the neighbouring group":
        # one clip per rank: every GEMM of the step has ONE row-vector group.  The same launch with four (rows per group = M / 4)
        a = census.sig_args(sig)
        sig = (sig[0], tuple((k, a["M"] // 4 if k == "rv_rpg" else v) for k, v in sig[1]))
    clean = census.run_case(emul.EmuBackend(), sig)
    assert all(e <= 1.0 for _, e, _ in clean), clean
    res = census.run_case(Faulty(fault), sig)
    flagged = [(label, e) for label, e, _ in res if not e <= 1.0]
    print(f"{fault}: {census.sig_str(sig, 200)}")
    for label, e in flagged:
        print(f"    flagged: {label}: excess {e:.3g}")
    assert flagged, f"the checker let '{fault}' through: {res}"
    if fault.startswith("truncated"):
        assert any("mean magnitude error" in label for label, _ in flagged), flagged
    if sig[0] == "gemm":
        err, tol = _relerr_bar(sig, fault)
        print(f"    today's bar: relerr {err:.3g} against {tol:.3g}: {'passes' if err <= tol else 'fails'}")
        assert (err <= tol) == (fault in PASSES_TODAYS_BAR), (fault, err, tol)
