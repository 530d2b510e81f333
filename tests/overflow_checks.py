"""A non-finite gradient anywhere skips the step: what tests/test_overflow.py (emulation and simulator, CPU) and tests/test_overflow_gpu.py
share.  GradScaler's inf check is folded into the kernels that write the gradients (svdx_gemm_tn's two epilogues, svdx_grad_finalize_batch)
plus svdx_check_finite_spans over the accumulated slots; the helpers here plant ONE non-finite value where the flag is known by
construction and return what went wrong as a list of strings (empty: the check holds).  Every "unchanged" is torch.equal on bits.

  1. detector sweeps through the C ABI: tn_plant_* / tn_false_positives / tn_flag_scope, gradfin_*, finite_spans_*, finite_flat_*
  2. coverage on a recording backend: coverage_step
  3. one poisoned launch in a whole Trainer step: tiny_trainer, PoisonTN, skipped_step, op_level_row_sliced, accumulated_slots
  4. the loss-scale state machine and the skipped optimizer kernels: prep_sequences, skipped_adamw
"""
import contextlib
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from svd_xtend_amd import kernels as K  # noqa: E402
import census  # noqa: E402
import emul  # noqa: E402
import ref64  # noqa: E402

INF, NAN = float("inf"), float("nan")
VALUES = (INF, -INF, NAN)
# bit patterns of what "not finite" covers: quiet NaN, the signalling pattern, a NaN with the sign set, +-inf.  (svdx_check_finite* test
# with isfinite, the GEMM epilogues with an exponent mask: both must take all of them.)
PAYLOADS = {"quiet NaN": 0x7fc00000, "signalling NaN": 0x7f800001, "negative NaN": -0x400000, "+inf": 0x7f800000, "-inf": -0x800000}
SENTINEL = 7.0
TN_STAGES = (0, 2, 3, 4, 18)


def sync(dev):
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()


def put_bits(t, idx, bits):
    """t (float32, 1-D view) [idx] = the float with these bits (no arithmetic touches a signalling pattern)"""
    t.view(torch.int32)[idx] = bits


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ---- 1. svdx_gemm_tn ----------------------------------------------------------------------------------------------------------------------
def tn_tile(stages):
    return 256 if (stages & ~K.TN_FLAT) == 18 else 128


def tn_shapes(stages):
    """(R, N, Kd): the smallest shape with a partial tile in both directions and a partial row tile, and one of whole tiles"""
    t = tn_tile(stages)
    return [(72, t + 8, t + 8), (64, t, t)]


def tn_positions(N, Kd, tile, quick=False):
    """output positions (row of C, column of C): the four corners, both sides of every tile seam in each direction (at both ends of the
    seam and where two seams cross), and the walk (i mod N, (7 i + 3) mod Kd), i < max(N, Kd): 7 is coprime to every width used, so every
    output row and every output column gets a launch.  quick: corners and seams only (the simulator's share)."""
    pos = [(0, 0), (0, Kd - 1), (N - 1, 0), (N - 1, Kd - 1)]
    rs = [s + d for s in range(tile, N, tile) for d in (-1, 0)]
    cs = [s + d for s in range(tile, Kd, tile) for d in (-1, 0)]
    pos += [(r, c) for r in rs for c in (0, Kd - 1)] + [(r, c) for c in cs for r in (0, N - 1)] + [(r, c) for r in rs for c in cs]
    if not quick:
        assert math.gcd(7, Kd) == 1
        pos += [(i % N, (7 * i + 3) % Kd) for i in range(max(N, Kd))]
        assert {p[0] for p in pos} == set(range(N)) and {p[1] for p in pos} == set(range(Kd))
    return pos


class _TN:
    """L launches of one svdx_gemm_tn configuration on stacked operands (launch i has its own A, B, C and flag), pitches one 8-column group
    wider than the operands"""

    def __init__(self, be, dev, dt, stages, shape, L, seed=0):
        self.be, self.dev, self.dt, self.stages, self.L = be, dev, dt, stages, L
        self.R, self.N, self.Kd = R, N, Kd = shape
        self.lda, self.ldb, self.ldc = N + 8, Kd + 8, Kd + 8
        g = torch.Generator().manual_seed(seed)
        A = torch.randn(R, self.lda, generator=g)
        B = torch.randn(R, self.ldb, generator=g) * R ** -0.5
        B = torch.where(B.abs() < 1e-3, torch.full_like(B, 0.25), B)           # no zero in B: inf * B is an infinity, never NaN by accident
        C = torch.randn(N, self.ldc, generator=g)
        self.As = A.to(dt).to(dev).repeat(L, 1, 1).contiguous()
        self.Bs = B.to(dt).to(dev).repeat(L, 1, 1).contiguous()
        self.Cs = C.to(dev).repeat(L, 1, 1).contiguous()
        self.Cs[:, :, Kd:] = SENTINEL
        self.flags = torch.full((L, 16), SENTINEL, device=dev)
        self.flags[:, 3] = 0.0
        self.ar = torch.arange(L, device=dev)

    def launch(self, mode, a_colsum=None):
        for i in range(self.L):
            self.be.gemm_tn(self.As[i], self.Bs[i], self.Cs[i], self.R, self.N, self.Kd, self.lda, self.ldb, self.ldc, out_mode=mode,
                            stages=self.stages, found_inf=self.flags[i, 3:4], a_colsum=None if a_colsum is None else a_colsum[i])
        sync(self.dev)

    def verdict(self, want_mask, what):
        """flag 1 in every launch, the three floats in front of it and the twelve behind untouched, the non-finite positions of C exactly
        `want_mask` [L, N, Kd], the pad columns of C untouched"""
        bad = []
        fl = self.flags.cpu()
        for i in (fl[:, 3] != 1.0).nonzero().flatten().tolist()[:5]:
            bad.append(f"{what}: launch {i}: flag {float(fl[i, 3])} (not raised)")
        around = torch.cat([fl[:, :3], fl[:, 4:]], 1)
        for i in (around != SENTINEL).any(1).nonzero().flatten().tolist()[:5]:
            bad.append(f"{what}: launch {i}: floats beside the flag written: {fl[i].tolist()}")
        got = ~torch.isfinite(self.Cs[:, :, :self.Kd])
        for i in (got != want_mask).flatten(1).any(1).nonzero().flatten().tolist()[:5]:
            bad.append(f"{what}: launch {i}: non-finite elements of C at {got[i].nonzero().tolist()[:6]}, planted {want_mask[i].nonzero().tolist()[:6]}")
        if not bool((self.Cs[:, :, self.Kd:] == SENTINEL).all()):
            bad.append(f"{what}: the pad columns of C were written")
        return bad


def _label(dt, stages, shape, mode):
    return f"gemm_tn {str(dt)[6:]} stages={stages & ~K.TN_FLAT}{' flat' if stages & K.TN_FLAT else ''} {shape} mode={mode}"


def tn_plant_add(be, dev, dt, stages, shape, quick=False):
    """OUT_F32_ADD: exactly one element of C preset to +inf / -inf / NaN (cycling over the positions), finite operands.
    -> (failures, launches)"""
    R, N, Kd = shape
    pos = tn_positions(N, Kd, tn_tile(stages), quick)
    t = _TN(be, dev, dt, stages, shape, len(pos))
    rows, cols = (torch.tensor(x, device=dev) for x in zip(*pos))
    t.Cs[t.ar, rows, cols] = torch.tensor([VALUES[i % 3] for i in range(len(pos))], device=dev)
    want = torch.zeros(len(pos), N, Kd, dtype=torch.bool, device=dev)
    want[t.ar, rows, cols] = True
    t.launch(K.OUT_F32_ADD)
    return t.verdict(want, _label(dt, stages, shape, "+=")), len(pos)


def tn_plant_store_bf16(be, dev, stages, shape, quick=False):
    """OUT_F32, bf16: A[r0, n0] = B[r0, k0] = 2^100 with the rest of row r0 of both operands zero -- every operand finite, the fp32 product
    2^200 overflows at (n0, k0) only.  r0 walks over the rows (the partial row tile included).  -> (failures, launches)"""
    R, N, Kd = shape
    pos = tn_positions(N, Kd, tn_tile(stages), quick)
    t = _TN(be, dev, torch.bfloat16, stages, shape, len(pos))
    rows, cols = (torch.tensor(x, device=dev) for x in zip(*pos))
    r0 = torch.tensor([(5 * i + R - 1) % R for i in range(len(pos))], device=dev)
    t.As[t.ar, r0, :N] = 0
    t.Bs[t.ar, r0, :Kd] = 0
    t.As[t.ar, r0, rows] = 2.0 ** 100
    t.Bs[t.ar, r0, cols] = 2.0 ** 100
    assert bool(torch.isfinite(t.As.float()).all()) and bool(torch.isfinite(t.Bs.float()).all())
    t.Cs[:, :, :Kd] = NAN                                   # store mode: whatever C held is gone
    want = torch.zeros(len(pos), N, Kd, dtype=torch.bool, device=dev)
    want[t.ar, rows, cols] = True
    t.launch(K.OUT_F32)
    return t.verdict(want, _label(torch.bfloat16, stages, shape, "store")), len(pos)


def tn_plant_store_f16(be, dev, stages, shape, quick=False):
    """OUT_F32, f16: no product of two halves overflows fp32 (65504^2 < 2^32), so finite f16 operands cannot make ONE output element
    non-finite: the granularity f16 operands can isolate is a row of C (an inf / NaN in A[r0, n0]) or a column (in B[r0, k0]).  Every row
    and every column once.  (The f16 epilogue is the same template as the bf16 one, which the per-element sweep covers.)"""
    R, N, Kd = shape
    lines = [("row", n) for n in range(N)] + [("col", k) for k in range(Kd)]
    if quick:
        tile = tn_tile(stages)
        keep = {0, N - 1} | {s + d for s in range(tile, N, tile) for d in (-1, 0)}
        lines = [x for x in lines if x[1] in keep]
    L = len(lines)
    t = _TN(be, dev, torch.float16, stages, shape, L)
    want = torch.zeros(L, N, Kd, dtype=torch.bool, device=dev)
    for i, (kind, j) in enumerate(lines):
        r0 = (5 * i + R - 1) % R
        (t.As if kind == "row" else t.Bs)[i, r0, j] = VALUES[i % 3]
        if kind == "row":
            want[i, j, :] = True
        else:
            want[i, :, j] = True
    t.Cs[:, :, :Kd] = NAN
    t.launch(K.OUT_F32)
    return t.verdict(want, _label(torch.float16, stages, shape, "store (row / column)")), L


def tn_false_positives(be, dev, dt, stages, shape, mode):
    """A, B and C as views inside buffers whose every other element is NaN (rows >= R, the pad columns inside the pitch, 256 elements in front
    of and behind each buffer: a zero fill would hide a kernel that masks a tail by multiplying with zero).  Finite operands: the flag
    stays 0, C is finite and within the census bound of its float64 reference, the NaN around C keeps its bits."""
    R, N, Kd = shape
    lda, ldb, ldc, G = N + 8, Kd + 8, Kd + 8, 256
    rows_a = (R + 63) // 64 * 64 + 64                        # a whole further row tile of NaN behind the operands
    g = torch.Generator().manual_seed(3)

    def embed(rows_alloc, rows, cols, ld, dtype, fill):
        buf = torch.full((2 * G + rows_alloc * ld,), NAN, dtype=dtype)
        view = torch.as_strided(buf, (rows, cols), (ld, 1), G)
        view.copy_(fill)
        buf = buf.to(dev)
        return buf, torch.as_strided(buf, (rows, cols), (ld, 1), G)

    abuf, A = embed(rows_a, R, N, lda, dt, torch.randn(R, N, generator=g).to(dt))
    bbuf, B = embed(rows_a, R, Kd, ldb, dt, (torch.randn(R, Kd, generator=g) * R ** -0.5).to(dt))
    cbuf, C = embed(N + 8, N, Kd, ldc, torch.float32, torch.ones(N, Kd) if mode == K.OUT_F32_ADD else torch.full((N, Kd), NAN))
    before = cbuf.clone()
    flag = torch.full((16,), SENTINEL, device=dev)
    flag[3] = 0.0
    be.gemm_tn(A, B, C, R, N, Kd, lda, ldb, ldc, out_mode=mode, stages=stages, found_inf=flag[3:4])
    sync(dev)
    what, bad = _label(dt, stages, shape, mode) + " inside NaN", []
    if flag.tolist() != [SENTINEL] * 3 + [0.0] + [SENTINEL] * 12:
        bad.append(f"{what}: flag buffer {flag.tolist()}")
    if not bool(torch.isfinite(C).all()):
        bad.append(f"{what}: C has {int((~torch.isfinite(C)).sum())} non-finite elements, first {(~torch.isfinite(C)).nonzero()[0].tolist()}")
    v, S, ka = ref64.gemm_tn(A, B)
    if mode == K.OUT_F32_ADD:
        v, S, ka = v + 1.0, S + 1.0, ka + 1
    res = []
    census.judge_single(res, "C", C, v, S, ka, 1)             # the bar of census.run_gemm_tn
    bad += [f"{what}: {label}: excess {e:.3g} at {idx}" for label, e, idx in res if not e <= 1.0]
    inside = torch.zeros_like(cbuf, dtype=torch.bool)
    torch.as_strided(inside, (N, Kd), (ldc, 1), G).fill_(True)
    if not same_bits(cbuf[~inside], before[~inside]):
        bad.append(f"{what}: the NaN around C changed")
    return bad


def tn_flag_scope(be, dev, dt, stages, refuses=True):
    """whose flag it is: the slab form refuses `found_inf` (its slabs are tested by the reducing launch); a column sum that goes non-finite
    while C stays finite does not raise it (that slot is an accumulated one: svdx_check_finite_spans' business)"""
    R, N, Kd = tn_shapes(stages)[0]
    t = _TN(be, dev, dt, stages, (R, N, Kd), 1)
    bad = []
    if refuses:
        try:
            slabs = torch.zeros(2, N, Kd, device=dev)
            be.gemm_tn(t.As[0], t.Bs[0], slabs, R, N, Kd, t.lda, t.ldb, Kd, out_mode=K.OUT_F32_SLAB, split_k=2, stages=stages,
                       found_inf=t.flags[0, 3:4])
            bad.append("the slab form took a found_inf pointer")
        except K.SvdxError as e:
            if "found_inf" not in str(e):
                bad.append(f"refused for another reason: {e}")
        sync(dev)
    cs = torch.ones(1, N, device=dev)
    cs[0, N // 3] = INF
    t.launch(K.OUT_F32_ADD, a_colsum=cs)
    if float(t.flags[0, 3]) != 0.0 or not bool(torch.isfinite(t.Cs[:, :, :Kd]).all()):
        bad.append(f"non-finite column sum, finite C: flag {float(t.flags[0, 3])}")
    if bool(torch.isfinite(cs).all()):
        bad.append("the planted column sum vanished")
    return bad


def tn_sweeps(be, dev, stages, quick):
    """every sweep of one `stages` code at its two shapes -> (failures, launches)"""
    bad, n = [], 0
    for shape in tn_shapes(stages):
        for dt in (torch.float16, torch.bfloat16):
            b, k = tn_plant_add(be, dev, dt, stages, shape, quick)
            bad, n = bad + b, n + k
        for fn in (tn_plant_store_bf16, tn_plant_store_f16):
            b, k = fn(be, dev, stages, shape, quick)
            bad, n = bad + b, n + k
        for dt in (torch.float16, torch.bfloat16):
            for mode in (K.OUT_F32, K.OUT_F32_ADD):
                bad += tn_false_positives(be, dev, dt, stages, shape, mode)
                n += 1
    return bad, n


# ---- 1. svdx_grad_finalize_batch ------------------------------------------------------------------------------------------------------------
# (nsplit, store, column-sum slabs, count, flag): jobs 0 and 1 share flag 0, jobs 2 and 4 have one each, job 3 has none
GRADFIN_JOBS = [(1, True, False, 4, 0), (2, False, True, 256 * 4, 0), (7, True, True, 256 * 4 * 3 + 4, 1), (2, False, False, 256 * 4, None),
                (7, False, False, 4, 2)]
GRADFIN_PAD = 8          # floats of slab memory behind `count` in every slice


def _gradfin_pack(dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    pack = []
    for ns, store, cs, cnt, fl in GRADFIN_JOBS:
        stride = cnt + GRADFIN_PAD
        pack.append(dict(slabs=(torch.randn(ns * stride, generator=g) * ns ** -0.5).to(dev), dst=torch.randn(cnt, generator=g).to(dev),
                         cs=torch.randn(ns, 64, generator=g).to(dev) if cs else None, co=torch.randn(64, generator=g).to(dev) if cs else None,
                         ns=ns, stride=stride, cnt=cnt, store=store, flag=fl))
    return pack


def _gradfin_run(be, dev, pack, plant=None):
    """plant: (job, 'slab' | 'dst', slice, element, value) -> (flags [3, 16], dst per job)"""
    flags = torch.full((3, 16), SENTINEL, device=dev)
    flags[:, 3] = 0.0
    jobs, dsts = [], []
    for j, q in enumerate(pack):
        slabs, dst = q["slabs"].clone(), q["dst"].clone()
        if plant is not None and plant[0] == j:
            _, where, z, e, val = plant
            if where == "slab":
                slabs[z * q["stride"] + e] = val
            else:
                dst[e] = val
        dsts.append(dst)
        jobs.append((slabs, q["ns"], q["stride"], dst, q["cnt"], q["cs"], None if q["co"] is None else q["co"].clone(), q["store"],
                     None if q["flag"] is None else flags[q["flag"], 3:4]))
    be.grad_finalize_batch(jobs)
    sync(dev)
    return flags.cpu(), dsts


def gradfin_plants():
    out = []
    for j, (ns, store, cs, cnt, fl) in enumerate(GRADFIN_JOBS):
        q4 = cnt // 4
        for z in sorted({0, ns - 1}):
            for n, v4 in enumerate(sorted({0, q4 // 2, q4 - 1})):
                out.append((j, "slab", z, 4 * v4 + (z + n) % 4, VALUES[(j + z + n) % 3], True))
            out.append((j, "slab", z, cnt + (z % GRADFIN_PAD), INF, False))          # slab memory beyond `count`
        if not store:
            for n, v4 in enumerate(sorted({0, q4 // 2, q4 - 1})):
                out.append((j, "dst", 0, 4 * v4 + (n + 1) % 4, VALUES[(j + n) % 3], True))
    return out


def gradfin_sweep(be, dev):
    """one non-finite value in one slab (first, middle and last f32x4 of the first and last slice) or -- accumulate form -- in the
    destination of one job of the pack: exactly that job's flag, nothing beside the flags, every other job's result as in the clean launch;
    a value behind `count` raises nothing.  -> (failures, launches)"""
    pack = _gradfin_pack(dev)
    clean_flags, clean = _gradfin_run(be, dev, pack)
    want_clean = torch.full((3, 16), SENTINEL)
    want_clean[:, 3] = 0.0
    bad = [] if torch.equal(clean_flags, want_clean) else [f"clean pack: flags {clean_flags[:, :5].tolist()}"]
    plants = gradfin_plants()
    for j, where, z, e, val, counts in plants:
        flags, dsts = _gradfin_run(be, dev, pack, (j, where, z, e, val))
        want = want_clean.clone()
        if counts and GRADFIN_JOBS[j][4] is not None:
            want[GRADFIN_JOBS[j][4], 3] = 1.0
        what = f"grad_finalize_batch: {val} in the {where} of job {j} (slice {z}, element {e})"
        if not torch.equal(flags, want):
            bad.append(f"{what}: flags {flags[:, :5].tolist()}, expected {want[:, 3].tolist()}")
        for i, (d, c) in enumerate(zip(dsts, clean)):
            if i != j or not counts:
                if not same_bits(d, c):
                    bad.append(f"{what}: job {i}'s destination differs from the clean launch")
            elif (~torch.isfinite(d)).nonzero().flatten().tolist() != [e]:
                bad.append(f"{what}: non-finite destination elements {(~torch.isfinite(d)).nonzero().flatten().tolist()[:6]}")
    return bad, len(plants) + 1


# ---- 1. svdx_check_finite_spans / svdx_check_finite -------------------------------------------------------------------------------------------
SPAN_COUNTS = (4, 8, 1020, 1024, 1028, 65536)
FLAT_SIZES = (4, 5, 7, 1023, 4 * 3000 + 3)


def _state(dev):
    st = torch.full((K.OPT_STATE_ALLOC,), SENTINEL, device=dev)
    st[3] = 0.0
    return st


def _state_verdict(st, want, what):
    st = st.cpu()
    ok = float(st[3]) == want and bool((st[:3] == SENTINEL).all()) and bool((st[4:] == SENTINEL).all())
    return [] if ok else [f"{what}: state {st[:6].tolist()}, expected found_inf = {want}"]


def finite_spans_sweep(be, dev):
    """every payload at the first and the last float of every span (raises) and at the float in front of and behind it (does not)"""
    rows, pos = [], 8
    for c in SPAN_COUNTS:
        rows.append((pos, c))
        pos += c + 8
    base = torch.randn(pos, generator=torch.Generator().manual_seed(1)).to(dev)
    spans = torch.tensor(rows, dtype=torch.int32, device=dev)
    st = _state(dev)
    be.check_finite_spans(base, spans, len(rows), st)
    sync(dev)
    bad, n = _state_verdict(st, 0.0, "check_finite_spans, finite buffer"), 1
    for off, c in rows:
        for idx, want in ((off, 1.0), (off + c - 1, 1.0), (off - 1, 0.0), (off + c, 0.0)):
            for name, bits in PAYLOADS.items():
                g = base.clone()
                put_bits(g, idx, bits)
                st = _state(dev)
                be.check_finite_spans(g, spans, len(rows), st)
                sync(dev)
                bad += _state_verdict(st, want, f"check_finite_spans: {name} at {idx} (span {off}+{c})")
                n += 1
    return bad, n


def finite_flat_sweep(be, dev):
    """svdx_check_finite over n floats: every payload at the first element, the last, each of the n % 4 tail elements (raises) and at
    index n itself (does not)"""
    bad, count = [], 0
    for n in FLAT_SIZES:
        base = torch.randn(n + 8, generator=torch.Generator().manual_seed(n)).to(dev)
        for idx in sorted({0, n - 1, n} | set(range(n - n % 4, n))):
            for name, bits in PAYLOADS.items():
                g = base.clone()
                put_bits(g, idx, bits)
                st = _state(dev)
                be.check_finite(g, n, st)
                sync(dev)
                bad += _state_verdict(st, 0.0 if idx == n else 1.0, f"check_finite n={n}: {name} at {idx}")
                count += 1
        st = _state(dev)
        be.check_finite(base, n, st)
        sync(dev)
        bad += _state_verdict(st, 0.0, f"check_finite n={n}, finite buffer")
    return bad, count + len(FLAT_SIZES)


# ---- 2. coverage: every gradient float has a detector ----------------------------------------------------------------------------------------
COVERAGE_CONFIGS = ("tiny_fp16", "tiny_bf16", "c2", "c2_clip", "c5", "c5_ref", "c4") + tuple(census.GEOM_EDGE)


class CoverageRecorder(census.Recorder):
    """the recording backend of the census, which also keeps -- for the launches that matter to the inf check -- where in which storage
    the destination lies"""

    def __init__(self):
        super().__init__()
        self.events = []
        for name in ("gemm_tn", "grad_finalize_batch", "gemm_finalize", "check_finite", "check_finite_spans", "zero_spans"):
            setattr(self, name, self._keep(name, getattr(self, name)))

    def _keep(self, name, inner):
        def call(*a, **kw):
            if self.on:
                self.events.append((name, a, kw))
            return inner(*a, **kw)
        return call


def _interval(t, g_flat, n):
    """[lo, hi) of the n floats at tensor `t` inside g_flat, or None when `t` lives in another storage"""
    if t.untyped_storage().data_ptr() != g_flat.untyped_storage().data_ptr():
        return None
    lo = t.storage_offset() - g_flat.storage_offset()
    return lo, lo + n


def coverage_step(name, rt_attrs=None):
    """One optimizer step (the second: packing is behind it) of census configuration `name` on the recording backend.  Returns a dict:
    n_flat, n_total, per micro-batch the flagged gemm_tn launches (interval, out_mode), the flagged grad_finalize_batch jobs, the
    single-launch gemm_finalize destinations inside the gradient buffer, the finite_spans table, and which finite check the optimizer ran."""
    from oracle.unet import SVD_CONFIG, TINY_CONFIG, no_default_init
    from svd_xtend_amd.train import Trainer
    from svd_xtend_amd.unet import UNetSpatioTemporalConditionModel
    topo, (B, T, h, w), dt, lora_r, kw = census.ALL_CONFIGS[name]
    cfg = dict(TINY_CONFIG if topo == "tiny" else SVD_CONFIG)
    rec = CoverageRecorder()
    rec.on = False
    with census._backend(rec), torch.no_grad():
        with no_default_init():
            m = UNetSpatioTemporalConditionModel(**cfg)
        if lora_r:
            from svd_xtend_amd.lora import LoraConfig
            for p in m.parameters():
                p.requires_grad_(False)
            with no_default_init():
                m.add_adapter(LoraConfig(r=lora_r, lora_alpha=lora_r, init_lora_weights="gaussian"))
        tr = Trainer(m, dtype=dt, lr=1e-5, **kw)
        tr.rt.gemm_variant = 4
        for k_, v_ in (rt_attrs or {}).items():
            assert hasattr(tr.rt, k_), k_
            setattr(tr.rt, k_, v_)
        cross = cfg["cross_attention_dim"]
        batch = dict(unet_in=torch.empty(B, T, 8, h, w), timesteps=torch.ones(B), ehs=torch.empty(B, 1, cross),
                     added_time_ids=torch.ones(B, 3), noisy_latents=torch.empty(B, T, 4, h, w), target=torch.empty(B, T, 4, h, w),
                     sigmas=torch.ones(B))
        tr.step([batch] * tr.grad_accum)
        rec.on = True
        tr.zero_grad()
        micro = []
        for _ in range(tr.grad_accum):
            rec.events = []
            tr.forward_backward(**batch)
            micro.append(rec.events)
        rec.events = []
        tr.finish_grads()
        tr.optimizer_step()
        tail = rec.events
    g = tr.g_flat
    out = dict(n_flat=tr.n_flat, n_total=tr.n_total, micro=[], tail=[e[0] for e in tail], found_inf=tr.rt.found_inf is not None,
               finite_spans=[] if tr.finite_spans is None else [tuple(r) for r in tr.finite_spans.tolist()])
    for ev in micro:
        tn, fin, single, unflagged = [], [], [], []
        for entry, a, kw_ in ev:
            if entry == "gemm_tn":
                args = dict(zip(("A", "B", "C", "R", "N", "K", "lda", "ldb", "ldc", "out_mode", "split_k", "a_colsum", "stages", "found_inf"), a))
                args.update(kw_)
                iv = _interval(args["C"], g, args["N"] * args["K"])
                if iv is None:
                    continue
                assert args["ldc"] == args["K"]
                (tn if args.get("found_inf") is not None else unflagged).append((iv, args.get("out_mode", K.OUT_F32_ADD)))
            elif entry == "grad_finalize_batch":
                for job in a[0]:
                    iv = _interval(job[3], g, job[4])
                    if iv is not None:
                        (fin if len(job) > 8 and job[8] is not None else unflagged).append((iv, bool(job[7])))
            elif entry == "gemm_finalize":
                args = dict(zip(("acc", "nsplit", "slab_stride", "C", "M", "N", "ldc"), a))
                iv = _interval(args["C"], g, args["M"] * args["N"])
                if iv is not None:
                    single.append(iv)
        out["micro"].append(dict(tn=tn, fin=fin, single=single, unflagged=unflagged))
    return out


def uncovered(n, intervals):
    """the parts of [0, n) no interval covers, and the pairs of intervals that overlap"""
    gaps, overlaps, pos = [], [], 0
    for lo, hi in sorted(intervals):
        if lo > pos:
            gaps.append((pos, lo))
        elif lo < pos:
            overlaps.append((lo, min(pos, hi)))
        pos = max(pos, hi)
    if pos < n:
        gaps.append((pos, n))
    return gaps, overlaps


def coverage_verdict(cov, name):
    """every recorded step: the full pass ran over n_flat, or flagged destinations + finite_spans cover [0, n_flat) with nothing uncovered;
    no flagged interval reaches the loss slot [n_flat, n_total)"""
    bad = []
    n = cov["n_flat"]
    full = "check_finite" in cov["tail"]
    flagged = [iv for mb in cov["micro"] for iv, _ in mb["tn"] + mb["fin"]]
    for lo, hi in flagged + [(o, o + c) for o, c in cov["finite_spans"]]:
        if hi > n:
            bad.append(f"{name}: a checked interval [{lo}, {hi}) reaches the loss slot at {n}")
    if any(mb["single"] for mb in cov["micro"]) and cov["found_inf"] and not full:
        bad.append(f"{name}: a single-launch gemm_finalize wrote a gradient and the step did not take the full pass")
    if not full:
        if "check_finite_spans" not in cov["tail"] and cov["finite_spans"]:
            bad.append(f"{name}: neither finite check ran")
        first = [iv for iv, _ in cov["micro"][0]["tn"] + cov["micro"][0]["fin"]]
        gaps, overlaps = uncovered(n, first + [(o, o + c) for o, c in cov["finite_spans"]])
        if gaps:
            bad.append(f"{name}: {sum(h - l for l, h in gaps)} gradient floats without a detector, first {gaps[:3]}")
        if overlaps:
            bad.append(f"{name}: detectors overlap at {overlaps[:3]}")
        for i, mb in enumerate(cov["micro"]):
            if mb["unflagged"]:
                bad.append(f"{name}: micro-batch {i}: {len(mb['unflagged'])} gradient-writing launches without the flag, first {mb['unflagged'][:3]}")
            if sorted(iv for iv, _ in mb["tn"] + mb["fin"]) != sorted(first):
                bad.append(f"{name}: micro-batch {i} flags other destinations than micro-batch 0")
            want_store = i == 0
            wrong = [iv for iv, mode in mb["tn"] if (mode == K.OUT_F32) != want_store] + [iv for iv, st in mb["fin"] if st != want_store]
            if wrong:
                bad.append(f"{name}: micro-batch {i}: {len(wrong)} flagged launches not in the {'store' if want_store else '+='} form")
    return bad


# ---- 3. one poisoned launch in a whole step -----------------------------------------------------------------------------------------------
def tiny_trainer(dev, dtype, lora_r=0, seed=5, **kw):
    """Trainer of the tiny topology on (1, 3, 16, 16) from seeded weights, and its seeded batch (tests/e2e_checks.run_steps' construction)"""
    from oracle.step import edm_inputs, make_synthetic_batch
    from oracle.unet import TINY_CONFIG, UNetSpatioTemporalConditionOracle, scaled_init_
    from svd_xtend_amd.train import Trainer
    from svd_xtend_amd.unet import UNetSpatioTemporalConditionModel
    cfg = TINY_CONFIG
    orc = UNetSpatioTemporalConditionOracle(**cfg)
    scaled_init_(orc, seed)
    b = make_synthetic_batch(1, 3, 16, 16, 77, cross_dim=cfg["cross_attention_dim"])
    unet_in, ts, ehs, ids, noisy, _ = edm_inputs(b)
    batch = {k: v.to(dev) for k, v in dict(unet_in=unet_in, timesteps=ts, ehs=ehs, added_time_ids=ids, noisy_latents=noisy,
                                           target=b["latents"], sigmas=b["sigmas"]).items()}
    m = UNetSpatioTemporalConditionModel(**cfg)
    m.load_state_dict(orc.state_dict(), strict=True)
    if lora_r:
        from svd_xtend_amd.lora import LoraConfig
        torch.manual_seed(seed + 5)
        m.add_adapter(LoraConfig(r=lora_r, lora_alpha=lora_r, init_lora_weights="gaussian"))
        gen = torch.Generator().manual_seed(seed + 17)
        for n, p in m.named_parameters():
            if ".lora_B." in n:
                p.data.copy_(torch.randn(p.shape, generator=gen) * 0.05)
    m.to(dev)
    return Trainer(m, dtype=dtype, lr=1e-3, **kw), batch


class PoisonTN:
    """Wraps the backend's gemm_tn: logs every launch and, for launch `target` (counted from the moment of entering), sets one element
    of the A operand (the activation gradient) inside [:R, :N] to `value`, makes the call and puts the saved value back -- a non-finite
    in that launch's output (and the column sums riding on it) and nowhere else.  n_limit: the column of A stays below it (a LoRA rank
    below the K granule: only the first `rank` output rows of the padded factor gradient reach the gradient buffer)."""

    def __init__(self, k, target=None, value=INF, n_limit=None):
        self.k, self.target, self.value, self.n_limit, self.log = k, target, value, n_limit, []

    def __enter__(self):
        self.own = vars(self.k).get("gemm_tn")              # (a backend that keeps its entries as instance attributes)
        self.inner = self.k.gemm_tn
        self.k.gemm_tn = self._call
        return self

    def __exit__(self, *exc):
        if self.own is not None:
            self.k.gemm_tn = self.own
        else:
            del self.k.gemm_tn
        return False

    def _call(self, A, B, C, R, N, Kd, lda, ldb, ldc, out_mode=K.OUT_F32_ADD, split_k=1, a_colsum=None, stages=0, found_inf=None):
        i = len(self.log)
        self.log.append(dict(R=R, N=N, K=Kd, out_mode=out_mode, split_k=split_k, flagged=found_inf is not None, colsum=a_colsum is not None))
        if i != self.target:
            return self.inner(A, B, C, R, N, Kd, lda, ldb, ldc, out_mode, split_k, a_colsum, stages, found_inf)
        el = torch.as_strided(A, (1,), (1,), A.storage_offset() + ((7 * i + 3) % R) * lda + (13 * i + 5) % min(N, self.n_limit or N))
        saved = el.clone()
        el.fill_(self.value)
        try:
            return self.inner(A, B, C, R, N, Kd, lda, ldb, ldc, out_mode, split_k, a_colsum, stages, found_inf)
        finally:
            el.copy_(saved)


def snapshot(tr):
    wt = tr.rt.wt16_flat
    return dict(p=tr.p_flat.clone(), m=tr.m_flat.clone(), v=tr.v_flat.clone(), w16=tr.rt.w16_flat.clone(),
                wt16=None if wt is None else wt.clone(), st=tr.opt_state.clone())


def tn_launches(tr, batch):
    """the gemm_tn launches of one step's sweeps, without touching the trainer's state beyond the gradient buffer"""
    with PoisonTN(tr.rt.k) as p:
        tr.zero_grad()
        for b in [batch] * tr.grad_accum:
            tr.forward_backward(**b)
    tr.micro = 0
    tr.rt.unchecked_grads = False
    return p.log


def distinct_launches(log, lo=0):
    """index of the first launch per distinct (R, N, K, out_mode), from index `lo` on"""
    first = {}
    for i, e in enumerate(log):
        if i >= lo:
            first.setdefault((e["R"], e["N"], e["K"], e["out_mode"]), i)
    return sorted(first.values())


def skipped_step(tr, batch, target, value=INF, then_clean=True, n_limit=None):
    """One step with launch `target` of its sweeps poisoned: the step is skipped (opt_state[7] = 1, the step count unchanged, the scale
    halved and the growth tracker 0 under dynamic scaling), masters, moments and both 16-bit twins keep their bits, with clipping the norm
    is not finite and opt_state[4] is the factor optim_prep wrote (tests/test_clip_grad_norm.py's contract for a skipped step); the next
    step, clean, is taken.  -> failures"""
    before = snapshot(tr)
    with PoisonTN(tr.rt.k, target, value, n_limit) as p:
        tr.zero_grad()
        for b in [batch] * tr.grad_accum:
            tr.forward_backward(**b)
        raised = None if tr.rt.found_inf is None else float(tr.rt.found_inf[0])
        tr.finish_grads()
        tr.optimizer_step()
    sync(tr.dev)
    what = f"launch {target} {p.log[target] if target is not None and target < len(p.log) else ''}"
    bad = []
    if target is None or target >= len(p.log):
        return [f"{what}: the step has {len(p.log)} gemm_tn launches"]
    folded = tr.rt.fold_finite and tr.rt.found_inf is not None
    if folded and p.log[target]["flagged"] and raised != 1.0:
        bad.append(f"{what}: the flag was {raised} when the sweep ended (the launch itself did not raise it)")
    after = snapshot(tr)
    st0, st1 = before["st"].tolist(), after["st"].tolist()
    if st1[7] != 1.0 or st1[0] != st0[0] or st1[3] != 0.0:
        bad.append(f"{what}: not skipped: skip {st1[7]}, step {st0[0]} -> {st1[0]}, found_inf {st1[3]}")
    if tr.dynamic and (st1[1] != 0.5 * st0[1] or st1[2] != 0.0):
        bad.append(f"{what}: scale {st0[1]} -> {st1[1]}, growth tracker {st1[2]}")
    if not tr.dynamic and (st1[1] != st0[1] or st1[2] != st0[2]):
        bad.append(f"{what}: static scale moved: {st0[1:3]} -> {st1[1:3]}")
    for k_ in ("p", "m", "v", "w16", "wt16"):
        if before[k_] is not None and not same_bits(before[k_], after[k_]):
            bad.append(f"{what}: {k_} changed in a skipped step")
    if tr.clip_out is not None:
        if math.isfinite(float(tr.clip_out[0])):
            bad.append(f"{what}: clipping reports the finite norm {float(tr.clip_out[0])}")
        if st1[4] != torch.tensor(1.0 / st0[1], dtype=torch.float64).float().item():
            bad.append(f"{what}: opt_state[4] = {st1[4]} in a skipped step, optim_prep wrote {1.0 / st0[1]}")
    if then_clean:
        tr.step([batch] * tr.grad_accum)
        sync(tr.dev)
        st2 = tr.opt_state.tolist()
        if st2[7] != 0.0 or st2[0] != st1[0] + 1.0 or same_bits(tr.p_flat, after["p"]):
            bad.append(f"{what}: the clean step after it: skip {st2[7]}, step {st1[0]} -> {st2[0]}")
        if tr.dynamic:
            tr.opt_state[1] = before["st"][1]                  # the next poisoned step starts from the same scale again
    return bad


def poisoned_steps(be, dev, dtype, lora_r=0, pick="distinct", part=None, rt_attrs=None, **kw):
    """Poisoned steps of the tiny Trainer on backend `be`.  pick: "all" launches of the step's last sweep, one per "distinct"
    (R, N, K, out_mode), "three" of those, or a tuple of launch indices; part = (i, n): every n-th of them from the i-th on.  The last
    poisoned step is followed by a clean one.  -> (failures, flagged gemm_tn launches of the step or None when not counted, steps poisoned)"""
    with backend(be):
        tr, batch = tiny_trainer(dev, dtype, lora_r=lora_r, **kw)
        for k_, v_ in (rt_attrs or {}).items():
            assert hasattr(tr.rt, k_), k_
            setattr(tr.rt, k_, v_)
        folded = tr.rt.fold_finite and tr.rt.found_inf is not None
        if isinstance(pick, tuple):                                   # launch indices known from another backend's run of the same step
            targets, log = list(pick), None
        else:
            log = tn_launches(tr, batch)
            per_sweep = len(log) // tr.grad_accum
            assert per_sweep * tr.grad_accum == len(log) and all(e["flagged"] == folded for e in log)
            lo = len(log) - per_sweep                                # grad_accum = 2: the launches of the second micro-batch only
            targets = list(range(lo, len(log))) if pick == "all" else distinct_launches(log, lo)
            if pick == "three":
                targets = [targets[0], targets[len(targets) // 2], targets[-1]]
        if part is not None:
            targets = targets[part[0]::part[1]]
        bad = []
        for i in targets:
            bad += skipped_step(tr, batch, i, VALUES[i % 3], then_clean=log is not None and i == targets[-1],
                                n_limit=lora_r if 0 < lora_r < 64 else None)
    return bad, (len(log) if folded else 0) if log is not None else None, len(targets)


def op_level_row_sliced(be, dev, dt, shape, overwrite, defer, value=INF):
    """ops.gemm_tn_acc on a weight gradient the host rule row-slices (M = 1024: the tiny step reaches no such launch): deferred route --
    rt.flush_deferred()'s table-driven reduction raises rt.found_inf; immediate route (the single-launch gemm_finalize carries no flag) --
    rt.unchecked_grads is set and svdx_check_finite over the destination raises it.  The clean call leaves everything down.  -> failures"""
    from svd_xtend_amd import ops
    M, (N, Kd) = 1024, shape
    sk, _ = ops._tn_formula(M, N, Kd)
    bad = [] if sk > 1 else [f"{shape}: the host rule does not slice this shape"]
    g = torch.Generator().manual_seed(5)
    dy, x = (torch.randn(M, N, generator=g).to(dt).to(dev), (torch.randn(M, Kd, generator=g) * M ** -0.5).to(dt).to(dev))
    for poisoned in (False, True):
        with census._backend(be):
            rt = ops.Runtime(dt, torch.device(dev))
        st = _state(dev)
        rt.found_inf, rt.grad_overwrite, rt.defer_grad_finalize = st[3:4], overwrite, defer
        dst = torch.ones(N, Kd, device=dev)
        a = dy.clone()
        if poisoned:
            a[M - 3, N // 3] = value
        ops.gemm_tn_acc(rt, a, x, dst, M, N, Kd, N, Kd, write_once=True)
        what = f"gemm_tn_acc {shape} overwrite={overwrite} defer={defer} {'poisoned' if poisoned else 'clean'}"
        if defer:
            if not rt.deferred_pending or rt.unchecked_grads:
                bad.append(f"{what}: nothing queued")
            rt.flush_deferred()
            sync(dev)
            bad += _state_verdict(st, 1.0 if poisoned else 0.0, what + " after flush_deferred")
        else:
            if not rt.unchecked_grads:
                bad.append(f"{what}: unchecked_grads not set by the single-launch reduction")
            sync(dev)
            bad += _state_verdict(st, 0.0, what + " (the single-launch reduction carries no flag)")
            be.check_finite(dst, N * Kd, st)
            sync(dev)
            bad += _state_verdict(st, 1.0 if poisoned else 0.0, what + " after the full pass")
        if bool(torch.isfinite(dst).all()) == poisoned:
            bad.append(f"{what}: destination finite = {not poisoned}")
    return bad


def accumulated_slots(tr, batch, rows=None):
    """after a clean sweep, +-inf / NaN written from the host into the first and the last float of every accumulated slot below n_flat (one
    at a time; the rows are derived here from zero_spans, as Trainer.finite_spans is, so a row missing from that table shows): the step is
    skipped; the same value in the loss slot [n_flat, n_total) does not skip.  The sweep runs once: every case restores its gradient
    buffer and runs the optimizer step alone.  -> (failures, optimizer steps)"""
    slots = [(c, min(n, tr.n_flat - c)) for c, n in tr.zero_spans.tolist() if c < tr.n_flat]
    places = [(o + d, True) for o, c in (slots if rows is None else [slots[r] for r in rows]) for d in sorted({0, c - 1})]
    places += [(tr.n_flat, False), (tr.n_total - 1, False)]
    tr.step(batch)
    tr.zero_grad()
    tr.forward_backward(**batch)
    grads = tr.g_flat.clone()
    bad = []
    for n, (idx, skips) in enumerate(places):
        before = snapshot(tr)
        tr.g_flat.copy_(grads)
        tr.g_flat[idx] = VALUES[n % 3]
        tr.finish_grads()
        tr.optimizer_step()
        sync(tr.dev)
        st0, st1 = before["st"].tolist(), tr.opt_state.tolist()
        what = f"{VALUES[n % 3]} at g_flat[{idx}] ({'a gradient slot' if skips else 'the loss slot'})"
        if skips:
            if st1[7] != 1.0 or st1[0] != st0[0] or not all(same_bits(before[k_], v_) for k_, v_ in snapshot(tr).items() if k_ != "st" and v_ is not None):
                bad.append(f"{what}: not skipped (skip {st1[7]}, step {st0[0]} -> {st1[0]})")
            if tr.dynamic:
                tr.opt_state[1] = before["st"][1]
        elif st1[7] != 0.0 or st1[0] != st0[0] + 1.0:
            bad.append(f"{what}: skipped the step")
    return bad, len(places) + 1


# ---- 4. the loss-scale state machine ---------------------------------------------------------------------------------------------------------
PREP_STEPS = 64
INTERVALS = (1, 2, 5)
BETAS = (0.9, 0.999)
SCHED = [3.0, 4.0, 64.0, 0.5, 0.0, 0.0, 1.0]          # cosine, 4 warm-up steps of 64: st[8] moves with the step count


def prep_sequences(interval):
    """found / not-found sequences of 64 steps: all clean, all bad, alternating, bad exactly on the growth boundary (the step on which
    the tracker would reach the interval), two seeded random ones"""
    n = PREP_STEPS
    seqs = {"all clean": [False] * n, "all bad": [True] * n, "alternating": [i % 2 == 1 for i in range(n)]}
    boundary, tracker = [], 0
    for i in range(n):
        hit = tracker + 1 >= interval and i % 3 != 0          # not every time: growth happens too
        boundary.append(hit)
        tracker = 0 if (hit or tracker + 1 >= interval) else tracker + 1
    seqs["bad on the growth boundary"] = boundary
    for s in (1, 2):
        seqs[f"random {s}"] = (torch.rand(n, generator=torch.Generator().manual_seed(s)) < 0.3).tolist()
    return seqs


def grad_scaler_rule(scale, tracker, found, interval, dynamic, growth=2.0, backoff=0.5):
    """torch/amp/grad_scaler.py, GradScaler.update -> torch._amp_update_scale_: found_inf -> scale *= backoff_factor, growth_tracker = 0;
    else growth_tracker += 1 and, when it reaches growth_interval, scale *= growth_factor and growth_tracker = 0.  GradScaler.step skips
    optimizer.step() when found_inf.  (With a static scale -- bf16, no GradScaler in the reference -- nothing moves; a non-finite gradient
    still skips.)"""
    if dynamic:
        if found:
            return scale * backoff, 0.0
        tracker += 1.0
        if tracker >= interval:
            return scale * growth, 0.0
    return scale, tracker


def torch_grad_scaler_trace(seq, interval, init_scale=65536.0):
    """[(scale, tracker, steps taken)] of torch.amp.GradScaler itself on the CPU over `seq`, or None where the installed torch has none"""
    try:
        scaler = torch.amp.GradScaler("cpu", init_scale=init_scale, growth_factor=2.0, backoff_factor=0.5, growth_interval=interval)
        p = torch.nn.Parameter(torch.zeros(4))
        opt = torch.optim.SGD([p], lr=0.0)
        taken, out = [0], []
        opt.register_step_post_hook(lambda *_: taken.__setitem__(0, taken[0] + 1))
        for found in seq:
            scaler.scale(torch.zeros(()))                      # (creates the scale tensor: step() refuses without one scale() call)
            p.grad = torch.full((4,), INF if found else 1.0)
            scaler.step(opt)
            scaler.update()
            out.append((float(scaler.get_scale()), float(scaler._growth_tracker), taken[0]))
        return out
    except Exception as e:  # noqa: BLE001 -- no CPU GradScaler in this torch: the restated rule stands alone
        print(f"torch.amp.GradScaler on the CPU: {e!r}")
        return None


def prep_sequence_check(be, dev, seq, interval, dynamic, what):
    """svdx_optim_prep over `seq`: scale, tracker, step count, skip flag, the cleared found_inf and the gradient factor 1 / scale exact
    (powers of two throughout); bc1, bc2 against float64 powers of the float betas the entry receives, at tests/kernel_checks.check_optim's
    bar (its relerr, 1e-5, over the pair); the schedule multiplier st[8] against the float64 lambda within 5e-6.  -> failures"""
    from kernel_checks import relerr
    st = torch.zeros(K.OPT_STATE_ALLOC, device=dev)
    st[1], st[4], st[5], st[6], st[8] = (65536.0 if dynamic else 1.0), 1.0, 1.0, 1.0, 1.0
    st[9:16] = torch.tensor(SCHED, device=dev)
    trace = []
    for found in seq:
        st[3] = 1.0 if found else 0.0
        be.optim_prep(st, BETAS[0], BETAS[1], 2.0, 0.5, interval, int(dynamic))
        trace.append(st.clone())
    sync(dev)
    trace = torch.stack(trace).cpu()
    b1, b2 = (float(torch.tensor(b, dtype=torch.float32)) for b in BETAS)
    scale, tracker, step, bad = (65536.0 if dynamic else 1.0), 0.0, 0.0, []
    host = torch.zeros(K.OPT_STATE_ALLOC)
    host[9:16] = torch.tensor(SCHED)
    for i, found in enumerate(seq):
        lam = emul.EmuBackend._lr_lambda(host, step * max(1.0, SCHED[6]))
        inv = 1.0 / scale
        scale, tracker = grad_scaler_rule(scale, tracker, found, interval, dynamic)
        step += 0.0 if found else 1.0
        got = trace[i].tolist()
        want = [step, scale, tracker, 0.0, inv]
        if got[:5] != want or got[7] != (1.0 if found else 0.0):
            bad.append(f"{what}: step {i} (found={found}): state {got[:8]}, expected {want} and skip {found}")
            break
        bc = torch.tensor([1.0 - b1 ** step, 1.0 - b2 ** step], dtype=torch.float64)
        if relerr(trace[i, 5:7], bc) > 1e-5:
            bad.append(f"{what}: step {i}: bias corrections {got[5:7]}, float64 {bc.tolist()}")
        if abs(got[8] - lam) > 5e-6:
            bad.append(f"{what}: step {i}: lr multiplier {got[8]}, float64 {lam}")
    return bad


# ---- 4. the optimizer kernels in a skipped step ---------------------------------------------------------------------------------------------
def skipped_adamw(be, dev, dt, skip=True):
    """svdx_adamw and svdx_adamw_tiled with opt_state[7] = 1 and a gradient buffer full of NaN, both param_modes; tiles with and without a
    transposed twin, a partial 36 x 48 tile of each kind: p, m, v, the 16-bit twin and the transposed twin keep their bits;
    svdx_grad_clip_coef leaves opt_state[4] alone.  (skip=False: the same call sequence on a step that is taken -- the buffers must move.)"""
    from svd_xtend_amd.train import build_adam_tiles
    g = torch.Generator().manual_seed(13)
    shapes = [(128, 192), (36, 48), (36, 48), (320,)]
    ps = [torch.nn.Parameter(torch.randn(s, generator=g)) for s in shapes]
    offs, off = [], 0
    for q in ps:
        offs.append(off)
        off = (off + q.numel() + 63) // 64 * 64
    n = off
    wt_map = {id(ps[0]): (64, 132), id(ps[1]): (64 + 192 * 132, 40)}            # twins [192, 132] and [48, 40]; the second 36 x 48 has none
    tiles = build_adam_tiles(ps, offs, wt_map, dev)
    assert {(int(r), int(c)) for r, c in tiles[:, 2:4].tolist()} >= {(36, 48), (64, 64)} and int((tiles[:, 4] < 0).sum()) and int((tiles[:, 4] >= 0).sum())
    n_t = 64 + 192 * 132 + 48 * 40
    bad = []
    for mode in (K.PARAMS_F32, K.PARAMS_BF16_REFERENCE):
        for tiled in (False, True):
            p, m, v = torch.randn(n, generator=g).to(dev), (torch.randn(n, generator=g) * 0.1).to(dev), torch.randn(n, generator=g).abs().to(dev)
            if mode == K.PARAMS_BF16_REFERENCE:
                p, m, v = (t.to(torch.bfloat16).float() for t in (p, m, v))
            pa, pt = torch.randn(n, generator=g).to(dt).to(dev), torch.randn(n_t, generator=g).to(dt).to(dev)
            grad = torch.full((n,), NAN, device=dev) if skip else torch.randn(n, generator=g).to(dev)
            st = torch.tensor([3, 64.0, 5, 0, 1 / 64.0, 0.271, 0.003, 1.0 if skip else 0.0, 0.37] + [0.0] * (K.OPT_STATE_ALLOC - 9), device=dev)
            keep = [t.clone() for t in (p, m, v, pa, pt, st)]
            if tiled:
                be.adamw_tiled(p, grad, m, v, tiles, tiles.shape[0], 1e-3, 0.9, 0.999, 1e-8, 1e-2, 0.5, st, pa, pt, param_mode=mode)
            else:
                be.adamw(p, grad, m, v, n, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 0.5, st, pa, param_mode=mode)
            sync(dev)
            what = f"{'adamw_tiled' if tiled else 'adamw'} param_mode={mode} {str(dt)[6:]}"
            for name, a, b in zip(("p", "m", "v", "p_act", "pt_act", "opt_state"), (p, m, v, pa, pt, st), keep):
                moved = not same_bits(a, b)
                if skip and moved:
                    bad.append(f"{what}: {name} changed in a skipped step")
                if not skip and not moved and name in ("p", "m", "p_act"):
                    bad.append(f"{what}: {name} did not move in a step that is taken")
    return bad


def skipped_clip_coef(be, dev):
    """svdx_grad_clip_coef in a skipped step: the norm of the NaN gradient is not finite and opt_state[4] keeps its bits"""
    import clip_checks as cc
    sizes = [5, 130, 3001]
    rows, offs, n = cc.span_rows(sizes)
    spans = torch.tensor(rows, dtype=torch.int32, device=dev)
    grad = torch.full((n + 64,), NAN, device=dev)
    part = torch.zeros(len(rows), dtype=torch.float64, device=dev)
    st = torch.zeros(K.OPT_STATE_ALLOC, device=dev)
    st[1], st[4], st[5], st[6], st[7], st[8] = 64.0, 1 / 64.0, 1.0, 1.0, 1.0, 1.0
    out = torch.zeros(2, device=dev)
    be.grad_sumsq_spans(grad, spans, len(rows), part)
    be.grad_clip_coef(part, spans, len(rows), len(sizes), 1.0, 1.0, st, out)
    sync(dev)
    bad = []
    if math.isfinite(float(out[0])):
        bad.append(f"grad_clip_coef: norm {float(out[0])} of a NaN gradient")
    if float(st[4]) != 1 / 64.0 or float(st[7]) != 1.0:
        bad.append(f"grad_clip_coef: opt_state[4] = {float(st[4])} after a skipped step (was {1 / 64.0})")
    return bad


@contextlib.contextmanager
def backend(be):
    with census._backend(be):
        yield be
