"""Shared checks of how far an operand reaches in memory (tests/test_reach.py on the simulator, tests/test_reach_gpu.py on the device).

The library changes kernels, or refuses the launch, where an operand's extent reaches 2^31 bytes (census.gemm_kernel_taken restates the
entry points' conditions); everywhere else the addressing is 64-bit arithmetic that was read and never run.  An extent is rows x pitch:
a large pitch puts a few rows far apart while only rows x cols elements are touched, so the line is crossed at the smallest shapes.

* `pitched_cases(entry, arg)`: one small signature per feature combination of the tiny censuses (the fewest rows that make two row
  tiles), with the pitch `arg` rewritten so that the extent of the operand it moves is (i) the largest admissible value below 2^31
  bytes, (ii) the smallest at or above 2^31, (iii) the smallest at or above 2^32.  `run_pitched` sends each through the entry's census
  runner: the same float64 reference, per-element bound, NaN prefill and guard bands.  No tolerance is introduced here.
* at (i) and (ii) `gemm` and `gemm_tn` answer with two kernels: the two results of the SAME operands must agree within the sum of their
  two bounds (`captured_bounds` takes the bounds census.judge_single forms).
* the forms the library refuses (`assert_refused`): K.SvdxError, a message that names the limit, every output's prefill untouched.
  Their accepted neighbour one step below the limit is the (i) case of the same signature and pitch.
* `T_LIMIT_CASES`: svdx_tattn_fwd / svdx_tattn_bwd at the stated limit T = 32 and in the two-block form between its tested sizes.

* `run_windowed`: the entries without a pitch at 4 GiB plus one unit, one full-size launch judged by the entry's runner on windows.  Among
  them what looks like a pitch and is none: `nchw_to_rows`'s ld and `transpose`'s ld_out are written over their whole width (padding
  columns are zeros), and the split-K slab output has no pitch at all (the slices are M x N, back to back): they reach 2^31 bytes only
  at their real size.  svdx_tsa_fwd one step below its limit is judged the same way.
* `run_gather_limit`: svdx_gemm_tn_gather served with dY's span at its limit and refused 16 bytes beyond."""
import collections
import contextlib
import dataclasses
import gc

import torch

import census
from svd_xtend_amd import kernels as K

# level -> the extent it reaches.  (iii) lies a row's width beyond 2^32 bytes, so that the OFFSET of the last row, not only its end, is past
# the line: a row offset narrowed to 32 bits then wraps whatever the row count
LEVELS = collections.OrderedDict([("i", None), ("ii", census.REACH_2G), ("iii", census.REACH_4G + (1 << 16))])
ALIGN = 8                     # every pitch is rewritten in steps of 8 elements: what the entries' alignment rules admit
MIN_ROWS = 129                # two row tiles, the second partial
SIM_MAX_S = 160               # spatial attention from here on is too slow for the simulator: it gets the largest smaller S of the census

# entry -> its pitch arguments ("gather.lda": the pitch of the gather's source rows)
PITCHES = collections.OrderedDict([
    ("gemm", ("lda", "gather.lda", "ldb", "ldc", "ldres")),
    ("gemm_tn", ("lda", "ldb")),
    ("attn_fwd", ("ld", "ld_o")),
    ("attn_bwd_prep", ("ld_o",)),
    ("attn_bwd_dkv", ("ld", "ld_o", "ld_d")),
    ("attn_bwd_dq", ("ld", "ld_o", "ld_d")),
    ("tattn_fwd", ("ld", "ld_o")),
    ("tattn_bwd", ("ld", "ld_o", "ld_d")),
    ("colsum", ("ldx",)),
    ("transpose", ("ld_in",)),
    ("softmax_rows", ("ld_in", "ld_out")),
    ("attn_small_fwd", ("ld", "ld_o")),
    ("rows_to_nchw", ("ld",)),
    ("edm_loss", ("ld",)),
])
PITCH_IDS = [f"{e}-{p}" for e, ps in PITCHES.items() for p in ps]
TINY_STEP = tuple(census.GEOM_TINY) + ("tiny_fp16", "tiny_bf16")


def with_args(sig, **kw):
    assert set(kw) <= {k for k, _ in sig[1]}, (sig[0], kw)
    return (sig[0], tuple((k, kw.get(k, v)) for k, v in sig[1]))


def set_pitch(sig, arg, ld):
    a = census.sig_args(sig)
    if arg == "gather.lda":
        return with_args(sig, gather=dataclasses.replace(a["gather"], lda=ld), lda=ld)
    if sig[0] == "gemm" and arg in ("ldc", "ldres") and a["res"] is not None and a["res"][2] == ("C", 0):
        return with_args(sig, ldc=ld, ldres=ld)                 # a residual added in place: one tensor, one pitch
    return with_args(sig, **{arg: ld})


def get_pitch(sig, arg):
    a = census.sig_args(sig)
    return a["gather"].lda if arg == "gather.lda" else a[arg]


def applies(sig, arg):
    a = census.sig_args(sig)
    if sig[0] == "gemm":
        gathered = a["gather"] is not None and a["gather"].mode != K.GATHER_PLAIN
        # (the slab output and the GEGLU epilogues fix ldc: N for the slices and the forward's pre, 2F for the backward's d(pre))
        return {"lda": not gathered, "gather.lda": gathered, "ldb": True, "ldc": a["out_mode"] != K.OUT_F32_SLAB and a["epilogue"] == K.EPI_NONE,
                "ldres": a["res"] is not None}[arg]
    return True


def pitched(sig, arg, level):
    """`sig` with the pitch `arg` rewritten for `level`, and the operand whose extent that sets (the one the pitch moves furthest);
    None where the pitch moves nothing (a single row) or would not fit an int"""
    ld0 = get_pitch(sig, arg)
    r0, r1 = census.reach(set_pitch(sig, arg, ld0)), census.reach(set_pitch(sig, arg, ld0 + ALIGN))
    slope = {n: (r1[n] - r0[n]) // ALIGN for n in r0 if r1[n] != r0[n]}          # bytes per element of pitch: (rows - 1) x element size
    if not slope:
        return None
    name = max(slope, key=lambda n: (slope[n], r0[n]))
    step = slope[name] * ALIGN
    if level == "i":
        k = (census.REACH_2G - 1 - r0[name]) // step
    else:
        k = -(-(LEVELS[level] - r0[name]) // step)
    ld = ld0 + k * ALIGN
    if ld >= 1 << 31:
        return None
    out = set_pitch(sig, arg, ld)
    ext = census.reach(out)[name]
    assert (ext < census.REACH_2G and ext + step >= census.REACH_2G) if level == "i" else (LEVELS[level] <= ext < LEVELS[level] + step), (arg, level, ext)
    return out, name


_TINY = {}


def tiny_signatures(entry):
    if not _TINY:
        for n in TINY_STEP:
            for s in census.census(n):
                _TINY.setdefault(s[0], set()).add(s)
        for n in census.COND_TINY:
            for s in census.census_cond(n):
                _TINY.setdefault(s[0], set()).add(s)
    return sorted(_TINY.get(entry, ()), key=repr)


def _rows(sig):
    """the rows a tile walks: the keys of the spatial attention, else the launch's row count"""
    a = census.sig_args(sig)
    return a["S"] if sig[0].startswith("attn_") else census.sig_rows(sig)


def coarse_key(sig):
    """what the simulator's quick pass keeps apart (SVDX_SIM_FULL=1: every feature combination): for `gemm` the tile, the gather's kind,
    the output mode, the epilogue and whether the launch is a dual / GroupNorm-statistics / residual form; else the feature combination
    without the operand types' second copy"""
    a = census.sig_args(sig)
    if sig[0] == "gemm":
        from svd_xtend_amd.ops import _tile_launched
        g = a["gather"]
        return (_tile_launched(a["variant"], a["M"], a["N"]), None if g is None else (g.mode, g.stride, g.ups), a["out_mode"], a["epilogue"],
                a["dual"] is not None, a["gn"] is not None, a["res"] is not None)
    if sig[0] == "gemm_tn":
        return (a["out_mode"], a["split_k"] > 1, a["a_colsum"] is not None)
    return ()


def base_signatures(entry, sim=False, full=True):
    """one signature of the tiny censuses per feature combination of `entry`: the fewest rows that still make two row tiles (MIN_ROWS),
    else the most there are.  On the simulator the spatial attention takes the largest S below SIM_MAX_S instead of the census shape the
    device runs (S >= 160: the deferred-rescale operands), and, unless `full`, one signature per `coarse_key`."""
    by = collections.OrderedDict()
    for s in tiny_signatures(entry):
        by.setdefault(census.feature_key(s), []).append(s)
    out = []
    for ss in by.values():
        if sim and entry.startswith("attn_") and entry != "attn_small_fwd":
            ok = [s for s in ss if census.sig_args(s)["S"] < SIM_MAX_S]
            out.append(max(ok, key=lambda s: (_rows(s), repr(s))))
            continue
        ok = [s for s in ss if _rows(s) >= MIN_ROWS]
        out.append(min(ok, key=lambda s: (_rows(s), repr(s))) if ok else max(ss, key=lambda s: (_rows(s), repr(s))))
    if sim and not full:
        first = collections.OrderedDict()
        for s in sorted(out, key=lambda s: (_rows(s), repr(s))):
            first.setdefault(coarse_key(s), s)
        out = list(first.values())
    return out


Case = collections.namedtuple("Case", "entry arg level base sig operand verdict")


def pitched_cases(entry, arg, sim=False, full=True):
    """[Case] of one pitch argument: the base signatures it applies to x the three levels.  verdict: census.gemm_kernel_taken"""
    out = []
    for base in base_signatures(entry, sim, full):
        if not applies(base, arg):
            continue
        for level in LEVELS:
            p = pitched(base, arg, level)
            if p is not None:
                out.append(Case(entry, arg, level, base, p[0], p[1], census.gemm_kernel_taken(p[0])))
    return out


@contextlib.contextmanager
def captured_bounds():
    """{label: (what the launch left, its per-element bound)} of the single-rounding outputs a runner judges meanwhile"""
    kept, orig = {}, census.judge_single

    def judge(res, label, got, ref, S, k_acc, e, rounding=True, extra=None):
        kept[label] = (got.detach().clone(), census.single_bound(got.dtype, ref, S, k_acc, e, extra))
        return orig(res, label, got, ref, S, k_acc, e, rounding, extra)
    census.judge_single = judge
    try:
        yield kept
    finally:
        census.judge_single = orig


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def assert_refused(be, sig, dev, verdict):
    """the library refuses `sig` on the host: K.SvdxError whose message names the limit, and every output still holds its prefill"""
    assert verdict.startswith("refused: ")
    ops = []
    try:
        census.run_case(be, sig, dev, operands_out=ops)
    except K.SvdxError as e:
        assert verdict[len("refused: "):] in str(e), (verdict, str(e))
    else:
        raise AssertionError(f"served, not refused ({verdict}): {census.sig_str(sig, 300)}")
    o = ops[0]
    outs = [n for n, (_, _, is_out) in o.decls.items() if is_out]
    assert outs
    for n in outs:
        want = torch.zeros_like(o.t[n])
        o.decls[n][1](want)
        assert torch.equal(_bits(o.t[n]), _bits(want)), f"{n} written by a refused launch: {census.sig_str(sig, 300)}"
    assert not o.damaged_guards()


def run_pitched(be, dev, cases, worst=None):
    """the cases of one pitch argument on backend `be`: -> the lines of what failed.  `worst`: {(entry, level): excess} to fold into"""
    bad, kept = [], {}
    for c in cases:
        tag = f"{c.entry} {c.arg} ({c.level}: {c.operand} = {census.reach(c.sig)[c.operand]} bytes)"
        if c.verdict is not None and c.verdict.startswith("refused"):
            assert c.level != "i", (tag, c.verdict)
            assert_refused(be, c.sig, dev, c.verdict)
            continue
        with captured_bounds() as bounds:
            res = census.run_case(be, c.sig, dev, seed_of=c.base)
        for label, excess, idx in res:
            if worst is not None and "rounding" not in label:
                worst[(c.entry, c.level)] = max(worst.get((c.entry, c.level), 0.0), excess)
            if not excess <= 1.0:
                bad.append(f"excess {excess:.4g} at {idx}: {label}: {tag}: {census.sig_str(c.sig, 400)}")
        if c.entry in ("gemm", "gemm_tn") and c.arg in ("lda", "gather.lda", "ldb") and c.level in ("i", "ii"):
            kept[(c.base, c.level)] = (bounds, c.verdict)
            if (c.base, "i") in kept and (c.base, "ii") in kept:
                (b1, v1), (b2, v2) = kept.pop((c.base, "i")), kept.pop((c.base, "ii"))
                assert v1 != v2 or K.TN_FLAT & census.sig_args(c.sig).get("stages", 0), f"one kernel on both sides of the line: {tag}: {v1}"
                assert b1.keys() == b2.keys() and b1
                for label in b1:
                    (g1, e1), (g2, e2) = b1[label], b2[label]
                    r = census._ratio(g1, g2.to(torch.float64), e1 + e2)
                    if worst is not None:
                        worst[(c.entry, "i vs ii")] = max(worst.get((c.entry, "i vs ii"), 0.0), float(r.max()))
                    if not float(r.max()) <= 1.0:
                        bad.append(f"the two kernels disagree by {float(r.max()):.4g} of their bounds' sum: {label}: {tag}: {census.sig_str(c.sig, 400)}")
        del bounds, res
        release(dev)
    return bad


def release(dev):
    """an Operands object and its fill closures refer to each other: its gigabytes go with the cycle collector, not with the last name"""
    gc.collect()
    if torch.device(dev).type == "cuda":
        torch.cuda.empty_cache()


def flat_staging(cases):
    """the gemm_tn cases again with the flat staging asked for (K.TN_FLAT): below the line it is the other kernel on the same operands"""
    return [c._replace(sig=with_args(c.sig, stages=census.sig_args(c.sig)["stages"] | K.TN_FLAT),
                       base=with_args(c.base, stages=census.sig_args(c.base)["stages"] | K.TN_FLAT),
                       verdict="gemm_tn kernel, flat staging") for c in cases]


# ---- stated limits, at the limit -----------------------------------------------------------------------------------------------------------
T_LIMIT_CASES = [(1, 32, 5, 1), (2, 31, 3, 2), (1, 24, 4, 1)]          # (B, T, HW, heads): also in kernel_checks.check_temporal_attention
T_REFUSED = 33


def tattn_signatures(B, T, HW, heads, dt="f16"):
    """the signatures of the temporal attention pair as the step records them (q / k / v and dq / dk / dv packed in one matrix each)"""
    base = {s[0]: s for s in tiny_signatures("tattn_fwd") + tiny_signatures("tattn_bwd") if census.sig_args(s)["q"][1] == dt}
    C = heads * 64
    was = {e: census.sig_args(s)["heads"] * 64 for e, s in base.items()}           # the packed operands sit C elements apart
    return [with_args(base[e], B=B, T=T, HW=HW, heads=heads, ld=3 * C, ld_o=C, **(dict(ld_d=3 * C) if e == "tattn_bwd" else {}),
                      **{k: v[:2] + ((v[2][0], v[2][1] // was[e] * C),) + v[3:] for k, v in base[e][1] if isinstance(v, tuple) and v and v[0] == "T" and v[2]})
            for e in ("tattn_fwd", "tattn_bwd")]


# ---- pitchless entries at 4 GiB (device only) ---------------------------------------------------------------------------------------------
# An entry that takes a count, or rows x C without a pitch, reaches 2^32 bytes only at its real size.  Its float64 reference over 2^31
# elements does not fit anywhere, so the launch runs ONCE on full-size operands and the entry's census runner judges WINDOWS of it: the
# first units, the last, and those that straddle byte offsets 2^31 and 2^32 of every operand.  A unit is what the count argument counts (an
# element, a row, a sample, an image).  The runner is given a backend that launches nothing: it plants the runner's own seeded inputs into
# the window of the full-size operands (pass 1) and, after the real launch, hands the window of the full-size outputs back to the runner
# (pass 2), which judges them against its float64 reference with its own bound.  Outside the windows the inputs are zero, so whatever
# a kernel reduces over the whole tensor has an exact reference; over the whole output a chunked scan finds elements that still hold
# the NaN prefill (an index that wrapped left them unwritten) or are not finite.  A wrap that writes twice lands in the windows at the
# start: the windows do not sit at equal distances from the wrap, so the values planted in one do not pass for those of another.
#
# Why the windows at 2^31 / 2^32 bytes notice a narrowed offset (argued, not run: no simulator-sized case exists).  Take svdx_add with
# `a + i * 8` computed in int: for i * 8 >= 2^31 elements the offset goes negative and the lane reads and writes BEFORE the buffer -- the
# low guard band or a fault; narrowed to unsigned it wraps at 2^32 elements, beyond these sizes, but a BYTE offset narrowed to 32 bits
# wraps at 2^32 bytes = element 2^31: the window that straddles it then holds the NaN prefill in its second half (unwritten) while the
# first window was written twice with values computed from zeros.  Either way the straddling window or the scan fails.
WINDOWED = collections.OrderedDict([          # entry -> (the argument that counts units, units per window)
    ("add", ("n", 1 << 16)), ("blend", ("n", 1 << 16)), ("blend_bwd", ("n", 1 << 16)), ("cast_from_f32", ("n", 1 << 16)), ("act_rows", ("n", 1 << 16)),
    ("geglu_fwd", ("M", 64)), ("geglu_bwd", ("M", 64)), ("add_rowvec", ("rows", 256)), ("concat2", ("rows", 256)), ("split2", ("rows", 256)),
    ("sum2x2", ("n_img", 4)), ("ln_fwd", ("rows", 256)), ("ln_bwd", ("rows", 256)),
    ("gn_stats", ("n_s", 4)), ("gn_apply", ("n_s", 4)), ("gn_bwd_stats", ("n_s", 4)), ("gn_bwd_apply", ("n_s", 4)),
    # written over their whole width, or without a pitch: no pitched case can take them to 2^31 bytes
    ("nchw_to_rows", ("n_img", 4)),           # unit: an image; `out` is n_img H W rows of ld elements, the padding columns written as zeros
    ("transpose", ("cols", 64)),              # unit: a column of the input = a row of ld_out elements of the output, zeros beyond `rows`
    ("gemm", ("n_img", 4)),                   # the split-K slab output [split_k][M][N] of a gathered convolution; unit: an image (ho wo rows of every slice)
])
# svdx_tsa_fwd is judged the same way, at its limit instead of 4 GiB (`tsa_limit`): a unit is a pixel, its rows lie T x HW apart
AT_LIMIT = {"tsa_fwd": ("HW", 64)}
_TSA_ROWS = ("x", "n1", "stats", "qkv", "o", "h1")
TRANSPOSE_ROWS, TRANSPOSE_LD_OUT = 1000, 1024          # ld_out / 64 x cols / 64 workgroups: cols = 2^21 + 1 keeps the grid's second dimension below 65536
WHOLE = ("zero", "check_finite", "ema_lerp")          # their runners judge in bounded pieces already: they run at full size as they are
COUNT_4G = (1 << 31) + (1 << 20)                      # 2^32 bytes of a 16-bit type plus 2^20 elements; as a float count, beyond 2^31
# reduced over every row of the launch: (the input that is zero in every window but the last, the outputs only the last window judges).
# What that leaves of svdx_ln_bwd: with dy = 0 the earlier windows' dx is `add` alone, so they judge the addressing of dx and add, not the
# reads of x, dy, gamma and the statistics (gamma, held once for the launch, is the last window's); those reads, and the affine sums, are
# judged in the last window -- the rows at and beyond 2^32 bytes -- and the scan covers every dx.
REDUCED = {"ln_bwd": ("dy", ("dgamma", "dbeta", "scratch"))}
_GN_TABLES = ("stats", "bstats")                      # [replica][sample][group][2]: the sample is not the leading dimension


class _Stop(Exception):
    pass


def _strip_alias(sig):
    return (sig[0], tuple((k, v[:2] + (None,) + v[3:]) if isinstance(v, tuple) and v and v[0] == "T" else (k, v) for k, v in sig[1]))


def _win(entry):
    return WINDOWED.get(entry) or AT_LIMIT[entry]


def _count(sig):
    a = census.sig_args(sig)
    return a["gather"].n_img if sig[0] == "gemm" else a[_win(sig[0])[0]]


def _slices(sig, name):
    """leading dimension of a tensor that is laid out [slice][unit][...]: the replicas of the GroupNorm tables, the split-K slabs"""
    if sig[0].startswith("gn_") and name in _GN_TABLES:
        return K.GN_REPLICAS
    if sig[0] == "tsa_fwd" and name in _TSA_ROWS:
        return census.sig_args(sig)["B"] * census.sig_args(sig)["T"]
    return census.sig_args(sig)["split_k"] if sig[0] == "gemm" and name == "C" else 1


def _resized(sig, units):
    cnt = _win(sig[0])[0]
    if sig[0] == "tsa_fwd":                                                   # (B = 1) one group: the same row vector for every row
        return with_args(sig, HW=units, rv_rpg=census.sig_args(sig)["T"] * units, rv_mod=0)
    if sig[0] == "gemm":
        g = census.sig_args(sig)["gather"]
        return with_args(sig, M=units * g.ho * g.wo, gather=dataclasses.replace(g, n_img=units))
    if sig[0] == "transpose":                                                 # a contiguous input: a unit is one column of it
        return with_args(sig, cols=units, ld_in=units, rows=TRANSPOSE_ROWS, ld_out=TRANSPOSE_LD_OUT)
    extra = dict(rpg=units, mod=0) if sig[0] == "add_rowvec" else {}          # one group: the same row vector wherever the window lies
    return with_args(sig, **{cnt: units}, **extra)


def base_4g(entry, i=0):
    """the signature of `entry` in the tiny censuses with the largest unit (the unfused GEGLU pair: the smallest real-width one), dtypes
    alternating over the entries; svdx_ln_bwd in its reducing form (the affine sums land in dgamma / dbeta, which the last window judges)"""
    sigs = tiny_signatures(entry) or sorted((s for s in census.census("e_1x1x8x8") if s[0] == entry), key=repr)
    assert sigs, entry
    if entry == "ln_bwd":
        sigs = [with_args(s, defer_reduce=False) for s in sigs if census.sig_args(s)["dgamma"] is not None]
    if entry == "gemm":
        sigs = [s for s in sigs if census.sig_args(s)["out_mode"] == K.OUT_F32_SLAB and census.sig_args(s)["split_k"] > 1 and
                census.sig_args(s)["gather"] is not None and census.sig_args(s)["gather"].mode == K.GATHER_CONV3X3 and
                (census.sig_args(s)["gather"].stride, census.sig_args(s)["gather"].ups) == (1, 0)]
    want = ("f16", "bf16")[i % 2]
    pick = [s for s in sigs if any(isinstance(v, tuple) and v and v[0] == "T" and v[1] == want for _, v in s[1])] or sigs
    return _strip_alias(max(pick, key=lambda s: (max(census.reach(s).values()) // _count(s), repr(s))))


def units_4g(sig, line=census.REACH_4G):
    """the smallest count that puts the largest 16-bit operand (the float slabs of the split-K output) one unit beyond `line` = 2^32 bytes
    (counts of elements: COUNT_4G)"""
    cnt, W = _win(sig[0])
    if cnt == "n":
        return COUNT_4G if line == census.REACH_4G else line // 2 + (1 << 12)
    r1, r2 = census.reach(_resized(sig, W)), census.reach(_resized(sig, 2 * W))
    per = max((r2[n] - r1[n]) // W for n in r1 if sig[0] == "gemm" or census.sig_args(sig)[n.split(".")[0]][1] in ("f16", "bf16"))
    return line // per + 1


class _Names:
    """positional arguments of a backend call by their names; what a runner's `_launch` passes"""

    def __init__(self, entry, fn):
        self.names, self.fn = [p.name for p in census._PARAMS[entry]], fn

    def __call__(self, *args):
        self.fn({n: v for n, v in zip(self.names, args) if isinstance(v, torch.Tensor)})


class _Window:
    """the backend a runner sees: pass 1 plants its inputs and stops it, pass 2 hands it the outputs of the real launch"""

    def __init__(self, entry, fn):
        setattr(self, entry, _Names(entry, fn))


def _unit_view(sig, name, t, units):
    """`t` with the unit as its leading dimension"""
    if _slices(sig, name) > 1:
        return t.view(_slices(sig, name), units, -1).transpose(0, 1)
    if sig[0] == "transpose" and name == "inp":
        return t.view(-1, units).t()
    return t.view(units, -1)


def window_layout(base, lines=(census.REACH_2G, census.REACH_4G), W=None, units=None):
    """(units per window, units of the launch, window signature, full signature, extents of both, element sizes, elements per unit, the
    windows' first units) -- host only"""
    entry = base[0]
    W = W or _win(entry)[1]
    U = units or max(units_4g(base, lines[1]), 4 * W)
    small, big = _resized(base, W), _resized(base, U)
    rw, r2w, rbig = census.reach(small), census.reach(_resized(base, 2 * W)), census.reach(big)
    esz = {n: census.DT_OF[census.Operands(small, "cpu").desc[n][1]].itemsize for n in rw}
    per = {n: (r2w[n] - rw[n]) // W // esz[n] for n in rw}                                   # elements per unit; 0: the same for every window
    assert all(rbig[n] == (per[n] * U * esz[n] if per[n] else rw[n]) or n in REDUCED.get(entry, ((), ()))[1] for n in rw), (rbig, per)
    starts = [0, U - W]
    for n in rw:
        for b in lines:
            if not per[n] or b >= rbig[n] or (entry == "transpose" and n == "inp"):       # (a unit of transpose's input is a column: every byte range holds all)
                continue
            k = _slices(base, n)
            at = (b // esz[n] % (U * per[n] // k)) // (per[n] // k)                          # the unit that holds byte b of this operand
            if any(s0 + (per[n] == 1) <= at < s0 + W for s0 in starts):                   # (a unit of one element: the line between two of them)
                continue
            s1 = min(max(at - W // 2, 0), U - W)
            for s0 in sorted(starts):                                                       # beside a window it would overlap, the line still inside
                if s0 < s1 + W and s1 < s0 + W:
                    s1 = min(s1, s0 - W) if at < s0 else max(s1, s0 + W)
            assert 0 <= s1 <= at < s1 + W <= U, (n, b, at, s1, starts)
            starts.append(s1)
    starts = sorted(starts)
    assert all(a + W <= b for a, b in zip(starts, starts[1:])), starts
    return W, U, small, big, rw, rbig, esz, per, starts


def run_windowed(be, dev, base, lines=(census.REACH_2G, census.REACH_4G), W=None, units=None):
    """-> ([(label, excess, index)] of every window through the entry's runner, the scan's findings, the windows' first units).
    `lines`, `W`: the byte offsets the windows straddle and the units per window -- smaller ones let the CPU tests run the machinery itself"""
    entry = base[0]
    W, U, small, big, rw, rbig, esz, per, starts = window_layout(base, lines, W, units)
    red_in, red_out = REDUCED.get(entry, (None, ()))
    full, is_out = {}, {}

    def window_sig(u0):
        return small if u0 == starts[-1] or not red_out else with_args(small, **{n: None for n in red_out})

    def plant(u0):
        def fn(t):
            for n, v in t.items():
                if n not in full:
                    numel = rbig[n] // esz[n]
                    buf = torch.zeros(numel + 2 * census.GUARD, dtype=v.dtype, device=dev)
                    buf[:census.GUARD] = census.GUARD_VALUE
                    buf[-census.GUARD:] = census.GUARD_VALUE
                    full[n] = buf
                    if is_out[n]:
                        for c0 in range(census.GUARD, census.GUARD + numel, 1 << 28):          # what the runner pre-fills its outputs with
                            buf[c0:min(c0 + (1 << 28), census.GUARD + numel)] = v.reshape(-1)[0]
                if is_out[n]:
                    continue
                pay = full[n][census.GUARD:-census.GUARD]
                if per[n]:
                    src = torch.zeros_like(v) if (n == red_in and u0 != starts[-1]) else v
                    _unit_view(base, n, pay, U)[u0:u0 + W].copy_(_unit_view(base, n, src.reshape(-1), W))
                else:
                    pay.copy_(v.reshape(-1))
            raise _Stop()
        return fn

    def hand_back(u0):
        def fn(t):
            for n, v in t.items():
                pay = full[n][census.GUARD:-census.GUARD]
                if is_out[n]:
                    flat = v.reshape(-1)
                    assert flat.data_ptr() == v.data_ptr()
                    if per[n]:
                        _unit_view(base, n, flat, W).copy_(_unit_view(base, n, pay, U)[u0:u0 + W])
                    elif pay.numel() == flat.numel():
                        flat.copy_(pay)
                elif n == red_in and u0 != starts[-1]:
                    v.zero_()
        return fn

    for u0 in starts:                                        # pass 1
        o = census.Operands(window_sig(u0), dev)
        try:
            orig_alloc = o.alloc

            def alloc(o=o, orig_alloc=orig_alloc):
                orig_alloc()
                is_out.update({n: d[2] for n, d in o.decls.items()})
                return o
            o.alloc = alloc
            census.RUNNERS[entry](_Window(entry, plant(u0)), o, census.sig_args(o.sig))
            raise AssertionError("the runner did not launch")
        except _Stop:
            pass
        del o
    views = {n: t[census.GUARD:-census.GUARD] for n, t in full.items()}
    kw = {k: census._rebuild(v, views, k) for k, v in big[1]}
    getattr(be, entry)(*kw.values())                         # the one real launch
    census._sync(dev)
    res = []
    for u0 in starts:                                        # pass 2
        o = census.Operands(window_sig(u0), dev)
        for label, excess, idx in census.RUNNERS[entry](_Window(entry, hand_back(u0)), o, census.sig_args(o.sig)):
            res.append((f"units {u0}..{u0 + W}: {label}", excess, idx))
        del o
    found = []
    for n, t in full.items():
        if not (bool((t[:census.GUARD] == census.GUARD_VALUE).all()) and bool((t[-census.GUARD:] == census.GUARD_VALUE).all())):
            found.append(f"{n}: written outside the operand")
        if is_out[n] and n != "scratch" and t.is_floating_point() and not (entry.startswith("gn_") and n in _GN_TABLES):      # (a workspace; fixed-point tables)
            pay = t[census.GUARD:-census.GUARD]
            for c0 in range(0, pay.numel(), 1 << 28):
                c = pay[c0:c0 + (1 << 28)]
                if not bool(torch.isfinite(c).all()):
                    i = int((~torch.isfinite(c)).nonzero()[0]) + c0
                    found.append(f"{n}: element {i} of {pay.numel()} is {float(c[i - c0])} after the launch (unit {i // max(per[n], 1)})")
                    break
    return res, found, starts


def whole_signature(entry):
    """`zero`, `check_finite`, `ema_lerp` at COUNT_4G elements"""
    if entry == "check_finite":              # (the step checks its gradients span by span: no census records this entry)
        return census.signature_of(entry, (torch.zeros(8), COUNT_4G, torch.zeros(K.OPT_STATE_ALLOC)), {})
    s = tiny_signatures(entry)[0]
    if entry == "zero":
        return with_args(s, t=census.sig_args(s)["t"][:4] + (COUNT_4G,))
    return with_args(s, n=COUNT_4G)


def run_whole(be, dev, entry):
    sig = whole_signature(entry)
    if entry != "check_finite":
        return census.run_case(be, sig, dev)
    o = census.Operands(sig, dev)                            # the runner's check with the non-finite value planted in the LAST element
    res = census._finite_check(be, o, "g", COUNT_4G, COUNT_4G - 1)
    bad = o.damaged_guards()
    return res + [("nothing written outside the operands", float("inf") if bad else 0.0, ())]


# ---- svdx_gemm_tn_gather at its span limit ------------------------------------------------------------------------------------------------
# The entry has no flat staging: ((R - 1) lda + N) 2 bytes of dY beyond census.TN_SPAN_MAX are refused (csrc/gemm_tn.hip).  lda >= N is a free
# pitch, so the limit is met at a small case of tests/conv_wgrad_checks.py: the largest admissible pitch is served and judged by that
# module's runner (float64 reference, its bound, sentinel bands), the next one (8 elements more) is refused.
GATHER_LIMIT_CASE, GATHER_LIMIT_MESSAGE = "3x3_s1_8x8_c320", "operands of 2 GiB and more are not supported"


def gather_limit():
    """(case, rows, N, the largest pitch of dY that svdx_gemm_tn_gather serves, the smallest it refuses)"""
    import conv_wgrad_checks as cw
    c = cw.BY_NAME[GATHER_LIMIT_CASE]
    R, N = cw.rows_of(c), c.cout_p
    ld = (census.TN_SPAN_MAX // 2 - N) // (R - 1) // ALIGN * ALIGN
    assert ((R - 1) * ld + N) * 2 <= census.TN_SPAN_MAX < ((R - 1) * (ld + ALIGN) + N) * 2
    return c, R, N, ld, ld + ALIGN


def run_gather_limit(be, dev, dt):
    """served one step below the limit (judged), refused at it: K.SvdxError that names the limit, the NaN prefill of every output untouched"""
    import conv_wgrad_checks as cw
    c, R, N, served, refused = gather_limit()
    sig = lambda ld: census.signature_of("gemm_tn_gather", (torch.zeros(8), torch.zeros(8), torch.zeros(8), R, N, ld, 9 * c.cin_p, cw.gather_of(c, c.cin_p, c.cin_p)), {})
    assert not census.gemm_kernel_taken(sig(served)).startswith("refused") and census.gemm_kernel_taken(sig(refused)).startswith("refused")
    worst = cw.run_case(be, dev, c, dt, 1, store=True, ld_dy=served)
    release(dev)
    x, dy, _, _, _ = cw.case_reference(c, dt)
    Kd = 9 * c.cin_p
    flats, dv = {}, {}
    flats["dy"], dv["dy"] = cw.pitched(dy, refused, dev)
    for name, t in (("x", x), ("slabs", torch.full((1, N, Kd), float("nan"))), ("cs", torch.full((1, N), float("nan")))):
        flats[name], dv[name] = cw.banded(t, dev)
    try:
        be.gemm_tn_gather(dv["dy"], dv["x"], dv["slabs"], R, N, refused, Kd, cw.gather_of(c, c.cin_p, c.cin_p), out_mode=K.OUT_F32_SLAB, split_k=1, a_colsum=dv["cs"])
    except K.SvdxError as e:
        assert GATHER_LIMIT_MESSAGE in str(e), str(e)
    else:
        raise AssertionError(f"svdx_gemm_tn_gather served a dY span of {((R - 1) * refused + N) * 2} bytes")
    census._sync(dev)
    assert bool(torch.isnan(dv["slabs"]).all()) and bool(torch.isnan(dv["cs"]).all()), "a refused launch wrote its outputs"
    cw.bands_intact(flats)
    del flats, dv
    release(dev)
    return worst


# ---- svdx_tsa_fwd at its limit ------------------------------------------------------------------------------------------------------------
TSA_SERVED, TSA_REFUSED = (1, 3, 372827), (1, 2, 559241)       # (B, T, HW) at C = 320: M 3C 2 = 2^31 - 128 bytes of q/k/v, and 1792 bytes beyond 2^31
TSA_LINES = (1 << 30, census.REACH_2G)                          # the windows: the first pixels, the last, and those across byte 2^30 of q/k/v


def tsa_signature(B, T, HW, C=K.TSA_MAX_C):
    base = [s for s in tiny_signatures("tsa_fwd") if census.sig_args(s)["n1"] is not None and census.sig_args(s)["x"][1] == "f16"][0]
    return _strip_alias(with_args(base, B=B, T=T, HW=HW, C=C, heads=C // 64, rv_ld=C, rv_rpg=B * T * HW, rv_mod=0))
