"""Shared checks of the GroupNorm affine gradients (svdx_gn_bwd_stats_affine, svdx_gn_bwd_blocks): the kernel cases, their float64
reference (autograd through F.group_norm (+ F.silu)), the per-channel error bound, and the runners the simulator
(tests/test_gn_affine.py) and the device (tests/test_gn_affine_gpu.py) both use.  The emulation of the entry is emul.EmuBackend's; the
step against the oracle is selection_checks.py's.  TEST INFRASTRUCTURE."""
from typing import NamedTuple

import torch
import torch.nn.functional as F

import census
import ref64
from census import _ratio, ulp_of
from conv_wgrad_checks import DT, banded, bands_intact
from kernel_checks import tol_for
from selection_checks import COS_BAR, gn_names
from svd_xtend_amd import kernels as K

G = 32


class Case(NamedTuple):
    n_s: int
    rows: int
    C: int

    @property
    def name(self):
        return f"{self.n_s}x{self.rows}x{self.C}"


CASES = [
    Case(3, 15, 64),        # fewer rows than rpi (32): idle worker rows
    Case(1, 1, 64),         # a single row
    Case(2, 70, 320),       # cg = 10: an 8-channel chunk straddles groups; 240 threads
    Case(1, 210, 64),       # clip-wide 3-D norm, several slabs of one sample
    Case(2, 129, 640),      # ragged last slab, rpi = 3
    Case(2, 40, 960),       # cg = 30
    Case(2, 33, 1280),      # rpi = 1
    Case(1, 9, 2560),       # the up-blocks' concat width, 320 threads
    Case(1, 520, 320),      # many partial rows of one sample
    # ADDED to the issue's nine: 129 partial rows -- more than 8 per reducing row group, which at the affine variant's coarser slabs
    # (1, 520, 320) with its 65 does not reach; few terms per channel, so that the significance guard still holds
    Case(129, 2, 320),
]
BY_NAME = {c.name: c for c in CASES}
# (silu, eps): 1e-5 the ResNet norms (with SiLU) and conv_norm_out, 1e-6 the transformer models' `norm` (no SiLU)
VARIANTS = [(0, 1e-5), (0, 1e-6), (1, 1e-5)]


def operands(c: Case, dt: torch.dtype, seed: int = 0):
    """x = 1.5 randn + 0.5, dy = randn (in `dt`), gamma = 1 + 0.3 randn, beta = 0.3 randn, and the values an accumulating launch finds
    in dgamma / dbeta"""
    g = torch.Generator().manual_seed(1009 * seed + 31 * c.n_s + 7 * c.rows + c.C)
    M = c.n_s * c.rows
    x = (1.5 * torch.randn(M, c.C, generator=g) + 0.5).to(dt)
    dy = torch.randn(M, c.C, generator=g).to(dt)
    gamma = 1 + 0.3 * torch.randn(c.C, generator=g)
    beta = 0.3 * torch.randn(c.C, generator=g)
    return x, dy, gamma, beta, torch.randn(c.C, generator=g), torch.randn(c.C, generator=g)


@torch.enable_grad()
def reference(c: Case, x, dy, gamma, beta, silu: int, eps: float):
    """float64.  dgamma / dbeta: autograd through F.group_norm (+ F.silu).  Per channel, for the bound: S_g = sum |dz| |xhat|, S_b =
    sum |dz|; cond = E[x^2] / var of the channel's group, the largest over the samples; amp_g = sum (|x| + |mean|) rstd (|dz| + 1/2 |dy|
    |gamma| |xhat| [silu]), amp_b the same without the first summand."""
    n_s, rows, C = c
    g64 = ref64.d(gamma).clone().requires_grad_(True)
    b64 = ref64.d(beta).clone().requires_grad_(True)
    y = F.group_norm(ref64.d(x).view(n_s, rows, C).permute(0, 2, 1), G, g64, b64, eps)
    if silu:
        y = F.silu(y)
    dg, db = torch.autograd.grad(y, (g64, b64), ref64.d(dy).view(n_s, rows, C).permute(0, 2, 1))
    xf = ref64.d(x).view(n_s, rows, G, C // G)
    mean = xf.mean((1, 3), keepdim=True)
    var = xf.var((1, 3), unbiased=False, keepdim=True)
    rstd = torch.rsqrt(var + eps)
    xhat = ((xf - mean) * rstd).reshape(n_s, rows, C)
    z = (xhat * ref64.d(gamma) + ref64.d(beta)).requires_grad_(True)
    (dz,) = torch.autograd.grad(F.silu(z) if silu else z * 1.0, z, ref64.d(dy).view(n_s, rows, C))
    dz, xhat = dz.detach(), xhat.detach()
    S_g, S_b = (dz.abs() * xhat.abs()).sum((0, 1)), dz.abs().sum((0, 1))
    cond = ((xf * xf).mean((1, 3)) / var.clamp(min=1e-300)[:, 0, :, 0]).amax(0)                 # [G]
    cond = cond.repeat_interleave(C // G)
    dxh = ((xf.abs() + mean.abs()) * rstd).reshape(n_s, rows, C)
    sil = 0.5 * ref64.d(dy).view(n_s, rows, C).abs() * ref64.d(gamma).abs() * xhat.abs() if silu else torch.zeros_like(dz)
    amp_g = (dxh * (dz.abs() + sil)).sum((0, 1))
    amp_b = (dxh * sil).sum((0, 1))
    return dict(dg=dg.detach(), db=db.detach(), S_g=S_g, S_b=S_b, cond=cond, amp_g=amp_g, amp_b=amp_b)


def bounds(c: Case, ref, c0_g=None, c0_b=None):
    """bound = 1/2 ulp_fp32(ref) + 2^-23 ((N + 36 + 2 cond) S + 4 amp), N = n_s * rows terms: N + 16 additions (worst-case summation over
    the terms, the LDS stage and the partial rows) + 20 + 2 cond roundings per term (the census' gn_bwd_apply count) + 4 amp for the
    cancellation inside xhat; an accumulating launch adds |c0| to S and one rounding.  -> (ref_g, bound_g, ref_b, bound_b)"""
    N = c.n_s * c.rows
    out = []
    for v, S, amp, c0 in ((ref["dg"], ref["S_g"], ref["amp_g"], c0_g), (ref["db"], ref["S_b"], ref["amp_b"], c0_b)):
        k = N + 36 + 2 * ref["cond"]
        if c0 is not None:
            v, S, k = v + ref64.d(c0), S + ref64.d(c0).abs(), k + 1
        out += [v, 0.5 * ulp_of(v, torch.float32) + 2.0 ** -23 * (k * S + 4 * amp)]
    return tuple(out)


def significant(ref, bound) -> float:
    """fraction of the reference elements that exceed 10 x their bound: zeros, or a dropped row, cannot pass then"""
    return float((ref.abs() > 10 * bound).double().mean())


_REF_CACHE = {}


def case_reference(c: Case, dt: torch.dtype, silu: int, eps: float):
    """operands, forward statistics (float64 sums, encoded), references: once per combination, shared, never modified"""
    key = (c, dt, silu, eps)
    if key not in _REF_CACHE:
        x, dy, gamma, beta, c0_g, c0_b = operands(c, dt)
        nst = K.GN_REPLICAS * c.n_s * G * K.GN_STAT_FLOATS
        stats = torch.zeros(nst)
        s0, s1 = ref64.gn_sums(x, c.n_s, c.rows, c.C, G)
        census._gn_encode(stats, c.n_s, G, c.rows * (c.C // G), 0, s0, s1)
        dx, b1, b2 = ref64.gn_bwd(dy, x, gamma, beta, c.n_s, c.rows, c.C, G, eps, silu)
        mag = ref64.gn_bwd_magnitudes(dy, x, gamma, beta, c.n_s, c.rows, c.C, G, eps, silu)
        _REF_CACHE[key] = dict(x=x, dy=dy, gamma=gamma, beta=beta, c0_g=c0_g, c0_b=c0_b, stats=stats, ref=reference(c, x, dy, gamma, beta, silu, eps),
                               dx=dx, bst=torch.stack([b1, b2], -1).view(-1, 2), mag=mag)
    return _REF_CACHE[key]


def run_case(be, dev, c: Case, dt: torch.dtype, silu: int, eps: float, verbose: bool = False):
    """svdx_gn_bwd_stats_affine of one case on `dev`: dgamma / dbeta per channel against the float64 reference (onto zeros and onto
    pre-existing values), deferred == immediate reduction and launch == launch bit for bit, the bstats it leaves judged as the census
    judges svdx_gn_bwd_stats, svdx_gn_bwd_apply fed with it inside the census' derived bound; every buffer between guard bands, the
    operands unchanged.  -> worst error / bound (dgamma, dbeta)"""
    R = case_reference(c, dt, silu, eps)
    n_s, rows, C = c
    ref = R["ref"]
    nst = R["stats"].numel()
    nblk = K.gn_bwd_blocks(n_s, rows, C, G)
    nan = float("nan")
    sync = (lambda: torch.cuda.synchronize()) if str(dev) != "cpu" else (lambda: None)
    worst = [0.0, 0.0]
    results = []
    for mode, c0 in (("zero", None), ("zero-deferred", None), ("zero-again", None), ("accumulate", (R["c0_g"], R["c0_b"]))):
        vg, bg, vb, bb = bounds(c, ref, *(c0 or (None, None)))
        sg, sb = significant(vg, bg), significant(vb, bb)
        if verbose:
            print(f"{c.name} {dt} silu={silu} eps={eps} {mode}: significant dgamma {sg:.3f} dbeta {sb:.3f}")
        assert sg >= 0.95 and sb >= 0.95, (c.name, dt, silu, mode, sg, sb)
        flats, dv = {}, {}
        for name, t in (("x", R["x"]), ("dy", R["dy"]), ("gamma", R["gamma"]), ("beta", R["beta"]), ("stats", R["stats"]),
                        ("bstats", torch.ones(nst)),                                   # not prezeroed: the launch clears what is there
                        ("partial", torch.full((nblk, 2 * C), nan)),
                        ("dgamma", torch.zeros(C) if c0 is None else c0[0]), ("dbeta", torch.zeros(C) if c0 is None else c0[1]),
                        ("dx", torch.full((n_s * rows, C), nan, dtype=dt))):
            flats[name], dv[name] = banded(t, dev)
        defer = mode == "zero-deferred"
        be.gn_bwd_stats_affine(dv["dy"], dv["x"], dv["stats"], dv["gamma"], dv["beta"], dv["bstats"], dv["dgamma"], dv["dbeta"], dv["partial"],
                               n_s, rows, C, G, eps, silu, prezeroed=0, defer_reduce=defer)
        if defer:
            sync()
            assert not dv["dgamma"].cpu().any() and not dv["dbeta"].cpu().any(), "a deferred launch touched the gradients"
            be.ln_param_reduce_batch([(dv["partial"], dv["dgamma"], dv["dbeta"], nblk, C)])
        be.gn_bwd_apply(dv["dy"], dv["x"], dv["stats"], dv["bstats"], dv["gamma"], dv["beta"], None, dv["dx"], n_s, rows, C, G, eps, silu)
        sync()
        got = {k: dv[k].cpu().clone() for k in ("dgamma", "dbeta", "partial", "bstats", "dx")}
        rg, rb = _ratio(got["dgamma"], vg, bg), _ratio(got["dbeta"], vb, bb)
        w = (float(rg.max()), float(rb.max()))
        if verbose:
            print(f"{c.name} {dt} silu={silu} eps={eps} {mode}: worst error / bound dgamma {w[0]:.3f} dbeta {w[1]:.3f}")
        assert w[0] <= 1.0 and w[1] <= 1.0, (c.name, dt, silu, eps, mode, w, int((rg > 1).sum()), int((rb > 1).sum()))
        worst = [max(worst[0], w[0]), max(worst[1], w[1])]
        assert bool(torch.isfinite(got["partial"]).all()), "a partial row was left unwritten"
        # the statistics for svdx_gn_bwd_apply: as the census judges svdx_gn_bwd_stats, and the dx they give inside its derived bound
        res = []
        census.judge_fixed(res, "bstats", census._gn_decoded(got["bstats"], n_s, G, rows * (C // G), 1).view(-1, 2), R["bst"], 2e-3)
        S, amp, cond = R["mag"]
        derived = 0.5 * ulp_of(R["dx"], dt) + 2.0 ** -23 * ((20 + 2 * cond) * S + 4 * amp)
        census.judge_rows(res, "dx", got["dx"], R["dx"], tol_for(dt), derived)
        assert res[0][1] <= 1.0 and res[1][1] <= 1.0, (c.name, dt, silu, eps, mode, res[:2])
        bands_intact(flats)
        for name in ("x", "dy", "gamma", "beta", "stats"):
            bits = torch.int32 if R[name].dtype == torch.float32 else torch.int16      # (the statistics are integers in a float buffer)
            assert torch.equal(dv[name].cpu().view(bits), R[name].view(bits)), f"{name} modified"
        results.append(got)
    z, zd, za = results[:3]
    for k in ("dgamma", "dbeta", "partial", "bstats", "dx"):
        bits = torch.int32 if z[k].dtype == torch.float32 else torch.int16
        assert torch.equal(z[k].view(bits), zd[k].view(bits)), (c.name, k, "deferred and immediate reduction differ")
        assert torch.equal(z[k].view(bits), za[k].view(bits)), (c.name, k, "two launches differ")
    return tuple(worst)


def sweep_case(be, dev, c: Case, dt: torch.dtype, verbose: bool = False):
    return [run_case(be, dev, c, dt, silu, eps, verbose=verbose) for silu, eps in VARIANTS]


# ---- one optimizer step of the tiny topology with trainable GroupNorm affines (selection_checks.py), against the CPU oracle -------------
TEMPORAL_NORM = ("temporal_transformer_block", "@norm")
ALL_THREE = ("temporal_transformer_block", "@conv", "@norm")
SELECTIONS = [TEMPORAL_NORM, "@norm", ALL_THREE, "conv_norm_out"]

# (calls, sha256 of the newline-joined entry names) of one Trainer.step of the tiny topology with the DEFAULT trainable set, recorded on
# the commit before the GroupNorm affines became trainable: the calls the emulation receives at ALL depths of emul.record, the 154 an
# emulation makes on itself included (80 svdx_small_linear and 64 svdx_outer_acc under their *_batch entries, 10 svdx_tattn_fwd under
# svdx_tsa_fwd).  The default set must keep issuing exactly these; the launches among them -- depth 0 -- are DEFAULT_LAUNCHES
PARENT_DEFAULT_LAUNCHES = (1595, "9de55de4aa1df7844284555f4b3413ee0e090e5288f95d01566524ecb678950e")
DEFAULT_LAUNCHES = 1441


def assert_step_parity(key, ref, got, bf16=False, emu=None):
    """e2e_checks.assert_parity + the selection itself + the cosine of EVERY GroupNorm tensor's gradient at the project's bar.
    emu: {name: gradient of the emulation's step} for the tensors listed in EMULATION_MISSES -- those are held to the same bar against
    the emulation instead (the precision of 16-bit saved activations, not the kernel's: see the summary of the pull request)."""
    import e2e_checks
    assert sorted(got["grads"]) == ref["names"], (key, set(got["grads"]) ^ set(ref["names"]))
    gn = set(gn_names(got["trainer"].model))
    norm = [n for n in ref["names"] if n in gn]
    assert norm and "conv_norm_out.weight" in norm
    low = []
    for n in norm:
        against = ref["grads"][n]
        if emu is not None and n in emu:
            against = emu[n]
        cval = e2e_checks.cosine(got["grads"][n], against)
        if cval < COS_BAR[bf16]:
            low.append((n, cval))
    assert not low, (key, low)
    r = e2e_checks.compare(ref, got)
    e2e_checks.assert_parity(key, r, bf16=bf16)
    return r
