"""The launch census of the passes AROUND the train step -- VAE encode / decode, the CLIP image path, the sampler's batch-2 UNet forward,
weight packing, the EMA update (tests/census.py: COND_CONFIGS) -- on the CPU (`-m "not gpu"`): that the geometries the GPU test runs
reach every dispatch class of the real workload, that every entry has a runner, tiny configurations of every pass through the emulation
and through the HIP sources on the simulator, and the new runners against planted faults."""
import collections
import os
import sys

import pytest
import torch
import torch.nn.functional as F

import census
import emul
from svd_xtend_amd import kernels as K

FULL = os.environ.get("SVDX_SIM_FULL") == "1"

# real-geometry dispatch classes that NO geometry run on the GPU reaches: (pass, class) -> reason.  Empty: the classes the small
# geometries miss (the tiles `ops._choose_cfg_v4` picks from M >= 30000 / M >= 100000 rows) run at their real signatures.
UNCOVERED = {}


def _run_all(be, sigs):
    bad, worst = [], collections.defaultdict(float)
    for sig in sigs:
        for label, excess, idx in census.run_case(be, sig):
            fam = census.family(sig, label)
            worst[fam] = max(worst[fam], excess)
            if not excess <= 1.0:
                bad.append(f"excess {excess:.3g} at {idx}: {label}: {census.sig_str(sig)}")
    return bad, worst


@pytest.mark.parametrize("what", sorted(census.COND_REAL))
def test_gpu_geometries_reach_every_dispatch_class_of_the_real_workload(what):
    real = {census.dispatch_class(s): s for s in census.census_cond(census.COND_REAL[what])}
    parts = census.cond_gpu_signatures(what)
    run = {census.dispatch_class(s) for c in parts.values() for s in c}
    missing = [k for k in real if k not in run and (what, k) not in UNCOVERED]
    small = {census.dispatch_class(s) for n, c in parts.items() if n in census.COND_GPU[what] for s in c}
    print(f"{what}: {len(real)} dispatch classes at the real geometry, {len(real.keys() & small)} of them reached by the small geometries "
          f"{census.COND_GPU[what]}, {len(real.keys() - small)} run at their real signatures; "
          f"{sum(len(c) for c in parts.values())} signatures on the GPU")
    assert not missing, "\n".join(census.sig_str(real[k], 500) for k in missing)
    assert all(k in real for w, k in UNCOVERED if w == what), "UNCOVERED names a class the real geometry does not have"


def test_the_real_geometries_are_the_workload():
    enc = census.census_cond("encode_real")
    assert {census.sig_args(s)["M"] for s in enc if s[0] == "gemm"} >= {14 * 320 * 512, 14 * 40 * 64}
    smp = census.census_cond("sampler_real")
    assert sum(smp.values()) >= 600 and any(s[0] == "gemm" and census.sig_args(s)["M"] == 2 * 14 * 40 * 64 for s in smp)
    step = census.census("c2")
    assert sum(1 for s in smp if s not in step) >= 140, "the batch-2 forward launches what the batch-1 step launches"
    clip = census.census_cond("clip_real")
    assert any(s[0] == "attn_small_fwd" and (census.sig_args(s)["S"], census.sig_args(s)["d"]) == (257, 80) for s in clip)
    nts = sorted(census.sig_args(s)["taps"][4] for s in clip if s[0] == "blur_axis")
    from svd_xtend_amd.clip import _gaussian_taps
    assert nts == sorted([_gaussian_taps(512 / 224, "cpu").numel(), _gaussian_taps(320 / 224, "cpu").numel()]), nts
    # the conditioner-only tile rule: variants 18 and 27 with gathers and fused GroupNorm statistics are in what the GPU runs
    seen = collections.defaultdict(set)
    for what in ("vae_encode", "vae_decode"):
        for c in census.cond_gpu_signatures(what).values():
            for s in c:
                if s[0] == "gemm":
                    k = dict((x for x in census.dispatch_class(s)[1:] if isinstance(x, tuple)))
                    seen[k["tile"]].add((k["gather"][0] if k["gather"] else 0, k["gn"]))
    assert {(1, True), (4, True), (3, False)} <= seen[18] and {(1, True), (4, True)} <= seen[27], dict(seen)
    assert any(s[0] == "geglu_fwd" for s in census.census_cond("sampler_2x3x16x24"))
    assert max(census.sig_args(s)["nsplit"] for s in census.census_cond("sampler_2x3x16x24") if s[0] == "gemm_finalize") >= 16


@pytest.mark.parametrize("name", sorted(census.COND_CONFIGS))
def test_every_entry_of_the_pass_has_a_runner_or_is_allow_listed(name):
    launches, distinct, checked, allowed, missing = census.coverage(census.census_cond(name))
    print(f"{name}: {launches} launches, {distinct} distinct signatures, {checked} checked, allow-listed launches {dict(allowed)}")
    assert not missing, f"{name}: entries with neither a runner nor an allow-list entry: {missing}"
    assert sum(allowed.values()) <= census.ALLOW_FRACTION * launches, (dict(allowed), launches)


def test_memsets_are_checked_not_allowed():
    assert "zero" not in census.ALLOW_LIST and "zero_spans" not in census.ALLOW_LIST
    assert {"zero", "zero_spans"} <= set(census.RUNNERS)
    for entry in ("act_rows", "attn_small_fwd", "bicubic_affine", "blur_axis", "patch_rows", "softmax_rows", "transpose", "rows_to_nchw",
                  "cast_from_f32", "cast_transpose_from_f32", "geglu_fwd", "ema_lerp"):
        assert entry in census.RUNNERS, entry


# a launch of the unfused GEGLU and a span memset at sizes the CPU carries (the tiny passes launch neither)
EXTRA_TINY = [
    ("geglu_fwd", dict(pre=("T", "f16", None, None, None), out=("T", "f16", None, None, None), M=37, F=64)),
    ("geglu_fwd", dict(pre=("T", "bf16", None, None, None), out=("T", "bf16", None, None, None), M=5, F=192)),
    ("zero_spans", dict(base=("T", "f32", None, None, None),
                        spans=("T", "i32", None, torch.tensor([[8, 64], [100, 4], [256, 1024]], dtype=torch.int32).numpy().tobytes(), None), n_spans=3)),
]


def _extra_sigs():
    return [(e, tuple((p.name, kw[p.name]) for p in census._PARAMS[e])) for e, kw in EXTRA_TINY]


@pytest.mark.parametrize("name", census.COND_TINY)
def test_emulation_meets_float64_reference_at_every_tiny_signature(name):
    sigs = [s for s in census.census_cond(name) if s[0] in census.RUNNERS]
    if name == "tiny_sampler":
        sigs += _extra_sigs()
    bad, worst = _run_all(emul.EmuBackend(), sigs)
    for fam, w in sorted(worst.items()):
        print(f"{w:8.3f}  {fam}")
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("name", census.COND_TINY)
def test_hip_sources_meet_float64_reference_on_simulator(name):
    """the HIP sources themselves (tests/sim): one signature per (entry, feature combination) of the tiny pass; all under SVDX_SIM_FULL=1"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "sim"))
    from backend import SimBackend
    sigs = [s for s in census.census_cond(name) if s[0] in census.RUNNERS]
    if name == "tiny_sampler":
        sigs += _extra_sigs()
    if not FULL:
        first = {}
        for s in sorted(sigs, key=lambda s: (_cost(s), repr(s))):
            first.setdefault(census.feature_key(s), s)
        sigs = list(first.values())
    print(f"{name}: {len(sigs)} signatures on the simulator")
    bad, worst = _run_all(SimBackend(), sigs)
    for fam, w in sorted(worst.items()):
        print(f"{w:8.3f}  {fam}")
    assert not bad, "\n".join(bad[:20])


def _cost(sig):
    a = census.sig_args(sig)
    n = 1
    for k in ("M", "N", "K", "n", "rows", "C", "R", "Ccols"):
        if isinstance(a.get(k), int):
            n *= max(a[k], 1)
    return n


def test_exhaustive_activation_check_on_the_emulation():
    """all 65536 bit patterns of both 16-bit types through both activations (the GPU test does the same on the kernel)"""
    for dt in (torch.float16, torch.bfloat16):
        for act in (0, 1):
            res = census.run_act_exhaustive(emul.EmuBackend(), dt, act, "cpu")
            for label, excess, idx in res:
                print(f"{dt} act {act}: {excess:8.3f}  {label}")
                assert excess <= 1.0, (dt, act, label, excess, idx)


# ---- planted faults --------------------------------------------------------------------------------------------------------------------
def _toward_zero(v32, dt):
    h = v32.to(dt)
    away = h.float().abs() > v32.abs()
    return torch.where(away, (h.view(torch.int16) - 1).view(dt), h)


class Faulty(emul.EmuBackend):
    def __init__(self, fault):
        self.fault = fault

    def act_rows(self, inp, out, n, act=0):
        assert self.fault == "act_rows: truncating cast"
        x = emul.V1(inp, n).float()
        emul.V1(out, n).copy_(_toward_zero(emul.gelu(x) if act == 0 else x * torch.sigmoid(1.702 * x), out.dtype))

    def blur_axis(self, inp, out, planes, H, W, taps, axis):
        assert self.fault == "blur_axis: reflect padding off by one"
        x = emul.V1(inp, planes * H * W).view(planes, 1, H, W)
        half = (taps.numel() - 1) // 2
        L = W if axis == 0 else H
        i = torch.arange(-half, L + half)
        i = torch.where(i < 0, -i - 1, i)                       # the edge sample repeated: -1 -> 0 where reflect has -1 -> 1
        i = torch.where(i >= L, 2 * L - 1 - i, i)
        xp = x[..., i] if axis == 0 else x[:, :, i]
        y = F.conv2d(xp, taps.view(1, 1, 1, -1) if axis == 0 else taps.view(1, 1, -1, 1))
        emul.V1(out, planes * H * W).copy_(y.reshape(-1))

    def bicubic_affine(self, inp, out, n_img, C, H, W, ho, wo, scale, shift):
        assert self.fault == "bicubic_affine: without align_corners"
        x = emul.V1(inp, n_img * C * H * W).view(n_img, C, H, W)
        y = F.interpolate(x, size=(ho, wo), mode="bicubic", align_corners=False)
        emul.V1(out, n_img * C * ho * wo).copy_((y * scale.view(1, C, 1, 1) + shift.view(1, C, 1, 1)).reshape(-1))

    def softmax_rows(self, inp, out, rows, cols, cols_out, ld_in, ld_out, scale):
        assert self.fault == "softmax_rows: padding columns not zero"
        super().softmax_rows(inp, out, rows, cols, cols_out, ld_in, ld_out, scale)
        emul.V(out, rows, cols_out, ld_out)[:, cols:] = 2.0 ** -14

    def attn_small_fwd(self, qkv, out, n_img, S, heads, d, dp, ld, ld_o, scale):
        assert self.fault == "attn_small_fwd: last key dropped when S % 4 != 0" and S % 4
        x = emul.V(qkv, n_img * S, 3 * heads * dp, ld).float().view(n_img, S, 3, heads, dp)
        q, k, v = (x[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        p = torch.softmax((q[..., :d] @ k[:, :, :S - 1, :d].transpose(-1, -2)) * scale, -1)
        o = torch.zeros(n_img, heads, S, dp)
        o[..., :d] = p @ v[:, :, :S - 1, :d]
        emul.V(out, n_img * S, heads * dp, ld_o).copy_(o.permute(0, 2, 1, 3).reshape(n_img * S, heads * dp).to(out.dtype))

    def transpose(self, inp, ld_in, out, ld_out, rows, cols):
        assert self.fault == "transpose: tail columns not zero-filled" and ld_out > rows
        emul.V(out, cols, ld_out, ld_out)[:, :rows] = emul.V(inp, rows, cols, ld_in).t()

    def patch_rows(self, inp, out, n_img, C, H, W, kh, kw, stride, pad, ho, wo, ldk, mul=1.0):
        assert self.fault == "patch_rows: mul ignored" and mul != 1.0
        super().patch_rows(inp, out, n_img, C, H, W, kh, kw, stride, pad, ho, wo, ldk, 1.0)

    def gemm(self, A, B, C, M, N, Kd, lda, ldb, ldc, bias=None, rowvec=None, rv_ld=0, rv_rpg=0, rv_mod=0, *rest, **kw):
        assert self.fault == "gemm: row-vector groups as if B = 1" and rowvec is not None and not rv_mod and M > rv_rpg
        super().gemm(A, B, C, M, N, Kd, lda, ldb, ldc, bias, rowvec, rv_ld, M, 0, *rest, **kw)


def _with(sig, **changes):
    return (sig[0], tuple((k, changes.get(k, v)) for k, v in sig[1]))


def _pick(name, entry, pred=lambda a: True):
    sigs = sorted((s for s in census.census_cond(name) if s[0] == entry and pred(census.sig_args(s))), key=lambda s: (_cost(s), repr(s)))
    assert sigs, f"no such {entry} signature in {name}"
    return sigs[0]


FAULTS = {
    "act_rows: truncating cast": lambda: _pick("tiny_clip", "act_rows"),
    "blur_axis: reflect padding off by one": lambda: _pick("tiny_clip", "blur_axis", lambda a: a["axis"] == 0),
    "bicubic_affine: without align_corners": lambda: _pick("tiny_clip", "bicubic_affine"),
    "softmax_rows: padding columns not zero": lambda: _pick("encode_1x40x24", "softmax_rows", lambda a: a["cols_out"] > a["cols"]),
    "attn_small_fwd: last key dropped when S % 4 != 0": lambda: _pick("tiny_clip", "attn_small_fwd", lambda a: a["S"] % 4),
    "transpose: tail columns not zero-filled": lambda: _pick("encode_1x40x24", "transpose", lambda a: a["ld_out"] > a["rows"]),
    "patch_rows: mul ignored": lambda: _with(_pick("tiny_encode", "patch_rows"), mul=0.5),
    "gemm: row-vector groups as if B = 1": lambda: _pick("tiny_sampler", "gemm", lambda a: a["rowvec"] is not None and not a["rv_mod"] and a["M"] == 2 * a["rv_rpg"]
                                                     and a["out_mode"] == K.OUT_ACT and a["epilogue"] == K.EPI_NONE),
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_checker_notices_planted_fault(fault):
    """numeric perturbations of a correct CPU result (nothing runs on a GPU): the clean emulation passes, the faulty one is flagged"""
    sig = FAULTS[fault]()
    clean = census.run_case(emul.EmuBackend(), sig)
    assert all(e <= 1.0 for _, e, _ in clean), clean
    res = census.run_case(Faulty(fault), sig)
    flagged = [(label, e) for label, e, _ in res if not e <= 1.0]
    print(f"{fault}: {census.sig_str(sig, 200)}")
    for label, e in flagged:
        print(f"    flagged: {label}: excess {e:.3g}")
    assert flagged, f"the checker let '{fault}' through: {res}"
    if "padding columns" in fault:
        assert any("padding columns are zero" in label for label, _ in flagged), flagged
