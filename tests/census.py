"""Launch census of one optimizer step, and the per-launch check that goes with it.

`census(name)` runs the second optimizer step of a configuration on a backend that performs no arithmetic and only records, per call,
a hashable SIGNATURE of the launch (the host code never reads a value back from the device inside a step, so the whole step runs on
it).  `run_case(backend, signature)` rebuilds seeded operands from the signature alone, launches the entry on the backend under test
and judges every output against the float64 reference of tests/ref64.py with the error model below.  `census_cond(name)` records the
passes around the step the same way (COND_CONFIGS: VAE encode / decode, the CLIP image path, the sampler's batch-2 forward, packing, EMA).
`census(name)` also records the geometries beyond the two benchmarked (GEOM_EDGE, GEOM_GRID, GEOM_TINY); `geom_gpu_signatures()` is what
the GPU runs of them: every signature of the edge geometries and one per dispatch class of the grid that nothing else reaches.
`reach(signature)` is the extent in bytes of every tensor argument, `gemm_kernel_taken` the entry points' own conditions on it.

Signature = (entry, ((argument name, value), ...)) in the order of `kernels.HipBackend`'s method.  A value is an int / float / bool / None,
a `kernels.Gather`, a tuple of per-job tuples for the `*_batch` entries, or -- for a tensor -- ("T", dtype name, alias, table, n) where
`alias` is None or (name of the first argument that shares the tensor's storage, offset to it in elements), `table` is the content of
an int32 table (span / tile tables: they are launch geometry, not data), else None, and `n` is the element count where the binding derives
an argument from it (the bias-gradient outputs), else None.

Error model (derived, not measured):

* single-rounding outputs: per element  |got - ref| <= 1/2 ulp_out(ref) + (K_acc + E) 2^-23 S.  ulp_out is the spacing of the output
  type at the reference (subnormal spacing as floor): one round-to-nearest into the output type.  S is the sum of the magnitudes of all
  accumulated terms, K_acc their number, E the epilogue terms: whatever the order of summation or the matrix unit's internal rounding,
  every partial sum is bounded by S and every accumulated term costs at most one fp32 rounding of a value <= S.
* rounding mode: over the elements with |ref| >= 0.25 rms(ref) (a selection that depends on the reference only), when there are at least
  1e5 of them, mean((got - ref)/ulp) and mean((|got| - |ref|)/ulp) lie within +-0.05 (round-to-nearest: 0 +- 0.289/sqrt(n); truncation:
  -0.5 in the second; rounding toward an infinity: +-0.5 in the first).
* multi-stage outputs: `tol_for` with the multiplier tests/kernel_checks.py uses for the family, per ROW with the row's own maximum in
  the denominator; each stage is judged from what the launch itself stored for the previous one.  The spatial attention backward adds
  its cancellation term after that bar (`_attn_bwd`): D comes from the stored, rounded o.
"""
import collections
import contextlib
import hashlib
import inspect
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from svd_xtend_amd import kernels as K  # noqa: E402
import emul  # noqa: E402  (the FORMAT of the fixed-point GroupNorm statistics buffers: gn_view / gn_fixed_scales)
import ref64  # noqa: E402
from kernel_checks import tol_for  # noqa: E402  (the project's bar for the multi-stage families)

# entries that launch nothing of their own: launch plans, clocks.  (The memsets `zero` / `zero_spans` have runners: the bytes are zero and
# nothing beside them is touched; so have the finite checks -- the flag stays down on finite floats and one planted value raises it -- and
# the loss-scale state machine `optim_prep`, against the float64 restatement of tests/overflow_checks.py.)
ALLOW_LIST = ("plan_begin", "plan_end", "stamp")
ALLOW_FRACTION = 0.02

_PARAMS = {n: list(inspect.signature(f).parameters.values())[1:] for n, f in inspect.getmembers(K.HipBackend, inspect.isfunction)
           if not n.startswith("_")}
_DT = {torch.float16: "f16", torch.bfloat16: "bf16", torch.float32: "f32", torch.float64: "f64", torch.int32: "i32", torch.int64: "i64",
       torch.uint8: "u8"}
DT_OF = {v: k for k, v in _DT.items()}
TABLE_MAX = 1 << 22            # int32 tables up to this many entries travel in the signature (as bytes)


class Recorder:
    """The method set of kernels.HipBackend; every call is counted under its signature and does nothing else."""

    def __init__(self):
        self.counts = collections.Counter()
        self.on = True
        self.n_calls = 0
        self.launch_log = None
        for name in _PARAMS:
            if name not in ("last_error", "wall_clock_khz"):
                setattr(self, name, self._make(name))

    def _make(self, name):
        def call(*a, **kw):
            self.n_calls += 1
            if self.on:
                self.counts[signature_of(name, a, kw)] += 1
            if name == "plan_end":
                raise K.SvdxError("the recording backend keeps no launch plan")
        return call

    def wall_clock_khz(self):
        return 100000

    def last_error(self):
        return ""


def _enc_tensor(t, seen, name):
    key = t.untyped_storage().data_ptr() if t.device.type != "meta" else id(t.untyped_storage())
    alias = None
    if key in seen:
        alias = (seen[key][0], t.storage_offset() - seen[key][1])
    else:
        seen[key] = (name, t.storage_offset())
    table = None
    if t.dtype == torch.int32 and t.numel() <= TABLE_MAX and t.device.type != "meta":
        table = t.detach().cpu().contiguous().numpy().tobytes()
    n = t.numel() if name.endswith("colsum_out") or (name.startswith("jobs.") and name.endswith(".6")) else None     # a size the binding derives
    return ("T", _DT[t.dtype], alias, table, n)


def _enc(v, seen, name):
    if isinstance(v, torch.Tensor):
        return _enc_tensor(v, seen, name)
    if isinstance(v, (bool, int, float, str, K.Gather)) or v is None:
        return v
    if isinstance(v, torch.dtype):
        return ("dtype", _DT[v])
    if isinstance(v, (tuple, list)):
        return tuple(_enc(x, seen, f"{name}.{i}") for i, x in enumerate(v))
    raise TypeError(f"{name}: {type(v)}")


_SIZED = {"zero": "t", "blur_axis": "taps"}        # entry -> the tensor argument whose element count the binding passes on (bytes / taps)


def signature_of(entry, args, kwargs):
    params = _PARAMS[entry]
    vals = {p.name: p.default for p in params}
    for p, a in zip(params, args):
        vals[p.name] = a
    vals.update(kwargs)
    seen = {}
    kv = tuple((p.name, _enc(vals[p.name], seen, p.name)) for p in params)
    if entry in _SIZED:
        kv = tuple((k, v[:4] + (vals[k].numel(),)) if k == _SIZED[entry] else (k, v) for k, v in kv)
    return (entry, kv)


def sig_args(sig):
    return dict(sig[1])


def sig_seed(sig):
    return int.from_bytes(hashlib.sha256(repr(sig).encode()).digest()[:6], "little")


def sig_str(sig, width=400):
    entry, kv = sig

    def short(v):
        if isinstance(v, tuple) and v and v[0] == "T":
            return v[1] + (f"@{v[2][0]}{v[2][1]:+d}" if v[2] else "") + (f"[table {len(v[3]) // 4}]" if v[3] is not None else "")
        if isinstance(v, tuple):
            return "(" + ",".join(short(x) for x in v[:6]) + (",..." if len(v) > 6 else "") + ")"
        if isinstance(v, K.Gather):
            return "Gather(" + ",".join(f"{k}={x}" for k, x in vars(v).items() if x) + ")"
        return repr(v)
    s = entry + "(" + ", ".join(f"{k}={short(v)}" for k, v in kv if v is not None) + ")"
    return s if len(s) <= width else s[:width] + "..."


# ---- configurations -------------------------------------------------------------------------------------------------------------------
# name -> (topology, (B, T, h, w), activation dtype, LoRA rank, Trainer keywords)
CONFIGS = {
    "tiny_fp16": ("tiny", (1, 3, 16, 16), torch.float16, 0, {}),
    "tiny_bf16": ("tiny", (1, 3, 16, 16), torch.bfloat16, 0, {}),
    "c2": ("svd", (1, 14, 40, 64), torch.float16, 0, {}),
    "c2_clip": ("svd", (1, 14, 40, 64), torch.float16, 0, dict(max_grad_norm=1.0)),
    "c5": ("svd", (1, 14, 40, 64), torch.bfloat16, 64, {}),
    "c5_ref": ("svd", (1, 14, 40, 64), torch.bfloat16, 64, dict(lora_param_dtype="reference")),
    "c4": ("svd", (1, 25, 72, 128), torch.float16, 0, dict(grad_accum=2)),
}
# ---- geometries beyond the two benchmarked (tests/test_census_geom.py, tests/test_census_geom_gpu.py) -----------------------------------------
# The model takes any latent height / width that are multiples of 8, any frame count and any batch size; which launches a geometry causes
# is decided by host code (ops._choose_cfg_v4, choose_split, gn_tile_ok, fused / unfused GEGLU, tsa_fwd / tattn_fwd).
# GEOM_EDGE: real topology, every distinct signature runs on the GPU.
GEOM_EDGE = {
    "e_1x1x8x8": ("svd", (1, 1, 8, 8), torch.float16, 0, {}),           # S = 64, 16, 4, 1; HW = 1; T = 1; 1x1 and 2x2 convolutions
    "e_3x5x8x24": ("svd", (3, 5, 8, 24), torch.bfloat16, 0, {}),        # B = 3; S = 192 .. 3; row-vector groups in tsa_fwd
    "e_1x14x24x40": ("svd", (1, 14, 24, 40), torch.float16, 0, {}),     # S = 960, 240, 60, 15: the deepest level is 3 x 5
    "e_2x16x16x8": ("svd", (2, 16, 16, 8), torch.bfloat16, 64, {}),     # T = 16, the fused op's limit; B = 2; dual operands at small M
    "e_1x17x16x24": ("svd", (1, 17, 16, 24), torch.float16, 0, {}),     # the first T beyond tsa_fwd
    "e_2x14x40x64": ("svd", (2, 14, 40, 64), torch.float16, 0, {}),     # batch 2 at the benchmark geometry (run: what c2 does not launch)
}
GEOM_EDGE_MINUS = {"e_2x14x40x64": "c2"}          # edge geometry -> the configuration whose signatures need not run again


def geom_refused(B, h, w, levels=4):
    """whether the model refuses the geometry: with B > 1 every level's pixel count must be a multiple of B (unet.forward_rows)"""
    return any(((h >> i) * (w >> i)) % B for i in range(levels))


def _grid():
    out = collections.OrderedDict()
    known = {(c[1], c[2], c[3]): n for n, c in list(CONFIGS.items()) + list(GEOM_EDGE.items()) if c[0] == "svd" and not c[4]}
    for dt, r, Ts, sizes in ((torch.float16, 0, (1, 14, 16, 17, 25), ((8, 8), (24, 40), (32, 32), (40, 64), (72, 128))),
                             (torch.bfloat16, 64, (1, 25), ((8, 8), (24, 40), (72, 128)))):
        for B in (1, 2):
            for T in Ts:
                for h, w in sizes:
                    if geom_refused(B, h, w):
                        continue
                    name = known.get(((B, T, h, w), dt, r), f"g_{B}x{T}x{h}x{w}_{'lora' if r else 'full'}")
                    out[name] = ("svd", (B, T, h, w), dt, r, {})
    return out


# GEOM_GRID: recorded host-only; a geometry another table already records goes under that table's name (one recording).  The grid
# SAMPLES an unbounded domain: a geometry outside it may reach a dispatch class nothing runs.  (How far an operand reaches in memory is
# part of the class -- `reach_key` -- and pinned beyond the grid by tests/reach_checks.py: every kernel change and refusal at 2 GiB,
# addressing up to 4 GiB plus one row.)
GEOM_GRID = _grid()
# the tiny topology at the edge geometries it admits: the emulation and the simulator on the CPU
GEOM_TINY = {
    "t_1x1x8x8": ("tiny", (1, 1, 8, 8), torch.float16, 0, {}),          # 1 x 1 deepest level, S = 1, T = 1
    "t_3x5x8x24": ("tiny", (3, 5, 8, 24), torch.bfloat16, 0, {}),       # B = 3, deepest level 1 x 3
    "t_1x2x24x40": ("tiny", (1, 2, 24, 40), torch.float16, 0, {}),      # deepest level 3 x 5: S = 960 .. 15
    "t_2x16x16x8": ("tiny", (2, 16, 16, 8), torch.bfloat16, 64, {}),    # T = 16, B = 2, LoRA
    "t_1x17x8x16": ("tiny", (1, 17, 8, 16), torch.float16, 0, {}),      # the first T beyond tsa_fwd
    "t_2x16x8x16": ("tiny", (2, 16, 8, 16), torch.float16, 0, {}),      # tsa_fwd at its limit T = 16 with the row vector grouped by B = 2
}
# GEOM_REACH: recorded host-only and never run as a whole.  Batch 4 of config 4 puts the widest activations (M = 921600 rows of 2560
# columns) beyond 2^32 bytes: its census names the entries that get a 4 GiB case of their own (tests/reach_checks.py) and is checked for
# launches the library would refuse (tests/test_census_geom.py).
GEOM_REACH = {"r_4x25x72x128_full": ("svd", (4, 25, 72, 128), torch.float16, 0, {})}
ALL_CONFIGS = dict(CONFIGS)
for _t in (GEOM_EDGE, GEOM_GRID, GEOM_TINY, GEOM_REACH):
    ALL_CONFIGS.update(_t)
_CACHE = {}


@contextlib.contextmanager
def _backend(be):
    prev = K._backend
    K._set_backend_for_tests(be)
    try:
        yield be
    finally:
        K._set_backend_for_tests(prev)


def census(name):
    """Counter[signature] of the SECOND optimizer step of configuration `name` (packing and caches are behind it, as in
    tools/launch_audit.py), with ops.Runtime as bench.py / GraphedStep run the step: its defaults, GEMM variant 4.  Host only: the
    model is built without weight initialisation (no value is ever read) and no kernel runs."""
    if name in _CACHE:
        return _CACHE[name]
    from oracle.unet import SVD_CONFIG, TINY_CONFIG, no_default_init
    from svd_xtend_amd.train import Trainer
    from svd_xtend_amd.unet import UNetSpatioTemporalConditionModel
    topo, (B, T, h, w), dt, lora_r, kw = ALL_CONFIGS[name]
    cfg = dict(TINY_CONFIG if topo == "tiny" else SVD_CONFIG)
    rec = Recorder()
    rec.on = False
    with _backend(rec), torch.no_grad():
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
        cross = cfg["cross_attention_dim"]
        batch = dict(unet_in=torch.empty(B, T, 8, h, w), timesteps=torch.ones(B), ehs=torch.empty(B, 1, cross),
                     added_time_ids=torch.ones(B, 3), noisy_latents=torch.empty(B, T, 4, h, w), target=torch.empty(B, T, 4, h, w),
                     sigmas=torch.ones(B))
        batches = [batch] * tr.grad_accum
        tr.step(batches)
        rec.on = True
        tr.step(batches)
    _CACHE[name] = rec.counts
    return rec.counts


# ---- the passes around the step ---------------------------------------------------------------------------------------------------------
# name -> (pass, geometry, model configuration: "real" = the SVD checkpoint's, "small" = the small configurations of tests/test_vae.py /
# tests/test_clip.py and the tiny UNet).  Recorded as the step is: host only, models built without weight initialisation, the recorder
# switched on for the pass itself.  Activation type: float16, what `prepare()` defaults to and the validation path runs.
VAE_SMALL = dict(in_channels=3, latent_channels=4, block_out_channels=(64, 128, 128, 128), layers_per_block=1, scaling_factor=0.18215)
CLIP_SMALL = dict(hidden_size=320, intermediate_size=640, projection_dim=64, num_hidden_layers=2, num_attention_heads=4, image_size=56,
                  patch_size=14, hidden_act="gelu")
CLIP_LAYERS = 2                    # of ViT-H's 32: every layer launches the same signatures (census_cond asserts it on the real tower)
COND_CONFIGS = {
    # the real workload's geometries (host only: the dispatch classes the GPU geometries below must cover)
    "encode_real": ("vae_encode", (14, 320, 512), "real"),
    "decode_real": ("vae_decode", (1, 14, 40, 64), "real"),
    "sampler_real": ("sampler_fwd", (2, 14, 40, 64), "real"),
    "clip_real": ("clip_image", (1, 320, 512), "real"),
    # what runs on the GPU
    "encode_3x320x512": ("vae_encode", (3, 320, 512), "real"),
    "encode_2x64x96": ("vae_encode", (2, 64, 96), "real"),
    "encode_1x40x24": ("vae_encode", (1, 40, 24), "real"),          # 15 tokens: the padded reduction of the attention's second GEMM
    "decode_1x4x40x64": ("vae_decode", (1, 4, 40, 64), "real"),
    "decode_1x4x16x24": ("vae_decode", (1, 4, 16, 24), "real"),
    "decode_2x2x5x3": ("vae_decode", (2, 2, 5, 3), "real"),
    "sampler_2x14x40x64": ("sampler_fwd", (2, 14, 40, 64), "real"),
    "sampler_2x3x16x24": ("sampler_fwd", (2, 3, 16, 24), "real"),
    "clip_1x320x512": ("clip_image", (1, 320, 512), "real"),
    "clip_small_ragged": ("clip_image", (2, 40, 72), "small"),        # tests/test_clip.py's small tower: 17 tokens, heads of 80
    "clip_small_quick_gelu": ("clip_image", (1, 64, 56), "small_quick_gelu"),
    "pack": ("pack", None, "real"),
    "ema": ("ema", None, "real"),
    # tiny: the emulation and the simulator on the CPU
    "tiny_encode": ("vae_encode", (2, 16, 24), "small"),
    "tiny_decode": ("vae_decode", (1, 2, 2, 3), "small"),
    "tiny_clip": ("clip_image", (2, 40, 72), "small"),
    "tiny_sampler": ("sampler_fwd", (2, 3, 16, 16), "small"),
    "tiny_pack": ("pack", None, "small"),
    "tiny_ema": ("ema", None, "small"),
}
COND_REAL = {"vae_encode": "encode_real", "vae_decode": "decode_real", "sampler_fwd": "sampler_real", "clip_image": "clip_real"}
COND_GPU = {     # pass -> the configurations whose union runs on the GPU
    "vae_encode": ("encode_3x320x512", "encode_2x64x96", "encode_1x40x24"),
    "vae_decode": ("decode_1x4x40x64", "decode_1x4x16x24", "decode_2x2x5x3"),
    "sampler_fwd": ("sampler_2x14x40x64", "sampler_2x3x16x24"),
    "clip_image": ("clip_1x320x512", "clip_small_ragged", "clip_small_quick_gelu"),
    "pack": ("pack",),
    "ema": ("ema",),
}
COND_TINY = ("tiny_encode", "tiny_decode", "tiny_clip", "tiny_sampler", "tiny_pack", "tiny_ema")


def _clip_config(kind):
    if kind == "real":
        return dict(num_hidden_layers=CLIP_LAYERS)
    return dict(CLIP_SMALL, hidden_act="quick_gelu") if kind == "small_quick_gelu" else dict(CLIP_SMALL)


def _finite(model):
    """what `build()` / `prepare()` read on the host must be a number: the blend factors"""
    for n, p in model.named_parameters():
        if n.endswith("mix_factor"):
            p.data.fill_(0.5)
    return model


def _cond_models(kind, which):
    from oracle.unet import SVD_CONFIG, TINY_CONFIG, no_default_init
    out = {}
    with no_default_init():
        if "vae" in which:
            from svd_xtend_amd.vae import AutoencoderKLTemporalDecoder
            out["vae"] = _finite(AutoencoderKLTemporalDecoder(**({} if kind == "real" else VAE_SMALL)))
        if "clip" in which:
            from svd_xtend_amd.clip import CLIPVisionModelWithProjection
            out["clip"] = CLIPVisionModelWithProjection(**_clip_config(kind))
        if "unet" in which:
            from svd_xtend_amd.unet import UNetSpatioTemporalConditionModel
            out["unet"] = _finite(UNetSpatioTemporalConditionModel(**dict(SVD_CONFIG if kind == "real" else TINY_CONFIG)))
    return out


def census_cond(name):
    """Counter[signature] of one pass around the step (COND_CONFIGS).  Packing is behind the recorded launches except in `pack`, which
    records `prepare()` of the three models and nothing else."""
    if name in _CACHE:
        return _CACHE[name]
    what, geo, kind = COND_CONFIGS[name]
    rec = Recorder()
    rec.on = False
    with _backend(rec), torch.no_grad():
        if what == "vae_encode":
            vae = _cond_models(kind, ("vae",))["vae"].prepare()
            n, H, W = geo
            rec.on = True
            vae.encode(torch.empty(n, 3, H, W))
        elif what == "vae_decode":
            vae = _cond_models(kind, ("vae",))["vae"].prepare()
            B, T, h, w = geo
            rec.on = True
            vae.decode(torch.empty(B * T, 4, h, w), num_frames=T)
        elif what == "clip_image":
            from svd_xtend_amd import clip as C
            b, h, w = geo
            tower = _cond_models(kind, ("clip",))["clip"].prepare()
            rec.on = True
            C.encode_image(torch.empty(b, 3, h, w), tower)
            if name == "clip_real":              # the layers beyond the first CLIP_LAYERS add launches, not signatures
                full = Recorder()
                with _backend(full):
                    from oracle.unet import no_default_init
                    with no_default_init():
                        whole = C.CLIPVisionModelWithProjection()
                    whole.prepare()
                    full.counts.clear()
                    C.encode_image(torch.empty(b, 3, h, w), whole)
                assert set(full.counts) == set(rec.counts), "the 32-layer tower launches signatures the 2-layer one does not"
        elif what == "sampler_fwd":
            unet = _cond_models(kind, ("unet",))["unet"]
            for p in unet.parameters():
                p.requires_grad_(False)
            unet.prepare()
            B, T, h, w = geo
            cross = unet.config.cross_attention_dim
            args = (torch.empty(B, T, 8, h, w), torch.tensor(1.0))
            kw = dict(encoder_hidden_states=torch.empty(B, 1, cross), added_time_ids=torch.ones(B, 3), return_dict=False)
            unet(*args, **kw)
            rec.on = True
            unet(*args, **kw)
        elif what == "pack":
            models = _cond_models(kind, ("vae", "clip", "unet"))
            for p in models["unet"].parameters():
                p.requires_grad_(False)
            rec.on = True
            for m in models.values():
                m.prepare()
        elif what == "ema":
            from svd_xtend_amd.train import Trainer
            from svd_xtend_amd.training_utils import EMAModel
            unet = _cond_models(kind, ("unet",))["unet"]
            Trainer(unet, dtype=torch.float16, lr=1e-5)           # configuration 2: the trainable set in the Trainer's flat master buffer
            ema = EMAModel(unet.parameters())
            ema.step(unet.parameters())
            rec.on = True
            ema.step(unet.parameters())
        else:
            raise KeyError(what)
    _CACHE[name] = rec.counts
    return rec.counts


def summary(counts):
    per = collections.Counter()
    for s, n in counts.items():
        per[s[0]] += n
    return per


# ---- error model ----------------------------------------------------------------------------------------------------------------------
_FMT = {torch.float16: (11, -14), torch.bfloat16: (8, -126), torch.float32: (24, -126), torch.float64: (53, -1022)}
ROUNDING_MIN_ELEMENTS = 100000
ROUNDING_MEAN_BOUND = 0.05


def ulp_of(ref, dt):
    """spacing of `dt` at |ref| (float64 tensor), the subnormal spacing as floor"""
    p, emin = _FMT[dt]
    e = (torch.frexp(ref.abs())[1] - 1).masked_fill(ref == 0, emin).clamp(min=emin).to(torch.int64) - (p - 1)
    return ((e + 1023) << 52).view(torch.float64)        # 2^e from its bits: exact on every device (ldexp goes through pow, which is not)


def _worst(ratio):
    if ratio.numel() == 0:
        return 0.0, ()
    i = int(torch.argmax(ratio))
    return float(ratio.reshape(-1)[i]), tuple(int(x) for x in torch.unravel_index(torch.tensor(i), ratio.shape)) if ratio.ndim else ()


def _ratio(got, ref, bound):
    g = got.to(torch.float64)
    err = (g - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp(min=1e-300))
    return torch.where(torch.isfinite(g), r, torch.full_like(r, float("inf")))


class RoundingMeans:
    """mean((got - ref)/ulp) and mean((|got| - |ref|)/ulp) over |ref| >= 0.25 rms(ref) -- the selection reads the reference only --
    accumulated over the pieces an output is judged in"""

    def __init__(self):
        self.n, self.s1, self.s2 = 0, 0.0, 0.0

    def add(self, got, ref, dt):
        g = got.to(torch.float64)
        sel = ref.abs() >= 0.25 * ref.pow(2).mean().sqrt()
        if bool(sel.any()):
            u = ulp_of(ref, dt)[sel]
            self.n += int(sel.sum())
            self.s1 += float(((g[sel] - ref[sel]) / u).sum())
            self.s2 += float(((g[sel].abs() - ref[sel].abs()) / u).sum())
        return self

    def means(self):
        return self.n, self.s1 / max(self.n, 1), self.s2 / max(self.n, 1)

    def report(self, res, label):
        """for outputs with enough selected elements: the two means as excess = |mean| / 0.05"""
        n, m1, m2 = self.means()
        if n >= ROUNDING_MIN_ELEMENTS:
            res.append((label + " rounding: mean signed error / ulp", abs(m1) / ROUNDING_MEAN_BOUND, ()))
            res.append((label + " rounding: mean magnitude error / ulp", abs(m2) / ROUNDING_MEAN_BOUND, ()))


def rounding_means(got, ref, dt):
    return RoundingMeans().add(got, ref, dt).means()


def single_bound(dt, ref, S, k_acc, e, extra=None):
    """the single-rounding bound of the error model, per element"""
    bound = 0.5 * ulp_of(ref, dt) + (k_acc + e) * 2.0 ** -23 * S
    return bound if extra is None else bound + extra


def judge_single(res, label, got, ref, S, k_acc, e, rounding=True, extra=None):
    """single-rounding bound; appends (label, excess = worst error / bound, worst index) and, for 16-bit outputs, the rounding-mode
    means.  `extra`: a further documented rounding point, per element."""
    dt = got.dtype
    bound = single_bound(dt, ref, S, k_acc, e, extra)
    res.append((label,) + _worst(_ratio(got, ref, bound)))
    if rounding and dt in (torch.float16, torch.bfloat16):
        RoundingMeans().add(got, ref, dt).report(res, label)


def judge_rows(res, label, got, ref, tol, derived=None):
    """multi-stage bound: tol * (the row's own largest |ref|), never more; `derived` (per element) lowers it where it is smaller;
    half a spacing of the output type at the reference is the floor (no result can be closer than its own rounding).  The rounding-mode
    means hold here as well: the errors of the intermediate roundings are zero-mean, so a biased final cast shows as it does elsewhere."""
    bound = tol * ref.abs().amax(-1, keepdim=True).expand_as(ref)
    if derived is not None:
        bound = torch.minimum(bound, derived)
    bound = torch.maximum(bound, 0.5 * ulp_of(ref, got.dtype))
    res.append((label,) + _worst(_ratio(got, ref, bound)))
    if got.dtype in (torch.float16, torch.bfloat16):
        RoundingMeans().add(got, ref, got.dtype).report(res, label)


def judge_exact(res, label, got, ref):
    res.append((label,) + _worst(_ratio(got, ref.to(torch.float64), torch.zeros_like(ref, dtype=torch.float64))))


def judge_fixed(res, label, got, ref, tol=1e-4):
    """fixed-point GroupNorm statistics, decoded, [entries, 2]: today's bar (largest error over largest reference), each of the two
    statistics on its own so that the sum does not hide under the magnitude of the sum of squares"""
    err = ((got.double() - ref).abs().amax(0) / (ref.abs().amax(0) + 1e-6)).amax()
    res.append((label, float(err) / tol if math.isfinite(float(err)) else float("inf"), ()))


# ---- operands from a signature ----------------------------------------------------------------------------------------------------------
def _v(t, rows, cols, ld):
    return torch.as_strided(t, (rows, cols), (ld, 1), t.storage_offset())


GUARD, GUARD_VALUE = 1024, 7


class Operands:
    """Tensors of one launch, rebuilt from the signature: seeded values, the recorded aliasing (arguments that shared a storage share
    one again, at the recorded distance), outputs pre-filled -- NaN for store forms, ones for accumulate forms."""

    def __init__(self, sig, dev):
        self.sig, self.dev = sig, torch.device(dev)
        self.gen = torch.Generator(device=self.dev).manual_seed(sig_seed(sig))
        self.desc = {}
        self._walk(sig[1])
        self.decls, self.t, self.bufs = {}, {}, {}

    def damaged_guards(self):
        """names of the buffers whose guard bands a launch wrote into"""
        return [r for r, b in self.bufs.items() if not (bool((b[:GUARD] == GUARD_VALUE).all()) and bool((b[-GUARD:] == GUARD_VALUE).all()))]

    def _walk(self, kv, prefix=""):
        for k, v in kv:
            if isinstance(v, tuple) and v and v[0] == "T":
                self.desc[prefix + k] = v
            elif isinstance(v, tuple):
                for i, job in enumerate(v):
                    if isinstance(job, tuple) and not (job and job[0] == "T"):
                        self._walk([(str(j), x) for j, x in enumerate(job)], f"{prefix}{k}.{i}.")
                    elif isinstance(job, tuple):
                        self.desc[f"{prefix}{k}.{i}"] = job

    def has(self, name):
        return name in self.desc

    def dtype(self, name):
        return DT_OF[self.desc[name][1]]

    def randn(self, *shape, scale=1.0):
        return torch.randn(*shape, generator=self.gen, device=self.dev) * scale

    # declarations: name, extent in elements, fill(flat view), output?
    def decl(self, name, extent, fill, out=False):
        if name in self.desc:
            self.decls[name] = (int(extent), fill, out)

    def mat(self, name, rows, cols, ld=None, scale=1.0, shift=0.0):
        ld = ld or cols
        self.decl(name, (rows - 1) * ld + cols, lambda t: _v(t, rows, cols, ld).copy_(self.randn(rows, cols, scale=scale) + shift))

    def vec(self, name, n, scale=1.0, shift=0.0, positive=False):
        self.decl(name, n, lambda t: t.copy_((self.randn(n).abs() if positive else self.randn(n)) * scale + shift))

    def out(self, name, rows, cols, ld=None, fill=float("nan")):
        ld = ld or cols
        self.decl(name, (rows - 1) * ld + cols, lambda t: _v(t, rows, cols, ld).fill_(fill), out=True)

    def table(self, name):
        tab = self.desc[name][3]
        assert tab is not None, f"{name}: the table did not travel in the signature"
        host = torch.frombuffer(bytearray(tab), dtype=torch.int32)
        self.decl(name, host.numel(), lambda t: t.copy_(host))
        return host.to(torch.int64)

    def alloc(self):
        groups = collections.OrderedDict()
        for name in self.decls:
            alias = self.desc[name][2]
            root, delta = (alias if alias is not None and alias[0] in self.decls else (name, 0))
            groups.setdefault(root, []).append((name, delta))
        for root, members in groups.items():
            lo = min(dl for _, dl in members)
            hi = max(dl + self.decls[n][0] for n, dl in members)
            dt = self.dtype(root)
            assert all(self.dtype(n) == dt for n, _ in members), (root, members)
            buf = torch.zeros(hi - lo + 2 * GUARD, dtype=dt, device=self.dev)
            buf[:GUARD] = GUARD_VALUE                      # guard bands on both sides of what the launch may touch
            buf[GUARD + hi - lo:] = GUARD_VALUE
            self.bufs[root] = buf
            for n, dl in members:
                self.t[n] = buf[GUARD + dl - lo:GUARD + dl - lo + self.decls[n][0]]
        for outs in (True, False):                      # inputs last: an in-place launch reads its input, not the pre-fill
            for n, (ext, fill, is_out) in self.decls.items():
                if is_out == outs:
                    fill(self.t[n])
        return self

    def __getitem__(self, name):
        return self.t.get(name)


# ---- case runners -------------------------------------------------------------------------------------------------------------------------

RUNNERS = {}
_UA = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}          # relative size of one rounding into the activation type


def _half_ulp_after(ref, rel, dt):
    """the last rounding of a chain: half a spacing at a value that earlier roundings may have moved by `rel` (into the next binade)"""
    return 0.5 * ulp_of(ref.abs() * (1.0 + rel), dt)


def runner(*names):
    def deco(f):
        for n in names:
            RUNNERS[n] = f
        return f
    return deco


def _sync(dev):
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()


def _gn_encode(stats, n_s, G, cnt, mode, s0, s1):
    """fixed-point statistics buffer (replica 0) from float64 sums"""
    k0, k1 = emul.gn_fixed_scales(cnt, mode)
    v = emul.gn_view(stats, n_s, G)
    v.zero_()
    v[0, ..., 0] = torch.round(s0 * 2.0 ** k0).to(torch.int64)
    v[0, ..., 1] = torch.round(s1 * 2.0 ** k1).to(torch.int64)


def _gn_decoded(stats, n_s, G, cnt, mode):
    k0, k1 = emul.gn_fixed_scales(cnt, mode)
    tot = emul.gn_view(stats, n_s, G).sum(0)
    return torch.stack([tot[..., 0].double() * 2.0 ** -k0, tot[..., 1].double() * 2.0 ** -k1], -1)


def _judge_gn_stats(res, label, stats, written, n_s, rows, C, G):
    """statistics a launch leaves beside the tensor it wrote: against float64 sums over that (rounded) tensor"""
    s0, s1 = ref64.gn_sums(written, n_s, rows, C, G)
    judge_fixed(res, label, _gn_decoded(stats, n_s, G, rows * (C // G), 0).view(-1, 2), torch.stack([s0, s1], -1).view(-1, 2))


def _n_groups(M, rpg, mod):
    return mod if mod else -(-M // rpg)


def _gather_src_rows(g):
    if g.mode == K.GATHER_TEMPORAL3:
        return g.n_img * g.t * g.hw
    if g.mode == K.GATHER_CONV3X3_DGRAD2:
        return g.n_img * g.hi * g.wi
    return g.n_img * (g.hi // 2 if g.ups else g.hi) * (g.wi // 2 if g.ups else g.wi)


def coalesced_columns(a, C, res):
    """Leading columns of an activation-output GEMM that leave through csrc/gemm_nt.hip's LDS-parked, coalesced stores (gemm_v4_kernel,
    epilogue A): the launch resolves to one of the four-/eight-wave tiles, C and the residual are 16-byte aligned with pitches that
    are multiples of 8, and the column tile is whole (n0 + BN <= N: a partial last tile takes the direct epilogue).  Every other
    element gets the residual in fp32 before its one rounding."""
    from svd_xtend_amd.ops import GEMM_TILES, _tile_launched
    width = {v: t.cols for v, t in GEMM_TILES.items() if v not in (26, 32, 34)}      # the tiles gemm_act reaches through gemm_v4_kernel
    bn = width.get(_tile_launched(a["variant"], a["M"], a["N"]))
    if bn is None or a["ldc"] % 8 or C.data_ptr() % 16 or (res is not None and (a["ldres"] % 8 or res.data_ptr() % 16)):
        return 0
    return a["N"] // bn * bn


def _rebuild(v, o, prefix):
    """the argument `v` of a signature with its tensor descriptors replaced by the operands"""
    if isinstance(v, tuple) and v and v[0] == "T":
        return o[prefix]
    if isinstance(v, tuple) and v and v[0] == "dtype":
        return DT_OF[v[1]]
    if isinstance(v, tuple):
        return tuple(_rebuild(x, o, f"{prefix}.{i}") for i, x in enumerate(v))
    return v


def _launch(be, o, overrides=None):
    entry, kv = o.sig
    kw = {k: _rebuild(v, o, k) for k, v in kv}
    kw.update(overrides or {})
    getattr(be, entry)(*kw.values())                 # positional: the emulation names some parameters differently
    _sync(o.dev)


PITCH_COPY_MAX = 1 << 28            # elements between the rows of C that run_gemm copies to compare; beyond: they are zero and stay zero


def _all_zero_rows(t, step=1 << 26):
    """whether every element of the (strided, integer-typed) matrix is zero, a bounded number of elements at a time"""
    rows = max(1, step // max(t.shape[1], 1))
    return not any(bool((t[r:r + rows] != 0).any()) for r in range(0, t.shape[0], rows))


@runner("gemm")
def run_gemm(be, o, a):
    M, N, Kd, dt = a["M"], a["N"], a["K"], o.dtype("A")
    g = a["gather"] if a["gather"] is not None and a["gather"].mode != K.GATHER_PLAIN else None
    if g is not None:
        nsrc = _gather_src_rows(g)
        o.mat("A", nsrc, g.cin, g.lda)
    else:
        o.mat("A", M, Kd, a["lda"])
    o.mat("B", N, Kd, a["ldb"], scale=Kd ** -0.5)
    dual = a["dual"]
    if dual is not None:
        K2, lda2, ldb2 = dual[2:5]
        seg = dual[5] if len(dual) > 5 else 0
        o.mat("dual.0", M, (N // seg) * K2 if seg else K2, lda2)
        o.mat("dual.1", N, K2, ldb2, scale=K2 ** -0.5)
    o.vec("bias", N)
    ng = _n_groups(M, a["rv_rpg"], a["rv_mod"]) if a["rowvec"] is not None else 0
    if ng:
        o.mat("rowvec", ng, N, a["rv_ld"])
    o.mat("res", M, N, a["ldres"])
    mode, sk, epi, Fd = a["out_mode"], a["split_k"], a["epilogue"], a["aux_dim"]
    if mode == K.OUT_F32_SLAB:
        o.out("C", sk * M, N)
    elif epi == K.EPI_GEGLU_BWD:
        o.out("C", M, 2 * Fd, a["ldc"])
        o.mat("aux_in", M, 2 * Fd)
    else:
        o.out("C", M, N, a["ldc"], fill=1.0 if mode in (K.OUT_F32_ATOMIC, K.OUT_F32_ADD) else float("nan"))
    if epi == K.EPI_GEGLU_FWD:
        o.out("aux_out", M, Fd)
    gn = a["gn"]
    if gn is not None:
        n_s, G = M // gn[1], N // gn[2]
        o.decl("gn.0", K.GN_REPLICAS * n_s * G * K.GN_STAT_FLOATS, lambda t: t.zero_(), out=True)
    o.alloc()
    # a pitch wider than N (the VAE's score rows, conv_out's 8 columns in zeroed 64-wide rows): what lies between the rows is not the launch's
    pitch = None
    if mode != K.OUT_F32_SLAB and epi != K.EPI_GEGLU_BWD and a["ldc"] > N and M > 1:
        pitch = torch.as_strided(o["C"], (M - 1, a["ldc"] - N), (a["ldc"], 1), o["C"].storage_offset() + N)
        pitch = pitch.view(torch.int16 if pitch.element_size() == 2 else torch.int32)
        # a gap of gigabytes (tests/reach_checks.py) is not copied: it is all zero bytes before the launch and all zero bytes after it
        pitch_before = pitch.clone() if pitch.numel() <= PITCH_COPY_MAX else None
        same = pitch_before is not None or _all_zero_rows(pitch)
    _launch(be, o)
    res = []
    if pitch is not None:
        same = bool((pitch == pitch_before).all()) if pitch_before is not None else same and _all_zero_rows(pitch)
        res.append(("columns N..ldc of C untouched", 0.0 if same else float("inf"), ()))
    A = _v(o["A"], nsrc, g.cin, g.lda) if g is not None else _v(o["A"], M, Kd, a["lda"])
    B = _v(o["B"], N, Kd, a["ldb"])
    d2 = None
    if dual is not None:
        d2 = (_v(o["dual.0"], M, (N // seg) * K2 if seg else K2, lda2), _v(o["dual.1"], N, K2, ldb2), seg)
    kw = dict(alpha=a["alpha"], gather=g, dual=d2, bias=o["bias"],
              rowvec=_v(o["rowvec"], ng, N, a["rv_ld"]) if ng else None, rv_rpg=a["rv_rpg"], rv_mod=a["rv_mod"],
              res=_v(o["res"], M, N, a["ldres"]) if o["res"] is not None else None)
    if mode == K.OUT_F32_SLAB:
        ksz = (Kd // 64 + sk - 1) // sk * 64
        for z in range(sk):
            Bz = torch.zeros_like(B)
            Bz[:, z * ksz:(z + 1) * ksz] = B[:, z * ksz:(z + 1) * ksz]
            v, S, ka, e = ref64.gemm_nt(A, Bz, M, alpha=a["alpha"], gather=g)
            judge_single(res, f"slab {z}", _v(o["C"], sk * M, N, N)[z * M:(z + 1) * M], v, S, min(ksz, Kd), e)
        return res
    if epi == K.EPI_GEGLU_BWD:
        dh, S, ka, e = ref64.gemm_nt(A, B, M, **kw)
        pre = _v(o["aux_in"], M, 2 * Fd, 2 * Fd)
        ref = ref64.geglu_bwd(dh, pre, Fd)
        fac = ref64.geglu_bwd(torch.ones_like(dh), pre, Fd).abs()                           # |gelu(g)|, |a gelu'(g)|
        dh2, S2 = torch.cat([dh, dh], 1).abs(), torch.cat([S, S], 1)
        # dh is rounded to the activation type (2^-p |dh|, on top of its fp32 accumulation), multiplied by gelu(g) / a gelu'(g) in fp32 --
        # 1 + erf cancels for g << 0, so the factor's error is absolute: a few 2^-23 of |g| / |a| (1 + |g|) -- and rounded once more
        p64 = ref64.d(pre)
        facmag = torch.cat([p64[:, Fd:].abs(), p64[:, :Fd].abs() * (1 + p64[:, Fd:].abs())], 1)
        derived = (_UA[dt] * dh2 + (ka + 16) * 2.0 ** -23 * S2) * fac + _half_ulp_after(ref, 2 * _UA[dt], dt) + 16 * 2.0 ** -23 * dh2 * facmag
        judge_rows(res, "geglu-bwd dpre", _v(o["C"], M, 2 * Fd, a["ldc"]), ref, tol_for(dt, 2), derived)
        return res
    c0 = torch.ones(M, N, dtype=torch.float64, device=o.dev) if mode in (K.OUT_F32_ATOMIC, K.OUT_F32_ADD) else None
    v, S, ka, e = ref64.gemm_nt(A, B, M, c0=c0, **kw)
    C = _v(o["C"], M, N, a["ldc"])
    extra = None
    if kw["res"] is not None and mode == K.OUT_ACT:
        # csrc/gemm_nt.hip, coalesced-store epilogue of the 128-row tiles: alpha A B^T + bias + row vector is rounded to the activation type,
        # parked in LDS, and the residual is added to THAT on the way out -- a second rounding point, at the magnitude of the value before
        # the residual (the reference model's `conv(x)` then `+ residual` in 16-bit autocast has the same two).  Granted to the columns
        # that take that path only.  profiles/census_gpu.txt
        extra = 0.5 * ulp_of((v - ref64.d(kw["res"])).abs() * (1 + 2.0 ** -12), dt)
        extra[:, coalesced_columns(a, C, o["res"]):] = 0.0
    judge_single(res, "C", C, v, S, ka, e, extra=extra)
    if epi == K.EPI_GEGLU_FWD:
        pre = C.to(torch.float64)
        h = ref64.geglu(pre, Fd)
        derived = 0.5 * ulp_of(h, dt) + 16 * 2.0 ** -23 * (pre[:, :Fd] * pre[:, Fd:]).abs()
        judge_rows(res, "geglu-fwd h (from the pre it wrote)", _v(o["aux_out"], M, Fd, Fd), h, tol_for(dt, 2), derived)
    if gn is not None:
        _judge_gn_stats(res, "GroupNorm statistics (of the tensor it wrote)", o["gn.0"], C.contiguous(), n_s, gn[1], N, G)
    return res


@runner("gemm_tn")
def run_gemm_tn(be, o, a):
    R, N, Kd, mode, sk = a["R"], a["N"], a["K"], a["out_mode"], a["split_k"]
    o.mat("A", R, N, a["lda"])
    o.mat("B", R, Kd, a["ldb"], scale=R ** -0.5)
    slab = mode == K.OUT_F32_SLAB
    o.out("C", sk * N if slab else N, Kd, a["ldc"], fill=1.0 if mode == K.OUT_F32_ADD else float("nan"))
    if slab:
        o.out("a_colsum", sk, N)
    else:
        o.out("a_colsum", 1, N, fill=1.0)
    o.out("found_inf", 1, 1, fill=0.0)
    o.alloc()
    _launch(be, o)
    res = []
    A, B = _v(o["A"], R, N, a["lda"]), _v(o["B"], R, Kd, a["ldb"])
    per = ((R + 63) // 64 + sk - 1) // sk * 64 if slab else R
    for z in range(sk if slab else 1):
        Az, Bz = A[z * per:(z + 1) * per], B[z * per:(z + 1) * per]
        v, S, ka = ref64.gemm_tn(Az, Bz)
        if mode == K.OUT_F32_ADD:
            v, S, ka = v + 1.0, S + 1.0, ka + 1
        C = _v(o["C"], N, Kd, a["ldc"]) if not slab else _v(o["C"], sk * N, Kd, Kd)[z * N:(z + 1) * N]
        judge_single(res, f"C[{z}]", C, v, S, ka, 1)
        if o["a_colsum"] is not None:
            cs, Sc = ref64.d(Az).sum(0), ref64.d(Az).abs().sum(0)
            if not slab:
                cs, Sc = cs + 1.0, Sc + 1.0
            judge_single(res, f"colsum(A)[{z}]", o["a_colsum"][z * N:(z + 1) * N], cs, Sc, Az.shape[0], 1)
    if o["found_inf"] is not None:
        judge_exact(res, "found_inf stays 0", o["found_inf"], torch.zeros(1, device=o.dev))
    return res


def _finalize_terms(o, a, M, N):
    ng = _n_groups(M, a["rv_rpg"], a["rv_mod"]) if a["rowvec"] is not None else 0
    o.vec("bias", N)
    if ng:
        o.mat("rowvec", ng, N, a["rv_ld"])
    o.mat("res", M, N, a["ldres"])
    return ng


@runner("gemm_finalize")
def run_gemm_finalize(be, o, a):
    M, N, ns, stride, accf = a["M"], a["N"], a["nsplit"], a["slab_stride"], int(a["accumulate_f32"])
    o.decl("acc", (ns - 1) * stride + M * N, lambda t: [_v(t[z * stride:], M, N, N).copy_(o.randn(M, N, scale=ns ** -0.5)) for z in range(ns)])
    ng = _finalize_terms(o, a, M, N)
    o.out("C", M, N, a["ldc"], fill=1.0 if accf == 1 else float("nan"))
    cn = a["colsum_out"][4] if a["colsum_out"] is not None else 0
    if cn:
        o.mat("colsum_slabs", ns, cn)
        o.out("colsum_out", 1, cn, fill=1.0)
    gn = a["gn"]
    if gn is not None:
        n_s, G = M // gn[1], N // gn[2]
        o.decl("gn.0", K.GN_REPLICAS * n_s * G * K.GN_STAT_FLOATS, lambda t: t.zero_(), out=True)
    o.alloc()
    _launch(be, o)
    res = []
    slabs = torch.stack([_v(o["acc"][z * stride:], M, N, N) for z in range(ns)])
    extra = [None if o["bias"] is None else o["bias"][None].expand(M, N),
             _v(o["rowvec"], ng, N, a["rv_ld"])[ref64.group_index(M, a["rv_rpg"], a["rv_mod"], o.dev)] if ng else None,
             _v(o["res"], M, N, a["ldres"]) if o["res"] is not None else None,
             torch.ones(M, N, device=o.dev) if accf == 1 else None]
    v, S, n = ref64.slab_sum(slabs, extra)
    C = _v(o["C"], M, N, a["ldc"])
    judge_single(res, "C", C, v, S, n, 1)
    if cn:
        v, S, n = ref64.slab_sum(_v(o["colsum_slabs"], ns, cn, cn), [torch.ones(cn, device=o.dev)])
        judge_single(res, "colsum_out", o["colsum_out"], v, S, n, 1)
    if gn is not None:
        _judge_gn_stats(res, "GroupNorm statistics (of the tensor it wrote)", o["gn.0"], C.contiguous(), n_s, gn[1], N, G)
    return res


@runner("grad_finalize_batch")
def run_grad_finalize_batch(be, o, a):
    jobs = a["jobs"]
    for i, j in enumerate(jobs):
        ns, stride, cnt, store = j[1], j[2], j[4], j[7]
        o.decl(f"jobs.{i}.0", (ns - 1) * stride + cnt,
               lambda t, ns=ns, stride=stride, cnt=cnt: [t[z * stride:z * stride + cnt].copy_(o.randn(cnt, scale=ns ** -0.5)) for z in range(ns)])
        o.out(f"jobs.{i}.3", 1, cnt, fill=float("nan") if store else 1.0)
        if j[6] is not None:
            o.mat(f"jobs.{i}.5", ns, j[6][4])
            o.out(f"jobs.{i}.6", 1, j[6][4], fill=1.0)
        if len(j) > 8:
            o.out(f"jobs.{i}.8", 1, 1, fill=0.0)
    o.alloc()
    _launch(be, o)
    res = []
    for i, j in enumerate(jobs):
        ns, stride, cnt, store = j[1], j[2], j[4], j[7]
        slabs = torch.stack([o[f"jobs.{i}.0"][z * stride:z * stride + cnt] for z in range(ns)])
        v, S, n = ref64.slab_sum(slabs, [None if store else torch.ones(cnt, device=o.dev)])
        judge_single(res, f"job {i} dst", o[f"jobs.{i}.3"], v, S, n, 1)
        if j[6] is not None:
            cn = j[6][4]
            v, S, n = ref64.slab_sum(_v(o[f"jobs.{i}.5"], ns, cn, cn), [torch.ones(cn, device=o.dev)])
            judge_single(res, f"job {i} colsum_out", o[f"jobs.{i}.6"], v, S, n, 1)
        if len(j) > 8 and j[8] is not None:
            judge_exact(res, f"job {i} found_inf stays 0", o[f"jobs.{i}.8"], torch.zeros(1, device=o.dev))
    return res


def _small_linear_decl(o, names, M, N, Kd, ldw, trans, acc):
    X, W, b, Y = names
    o.mat(X, M, N if trans else Kd)
    o.mat(W, N, Kd, ldw, scale=(N if trans else Kd) ** -0.5)
    o.vec(b, N)
    o.out(Y, M, Kd if trans else N, fill=1.0 if acc else float("nan"))


def _small_linear_judge(res, label, o, names, M, N, Kd, ldw, trans, silu_in, acc):
    X, W, b, Y = names
    w = ref64.d(_v(o[W], N, Kd, ldw))
    x = ref64.d(_v(o[X], M, N if trans else Kd, N if trans else Kd))
    if silu_in:
        x = torch.nn.functional.silu(x)
    v, S = (x @ w, x.abs() @ w.abs()) if trans else (x @ w.t(), x.abs() @ w.abs().t())
    e = 2 + (8 if silu_in else 0)
    if o[b] is not None and not trans:
        v, S, e = v + ref64.d(o[b])[None], S + ref64.d(o[b]).abs()[None], e + 1
    if acc:
        v, S, e = v + 1.0, S + 1.0, e + 1
    judge_single(res, label, _v(o[Y], M, Kd if trans else N, Kd if trans else N), v, S, N if trans else Kd, e)


@runner("small_linear")
def run_small_linear(be, o, a):
    names = ("X", "W", "bias", "Y")
    _small_linear_decl(o, names, a["M"], a["N"], a["K"], a["ldw"], a["trans"], a["accumulate"])
    o.alloc()
    _launch(be, o)
    res = []
    _small_linear_judge(res, "Y", o, names, a["M"], a["N"], a["K"], a["ldw"], a["trans"], a["silu_in"], a["accumulate"])
    return res


@runner("small_linear_batch")
def run_small_linear_batch(be, o, a):
    M, trans = a["M"], a["trans"]
    for i, j in enumerate(a["jobs"]):
        _small_linear_decl(o, [f"jobs.{i}.{c}" for c in range(4)], M, j[4], j[5], j[6], trans, j[8])
    o.alloc()
    _launch(be, o)
    res = []
    for i, j in enumerate(a["jobs"]):
        _small_linear_judge(res, f"job {i} Y", o, [f"jobs.{i}.{c}" for c in range(4)], M, j[4], j[5], j[6], trans, j[7], j[8])
    return res


@runner("outer_acc_batch")
def run_outer_acc_batch(be, o, a):
    M = a["M"]
    for i, (dY, X, dW, N, Kd, sc) in enumerate(a["jobs"]):
        o.mat(f"jobs.{i}.0", M, N)
        o.mat(f"jobs.{i}.1", M, Kd)
        o.out(f"jobs.{i}.2", N, Kd, fill=1.0)
    o.alloc()
    _launch(be, o)
    res = []
    for i, (dY, X, dW, N, Kd, sc) in enumerate(a["jobs"]):
        dy = ref64.d(_v(o[f"jobs.{i}.0"], M, N, N))
        x = ref64.d(_v(o[f"jobs.{i}.1"], M, Kd, Kd)) if X is not None else torch.ones(M, 1, dtype=torch.float64, device=o.dev)
        judge_single(res, f"job {i} dW", _v(o[f"jobs.{i}.2"], N, Kd, Kd), 1.0 + sc * (dy.t() @ x), 1.0 + abs(sc) * (dy.abs().t() @ x.abs()), M + 1, 2)
    return res


@runner("ln_param_reduce_batch")
def run_ln_param_reduce_batch(be, o, a):
    for i, (pt, dg, db, nblk, C) in enumerate(a["jobs"]):
        o.mat(f"jobs.{i}.0", nblk, 2 * C)
        o.out(f"jobs.{i}.1", 1, C, fill=1.0)
        o.out(f"jobs.{i}.2", 1, C, fill=1.0)
    o.alloc()
    _launch(be, o)
    res = []
    for i, (pt, dg, db, nblk, C) in enumerate(a["jobs"]):
        v, S, n = ref64.slab_sum(_v(o[f"jobs.{i}.0"], nblk, 2 * C, 2 * C), [torch.ones(2 * C, device=o.dev)])
        judge_single(res, f"job {i} dgamma", o[f"jobs.{i}.1"], v[:C], S[:C], n, 1)
        judge_single(res, f"job {i} dbeta", o[f"jobs.{i}.2"], v[C:], S[C:], n, 1)
    return res


@runner("timestep_embed")
def run_timestep_embed(be, o, a):
    n, dim = a["n"], a["dim"]
    o.decl("t", n, lambda t: t.copy_(o.randn(n).abs() * 40.0))
    o.out("out", n, dim)
    o.alloc()
    _launch(be, o)
    ref, arg = ref64.timestep_embed(o["t"], dim)
    # argument t * exp(-ln(1e4) i / half): fp32 exp and product (4 roundings of |arg|), then sin / cos to a few fp32 spacings of 1
    bound = (8 * arg + 4) * 2.0 ** -23
    return [("out",) + _worst(_ratio(_v(o["out"], n, dim, dim), ref, bound))]


def run_case(be, sig, dev=None, operands_out=None, seed_of=None):
    """Launch `sig` on backend `be` with operands rebuilt from the signature and judge every output: [(label, excess, worst index)],
    excess = error / bound (<= 1 passes).  `be` may be a kernel_checks.Pair (its implementation under test is used).  `seed_of`: the
    signature whose seed the operands take (two signatures that differ in a pitch only then hold the same values)."""
    be = getattr(be, "impl", be)
    dev = dev or ("cuda" if isinstance(be, K.HipBackend) and type(be).__name__ == "HipBackend" else "cpu")
    o = Operands(sig, dev)
    if seed_of is not None:
        o.gen.manual_seed(sig_seed(seed_of))
    if operands_out is not None:
        operands_out.append(o)                  # the caller wants the tensors of the launch as well (o["C"], ...)
    res = RUNNERS[sig[0]](be, o, sig_args(sig))
    bad = o.damaged_guards()
    res.append((f"nothing written outside the operands{' (' + ', '.join(bad) + ')' if bad else ''}", float("inf") if bad else 0.0, ()))
    return res


# ---- norms ---------------------------------------------------------------------------------------------------------------------------------
def _gn_common(o, a, with_dy):
    n_s, rows, C, G = a["n_s"], a["rows"], a["C"], a["G"]
    o.mat("x", n_s * rows, C, scale=1.5, shift=0.3)
    if with_dy:
        o.mat("dy", n_s * rows, C)
    o.vec("gamma", C, scale=0.1, shift=1.0)
    o.vec("beta", C, scale=0.1)
    nst = K.GN_REPLICAS * n_s * G * K.GN_STAT_FLOATS
    if a["stats"] is not None and o.sig[0] != "gn_stats":
        def fill(t):
            s0, s1 = ref64.gn_sums(_v(o["x"], n_s * rows, C, C), n_s, rows, C, G)
            _gn_encode(t, n_s, G, rows * (C // G), 0, s0, s1)
        o.decl("stats", nst, fill)
    return n_s, rows, C, G, nst


@runner("gn_stats")
def run_gn_stats(be, o, a):
    n_s, rows, C, G, nst = _gn_common(o, a, False)
    o.decl("stats", nst, lambda t: t.fill_(0.0 if a["prezeroed"] else 1.0), out=True)       # not prezeroed: the launch clears what is there
    o.alloc()
    _launch(be, o)
    res = []
    _judge_gn_stats(res, "stats", o["stats"], _v(o["x"], n_s * rows, C, C), n_s, rows, C, G)
    return res


@runner("gn_apply")
def run_gn_apply(be, o, a):
    n_s, rows, C, G, nst = _gn_common(o, a, False)
    o.out("y", n_s * rows, C)
    o.alloc()
    _launch(be, o)
    x = _v(o["x"], n_s * rows, C, C)
    ref = ref64.gn_fwd(x, o["gamma"], o["beta"], n_s, rows, C, G, a["eps"], a["silu"])
    S, cond = ref64.gn_fwd_S(x, o["gamma"], o["beta"], n_s, rows, C, G, a["eps"])
    res = []
    # fp32 roundings of the magnitude sum S: mean, E[x^2], variance (cond = E[x^2] / var roundings for each of the two it is the difference
    # of), rstd: 4 + 2 cond; x - mean, times rstd: 2; times gamma, + beta: 2 -- SiLU's slope (<= 1.1) carries them to the output -- and of
    # the result: sigmoid (exp, 1 +, reciprocal) and the product: 4, with SiLU only
    n_round = (8 + 2 * cond) * (1.1 if a["silu"] else 1.0)
    judge_single(res, "y", _v(o["y"], n_s * rows, C, C), ref, n_round * S + (4 * ref.abs() if a["silu"] else 0.0), 0, 1)
    return res


def _gn_bwd_ref(o, a, n_s, rows, C, G):
    return ref64.gn_bwd(_v(o["dy"], n_s * rows, C, C), _v(o["x"], n_s * rows, C, C), o["gamma"], o["beta"], n_s, rows, C, G, a["eps"], a["silu"])


@runner("gn_bwd_stats")
def run_gn_bwd_stats(be, o, a):
    n_s, rows, C, G, nst = _gn_common(o, a, True)
    o.decl("bstats", nst, lambda t: t.fill_(0.0 if a["prezeroed"] else 1.0), out=True)
    o.alloc()
    _launch(be, o)
    _, s1, s2 = _gn_bwd_ref(o, a, n_s, rows, C, G)
    res = []
    judge_fixed(res, "bstats", _gn_decoded(o["bstats"], n_s, G, rows * (C // G), 1).view(-1, 2), torch.stack([s1, s2], -1).view(-1, 2), 2e-3)
    return res


@runner("gn_bwd_apply")
def run_gn_bwd_apply(be, o, a):
    """dx = rstd (dz gamma - (s1 + xhat s2) / count) + add from the statistics of both passes.  Rounding points: the inputs (given) and
    the output; fp32 arithmetic in between.  Derived bound, per element, with S the magnitude sum of that expression (+ |add|):
    half an output spacing
    + 2^-23 S (20 + 2 cond): mean, E[x^2], variance (cond = E[x^2] / var roundings of it each for the two it is the difference of), rstd:
      4; xhat: 2; z = xhat gamma + beta: 2; silu'(z) (sigmoid, 1 - s, two products, one sum): 6; dz gamma: 2; s1 / count, xhat s2 / count,
      the two sums: 4 -- counted against S although most touch one term only; times rstd and + add: 2 (the 20 is their total)
    + 2^-23 * 4 amp: xhat = (x - mean) rstd cancels; its absolute error, 4 roundings of (|x| + |mean|) rstd, reaches dx through xhat s2 /
      count and through silu'(z).
    The fixed-point quantisation of the statistics (2^-17 absolute or finer on sums of 1e5 .. 1e7 terms) is below one of these roundings.
    Never more than the family's bar, tol_for(dt) on the row's own maximum."""
    n_s, rows, C, G, nst = _gn_common(o, a, True)

    def fill(t):
        _, s1, s2 = _gn_bwd_ref(o, a, n_s, rows, C, G)
        _gn_encode(t, n_s, G, rows * (C // G), 1, s1, s2)
    o.decl("bstats", nst, fill)
    o.mat("add", n_s * rows, C)
    o.out("dx", n_s * rows, C)
    o.alloc()
    _launch(be, o)
    dt = o.dtype("x")
    dx, _, _ = _gn_bwd_ref(o, a, n_s, rows, C, G)
    S, amp, cond = ref64.gn_bwd_magnitudes(_v(o["dy"], n_s * rows, C, C), _v(o["x"], n_s * rows, C, C), o["gamma"], o["beta"], n_s, rows, C, G,
                                            a["eps"], a["silu"])
    if o["add"] is not None:
        add = ref64.d(_v(o["add"], n_s * rows, C, C))
        dx, S = dx + add, S + add.abs()
    derived = 0.5 * ulp_of(dx, dt) + 2.0 ** -23 * ((20 + 2 * cond) * S + 4 * amp)
    res = []
    judge_rows(res, "dx", _v(o["dx"], n_s * rows, C, C), dx, tol_for(dt), derived)
    return res


def _judge_ln_stats(res, label, stats, x, mean, rstd, rows, C):
    x = ref64.d(x)
    ex2 = (x * x).mean(1) + mean * mean
    st = _v(stats, rows, 2, 2)
    res.append((label + " mean",) + _worst(_ratio(st[:, 0], mean, 0.5 * ulp_of(mean, torch.float32) + (C + 2) * 2.0 ** -23 * x.abs().mean(1))))
    b = 0.5 * ulp_of(rstd, torch.float32) + 0.5 * rstd ** 3 * (C + 4) * 2.0 ** -23 * ex2 + 4 * 2.0 ** -23 * rstd
    res.append((label + " rstd",) + _worst(_ratio(st[:, 1], rstd, b)))


@runner("ln_fwd")
def run_ln_fwd(be, o, a):
    rows, C = a["rows"], a["C"]
    o.mat("x", rows, C, scale=2.0, shift=0.5)
    o.vec("gamma", C, scale=0.1, shift=1.0)
    o.vec("beta", C, scale=0.1)
    o.out("y", rows, C)
    o.out("stats", rows, 2)
    o.alloc()
    _launch(be, o)
    x = _v(o["x"], rows, C, C)
    y, mean, rstd, S = ref64.ln_fwd(x, o["gamma"], o["beta"], a["eps"])
    res = []
    judge_single(res, "y", _v(o["y"], rows, C, C), y, S, C, 8)        # mean and variance: C accumulated terms; 8 roundings of the epilogue
    _judge_ln_stats(res, "stats", o["stats"], x, mean, rstd, rows, C)
    return res


LN_EPS = 1e-5


@runner("ln_bwd")
def run_ln_bwd(be, o, a):
    """dx = rstd (g - mean(g) - xhat mean(g xhat)) + add + add2_scale add2, g = dy gamma: one rounding point, the output; fp32 in between.
    Derived bound per element, S the magnitude sum of the expression: half an output spacing + 2^-23 (12 S + C red + 3 amp) --
    12: xhat (2), g (1), g xhat (1), the two subtractions and the product with xhat (3), times rstd (1), the two adds with add2's scale
    (3), the division of the row sums (1); C red: the two row reductions, C accumulated terms each, `red` being their share of S;
    3 amp: the cancellation inside xhat = (x - mean) rstd, three roundings of (|x| + |mean|) rstd, through both places xhat enters.
    Never more than the family's bar, tol_for(dt) on the row's own maximum.  The affine gradients are fp32 sums over the rows:
    single-rounding bound with S = sum |dy| (|x| + |mean|) rstd (xhat is recomputed in fp32 from the saved statistics)."""
    rows, C = a["rows"], a["C"]
    o.mat("x", rows, C, scale=2.0, shift=0.5)
    o.mat("dy", rows, C)
    o.vec("gamma", C, scale=0.1, shift=1.0)

    def fill(t):
        _, mean, rstd, _ = ref64.ln_fwd(_v(o["x"], rows, C, C), o["gamma"], o["gamma"], LN_EPS)
        _v(t, rows, 2, 2).copy_(torch.stack([mean, rstd], 1))
    o.decl("stats", rows * 2, fill)
    o.mat("add", rows, C)
    o.mat("add2", rows, C)
    o.out("dx", rows, C)
    o.out("dgamma", 1, C, fill=1.0)
    o.out("dbeta", 1, C, fill=1.0)
    nblk = K.ln_bwd_blocks(rows, C) if a["defer_reduce"] else K.LN_PARTIAL_ROWS
    o.out("scratch", nblk, 2 * C)
    o.alloc()
    _launch(be, o)
    x, dy = _v(o["x"], rows, C, C), _v(o["dy"], rows, C, C)
    dx, dg, db, _, Sb = ref64.ln_bwd(dy, x, o["gamma"], LN_EPS)
    for nm, sc in (("add", 1.0), ("add2", a["add2_scale"])):
        if o[nm] is not None:
            dx = dx + sc * ref64.d(_v(o[nm], rows, C, C))
    res = []
    dt = o.dtype("x")
    S, red, amp = ref64.ln_bwd_magnitudes(dy, x, o["gamma"], LN_EPS)
    for nm, sc in (("add", 1.0), ("add2", a["add2_scale"])):
        if o[nm] is not None:
            S = S + abs(sc) * ref64.d(_v(o[nm], rows, C, C)).abs()
    derived = 0.5 * ulp_of(dx, dt) + 2.0 ** -23 * (12 * S + C * red + 3 * amp)
    judge_rows(res, "dx", _v(o["dx"], rows, C, C), dx, tol_for(dt), derived)
    if o["dgamma"] is not None:
        _, mean, rstd, _ = ref64.ln_fwd(x, o["gamma"], o["gamma"], LN_EPS)
        Sg = (ref64.d(dy).abs() * (ref64.d(x).abs() + mean.abs()[:, None]) * rstd[:, None]).sum(0)
        if a["defer_reduce"]:
            pt = ref64.d(_v(o["scratch"], nblk, 2 * C, 2 * C)).sum(0)
            got_g, got_b, one = pt[:C], pt[C:], 0.0
            judge_exact(res, "dgamma untouched", o["dgamma"], torch.ones(C, device=o.dev))
        else:
            got_g, got_b, one = o["dgamma"], o["dbeta"], 1.0
        for nm, got, ref, S in (("dgamma", got_g, dg, Sg), ("dbeta", got_b, db, Sb)):
            bound = 0.5 * ulp_of(ref + one, torch.float32) + (rows + 8) * 2.0 ** -23 * (S + one)
            res.append((nm,) + _worst(_ratio(got, ref + one, bound)))
    return res


# ---- attention -------------------------------------------------------------------------------------------------------------------------------
def _hv(t, nb, S, heads, ld):
    return torch.as_strided(t, (nb, heads, S, 64), (S * ld, 64, ld, 1), t.storage_offset())


def _attn_decl(o, a, names=("q", "k", "v")):
    nb, heads, S, ld = a["nb"], a["heads"], a["S"], a["ld"]
    C = heads * 64
    for nm in names:
        o.mat(nm, nb * S, C, ld)
    if S >= 160:
        # keys that grow along the sequence, as tests/kernel_checks.py's: the running maximum of the online softmax moves by more than
        # the deferred-rescale threshold (2^8) between key tiles -- run_attn_fwd checks on the float64 scores that it does.  Scores have
        # the standard deviation of the ramp.  Its top is kernel_checks' 4.0 up to S = 2560; at S = 9216 that puts the early keys'
        # probabilities at e^-17 = 4e-8, below half of fp16's smallest subnormal, and their dV / dK rows (1e-5 of the tensor's maximum)
        # hold no correct digit in ANY kernel that hands fp16 probabilities to the matrix unit, while every row is judged on its own
        # maximum here: 2.0 there (probabilities >= 1e-5)
        top = 4.0 if S < 4096 else 2.0
        prev = o.decls["k"][1]
        o.decls["k"] = (o.decls["k"][0], lambda t: (prev(t), _v(t, nb * S, C, ld).mul_(
            torch.linspace(0.3, top, S, device=o.dev).repeat(nb)[:, None].to(t.dtype))), False)
    return nb, heads, S, C


def _attn_chunks(nb, heads, S):
    """(sample, head range) pieces whose float64 score matrices stay below ~1.5 GB"""
    hs = max(1, min(heads, int(1.5e9 // (8 * S * S))))
    return [(b, h0, min(heads, h0 + hs)) for b in range(nb) for h0 in range(0, heads, hs)]


def _attn_derived_o(ref, Spv, smax, S, dt, hd=64):
    """o = P V with P = exp(s - lse): P is rounded to the activation type before the matrix unit takes it (one rounding of every term of
    P|V|), the normaliser is a sum of the same P (another 2^-p of |o| <= P|V|), fp32 accumulation of S + 64 terms, an error of
    (64 + 2) 2^-23 max|q||k| scale in a score moves P by as much relatively (twice: numerator and normaliser), and the output is rounded."""
    return (2 * _UA[dt] + (S + hd + 2 * (hd + 2) * smax[..., None]) * 2.0 ** -23) * Spv + _half_ulp_after(ref, 2 * _UA[dt], dt)


@runner("attn_fwd")
def run_attn_fwd(be, o, a):
    nb, heads, S, C = _attn_decl(o, a)
    o.out("o", nb * S, C, a["ld_o"])
    o.out("lse", 1, nb * heads * S)
    o.alloc()
    _launch(be, o)
    dt, sc = o.dtype("q"), a["scale"]
    q, k, v = (_hv(o[n], nb, S, heads, a["ld"]) for n in ("q", "k", "v"))
    got_o, got_l = _hv(o["o"], nb, S, heads, a["ld_o"]), o["lse"].view(nb, heads, S)
    wo, wl, rm = (0.0, ()), (0.0, ()), RoundingMeans()
    for b in range(nb):
        parts = [ref64.attention(q[b, h0:h1], k[b, h0:h1], v[b, h0:h1], sc) for _, h0, h1 in _attn_chunks(1, heads, S)]
        ref, lse, Spv, smax = (torch.cat([p[i] for p in parts], 0) for i in range(4))
        bar = tol_for(dt, 2) * ref.abs().amax((0, 2), keepdim=True).expand_as(ref)          # a row of the output holds all heads
        bound = torch.maximum(torch.minimum(bar, _attn_derived_o(ref, Spv, smax, S, dt)), 0.5 * ulp_of(ref, dt))
        w = _worst(_ratio(got_o[b], ref, bound))
        wo = max(wo, (w[0], (b,) + w[1]))
        rm.add(got_o[b], ref, dt)
        # lse = log sum exp(s): the score error above, the relative error of a sum of S positive terms, exp / log to 4 spacings
        lb = (66 * smax + S + 8) * 2.0 ** -23 * (1 + lse.abs()) + 0.5 * ulp_of(lse, torch.float32)
        w = _worst(_ratio(got_l[b], lse, lb.clamp(max=2e-2)))
        wl = max(wl, (w[0], (b,) + w[1]))
    res = [("o",) + wo, ("lse",) + wl]
    rm.report(res, "o")
    if S >= 160:
        res.append(("the operands drive the deferred rescale", 0.0 if _rescale_driven(q[0, 0], k[0, 0], sc) else float("inf"), ()))
    return res


RESCALE_THR_LOG2, KEY_TILE = 8.0, 64         # csrc/attention.hip: RESCALE_THR, keys per tile of the forward kernel


def _rescale_driven(q, k, scale):
    """whether some query row's key-tile maximum (log2 units) exceeds the reference maximum it kept by more than the threshold"""
    s = (ref64.d(q) @ ref64.d(k).t()) * (scale * math.log2(math.e))
    tm = torch.stack([c.amax(1) for c in torch.split(s, KEY_TILE, 1)], 1)
    ref, hit = tm[:, 0].clone(), False
    for t in range(1, tm.shape[1]):
        jump = tm[:, t] - ref > RESCALE_THR_LOG2
        hit = hit or bool(jump.any())
        ref = torch.where(jump, tm[:, t], ref)
    return hit


@runner("attn_bwd_prep")
def run_attn_bwd_prep(be, o, a):
    nb, heads, S, ld_o = a["nb"], a["heads"], a["S"], a["ld_o"]
    o.mat("o", nb * S, heads * 64, ld_o)
    o.mat("d_o", nb * S, heads * 64, ld_o)
    o.out("D", 1, nb * heads * S)
    o.alloc()
    _launch(be, o)
    x, y = ref64.d(_hv(o["o"], nb, S, heads, ld_o)), ref64.d(_hv(o["d_o"], nb, S, heads, ld_o))
    res = []
    judge_single(res, "D", o["D"].view(nb, heads, S), (x * y).sum(-1), (x * y).abs().sum(-1), 64, 1)
    return res


def _attn_bwd(be, o, a, outs):
    """dq / dk / dv: P and dS = P (dP - D) are rounded to the activation type before the matrix unit takes them (2^-p of every term of
    the magnitude sums below), fp32 accumulation over S or 64 terms, one output rounding; lse and D come in as fp32.  Bound: the smaller
    of that and today's bar tol_for(dt, 4) on the row's own maximum -- plus the cancellation term.

    Cancellation term.  D_i = sum_c o_ic dO_ic enters as the step forms it (svdx_attn_bwd_prep): from the o the forward STORED, rounded to
    the activation type, while the float64 reference differentiates the unrounded o.  Per element |o~ - o| <= 2^-p |o| (+ half of fp16's
    subnormal spacing), so |D~_i - D_i| <= cD_i = sum_c (2^-p |o_ic| + sub) |dO_ic|.  dS_ij = P_ij (dP_ij - D_i) moves by P_ij cD_i, and
    the final products carry it to  dq_i: scale cD_i sum_j P_ij |k_j|,  dk_j: scale sum_i P_ij cD_i |q_i|  (dv does not read D).  No kernel
    can do better on these operands, whatever the reference's own magnitude -- with ONE key P = 1 and dS is exactly 0 in float64, every
    implementation returns this residue, and a bar on the row's own maximum (0) has no room for it -- so the term is added after the
    bar's ceiling, at every S, with the rounding of the result it moves (1 + 2 * 2^-p)."""
    nb, heads, S, C = _attn_decl(o, a)
    ld, ld_o, ld_d, sc, dt = a["ld"], a["ld_o"], a["ld_d"], a["scale"], o.dtype("q")
    o.mat("d_o", nb * S, C, ld_o)
    q, k, v, do = (lambda: _hv(o["q"], nb, S, heads, ld)), (lambda: _hv(o["k"], nb, S, heads, ld)), (lambda: _hv(o["v"], nb, S, heads, ld)), \
        (lambda: _hv(o["d_o"], nb, S, heads, ld_o))

    def fill_lse(t):
        for b, h0, h1 in _attn_chunks(nb, heads, S):
            t.view(nb, heads, S)[b, h0:h1] = ref64.attention(q()[b, h0:h1], k()[b, h0:h1], v()[b, h0:h1], sc)[1]

    def fill_D(t):
        for b, h0, h1 in _attn_chunks(nb, heads, S):
            ref = ref64.attention(q()[b, h0:h1], k()[b, h0:h1], v()[b, h0:h1], sc)[0].to(dt)        # o as svdx_attn_fwd stores it
            t.view(nb, heads, S)[b, h0:h1] = (ref64.d(ref) * ref64.d(do()[b, h0:h1])).sum(-1)
    o.decl("lse", nb * heads * S, fill_lse)
    o.decl("D", nb * heads * S, fill_D)
    for nm in outs:
        o.out(nm, nb * S, C, ld_d)
    o.alloc()
    _launch(be, o)
    worst, rms = {nm: (0.0, ()) for nm in outs}, {nm: RoundingMeans() for nm in outs}
    sub = 2.0 ** -25 if dt == torch.float16 else 0.0     # half of fp16's subnormal spacing: the absolute floor of one rounded P / dS term
    for b in range(nb):
        acc = {nm: [[], [], []] for nm in outs}
        for _, h0, h1 in _attn_chunks(1, heads, S):
            qq, kk, vv, dd = (ref64.d(t()[b, h0:h1]) for t in (q, k, v, do))
            dq, dk, dv, _ = ref64.attention_bwd(qq, kk, vv, dd, sc)
            p = torch.softmax((qq @ kk.transpose(-1, -2)) * sc, -1)
            Dv = (p * (dd @ vv.transpose(-1, -2))).sum(-1, keepdim=True)
            ads = p * (dd.abs() @ vv.abs().transpose(-1, -2) + Dv.abs())
            one = torch.ones(h1 - h0, S, 1, dtype=torch.float64, device=o.dev)
            cD = ((_UA[dt] * (p @ vv).abs() + sub) * dd.abs()).sum(-1, keepdim=True) * (1 + 2 * _UA[dt])
            canc = dict(dq=sc * cD * (p @ kk.abs()), dk=sc * ((p * cD).transpose(-1, -2) @ qq.abs()), dv=None)
            mags = dict(dq=(dq, sc * (ads @ kk.abs()), sc * kk.abs().sum(1, keepdim=True) * one), dk=(dk, sc * (ads.transpose(-1, -2) @ qq.abs()), sc * qq.abs().sum(1, keepdim=True) * one),
                        dv=(dv, p.transpose(-1, -2) @ dd.abs(), dd.abs().sum(1, keepdim=True) * one))
            for nm in outs:
                ref, Sm, fl = mags[nm]
                r = 2 if nm == "dv" else 3
                acc[nm][0].append(ref)
                acc[nm][1].append((r * _UA[dt] + (S + 3 * 64 + 8) * 2.0 ** -23) * Sm + sub * fl)
                acc[nm][2].append(torch.zeros_like(ref) if canc[nm] is None else canc[nm])
            del p, ads, canc
        for nm in outs:
            ref, derived, cterm = (torch.cat(x, 0) for x in acc[nm])
            r = 2 if nm == "dv" else 3
            bar = tol_for(dt, 4) * ref.abs().amax((0, 2), keepdim=True).expand_as(ref)          # a row holds all heads
            bound = torch.maximum(torch.minimum(bar, derived + _half_ulp_after(ref, r * _UA[dt], dt)) + cterm, 0.5 * ulp_of(ref, dt))
            w = _worst(_ratio(_hv(o[nm], nb, S, heads, ld_d)[b], ref, bound))
            worst[nm] = max(worst[nm], (w[0], (b,) + w[1]))
            rms[nm].add(_hv(o[nm], nb, S, heads, ld_d)[b], ref, dt)
    res = [(nm,) + worst[nm] for nm in outs]
    for nm in outs:
        rms[nm].report(res, nm)
    return res


@runner("attn_bwd_dkv")
def run_attn_bwd_dkv(be, o, a):
    return _attn_bwd(be, o, a, ("dk", "dv"))


@runner("attn_bwd_dq")
def run_attn_bwd_dq(be, o, a):
    return _attn_bwd(be, o, a, ("dq",))


def _tv(t, B, T, HW, heads, ld):
    return torch.as_strided(t, (B, HW, heads, T, 64), (T * HW * ld, ld, 64, HW * ld, 1), t.storage_offset())


def _judge_tattn_o(res, label, got, q, k, v, sc, T, dt, mult):
    ref, _, Spv, smax = ref64.attention(q, k, v, sc)
    bar = tol_for(dt, mult) * ref.abs().amax((2, 4), keepdim=True).expand_as(ref)        # a row = one (frame, pixel) over heads and channels
    bound = torch.maximum(torch.minimum(bar, _attn_derived_o(ref, Spv, smax, T, dt)), 0.5 * ulp_of(ref, dt))
    res.append((label,) + _worst(_ratio(got, ref, bound)))
    RoundingMeans().add(got, ref, dt).report(res, label)


@runner("tattn_fwd")
def run_tattn_fwd(be, o, a):
    B, T, HW, heads, ld = a["B"], a["T"], a["HW"], a["heads"], a["ld"]
    M, C = B * T * HW, heads * 64
    for nm in ("q", "k", "v"):
        o.mat(nm, M, C, ld)
    o.out("o", M, C, a["ld_o"])
    o.alloc()
    _launch(be, o)
    res = []
    q, k, v = (_tv(o[n], B, T, HW, heads, ld) for n in ("q", "k", "v"))
    _judge_tattn_o(res, "o", _tv(o["o"], B, T, HW, heads, a["ld_o"]), q, k, v, a["scale"], T, o.dtype("q"), 1)
    return res


@runner("tattn_bwd")
def run_tattn_bwd(be, o, a):
    """as the spatial backward (P and dS rounded to the activation type, fp32 sums over T or 64 terms, output rounding); bar tol_for(dt, 2)"""
    B, T, HW, heads, ld, ld_d, sc = a["B"], a["T"], a["HW"], a["heads"], a["ld"], a["ld_d"], a["scale"]
    M, C, dt = B * T * HW, heads * 64, o.dtype("q")
    for nm in ("q", "k", "v"):
        o.mat(nm, M, C, ld)
    o.mat("d_o", M, C, a["ld_o"])
    for nm in ("dq", "dk", "dv"):
        o.out(nm, M, C, ld_d)
    o.alloc()
    _launch(be, o)
    qq, kk, vv = (ref64.d(_tv(o[n], B, T, HW, heads, ld)) for n in ("q", "k", "v"))
    dd = ref64.d(_tv(o["d_o"], B, T, HW, heads, a["ld_o"]))
    dq, dk, dv, _ = ref64.attention_bwd(qq, kk, vv, dd, sc)
    p = torch.softmax((qq @ kk.transpose(-1, -2)) * sc, -1)
    Dv = (p * (dd @ vv.transpose(-1, -2))).sum(-1, keepdim=True)
    ads = p * (dd.abs() @ vv.abs().transpose(-1, -2) + Dv.abs())
    res = []
    for nm, ref, Sm, r in (("dq", dq, sc * (ads @ kk.abs()), 3), ("dk", dk, sc * (ads.transpose(-1, -2) @ qq.abs()), 3),
                           ("dv", dv, p.transpose(-1, -2) @ dd.abs(), 2)):
        bar = tol_for(dt, 2) * ref.abs().amax((2, 4), keepdim=True).expand_as(ref)
        derived = (r * _UA[dt] + (T + 3 * 64 + 8) * 2.0 ** -23) * Sm + _half_ulp_after(ref, r * _UA[dt], dt)
        bound = torch.maximum(torch.minimum(bar, derived), 0.5 * ulp_of(ref, dt))
        res.append((nm,) + _worst(_ratio(_tv(o[nm], B, T, HW, heads, ld_d), ref, bound)))
        RoundingMeans().add(_tv(o[nm], B, T, HW, heads, ld_d), ref, dt).report(res, nm)
    return res


@runner("tsa_fwd")
def run_tsa_fwd(be, o, a):
    """One launch, four stages, each judged from what the launch stored for the previous one: n1 = LayerNorm(x) (single rounding);
    q/k/v = n1 Wqkv^T from the n1 it wrote (single rounding, K = C); o = attention over frames from its q/k/v (bar tol_for(dt, 2));
    h1 = o Wo^T + bo + cvec + x from its o (single rounding)."""
    B, T, HW, C, heads = a["B"], a["T"], a["HW"], a["C"], a["heads"]
    M, dt = B * T * HW, o.dtype("x")
    o.decl("x", M * C, lambda t: (_v(t, M, C, C).copy_(o.randn(M, C)), _v(t, M, C, C)[:, :8].add_(3.0)))
    o.vec("gamma", C, scale=0.1, shift=1.0)
    o.vec("beta", C, scale=0.1)
    o.decl("wqkv", 3 * C * C, lambda t: (_v(t, 3 * C, C, C).copy_(o.randn(3 * C, C, scale=C ** -0.5)), _v(t, C, C, C).mul_(2.0)))
    o.mat("wo", C, C, scale=C ** -0.5)
    o.vec("bo", C, scale=0.1)
    ng = _n_groups(M, a["rv_rpg"], a["rv_mod"]) if a["cvec"] is not None else 0
    if ng:
        o.mat("cvec", ng, C, a["rv_ld"])
    for nm, cols in (("n1", C), ("stats", 2), ("qkv", 3 * C), ("o", C), ("h1", C)):
        o.out(nm, M, cols)
    o.alloc()
    _launch(be, o, dict(qkv=o["qkv"].view(M, 3 * C)))        # (the emulation slices its q / k / v out of a matrix)
    res = []
    x = _v(o["x"], M, C, C)
    y, mean, rstd, S = ref64.ln_fwd(x, o["gamma"], o["beta"], a["eps"])
    if o["n1"] is not None:
        n1 = _v(o["n1"], M, C, C)
        judge_single(res, "n1", n1, y, S, C, 8)
    else:
        n1 = y.to(dt)
    _judge_ln_stats(res, "stats", o["stats"], x, mean, rstd, M, C)
    qkv = _v(o["qkv"], M, 3 * C, 3 * C)
    v, S, ka, e = ref64.gemm_nt(n1, _v(o["wqkv"], 3 * C, C, C), M)
    if o["n1"] is not None:
        judge_single(res, "qkv (from the n1 it wrote)", qkv, v, S, ka, e)
    else:
        judge_rows(res, "qkv", qkv, v, tol_for(dt, 2))
    q, k, vv = (_tv(qkv[:, i * C:], B, T, HW, heads, 3 * C) for i in range(3))
    _judge_tattn_o(res, "o (from the q/k/v it wrote)", _tv(o["o"], B, T, HW, heads, C), q, k, vv, a["scale"], T, dt, 2)
    v, S, ka, e = ref64.gemm_nt(_v(o["o"], M, C, C), _v(o["wo"], C, C, C), M, bias=o["bo"], rowvec=_v(o["cvec"], ng, C, a["rv_ld"]) if ng else None,
                                rv_rpg=a["rv_rpg"], rv_mod=a["rv_mod"], res=x)
    judge_single(res, "h1 (from the o it wrote)", _v(o["h1"], M, C, C), v, S, ka, e)
    return res


# ---- elementwise ---------------------------------------------------------------------------------------------------------------------------
@runner("add")
def run_add(be, o, a):
    n = a["n"]
    o.mat("a", 1, n)
    o.mat("b", 1, n)
    o.out("out", 1, n)
    o.alloc()
    _launch(be, o)
    x, y = ref64.d(o["a"]), ref64.d(o["b"])
    res = []
    judge_single(res, "out", o["out"], x + y, x.abs() + y.abs(), 0, 1)
    return res


@runner("blend")
def run_blend(be, o, a):
    n = a["n"]
    o.mat("a", 1, n)
    o.mat("b", 1, n)
    o.vec("mix", 1)
    o.out("out", 1, n)
    o.alloc()
    _launch(be, o)
    al = torch.sigmoid(ref64.d(o["mix"]))
    x, y = ref64.d(o["a"]), ref64.d(o["b"])
    res = []
    judge_single(res, "out", o["out"], al * x + (1 - al) * y, al * x.abs() + (1 - al) * y.abs(), 0, 8)     # sigmoid, 1 - alpha, two products, one sum
    return res


@runner("blend_bwd")
def run_blend_bwd(be, o, a):
    n = a["n"]
    o.mat("dy", 1, n)
    o.vec("mix", 1)
    o.out("da", 1, n)
    o.out("db", 1, n)
    o.alloc()
    _launch(be, o)
    al = torch.sigmoid(ref64.d(o["mix"]))
    dy = ref64.d(o["dy"])
    res = []
    if o["da"] is not None:
        judge_single(res, "da", o["da"], al * dy, (al * dy).abs(), 0, 6)
    judge_single(res, "db", o["db"], (1 - al) * dy, (1 - al) * dy.abs(), 0, 6)
    return res


@runner("add_rowvec")
def run_add_rowvec(be, o, a):
    rows, C = a["rows"], a["C"]
    ng = _n_groups(rows, a["rpg"], a["mod"])
    o.mat("x", rows, C)
    o.mat("vec", ng, C, a["rv_ld"])
    o.out("out", rows, C)
    o.alloc()
    _launch(be, o)
    x = ref64.d(_v(o["x"], rows, C, C))
    v = ref64.d(_v(o["vec"], ng, C, a["rv_ld"]))[ref64.group_index(rows, a["rpg"], a["mod"], o.dev)]
    res = []
    judge_single(res, "out", _v(o["out"], rows, C, C), x + v, x.abs() + v.abs(), 0, 1)
    return res


@runner("concat2")
def run_concat2(be, o, a):
    rows, Ca, Cb = a["rows"], a["Ca"], a["Cb"]
    o.mat("a", rows, Ca)
    o.mat("b", rows, Cb)
    o.out("out", rows, Ca + Cb)
    o.alloc()
    _launch(be, o)
    res = []
    judge_exact(res, "out", _v(o["out"], rows, Ca + Cb, Ca + Cb), torch.cat([_v(o["a"], rows, Ca, Ca), _v(o["b"], rows, Cb, Cb)], 1))
    return res


@runner("split2")
def run_split2(be, o, a):
    rows, Ca, Cb = a["rows"], a["Ca"], a["Cb"]
    o.mat("inp", rows, Ca + Cb)
    o.out("a", rows, Ca)
    o.out("b", rows, Cb)
    o.alloc()
    _launch(be, o)
    i = _v(o["inp"], rows, Ca + Cb, Ca + Cb)
    res = []
    judge_exact(res, "a", _v(o["a"], rows, Ca, Ca), i[:, :Ca])
    judge_exact(res, "b", _v(o["b"], rows, Cb, Cb), i[:, Ca:])
    return res


@runner("sum2x2")
def run_sum2x2(be, o, a):
    n_img, h, w, C = a["n_img"], a["h"], a["w"], a["C"]
    o.mat("inp", n_img * 4 * h * w, C)
    o.out("out", n_img * h * w, C)
    o.alloc()
    _launch(be, o)
    x = ref64.d(o["inp"]).view(n_img, 1, 2 * h, 2 * w, C).permute(0, 4, 1, 2, 3).reshape(n_img * C, 1, 2 * h, 2 * w)
    pool = lambda t: (4 * torch.nn.functional.avg_pool2d(t, 2)).view(n_img, C, h * w).permute(0, 2, 1).reshape(n_img * h * w, C)
    res = []
    judge_single(res, "out", _v(o["out"], n_img * h * w, C, C), pool(x), pool(x.abs()), 4, 0)
    return res


@runner("nchw_to_rows")
def run_nchw_to_rows(be, o, a):
    n_img, C, H, W, ld, mul = a["n_img"], a["C"], a["H"], a["W"], a["ld"], a["mul"]
    o.mat("inp", 1, n_img * C * H * W)
    o.out("out", n_img * H * W, ld)
    o.alloc()
    _launch(be, o)
    x = ref64.d(o["inp"]).view(n_img, C, H * W).permute(0, 2, 1).reshape(-1, C) * mul
    ref = torch.zeros(n_img * H * W, ld, dtype=torch.float64, device=o.dev)          # the padding channels are written as zeros
    ref[:, :C] = x
    res = []
    judge_single(res, "out", _v(o["out"], n_img * H * W, ld, ld), ref, ref.abs(), 0, 1)
    return res


# ---- loss / optimizer ------------------------------------------------------------------------------------------------------------------
LOSS_SCALE = 1024.0


@runner("edm_loss")
def run_edm_loss(be, o, a):
    B, T, C, HW, ld = a["B"], a["T"], a["C"], a["HW"], a["ld"]
    M, n, ld_d = B * T * HW, B * T * C * HW, -(-C // 64) * 64                              # include/svdx.h: dpred rows have the padded pitch
    o.mat("pred", M, C, ld)
    o.mat("noisy", 1, n)
    o.mat("target", 1, n)
    o.vec("sigma", B, scale=1.0, shift=0.3, positive=True)
    o.out("loss", 1, 1, fill=1.0)                                                          # the loss is ADDED to its slot (micro-batches)
    o.out("dpred", M, ld_d)
    st = [0.0] * K.OPT_STATE_ALLOC
    st[1], st[4], st[5], st[6], st[8] = LOSS_SCALE, 1.0 / LOSS_SCALE, 1.0, 1.0, 1.0
    o.decl("opt_state", K.OPT_STATE_ALLOC, lambda t: t.copy_(torch.tensor(st)))
    o.alloc()
    _launch(be, o, dict(dpred=o["dpred"].view(M, ld_d)))                     # (the emulation reads the pitch off the tensor)
    p = ref64.d(_v(o["pred"], M, C, ld)).view(B, T, HW, C).permute(0, 1, 3, 2)
    loss, dp, S_loss, S_dp = ref64.edm_loss(p, o["noisy"].view(B, T, C, HW), o["target"].view(B, T, C, HW), o["sigma"], LOSS_SCALE)
    res = []
    # n weighted squares (6 fp32 operations each) summed in fp32 in some order, added to the slot
    judge_single(res, "loss", o["loss"], (loss + 1.0).reshape(1), (S_loss + 1.0).reshape(1), n + 1, 8)
    judge_single(res, "dpred", _v(o["dpred"], M, C, ld_d), dp.permute(0, 1, 3, 2).reshape(M, C), S_dp.permute(0, 1, 3, 2).reshape(M, C), 0, 12)
    return res


ADAM_STEP = 3


@runner("adamw_tiled")
def run_adamw_tiled(be, o, a):
    """fp32-master mode against torch.optim.AdamW on float64 at step 3 (the bias corrections go in through opt_state[5], [6] as the
    kernel reads them; opt_state[4] is the gradient factor, [8] the lr multiplier).  Every output element is a handful of fp32 operations:
    single-rounding bound with the magnitudes of its terms; the 16-bit copies are judged from the float parameter the launch wrote.
    param_mode 1 (bf16-reference recipe): torch.optim.AdamW on bf16 tensors, element for element up to ONE bf16 step on at most 2e-3 of
    the elements (tests/kernel_checks.py check_optim's bar: a float scalar of the device vs torch's double in the last place)."""
    tiles = o.table("tiles").view(-1, 6)[:a["n_tiles"]]
    n = int((tiles[:, 0] + (tiles[:, 2] - 1) * tiles[:, 1] + tiles[:, 3]).max())
    has_t = tiles[:, 4] >= 0
    nt = int((tiles[:, 4] + (tiles[:, 3] - 1) * tiles[:, 5] + tiles[:, 2])[has_t].max()) if bool(has_t.any()) else 1
    ref_mode = a["param_mode"] == K.PARAMS_BF16_REFERENCE
    rb = (lambda t: t.to(torch.bfloat16).float()) if ref_mode else (lambda t: t)
    o.decl("p", n, lambda t: t.copy_(rb(o.randn(n, scale=0.05))))
    o.decl("g", n, lambda t: t.copy_(rb(o.randn(n, scale=0.3))))
    o.decl("m", n, lambda t: t.copy_(rb(o.randn(n, scale=0.03))))
    o.decl("v", n, lambda t: t.copy_(rb(o.randn(n, scale=0.03).pow(2) + 1e-4)))
    o.out("p_act", 1, n)
    o.out("pt_act", 1, nt)
    b1, b2, gm, lrm = a["beta1"], a["beta2"], 0.5, 0.75
    st = [0.0] * K.OPT_STATE_ALLOC
    st[0], st[1], st[4], st[5], st[6], st[8] = float(ADAM_STEP), 1.0 / gm, gm, 1 - b1 ** ADAM_STEP, 1 - b2 ** ADAM_STEP, lrm
    if ref_mode:
        st[4] = gm = 1.0
    o.decl("opt_state", K.OPT_STATE_ALLOC, lambda t: t.copy_(torch.tensor(st)))
    o.alloc()
    p0, m0, v0, g0 = (o[nm].clone() for nm in ("p", "m", "v", "g"))
    _launch(be, o, dict(tiles=o["tiles"].view(-1, 6)))
    res = []
    cover = torch.zeros(n, dtype=torch.bool, device=o.dev)
    tl = tiles.to(o.dev)
    rr, cc = torch.meshgrid(torch.arange(64, device=o.dev), torch.arange(64, device=o.dev), indexing="ij")
    worst = collections.defaultdict(lambda: (0.0, ()))

    def note(label, ratio, base=0):
        w = _worst(ratio)
        if w[0] > worst[label][0]:
            worst[label] = (w[0], tuple(base + i for i in w[1]))
    for t0 in range(0, tl.shape[0], 8192):                 # the elements of 8192 tiles at a time (and of their transposed twins)
        t = tl[t0:t0 + 8192]
        live = (rr[None] < t[:, 2, None, None]) & (cc[None] < t[:, 3, None, None])
        idx = (t[:, 0, None, None] + rr[None] * t[:, 1, None, None] + cc[None])[live]
        cover[idx] = True
        if o["pt_act"] is not None:
            tw = (t[:, 4] >= 0)[:, None, None] & live
            src = (t[:, 0, None, None] + rr[None] * t[:, 1, None, None] + cc[None])[tw]
            dst = (t[:, 4, None, None] + cc[None] * t[:, 5, None, None] + rr[None])[tw]
            pw = ref64.d(o["p"][src])
            note("transposed twin (from the p it wrote)", _ratio(o["pt_act"][dst], pw, 0.5 * ulp_of(pw, o["pt_act"].dtype)))
    gmul = gm * a["grad_mul"]
    lr = a["lr"] * lrm
    CH = 1 << 26
    for i0 in range(0, n, CH):
        sl = slice(i0, min(n, i0 + CH))
        cv = cover[sl]
        if ref_mode:
            ps = torch.nn.Parameter(p0[sl].cpu().to(torch.bfloat16))            # torch's CPU kernels: the op sequence the recipe is pinned to
            ps.grad = (g0[sl] * gmul).cpu().to(torch.bfloat16)
            opt = torch.optim.AdamW([ps], lr=lr, betas=(b1, b2), eps=a["eps"], weight_decay=a["wd"], foreach=False)
            opt.state[ps] = dict(step=torch.tensor(float(ADAM_STEP - 1)), exp_avg=m0[sl].cpu().to(torch.bfloat16), exp_avg_sq=v0[sl].cpu().to(torch.bfloat16))
            opt.step()
            for nm, ref in (("p", ps.detach()), ("m", opt.state[ps]["exp_avg"]), ("v", opt.state[ps]["exp_avg_sq"])):
                got, ref = o[nm][sl][cv], ref.float().to(o.dev)[cv]
                note(f"{nm} stays bf16-valued", _ratio(got, got.to(torch.bfloat16).double(), torch.zeros_like(got, dtype=torch.float64)), i0)
                off = (got != ref)
                worst[f"{nm}: elements off torch's bf16 AdamW / 2e-3"] = (worst[f"{nm}: elements off torch's bf16 AdamW / 2e-3"][0] + float(off.sum()) / max(1, int(cover.sum())) / 2e-3, ())
                note(f"{nm}: largest deviation / one bf16 step", (got - ref).abs().double() / ulp_of(torch.maximum(got.abs(), ref.abs()).double(), torch.bfloat16), i0)
        else:
            pr, mr, vr = ref64.adamw_step(p0[sl], ref64.d(g0[sl]) * gmul, m0[sl], v0[sl], lr, b1, b2, a["eps"], a["wd"], ADAM_STEP)
            g64 = (ref64.d(g0[sl]) * gmul).abs()
            # fp32 roundings, counted: g * factor (1, carried by both moments); m = b1 m + (1 - b1) g: the two coefficients, two products,
            # one sum: 5 + 1 = 6 of S_m; v: the same with g * g: 7 + 1 = 8 of S_v; p = p * (1 - lr wd) - step * m / (sqrt(v) / sqrt(bc2) + eps):
            # lr * multiplier, lr * wd, 1 - .., the product, the final subtraction: 5 of |p|; the update: m (6), v through its square root
            # (8 / 2), sqrt, bias correction (2: rsqrt, product), + eps, lr / bc1, times m, division: 6 + 4 + 7 = 17 of its magnitude sum
            # S_u = step S_m / denominator (m may cancel: its error does not)
            Sm = b1 * ref64.d(m0[sl]).abs() + (1 - b1) * g64
            Su = lr / (1 - b1 ** ADAM_STEP) * Sm / (vr.sqrt() / math.sqrt(1 - b2 ** ADAM_STEP) + a["eps"])
            for nm, ref, S in (("m", mr, 6 * Sm), ("v", vr, 8 * (b2 * ref64.d(v0[sl]).abs() + (1 - b2) * g64 * g64)),
                               ("p", pr, 5 * ref64.d(p0[sl]).abs() + 17 * Su)):
                note(nm, _ratio(o[nm][sl][cv], ref[cv], 0.5 * ulp_of(ref[cv], torch.float32) + 2.0 ** -23 * S[cv]), i0)
            del pr, mr, vr, g64, Sm, Su
        for nm, orig in (("p", p0), ("m", m0), ("v", v0)):
            note(f"{nm} outside the tiles untouched", (o[nm][sl][~cv] != orig[sl][~cv]).double() * float("inf") if bool((o[nm][sl][~cv] != orig[sl][~cv]).any()) else torch.zeros(1), i0)
        if o["p_act"] is not None:
            pw = ref64.d(o["p"][sl][cv])
            got = o["p_act"][sl][cv]
            note("p_act (from the p it wrote)", _ratio(got, pw, 0.5 * ulp_of(pw, got.dtype)), i0)
            if not ref_mode and i0 == 0:
                n_sel, m1, m2 = rounding_means(got, pw, got.dtype)
                if n_sel >= ROUNDING_MIN_ELEMENTS:
                    res.append(("p_act rounding: mean signed error / ulp", abs(m1) / ROUNDING_MEAN_BOUND, ()))
                    res.append(("p_act rounding: mean magnitude error / ulp", abs(m2) / ROUNDING_MEAN_BOUND, ()))
    return res + [(k,) + v for k, v in worst.items()]


@runner("grad_sumsq_spans")
def run_grad_sumsq_spans(be, o, a):
    spans = o.table("spans").view(-1, 3)[:a["n_spans"]]
    n = int((spans[:, 0] + spans[:, 1]).max())
    o.mat("g", 1, n)
    o.out("partial", 1, a["n_spans"])
    o.alloc()
    _launch(be, o, dict(spans=o["spans"].view(-1, 3)))
    g2 = ref64.d(o["g"]).pow(2)
    cs = torch.cat([torch.zeros(1, dtype=torch.float64, device=o.dev), g2.cumsum(0)])
    lo, hi = spans[:, 0].to(o.dev), (spans[:, 0] + spans[:, 1]).to(o.dev)
    ref = torch.stack([g2[l:h].sum() for l, h in zip(lo.tolist(), hi.tolist())]) if len(lo) <= 64 else cs[hi] - cs[lo]
    # float64 accumulation of `count` squares (each exact in float64); the cumulative-sum reference adds n 2^-52 of the running total
    bound = (spans[:, 1].to(o.dev).double() + 2) * 2.0 ** -52 * ref + (n * 2.0 ** -52 * cs[-1] if len(lo) > 64 else 0.0)
    return [("partial",) + _worst(_ratio(o["partial"], ref, bound))]


@runner("grad_clip_coef")
def run_grad_clip_coef(be, o, a):
    """(total_norm, coef) and opt_state[4] *= coef from the per-span float64 sums: sqrt of their float64 total times the unscale factor,
    coef = min(1, max_norm / (norm + 1e-6)) -- clip_grad_norm_'s arithmetic -- rounded to fp32: a few fp32 roundings of the results."""
    ns, nt = a["n_spans"], a["n_tensors"]
    assert a["param_mode"] == K.PARAMS_F32, "the bf16-reference recipe of the coefficient is pinned by tests/test_clip_grad_norm.py"
    o.table("spans")
    o.decl("partial", ns, lambda t: t.copy_(o.randn(ns).double().pow(2) * 30.0))
    inv = 1.0 / LOSS_SCALE
    st = [0.0] * K.OPT_STATE_ALLOC
    st[0], st[1], st[4], st[5], st[6], st[8] = 3.0, LOSS_SCALE, inv, 1.0, 1.0, 1.0
    o.decl("opt_state", K.OPT_STATE_ALLOC, lambda t: t.copy_(torch.tensor(st)))
    o.out("out", 1, 2)
    o.alloc()
    o["partial"].mul_(LOSS_SCALE ** 2 / a["grad_mul"] ** 2)
    _launch(be, o, dict(spans=o["spans"].view(-1, 3)))
    norm = torch.sqrt(o["partial"].sum()) * (inv * a["grad_mul"])
    coef = torch.clamp(a["max_norm"] / (norm + 1e-6), max=1.0)
    ref = torch.stack([norm, coef])
    res = [("out (norm, coef)",) + _worst(_ratio(o["out"], ref, 4 * ulp_of(ref, torch.float32))),
           ("opt_state[4] *= coef",) + _worst(_ratio(o["opt_state"][4:5], (inv * coef).reshape(1), 4 * ulp_of((inv * coef).reshape(1), torch.float32)))]
    keep = [i for i in range(K.OPT_STATE_ALLOC) if i != 4]
    judge_exact(res, "the rest of opt_state untouched", o["opt_state"][keep], torch.tensor(st, device=o.dev)[keep])
    return res


# ---- memsets -------------------------------------------------------------------------------------------------------------------------------
def _all_bits_zero(t):
    return bool((t.contiguous().view(torch.uint8) == 0).all())


@runner("zero")
def run_zero(be, o, a):
    """every byte of the tensor is zero afterwards (a -0.0 is not); the guard bands either side are run_case's check"""
    n = a["t"][4]
    o.decl("t", n, lambda t: t.fill_(1.0), out=True)
    o.alloc()
    _launch(be, o)
    return [("all bytes zero", 0.0 if _all_bits_zero(o["t"]) else float("inf"), ())]


@runner("zero_spans")
def run_zero_spans(be, o, a):
    """include/svdx.h: spans int32 [n_spans, 2] (offset, count in floats, count a multiple of 4): those floats are zero bytes afterwards,
    every other float of the buffer keeps its value"""
    spans = o.table("spans").view(-1, 2)[:a["n_spans"]]
    n = int((spans[:, 0] + spans[:, 1]).max())
    o.decl("base", n, lambda t: t.fill_(1.0), out=True)
    o.alloc()
    _launch(be, o, dict(spans=o["spans"].view(-1, 2)))
    inside = torch.zeros(n + 1, dtype=torch.int32, device=o.dev)
    inside.index_add_(0, spans[:, 0].to(o.dev), torch.ones(len(spans), dtype=torch.int32, device=o.dev))
    inside.index_add_(0, (spans[:, 0] + spans[:, 1]).to(o.dev), -torch.ones(len(spans), dtype=torch.int32, device=o.dev))
    inside = inside.cumsum(0)[:n] > 0
    bits = o["base"].view(torch.int32)
    return [("spans: all bytes zero", 0.0 if bool((bits[inside] == 0).all()) else float("inf"), ()),
            ("outside the spans untouched", 0.0 if bool((o["base"][~inside] == 1.0).all()) else float("inf"), ())]


# ---- the inf check and the loss-scale state machine ------------------------------------------------------------------------------------------
STATE_FILL = 7.0           # what the state floats a finite check must not touch are pre-filled with
NON_FINITE = (float("inf"), float("-inf"), float("nan"))


def _finite_check(be, o, g_name, n, place, overrides=None):
    """a finite buffer leaves opt_state[3] at 0; one non-finite float at `place` raises it; the rest of the state is never written"""
    o.vec(g_name, n)
    o.decl("opt_state", K.OPT_STATE_ALLOC, lambda t: t.fill_(STATE_FILL), out=True)
    o.alloc()
    want = torch.full((K.OPT_STATE_ALLOC,), STATE_FILL, device=o.dev)
    res = []
    for planted in (False, True):
        o["opt_state"][3] = 0.0
        want[3] = 1.0 if planted else 0.0
        if planted:
            o[g_name][place] = NON_FINITE[sig_seed(o.sig) % 3]
        _launch(be, o, overrides() if overrides else None)
        judge_exact(res, f"found_inf raised by the float at {place}" if planted else "found_inf stays 0", o["opt_state"], want)
    return res


@runner("check_finite_spans")
def run_check_finite_spans(be, o, a):
    """the recorded span table; the planted float is element (seed / n_spans) mod count of span seed mod n_spans"""
    spans = o.table("spans").view(-1, 2)[:a["n_spans"]]
    off, cnt = spans[sig_seed(o.sig) % len(spans)].tolist()
    return _finite_check(be, o, "g", int((spans[:, 0] + spans[:, 1]).max()), off + (sig_seed(o.sig) // len(spans)) % cnt,
                         lambda: dict(spans=o["spans"].view(-1, 2)))


@runner("check_finite")
def run_check_finite(be, o, a):
    """the recorded n; the planted float is element seed mod n"""
    return _finite_check(be, o, "g", a["n"], sig_seed(o.sig) % a["n"])


@runner("optim_prep")
def run_optim_prep(be, o, a):
    """the recorded arguments from step 3 at scale 1024 (1 when static), found and not found, the growth tracker at 0 and one short of the
    interval: step, scale, tracker, the cleared flag, 1 / scale and the skip flag exact, the bias corrections and the schedule multiplier at
    tests/kernel_checks.check_optim's bars, against the float64 restatement of GradScaler's rule (tests/overflow_checks.grad_scaler_rule)"""
    import overflow_checks as oc
    from kernel_checks import relerr
    o.decl("opt_state", K.OPT_STATE_ALLOC, lambda t: t.zero_(), out=True)
    o.alloc()
    interval, dynamic = a["growth_interval"], a["dynamic"]
    b1, b2 = (float(torch.tensor(b, dtype=torch.float32)) for b in (a["beta1"], a["beta2"]))
    res = []
    for found in (False, True):
        for tracker in sorted({0.0, float(max(interval - 1, 0))}):
            scale = 1024.0 if dynamic else 1.0
            st = [3.0, scale, tracker, 1.0 if found else 0.0, STATE_FILL, STATE_FILL, STATE_FILL, STATE_FILL, STATE_FILL] + [0.0] * 7
            st += [STATE_FILL] * (K.OPT_STATE_ALLOC - len(st))
            o["opt_state"].copy_(torch.tensor(st))
            _launch(be, o)
            got = o["opt_state"].cpu()
            s1, t1 = oc.grad_scaler_rule(scale, tracker, found, interval, dynamic, a["growth"], a["backoff"])
            step = 3.0 if found else 4.0
            label = f"found={found} tracker={tracker:g}: "
            judge_exact(res, label + "step, scale, tracker, found_inf, 1 / scale", got[:5], torch.tensor([step, s1, t1, 0.0, 1.0 / scale], dtype=torch.float32))
            judge_exact(res, label + "skip", got[7:8], torch.tensor([1.0 if found else 0.0]))
            bc = torch.tensor([1.0 - b1 ** step, 1.0 - b2 ** step], dtype=torch.float64)
            res.append((label + "bias corrections", relerr(got[5:7], bc) / 1e-5, ()))
            res.append((label + "lr multiplier (constant schedule)", abs(float(got[8]) - 1.0) / 5e-6, ()))
            judge_exact(res, label + "schedule and rule floats untouched", got[9:], torch.tensor(st[9:]))
    return res


# ---- the conditioners' own kernels (csrc/encoders.hip) and the layout passes --------------------------------------------------------------
@runner("patch_rows")
def run_patch_rows(be, o, a):
    """out = round(mul * in) at the im2col position: one product in fp32 (none when mul == 1: K_acc = 0, E = 1 / 0), one rounding.
    include/svdx.h: the columns C*kh*kw .. ldk are ZERO (the GEMM behind it reduces over them)."""
    n, C, H, W, kh, kw, ho, wo, ldk = (a[k] for k in ("n_img", "C", "H", "W", "kh", "kw", "ho", "wo", "ldk"))
    o.mat("inp", 1, n * C * H * W, scale=0.5)
    o.out("out", n * ho * wo, ldk)
    o.alloc()
    _launch(be, o)
    ref = ref64.patch_rows(o["inp"].view(n, C, H, W), kh, kw, a["stride"], a["pad"], ldk, a["mul"])
    got = _v(o["out"], n * ho * wo, ldk, ldk)
    res = []
    judge_single(res, "out", got, ref, ref.abs(), 0, 0 if a["mul"] == 1.0 else 1)
    kk = C * kh * kw
    if ldk > kk:
        judge_exact(res, "padding columns are zero", got[:, kk:], torch.zeros_like(got[:, kk:]))
    return res


@runner("transpose")
def run_transpose(be, o, a):
    rows, cols, ld_in, ld_out = a["rows"], a["cols"], a["ld_in"], a["ld_out"]
    o.mat("inp", rows, cols, ld_in)
    o.out("out", cols, ld_out)
    o.alloc()
    _launch(be, o)
    ref = torch.zeros(cols, ld_out, dtype=o.dtype("inp"), device=o.dev)
    ref[:, :rows] = _v(o["inp"], rows, cols, ld_in).t()
    res = []
    judge_exact(res, "out (a move: bit-exact, the columns rows..ld_out zero)", _v(o["out"], cols, ld_out, ld_out), ref)
    return res


@runner("rows_to_nchw")
def run_rows_to_nchw(be, o, a):
    n, C, H, W, ld = a["n_img"], a["C"], a["H"], a["W"], a["ld"]
    o.mat("inp", n * H * W, C, ld)
    o.out("out", 1, n * C * H * W)
    o.alloc()
    _launch(be, o)
    ref = _v(o["inp"], n * H * W, C, ld).to(torch.float64).view(n, H * W, C).permute(0, 2, 1).reshape(-1)
    res = []
    judge_exact(res, "out (a widening move: exact)", o["out"], ref)
    return res


@runner("cast_from_f32")
def run_cast_from_f32(be, o, a):
    n = a["n"]
    o.mat("inp", 1, n, scale=0.05)
    o.out("out", 1, n)
    o.alloc()
    _launch(be, o)
    x = ref64.d(o["inp"])
    res = []
    judge_single(res, "out", o["out"], x, x.abs(), 0, 0)             # one rounding, nothing else
    return res


@runner("cast_transpose_from_f32")
def run_cast_transpose_from_f32(be, o, a):
    R, Cc = a["R"], a["Ccols"]
    o.mat("inp", R, Cc, scale=0.05)
    o.out("out", Cc, R)
    o.alloc()
    _launch(be, o)
    x = ref64.d(_v(o["inp"], R, Cc, Cc)).t()
    res = []
    judge_single(res, "out", _v(o["out"], Cc, R, R), x, x.abs(), 0, 0)
    return res


@runner("ema_lerp")
def run_ema_lerp(be, o, a):
    """shadow -= omd (shadow - p) in fp32, omd as the float the binding passes: the difference, the product, the subtraction -- three
    roundings (E = 3) of values bounded by S = |shadow| + omd (|shadow| + |p|)"""
    n = a["n"]
    o.decl("shadow", n, lambda t: t.copy_(o.randn(n, scale=0.05)), out=True)
    o.mat("p", 1, n, scale=0.05)
    o.alloc()
    s0 = o["shadow"].clone()
    _launch(be, o)
    omd = float(torch.tensor(a["one_minus_decay"], dtype=torch.float32))
    res, CH = [], 1 << 26
    worst = (0.0, ())
    for i0 in range(0, n, CH):
        s, w = ref64.d(s0[i0:i0 + CH]), ref64.d(o["p"][i0:i0 + CH])
        ref, S = ref64.ema_lerp(s, w, omd)
        wv = _worst(_ratio(o["shadow"][i0:i0 + CH], ref, 0.5 * ulp_of(ref, torch.float32) + 3 * 2.0 ** -23 * S))
        worst = max(worst, (wv[0], tuple(i0 + i for i in wv[1])))
    return [("shadow",) + worst]


# -- activations.  csrc/common.h computes no libm function: the normal CDF comes from Abramowitz & Stegun 7.1.26 (published bound of the
# approximation in exact arithmetic: |erf error| <= 1.5e-7, i.e. 0.75e-7 on the CDF) evaluated with one v_exp_f32, one v_rcp_f32 and fp32
# FMAs; the sigmoid is v_rcp_f32(1 + v_exp_f32(.)).  The CDNA ISA guide gives both transcendental instructions 1 ulp, and both flush fp32
# denormals: a result below 2^-126 is zero.  Everything else is counted roundings (units of 2^-23 = one fp32 spacing of a value in [1, 2)).
AS_ERF_BOUND = 1.5e-7
_AS_P, _AS_A = 0.3275911, (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)
FP32_MIN_NORMAL = 2.0 ** -126


def gelu_cdf_error(x):
    """absolute error bound of gelu_parts(x).cdf for float64 x (any shape): h = P(t) E with t = 1 / (1 + p |x| / sqrt 2), E = exp(-x^2 / 2),
    P the degree-5 polynomial without constant term.  Relative error of h, in units of 2^-23:
      E: the two products of its argument a = x^2 log2(e) / 2 move it by 2^-23 a absolutely, E by ln 2 of that relatively: 0.7 a; v_exp: 1
      t: one FMA (1/2), v_rcp (1): 1.5, carried to P by its relative sensitivity kappa = |t P'(t) / P(t)|
      P: four FMAs and two products, each a rounding of a partial sum bounded by sum |a_i| t^i: 3 cond, cond = that sum / |P(t)|
    then 1 - h for x >= 0 (1/2), the published bound of the approximation itself, and the flush of h below the smallest normal."""
    ax = x.abs()
    t = 1.0 / (1.0 + _AS_P * ax / math.sqrt(2.0))
    pw = torch.stack([t ** (i + 1) for i in range(5)])
    co = torch.tensor(_AS_A, dtype=torch.float64, device=x.device).view(5, *([1] * x.ndim))
    P = (co * pw).sum(0)
    dP = (co * pw * torch.arange(1, 6, dtype=torch.float64, device=x.device).view(5, *([1] * x.ndim))).sum(0)        # t P'(t)
    cond = (co.abs() * pw).sum(0) / P.abs()
    kappa = dP.abs() / P.abs()
    h = 0.5 * P * torch.exp(-0.5 * x * x)
    units = 0.7 * (0.5 * x * x * math.log2(math.e)) + 1.0 + 1.5 * kappa + 3.0 * cond
    return h * units * 2.0 ** -23 + 2.0 ** -24 + 0.5 * AS_ERF_BOUND + FP32_MIN_NORMAL


def act_bound(x, act, dt, ref):
    """per-element bound of act_rows / the GEGLU gate for float64 inputs x: half an output spacing + |x| (error of the CDF / sigmoid) + the
    rounding of the product"""
    if act == 0:
        inner = gelu_cdf_error(x)
    else:
        # y = 1.702 x, the argument -log2(e) y (two roundings of |arg|: e moves by 0.7 |arg| units relatively), v_exp (1), 1 + e (1/2),
        # v_rcp (1): s = 1 / (1 + e) moves by (1 - s) times e's error plus 1.5; a flushed result costs the smallest normal
        arg = (1.702 * math.log2(math.e)) * x.abs()
        s = torch.sigmoid(1.702 * x)
        inner = s * ((1.0 - s) * (0.7 * arg + 1.0) + 1.5) * 2.0 ** -23 + FP32_MIN_NORMAL
    return 0.5 * ulp_of(ref, dt) + x.abs() * inner + 2.0 ** -24 * ref.abs()


def judge_act(res, label, got, x, act, gate=None):
    """out = [gate *] act(x): class by class.  Finite inputs: the derived bound (a finite reference wants a finite result); NaN and
    infinite inputs: the reference's class -- NaN, or the infinity / zero with its sign."""
    x64 = ref64.d(x)
    ref = ref64.act(x64, act)
    g64 = None if gate is None else ref64.d(gate)
    bound = act_bound(torch.where(torch.isfinite(x64), x64, torch.zeros_like(x64)), act, got.dtype, ref)
    if g64 is not None:
        # a * gelu(g): gelu(g) stays in fp32, one more product rounding
        bound = g64.abs() * (bound - 0.5 * ulp_of(ref, got.dtype)) + 0.5 * ulp_of(g64 * ref, got.dtype) + 2.0 ** -24 * (g64 * ref).abs()
        ref = g64 * ref
    fin = torch.isfinite(x64) & torch.isfinite(ref)
    g = got.to(torch.float64)
    res.append((label,) + _worst(torch.where(fin, _ratio(got, torch.where(fin, ref, torch.zeros_like(ref)), bound), torch.zeros_like(ref))))
    same = torch.where(torch.isnan(ref), torch.isnan(g), (g == ref) & (torch.signbit(g) == torch.signbit(ref)))
    wrong = ~fin & ~same
    res.append((label + ": class of the result at NaN / infinite inputs", float("inf") if bool(wrong.any()) else 0.0,
                tuple(int(i) for i in wrong.nonzero()[0]) if bool(wrong.any()) else ()))
    if got.dtype in (torch.float16, torch.bfloat16) and bool(fin.all()):
        RoundingMeans().add(got, ref, got.dtype).report(res, label)


@runner("act_rows")
def run_act_rows(be, o, a):
    n = a["n"]
    o.mat("inp", 1, n, scale=2.0)
    o.out("out", 1, n)                 # the CLIP tower runs it in place: `out` then aliases `inp` and the pre-fill is overwritten by the input
    o.alloc()
    x = o["inp"].clone()
    _launch(be, o)
    res = []
    judge_act(res, "out", o["out"], x, a["act"])
    return res


@runner("geglu_fwd")
def run_geglu_fwd(be, o, a):
    M, Fd = a["M"], a["F"]
    o.mat("pre", M, 2 * Fd)
    o.out("out", M, Fd)
    o.alloc()
    _launch(be, o)
    pre = _v(o["pre"], M, 2 * Fd, 2 * Fd)
    res = []
    judge_act(res, "out", _v(o["out"], M, Fd, Fd), pre[:, Fd:], 0, gate=pre[:, :Fd])
    return res


@runner("geglu_bwd")
def run_geglu_bwd(be, o, a):
    """the unfused form (the step launches it where the fused epilogue does not apply): dpre = [dout gelu(g), dout a gelu'(g)] from a
    16-bit dout -- the factor in fp32 (its error absolute: a few 2^-23 of |g| / |a| (1 + |g|), as in the GEMM's GEGLU-backward epilogue),
    one product, one rounding.  Ceiling: that family's bar, tol_for(dt, 2) on the row's own maximum."""
    M, Fd = a["M"], a["F"]
    o.mat("dout", M, Fd)
    o.mat("pre", M, 2 * Fd)
    o.out("dpre", M, 2 * Fd)
    o.alloc()
    _launch(be, o)
    dt = o.dtype("pre")
    pre, dh = _v(o["pre"], M, 2 * Fd, 2 * Fd), ref64.d(_v(o["dout"], M, Fd, Fd))
    ref = ref64.geglu_bwd(dh, pre, Fd)
    p64 = ref64.d(pre)
    facmag = torch.cat([p64[:, Fd:].abs(), p64[:, :Fd].abs() * (1 + p64[:, Fd:].abs())], 1)
    derived = 0.5 * ulp_of(ref, dt) + 2.0 ** -24 * ref.abs() + 16 * 2.0 ** -23 * torch.cat([dh, dh], 1).abs() * facmag
    res = []
    judge_rows(res, "dpre", _v(o["dpre"], M, 2 * Fd, 2 * Fd), ref, tol_for(dt, 2), derived)
    return res


@runner("colsum")
def run_colsum(be, o, a):
    """out[g, c] (+)= the sum of x[r, c] over the rows of group g, in fp32: single-rounding bound with as many accumulated terms as the
    largest group has rows (through the scratch slabs or atomics, in any order), + 1 for the value it adds to"""
    rows, C, ldx, ng, rpg, mod, accf = a["rows"], a["C"], a["ldx"], a["n_groups"], a["rpg"], a["mod"], int(a["accumulate"])
    o.mat("x", rows, C, ldx)
    o.out("out", ng, C, fill=1.0 if accf else float("nan"))
    o.out("scratch", 1, K.colsum_slabs(rows, rpg, mod) * ng * C)
    o.alloc()
    _launch(be, o)
    x = ref64.d(_v(o["x"], rows, C, ldx))
    gi = ref64.group_index(rows, rpg, mod, o.dev)
    assert int(gi.max()) < ng, (rows, rpg, mod, ng)
    base = torch.full((ng, C), float(accf), dtype=torch.float64, device=o.dev)
    v, S = base.clone().index_add_(0, gi, x), base.clone().index_add_(0, gi, x.abs())
    res = []
    judge_single(res, "out", _v(o["out"], ng, C, C), v, S, int(torch.bincount(gi).max()), 1 + accf)
    return res


@runner("softmax_rows")
def run_softmax_rows(be, o, a):
    """p = exp2(x sl2 - max sl2) / sum, sl2 = scale log2(e) as a float.  Rounding points: the input (given) and the output; fp32 between.
    The argument of the exponential is an FMA against the rounded maximum: with the rounding of sl2 itself, 2^-23 (|x| + |max|) sl2
    absolutely (log2 units), ln 2 of that relatively on p -- twice, numerator and normaliser; v_exp 1 ulp, twice; the sum of `cols`
    positive terms, the reciprocal, the product: (cols + 3) / 2 ... counted whole below.  Ceiling: the family's bar, tol_for(dt), on the row's
    own maximum.  Columns cols..cols_out are ZERO (include/svdx.h): the P v GEMM behind it reduces over them."""
    rows, cols, cols_out, ld_in, ld_out, sc = (a[k] for k in ("rows", "cols", "cols_out", "ld_in", "ld_out", "scale"))
    o.mat("inp", rows, cols, ld_in, scale=3.0)
    o.out("out", rows, cols_out, ld_out)
    o.alloc()
    x = ref64.d(_v(o["inp"], rows, cols, ld_in)).clone()
    _launch(be, o)
    dt = o.dtype("inp")
    sl2 = float(torch.tensor(sc, dtype=torch.float32)) * math.log2(math.e)
    ref = torch.softmax(x * float(torch.tensor(sc, dtype=torch.float32)), -1)
    amag = (x.abs() + x.abs().amax(-1, keepdim=True)) * abs(sl2)
    derived = ref * (2 * 0.7 * amag + 2 + cols + 3) * 2.0 ** -23 + 0.5 * ulp_of(ref, dt)
    got = _v(o["out"], rows, cols_out, ld_out)
    res = []
    judge_rows(res, "out", got[:, :cols], ref, tol_for(dt), derived)
    if cols_out > cols:
        judge_exact(res, "padding columns are zero", got[:, cols:], torch.zeros_like(got[:, cols:]))
    return res


@runner("attn_small_fwd")
def run_attn_small_fwd(be, o, a):
    """csrc/attention.hip's arithmetic at a head dimension d <= dp <= 128: the bound of attn_fwd with d in place of 64 and the bar
    tests/kernel_checks.py holds this family to, tol_for(dt), on the row's own maximum (a row holds all heads).  The padding channels
    d..dp of every head are written as zeros."""
    n, S, heads, d, dp, ld, ld_o, sc = (a[k] for k in ("n_img", "S", "heads", "d", "dp", "ld", "ld_o", "scale"))
    o.mat("qkv", n * S, 3 * heads * dp, ld)
    o.out("out", n * S, heads * dp, ld_o)
    o.alloc()
    _launch(be, o)
    dt = o.dtype("qkv")
    x = torch.as_strided(o["qkv"], (n, 3, heads, S, dp), (S * ld, heads * dp, dp, ld, 1), o["qkv"].storage_offset())
    got = torch.as_strided(o["out"], (n, heads, S, dp), (S * ld_o, dp, ld_o, 1), o["out"].storage_offset())
    ref, _, Spv, smax = ref64.attention(x[:, 0, ..., :d], x[:, 1, ..., :d], x[:, 2, ..., :d], sc)
    bar = tol_for(dt) * ref.abs().amax((1, 3), keepdim=True).expand_as(ref)
    bound = torch.maximum(torch.minimum(bar, _attn_derived_o(ref, Spv, smax, S, dt, d)), 0.5 * ulp_of(ref, dt))
    res = [("out",) + _worst(_ratio(got[..., :d], ref, bound))]
    RoundingMeans().add(got[..., :d], ref, dt).report(res, "out")
    if dp > d:
        judge_exact(res, "padding channels are zero", got[..., d:], torch.zeros_like(got[..., d:]))
    return res


def gaussian_taps(nt, dev):
    """normalised Gaussian window of nt taps, sigma = nt / 4 (clip._gaussian_taps: the window is about 4 sigma)"""
    xs = torch.arange(nt, dtype=torch.float32) - nt // 2
    g = torch.exp(-xs.pow(2) / (2 * (nt / 4.0) ** 2))
    return (g / g.sum()).to(dev)


@runner("blur_axis")
def run_blur_axis(be, o, a):
    """out = sum_k taps[k] in[reflect(i + k - half)] in fp32: nt products (E = nt, unless contracted) and nt accumulations (K_acc = nt)"""
    planes, H, W, axis, nt = a["planes"], a["H"], a["W"], a["axis"], a["taps"][4]
    o.mat("inp", 1, planes * H * W, scale=0.5)
    o.decl("taps", nt, lambda t: t.copy_(gaussian_taps(nt, o.dev)))
    o.out("out", 1, planes * H * W)
    o.alloc()
    _launch(be, o)
    ref, S = ref64.blur_axis(o["inp"].view(planes, H, W), o["taps"], axis)
    res = []
    judge_single(res, "out", o["out"].view(planes, H, W), ref, S, nt, nt)
    return res


@runner("bicubic_affine")
def run_bicubic_affine(be, o, a):
    """out = scale[c] bicubic(in)(y ry, x rx) + shift[c], align_corners, A = -0.75, all fp32.  Counted: 16 + 4 products and as many
    accumulations (K_acc = 20, E = 20), the two affine operations (E + 2), against S = |scale| sum |wy| |wx| |in| + |shift|.  On top, from
    the coordinate arithmetic: the source coordinate ry * yo carries two roundings (the ratio, the product), 2^-23 of its magnitude,
    which moves every weight by its derivative (`pos`); and each weight is a cubic in Horner form whose partial sums reach 36 (outer
    taps: |A| x^3 + 5 |A| x^2 + 8 |A| x + 4 |A| at x = 2) and 4.5 (inner taps), one rounding each: `wgt`."""
    n, C, H, W, ho, wo = (a[k] for k in ("n_img", "C", "H", "W", "ho", "wo"))
    o.mat("inp", 1, n * C * H * W, scale=0.5)
    o.vec("scale", C, scale=0.2, shift=2.0)
    o.vec("shift", C, scale=0.5)
    o.out("out", 1, n * C * ho * wo)
    o.alloc()
    _launch(be, o)
    x = o["inp"].view(n, C, H, W)
    ref = ref64.bicubic_affine(x, ho, wo, o["scale"], o["shift"])
    S, pos, wgt = ref64.bicubic_magnitudes(x, ho, wo)
    sc, sh = ref64.d(o["scale"]).abs().view(1, C, 1, 1), ref64.d(o["shift"]).abs().view(1, C, 1, 1)
    res = []
    judge_single(res, "out", o["out"].view(n, C, ho, wo), ref, sc * S + sh, 20, 22, extra=2.0 ** -23 * sc * (pos + wgt))
    return res


# ---- what the tests iterate over ---------------------------------------------------------------------------------------------------------
_FLAG_ARGS = ("out_mode", "epilogue", "trans", "silu_in", "accumulate", "silu", "prezeroed", "defer_reduce", "accumulate_f32", "variant", "mod",
              "rv_mod", "param_mode", "stages")


def feature_key(sig):
    """(entry, feature combination): which optional operands are there, the flag arguments, the gather's kind, whether K / the rows are split"""
    entry, kv = sig
    key = [entry]
    for k, v in kv:
        if isinstance(v, K.Gather):
            key.append((k, v.mode, v.stride, v.ups))
        elif isinstance(v, tuple) and v and v[0] == "T":
            key.append((k, v[1], v[2] is not None and v[2][1] == 0))             # dtype, written in place of another argument
        elif isinstance(v, tuple) and v and v[0] != "dtype":
            key.append((k, len(v) if entry.endswith("_batch") else tuple(x is not None and not isinstance(x, int) for x in v)))
        elif v is None:
            key.append((k, None))
        elif k in _FLAG_ARGS:
            key.append((k, bool(v) if k in ("mod", "rv_mod") else v))
        elif k in ("split_k", "nsplit"):
            key.append((k, v > 1))
    return tuple(key)


class _Declared(Exception):
    pass


class _DeclaredOperands(Operands):
    """the declarations of a runner without its tensors: `alloc()` ends the runner"""

    def alloc(self):
        raise _Declared()


_REACH = {}
REACH_2G, REACH_4G = 1 << 31, 1 << 32
TN_SPAN_MAX = 0x7ffffff0          # csrc/gemm_tn.hip: spans up to this value go through buffer descriptors


def reach(sig):
    """{tensor argument: extent in bytes} of a launch, as the entry computes it -- which is how the entry's runner declares its operands
    (GEMM A over the gather's source rows with the gather's pitch, B = (N - 1) ldb + K, C / res / aux over M rows of their pitch, gemm_tn's A
    and B over R rows, q / k / v / o over nb S rows of `ld`, ...).  Host only: nothing is allocated."""
    if sig not in _REACH:
        o = _DeclaredOperands(sig, "cpu")
        try:
            RUNNERS[sig[0]](None, o, sig_args(sig))
            raise AssertionError(f"{sig[0]}: the runner ended without allocating")
        except _Declared:
            pass
        _REACH[sig] = {n: ext * DT_OF[o.desc[n][1]].itemsize for n, (ext, _, _) in o.decls.items()}
    return _REACH[sig]


def reach_class(nbytes):
    """0: below 2^31 bytes; 1: 2^31 and more; 2: 2^32 and more"""
    return (nbytes >= REACH_2G) + (nbytes >= REACH_4G)


_GEMM_IN, _GEMM_OUT = ("A", "B", "dual.0", "dual.1"), ("C", "res", "aux_in", "aux_out")


def reach_key(sig):
    """the reach classes the entry's code distinguishes.  `gemm`: A or B (svdx_gemm leaves the tile kernels for the 64-bit-pointer kernel,
    the dual / GroupNorm / GEGLU forms refuse) and C, res or aux (the store path stays, its offsets grow); `gemm_tn`: A or B (buffer
    descriptors or the flat staging); every other entry: its largest operand."""
    if sig[0] not in RUNNERS:
        return ()
    r = reach(sig)
    big = lambda names: reach_class(max([r[n] for n in names if n in r], default=0))
    if sig[0] == "gemm":
        return (("reach A/B", big(_GEMM_IN)), ("reach C/res/aux", big(_GEMM_OUT)))
    if sig[0] == "gemm_tn":               # (svdx_gemm_tn's own line: spans beyond TN_SPAN_MAX, 16 bytes short of 2^31, take the flat staging)
        span = max(r["A"], r["B"])
        return (("reach A/B", (span > TN_SPAN_MAX) + (span >= REACH_4G)),)
    return (("reach", big(r)),)


def gemm_kernel_taken(sig):
    """which code a `gemm` / `gemm_tn` / `gemm_tn_gather` / `tsa_fwd` launch takes, from the conditions of the entry points
    (csrc/gemm_nt.hip gemm_entry, csrc/gemm_tn.hip svdx_gemm_tn / svdx_gemm_tn_gather, csrc/tsa.hip svdx_tsa_fwd): a kernel's name, or
    "refused: ..." where the library returns an error before it launches anything."""
    a = sig_args(sig)
    if sig[0] == "gemm_tn_gather":              # (no runner of its own: tests/conv_wgrad_checks.py) the spans as svdx_gemm_tn_gather forms them
        g = a["gather"]
        src = a["R"] if g.mode == K.GATHER_TEMPORAL3 else g.n_img * (g.hi >> g.ups) * (g.wi >> g.ups)
        if max(((a["R"] - 1) * a["lda"] + a["N"]) * 2, ((src - 1) * g.lda + g.cin) * 2) > TN_SPAN_MAX:
            return "refused: svdx_gemm_tn_gather: operands of 2 GiB and more are not supported"
        return "gemm_tn kernel, gathered, buffer descriptors"
    if sig[0] not in ("gemm", "gemm_tn", "tsa_fwd"):
        return None
    r = reach(sig)
    if sig[0] == "gemm":
        flat = r["A"] >= REACH_2G or r["B"] >= REACH_2G
        if a["dual"] is not None and (flat or r["dual.0"] >= REACH_2G or r["dual.1"] >= REACH_2G):
            return "refused: svdx_gemm_dual: operands too large for the buffer-addressed kernel"
        if a["variant"] >= 2 and not flat:
            return "tile kernel (buffer descriptors)"
        if a["epilogue"] != K.EPI_NONE:
            return "refused: svdx_gemm: fused epilogue unavailable (buffer too large for variant 4)"
        if a["gn"] is not None:
            return "refused: svdx_gemm_gn: statistics unavailable (buffer too large for variant 4)"
        return "gemm_kernel (64-bit pointers)"
    if sig[0] == "gemm_tn":
        buf = r["A"] <= TN_SPAN_MAX and r["B"] <= TN_SPAN_MAX and not (a["stages"] & K.TN_FLAT)
        return "gemm_tn kernel, buffer descriptors" if buf else "gemm_tn kernel, flat staging"
    if a["B"] * a["T"] * a["HW"] * 3 * a["C"] * 2 >= REACH_2G:
        return "refused: svdx_tsa_fwd: activation too large for 32-bit buffer offsets"
    return "tsa_fwd kernel"



def dispatch_class(sig):
    """What decides which code a launch runs: the entry, the dtypes of its tensors, every flag argument; for `gemm` also the tile it
    resolves to, whether K is split, the gather's kind, fused GroupNorm statistics, which epilogue operands are there, and N and K (the
    weight's shape: the tile rules and the K loop depend on them; M is what the geometry scales); and how far its operands reach in memory
    (`reach_key`: below 2^31 bytes, 2^31 and more, 2^32 and more)."""
    return _dispatch_class(sig) + reach_key(sig)


def _dispatch_class(sig):
    entry, kv = sig
    a = dict(kv)
    key = [entry]
    for k, v in kv:
        if isinstance(v, tuple) and v and v[0] == "T":
            key.append((k, v[1]))
        elif k in _FLAG_ARGS and not (entry == "gemm" and k == "variant"):
            key.append((k, bool(v) if k in ("mod", "rv_mod") else v))
    if entry == "gemm":
        from svd_xtend_amd.ops import _tile_launched
        g = a["gather"]
        key += [("tile", _tile_launched(a["variant"], a["M"], a["N"])), ("split", a["split_k"] > 1),
                ("gather", None if g is None else (g.mode, g.stride, g.ups)), ("gn", a["gn"] is not None),
                ("operands", tuple(a[k] is not None for k in ("bias", "rowvec", "res", "dual", "aux_out", "aux_in"))), ("N", a["N"]), ("K", a["K"])]
    return tuple(key)


def cond_gpu_signatures(what):
    """{part name: Counter[signature]} of what the GPU test runs for pass `what`: the small geometries of COND_GPU and, under the name of
    the real geometry, those of ITS signatures whose dispatch class none of the small geometries reaches (tiles chosen from the row count)."""
    parts = collections.OrderedDict((n, census_cond(n)) for n in COND_GPU[what])
    if what in COND_REAL:
        reached = {dispatch_class(s) for c in parts.values() for s in c}
        real = census_cond(COND_REAL[what])
        rest = collections.Counter({s: n for s, n in real.items() if dispatch_class(s) not in reached})
        if rest:
            parts[COND_REAL[what]] = rest
    return parts


STEP_GPU = ("c2", "c2_clip", "c5", "c5_ref", "c4")          # what tests/test_census_gpu.py runs


def sig_rows(sig):
    """the row count of a launch: what the geometry scales (0 for the entries that have none)"""
    a = sig_args(sig)
    for keys in (("M",), ("R",), ("n_s", "rows"), ("rows",), ("nb", "S"), ("B", "T", "HW"), ("n_img", "h", "w"), ("n",)):
        if all(isinstance(a.get(k), int) for k in keys):
            return math.prod(a[k] for k in keys)
    return 0


def geom_gpu_signatures():
    """{part name: Counter[signature]} of what tests/test_census_geom_gpu.py runs: every signature of the GEOM_EDGE geometries (less
    what GEOM_EDGE_MINUS says runs already) and, as part "grid", one signature for every dispatch class of GEOM_GRID that neither those
    nor the step's own configurations (STEP_GPU) reach: the one with the fewest rows -- a class only large row counts reach runs there;
    those of them with an operand of 2^31 bytes or more form the part "grid_reach"."""
    if "geom_gpu" in _CACHE:
        return _CACHE["geom_gpu"]
    parts = collections.OrderedDict()
    for n in GEOM_EDGE:
        skip = census(GEOM_EDGE_MINUS[n]) if n in GEOM_EDGE_MINUS else ()
        parts[n] = collections.Counter({s: k for s, k in census(n).items() if s not in skip})
    reached = {dispatch_class(s) for c in parts.values() for s in c} | {dispatch_class(s) for n in STEP_GPU for s in census(n)}
    best = {}
    for n in GEOM_GRID:
        for s, k in census(n).items():
            cls = dispatch_class(s)
            if cls not in reached:
                key = (sig_rows(s), repr(s))
                if cls not in best or key < best[cls][0]:
                    best[cls] = (key, s)
    # (the classes that differ from another by their reach alone -- batch 2 of config 4 at its real shape, gigabytes each -- as a part of their own)
    parts["grid"] = collections.Counter({s: 1 for _, s in best.values() if not any(v for _, v in reach_key(s))})
    parts["grid_reach"] = collections.Counter({s: 1 for _, s in best.values() if any(v for _, v in reach_key(s))})
    _CACHE["geom_gpu"] = parts
    return parts


def run_act_exhaustive(be, dt, act, dev):
    """every bit pattern of the 16-bit type `dt` through svdx_act_rows in ONE launch: [(label, excess, index = the bit pattern)]"""
    be = getattr(be, "impl", be)
    x = torch.arange(65536, dtype=torch.int32, device=dev).to(torch.int16).view(dt)
    buf = torch.full((65536 + 2 * GUARD,), GUARD_VALUE, dtype=dt, device=dev)
    out = buf[GUARD:GUARD + 65536]
    out.fill_(1.0)
    be.act_rows(x, out, 65536, act)
    _sync(dev)
    res = []
    judge_act(res, "out", out, x, act)
    ok = bool((buf[:GUARD] == GUARD_VALUE).all()) and bool((buf[-GUARD:] == GUARD_VALUE).all())
    res.append(("nothing written outside the operands", 0.0 if ok else float("inf"), ()))
    return res


def coverage(counts):
    """(launches, distinct signatures, distinct signatures with a runner, allow-listed launches by entry, entries with neither)"""
    allowed, missing = collections.Counter(), set()
    for s, n in counts.items():
        if s[0] in RUNNERS:
            continue
        if s[0] in ALLOW_LIST:
            allowed[s[0]] += n
        else:
            missing.add(s[0])
    return sum(counts.values()), len(counts), sum(1 for s in counts if s[0] in RUNNERS), allowed, sorted(missing)


def family(sig, label):
    import re
    return sig[0] + ": " + re.sub(r"job \d+ |\[\d+\]|slab \d+| of tile at \d+", "", label)
