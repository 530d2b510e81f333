"""CPU (`-m "not gpu"`): the latent cache (svd_xtend_amd/latent_cache.py), its kernel svdx_latent_batch on the wave64 simulator, and
`TrainLoop(latent_cache=...)` over the emulated kernels.  The kernel's result is DEFINED as the torch statements of
tests/emul.py (`latent_statements`, here `lc.statements`): every comparison with them is `torch.equal`."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.join(HERE, "sim"))

import latent_cache_checks as lc  # noqa: E402

T = 3


def towers(seed=0, grad_accum=1):
    import train_svd_amd as ex
    from svd_xtend_amd.train import Trainer
    args = ex.parse_args(["--tiny", "--seed", str(seed)])
    unet, vae, enc = ex.build_models(args, torch.device("cpu"), torch.float32)
    return Trainer(unet, dtype=torch.float32, lr=1e-3, grad_accum=grad_accum), vae, enc


def videos(H=64, W=64, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand(n, 3, H, W, generator=g) * 2 - 1 for n in (5, 4)]


def item(cache, vids, v, start, B=1):
    """B copies of nothing: sample b reads window (v, start + b) when it fits, so the samples of a batch differ."""
    first, idx = [], []
    for b in range(B):
        s = start + b if start + b + T <= vids[v].shape[0] else start
        first.append(vids[v][s])
        idx.append(cache.window(v, s, T))
    return dict(first_frame=torch.stack(first), index=torch.tensor(idx, dtype=torch.int64))


# ---- 1. the kernel on the simulator ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sim():
    from backend import SimBackend
    return SimBackend()


@pytest.mark.parametrize("shape", lc.SHAPES, ids=lambda s: "c{}_{}x{}_T{}_B{}_off{}".format(*s))
def test_kernel_on_simulator_bit_for_bit(sim, shape):
    """Every index pattern (distinct, equal, overlapping, 0, F - T, and -1 / F, which must give the clamped windows) at every shape:
    the three outputs equal the statements bit for bit, and no guard band around any input or output is touched."""
    for k, pattern in enumerate(lc.PATTERNS):
        lc.run_case(sim, "cpu", shape, pattern, k)


def test_kernel_inputs_make_contraction_visible(sim):
    """The data of these cases tells a + b * c in two roundings from the fused multiply-add: were the comparison blind to it, a
    contracted build would pass.  Asserted on the CPU, on the very tensors the launch then reads."""
    shape = (4, 8, 8, 14, 3, 0)
    for k, pattern in enumerate(lc.PATTERNS):
        t, _ = lc.make_case(shape, pattern, k)
        n = lc.contraction_visible(t)
        assert n > 0.05 * 14 * 4 * 64, (pattern, n)
        lc.run_case(sim, "cpu", shape, pattern, k)


# ---- 2. argument validation, no device ------------------------------------------------------------------------------------------
def test_argument_validation_without_device():
    from svd_xtend_amd import build, kernels
    lib = kernels.load_library(build.build())
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)

    def call(mean=p, F=8, Tn=3, B=1, chw=4):
        return lib.svdx_latent_batch(mean, p, F, p, p, p, p, p, p, p, p, 0.18215, p, p, p, B, Tn, chw, None)

    def last():
        msg = ctypes.create_string_buffer(256)
        lib.svdx_last_error(msg, 256)
        return msg.value

    for kw in (dict(mean=None), dict(Tn=0), dict(F=2, Tn=3), dict(B=0), dict(chw=0)):
        assert call(**kw) != 0, kw
        assert b"svdx_latent_batch" in last(), (kw, last())


# ---- 3. cache contents ----------------------------------------------------------------------------------------------------------
def test_cache_contents_save_load_and_window(emu_backend, tmp_path):
    from svd_xtend_amd.clip import encode_image
    from svd_xtend_amd.latent_cache import LatentCache
    from svd_xtend_amd.vae import AutoencoderKLTemporalDecoder
    import train_svd_amd as ex
    _, vae, enc = towers()
    vids = videos()
    cache = LatentCache.build(vae, enc, vids)
    again = LatentCache.build(vae, enc, vids)
    for name in ("mean", "std", "embed"):
        assert torch.equal(getattr(cache, name), getattr(again, name)), name
    assert cache.video_start.tolist() == [0, 5, 9] and cache.video_start.dtype == torch.int64
    assert cache.mean.shape == (9, 4, 8, 8) and cache.embed.shape == (9, 64) and cache.mean.dtype == torch.float32
    # the same calls with the same chunking: whole videos (9 frames are far below max_frames), and chunks of 2
    for chunk, c in ((None, cache), (2, LatentCache.build(vae, enc, vids, chunk=2))):
        row = 0
        for v in vids:
            step = chunk or v.shape[0]
            for i in range(0, v.shape[0], step):
                d = vae.encode(v[i:i + step]).latent_dist
                n = d.mean.shape[0]
                assert torch.equal(c.mean[row:row + n], d.mean) and torch.equal(c.std[row:row + n], d.std), (chunk, row)
                assert torch.equal(c.embed[row:row + n], encode_image(v[i:i + step], enc).to(torch.float32)), (chunk, row)
                row += n
    # disk
    folder = str(tmp_path / "cache")
    cache.save(folder)
    assert sorted(os.listdir(folder)) == ["latent_cache.safetensors", "meta.json"]
    back = LatentCache.load(folder, "cpu", vae=vae, image_encoder=enc, height=64, width=64)
    for name in ("mean", "std", "embed", "video_start"):
        assert torch.equal(getattr(back, name), getattr(cache, name)), name
    assert back.meta == cache.meta and set(cache.meta) >= {"H", "W", "c", "h", "w", "embed_dim", "dtype", "scaling_factor", "sha256"}
    # a cache from other weights, another scaling factor or another resolution never loads
    _, vae2, enc2 = towers()
    LatentCache.load(folder, "cpu", vae=vae2, image_encoder=enc2)                      # the same weights: fine
    vae2.encoder.conv_in.weight.data[0, 0, 0, 0] += 1e-3
    with pytest.raises(ValueError):
        LatentCache.load(folder, "cpu", vae=vae2, image_encoder=enc2)
    _, _, enc3 = towers()
    enc3.visual_projection.weight.data[0, 0] += 1e-3
    with pytest.raises(ValueError):
        LatentCache.load(folder, "cpu", vae=vae, image_encoder=enc3)
    vae4 = AutoencoderKLTemporalDecoder(**ex.TINY["vae"], scaling_factor=0.5)
    vae4.load_state_dict(vae.state_dict())
    vae4.prepare(torch.float32)
    with pytest.raises(ValueError):
        LatentCache.load(folder, "cpu", vae=vae4, image_encoder=enc)
    with pytest.raises(ValueError):
        LatentCache.load(folder, "cpu", vae=vae, image_encoder=enc, height=128, width=64)
    # window: the only producer of an index
    assert cache.window(0, 0, T) == 0 and cache.window(0, 2, T) == 2 and cache.window(1, 0, T) == 5 and cache.window(1, 1, T) == 6
    for v, s in ((0, 3), (1, 2), (0, -1), (-1, 0), (2, 0)):
        with pytest.raises(IndexError):
            cache.window(v, s, T)


# ---- 4. batch from cache == the statements over the cache -----------------------------------------------------------------------
def recording(loop, forced_p=None):
    """Wrap loop._draw: keep a copy of the draws of the last micro-batch; `forced_p` replaces the dropout draw."""
    kept, orig = {}, loop._draw

    def draw(*a, **k):
        d = orig(*a, **k)
        if forced_p is not None:
            d["p_drop"].copy_(forced_p)
        kept.clear()
        kept.update({n: t.clone() for n, t in d.items()})
        return d
    loop._draw = draw
    return kept


@pytest.mark.parametrize("B", [1, 2])
def test_batch_from_cache_equals_the_statements(emu_backend, B):
    from svd_xtend_amd.latent_cache import LatentCache
    from svd_xtend_amd.loop import BATCH_KEYS, TrainLoop
    tr, vae, enc = towers()
    vids = videos()
    cache = LatentCache.build(vae, enc, vids)
    it = item(cache, vids, 0, 1, B)
    # dropout: None, 0.0, and 0.5 with the draw forced into each band: p < prob zeroes the embedding, prob <= p < 2 prob both,
    # 2 prob <= p < 3 prob the conditioning latent, beyond nothing (train_svd.py:992-1011); with B = 2 two bands share a batch
    runs = [(None, None), (0.0, None)] + [(0.5, [p, q][:B]) for p, q in ((0.25, 1.25), (0.75, 1.75), (1.25, 0.25), (1.75, 0.75))]
    seen = set()
    for prob, forced in runs:
        loop = TrainLoop(tr, vae, enc, conditioning_dropout_prob=prob, seed=3, use_graph=False, latent_cache=cache, num_frames=T)
        d = recording(loop, None if forced is None else torch.tensor(forced))
        got = loop.prepare_batch(it)
        assert tuple(got) == BATCH_KEYS
        log_normal = lambda u, loc, scale: (loc + scale * (2.0 ** 0.5) * torch.erfinv(2.0 * (u * (1 - 2e-7) + 1e-7) - 1.0)).exp()   # noqa: E731
        cond_sigmas, sigmas = log_normal(d["u_cond"], -3.0, 0.5), log_normal(d["u_sig"], 0.7, 1.6)
        cpix = d["n_cpix"] * cond_sigmas[:, None, None, None, None] + it["first_frame"][:, None]
        dist = vae.encode(cpix.reshape(B, 3, 64, 64)).latent_dist
        cm, cs = dist.mean.clone(), dist.std.clone()
        ehs = cache.embed[it["index"]].unsqueeze(1)
        keep = torch.ones(B)
        if prob is not None:
            p = d["p_drop"]
            ehs = ehs * (p >= 2 * prob).to(torch.float32).reshape(B, 1, 1)
            keep = 1 - ((p >= prob) & (p < 3 * prob)).to(torch.float32)
            seen.update((bool(e.abs().max() == 0), float(k) == 0.0) for e, k in zip(ehs, keep))
        want = dict(zip(("unet_in", "noisy_latents", "target"),
                        lc.statements(cache.mean, cache.std, it["index"], d["eps"], d["noise"], cm, cs, sigmas, (sigmas ** 2 + 1) ** 0.5, keep,
                                      vae.config.scaling_factor)))
        want.update(timesteps=0.25 * sigmas.log(), ehs=ehs, sigmas=sigmas,
                    added_time_ids=torch.stack([torch.tensor(7.0), torch.tensor(127.0), cond_sigmas[0]]).unsqueeze(0).repeat(B, 1))
        for k in BATCH_KEYS:
            assert got[k].shape == want[k].shape and got[k].dtype == torch.float32 and got[k].is_contiguous(), k
            assert torch.equal(got[k], want[k]), (prob, forced, k)
        if prob is None or forced is None:
            assert float(got["ehs"].abs().max()) > 0 and float(got["unet_in"][:, :, 4:].abs().max()) > 0
    assert seen == {(True, False), (True, True), (False, True), (False, False)}, seen      # (embedding zeroed, latent zeroed)


# ---- 5. cached against uncached, same seed --------------------------------------------------------------------------------------
def test_cached_loop_against_uncached_loop_same_seed(emu_backend):
    from svd_xtend_amd.latent_cache import LatentCache
    from svd_xtend_amd.loop import TrainLoop
    tr, vae, enc = towers()
    vids = videos()
    cache = LatentCache.build(vae, enc, vids)
    decisions = set()
    for seed, (v, start) in enumerate(((0, 0), (0, 2), (1, 1), (1, 0), (0, 1), (1, 1))):
        plain = TrainLoop(tr, vae, enc, conditioning_dropout_prob=0.2, seed=seed, use_graph=False)
        cached = TrainLoop(tr, vae, enc, conditioning_dropout_prob=0.2, seed=seed, use_graph=False, latent_cache=cache, num_frames=T)
        seen, encode = [], vae.encode

        def spy(x, *a, **k):
            r = encode(x, *a, **k)
            seen.append((r.latent_dist.mean.clone(), r.latent_dist.std.clone()))
            return r
        vae.encode = spy
        try:
            a = plain.prepare_batch(vids[v][start:start + T].unsqueeze(0))
        finally:
            del vae.encode
        b = cached.prepare_batch(item(cache, vids, v, start))
        for k in ("sigmas", "timesteps", "added_time_ids"):
            assert torch.equal(a[k], b[k]), (seed, k)
        da = (float(a["ehs"].abs().max()) == 0, float(a["unet_in"][:, :, 4:].abs().max()) == 0)
        assert da == (float(b["ehs"].abs().max()) == 0, float(b["unet_in"][:, :, 4:].abs().max()) == 0), seed
        decisions.add(da)
        # the moments behind `target`: the cache's rows (a 5- or 4-frame call) against the uncached call's (T + 1 frames).  atol 1e-6 is
        # what tests/test_vae.py::test_frames_are_chunked_below_the_buffer_limit grants the encoder for another frame count.  Moments,
        # not batches: the posterior sample amplifies a difference in std by |eps|.
        (mean, std), = seen
        row = cache.window(v, start, T)
        assert torch.allclose(cache.mean[row:row + T], mean[:T], atol=1e-6) and torch.allclose(cache.std[row:row + T], std[:T], atol=1e-6), seed
        if not da[0]:
            assert torch.allclose(a["ehs"], b["ehs"], atol=1e-6)
    assert len(decisions) > 1, decisions           # the seeds cover more than one dropout outcome


# ---- 6. loop behaviour ----------------------------------------------------------------------------------------------------------
def test_pipelined_cached_loop_equals_sequential_steps(emu_backend):
    """tests/test_train_loop.py::test_pipelined_loop_equals_sequential_steps over a cache: three steps, EMA on."""
    from svd_xtend_amd.latent_cache import LatentCache
    from svd_xtend_amd.loop import TrainLoop
    from svd_xtend_amd.training_utils import EMAModel
    vids = videos()
    out = []
    for mode in ("pipelined", "sequential"):
        tr, vae, enc = towers()
        cache = LatentCache.build(vae, enc, vids)
        items = [item(cache, vids, v, s) for v, s in ((0, 0), (1, 1), (0, 2))]
        ema = EMAModel(tr.model.parameters(), decay=0.5)
        loop = TrainLoop(tr, vae, enc, conditioning_dropout_prob=0.1, seed=9, use_graph=False, ema=ema if mode == "pipelined" else None,
                         latent_cache=cache, num_frames=T)
        losses = []
        if mode == "pipelined":
            loop.start(items[0])
            for i in range(3):
                losses.append(loop.step(items[i + 1] if i + 1 < 3 else None))
            assert loop.global_step == 3 and ema.optimization_step == 3
        else:
            for it in items:
                tr.step(loop.prepare_batch(it))
                losses.append(float(tr.last_loss()))
        out.append((losses, tr.p_flat.clone()))
    assert out[0][0] == out[1][0], out
    assert torch.equal(out[0][1], out[1][1])
    assert all(l == l and l > 0 for l in out[0][0])


def test_grad_accum_and_item_count(emu_backend):
    from svd_xtend_amd.latent_cache import LatentCache
    from svd_xtend_amd.loop import TrainLoop
    tr, vae, enc = towers(grad_accum=2)
    vids = videos()
    cache = LatentCache.build(vae, enc, vids)
    loop = TrainLoop(tr, vae, enc, conditioning_dropout_prob=0.1, seed=4, use_graph=False, latent_cache=cache, num_frames=T)
    with pytest.raises(ValueError):
        loop.start(item(cache, vids, 0, 0))                          # one item where two are due
    loop.start([item(cache, vids, 0, 0), item(cache, vids, 1, 1)])
    with pytest.raises(ValueError):
        loop.step([item(cache, vids, 0, 1)])
    l1 = loop.step([item(cache, vids, 0, 1), item(cache, vids, 1, 0)])
    l2 = loop.step(None)
    assert l1 == l1 and l1 > 0 and l2 == l2 and l2 > 0 and loop.global_step == 2
    # what is not a cached micro-batch is refused, and so is an index the cache cannot serve
    with pytest.raises(TypeError):
        loop.prepare_batch(vids[0][:T].unsqueeze(0))
    with pytest.raises(IndexError):
        loop.prepare_batch(dict(first_frame=vids[0][:1], index=torch.tensor([cache.n_frames - T + 1])))
    with pytest.raises(ValueError):
        TrainLoop(tr, vae, enc, use_graph=False, latent_cache=cache)                     # no num_frames


_DEFAULT_PATH_SCRIPT = """
import sys
sys.path[:0] = [{root!r}, {tests!r}, {examples!r}]
import torch
import emul
from svd_xtend_amd import kernels
kernels._set_backend_for_tests(emul.EmuBackend())
rec = emul.record(kernels._backend)
import train_svd_amd as ex
from svd_xtend_amd.loop import BATCH_KEYS, TrainLoop
from svd_xtend_amd.train import Trainer
args = ex.parse_args(["--tiny", "--seed", "0"])
unet, vae, enc = ex.build_models(args, torch.device("cpu"), torch.float32)
loop = TrainLoop(Trainer(unet, dtype=torch.float32, lr=1e-3), vae, enc, conditioning_dropout_prob=0.1, seed=11, use_graph=False)
clip = torch.rand(1, 3, 3, 64, 64, generator=torch.Generator().manual_seed(5)) * 2 - 1
b = loop.prepare_batch(clip)
assert "svd_xtend_amd.latent_cache" not in sys.modules and rec and "svdx_latent_batch" not in rec.names()
torch.save({{k: b[k] for k in BATCH_KEYS}}, {out!r})
"""


def test_default_loop_is_untouched_by_the_new_module(emu_backend, tmp_path):
    """latent_cache=None: prepare_batch for a fixed seed gives the bits it gives in a process that never imports the new module and
    never calls svdx_latent_batch (the recorder of tests/emul.py sees every call that process makes, and sees some)."""
    import svd_xtend_amd.latent_cache  # noqa: F401  -- imported here, never there
    from svd_xtend_amd.loop import BATCH_KEYS, TrainLoop
    out = str(tmp_path / "batch.pt")
    script = _DEFAULT_PATH_SCRIPT.format(root=ROOT, tests=HERE, examples=os.path.join(ROOT, "examples"), out=out)
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    there = torch.load(out)
    tr, vae, enc = towers()
    loop = TrainLoop(tr, vae, enc, conditioning_dropout_prob=0.1, seed=11, use_graph=False, latent_cache=None)
    clip = torch.rand(1, 3, 3, 64, 64, generator=torch.Generator().manual_seed(5)) * 2 - 1
    here = loop.prepare_batch(clip)
    for k in BATCH_KEYS:
        assert torch.equal(here[k], there[k]), k
