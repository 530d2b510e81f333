"""`-m gpu`: svdx_latent_batch on the device bit for bit against the torch statements evaluated on the CPU (the check that shows a
contracted multiply-add or an approximate division, which the simulator's host build cannot), the cache against the uncached encoder
call, and examples/train_svd_amd.py --latent_cache end to end.  Tiny topologies, 64 x 64 pixels (128 x 128 under the example: its
validation sampler's batch of 2 needs an even pixel count at the coarsest level), T = 3."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "examples"))

import latent_cache_checks as lc  # noqa: E402

pytestmark = pytest.mark.gpu
T = 3
C2_LAUNCH = (4, 40, 64, 14, 1, 0)          # 14 frames at 512 x 320, one clip: the launch of the benchmarked geometry


def rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


@pytest.mark.parametrize("shape", lc.SHAPES + [C2_LAUNCH], ids=lambda s: "c{}_{}x{}_T{}_B{}_off{}".format(*s))
def test_kernel_on_device_bit_for_bit(shape):
    from svd_xtend_amd import kernels
    be = kernels.backend()
    for k, pattern in enumerate(lc.PATTERNS):
        if shape[1] * shape[2] >= 64 and shape[3] == 14:
            t, _ = lc.make_case(shape, pattern, k)
            assert lc.contraction_visible(t) > 0.05 * 14 * shape[0] * shape[1] * shape[2], pattern      # a contracted build cannot pass
        lc.run_case(be, "cuda", shape, pattern, k)


def towers(dtype):
    import train_svd_amd as ex
    from svd_xtend_amd.train import Trainer
    args = ex.parse_args(["--tiny", "--seed", "0"])
    unet, vae, enc = ex.build_models(args, torch.device("cuda"), dtype)
    return Trainer(unet, dtype=dtype, lr=1e-3), vae, enc


def test_cached_moments_against_the_uncached_call_fp16():
    """The cache's rows of a window (built by 5- and 4-frame calls) against the moments of the uncached loop's T + 1-frame call, in the
    metric of tests/test_vae.py::test_encoder_matches_oracle_small at TWICE its fp16 bar (each call is within one bar of the oracle);
    the embedding against a one-frame encode_image at twice the fp16 bar of tests/test_clip.py's GPU test."""
    from svd_xtend_amd.clip import encode_image
    from svd_xtend_amd.latent_cache import LatentCache
    from svd_xtend_amd.loop import TrainLoop
    tr, vae, enc = towers(torch.float16)
    g = torch.Generator().manual_seed(5)
    vids = [torch.rand(n, 3, 64, 64, generator=g) * 2 - 1 for n in (5, 4)]
    cache = LatentCache.build(vae, enc, vids)
    assert cache.mean.is_cuda and cache.mean.dtype == torch.float32 and cache.meta["dtype"] == "float16"
    for seed, (v, start) in enumerate(((0, 2), (1, 0))):
        plain = TrainLoop(tr, vae, enc, conditioning_dropout_prob=0.1, seed=seed, use_graph=False)
        cached = TrainLoop(tr, vae, enc, conditioning_dropout_prob=0.1, seed=seed, use_graph=False, latent_cache=cache, num_frames=T)
        seen, encode = [], vae.encode

        def spy(x, *a, **k):
            r = encode(x, *a, **k)
            seen.append((r.latent_dist.mean.clone(), r.latent_dist.logvar.clone()))
            return r
        vae.encode = spy
        try:
            a = plain.prepare_batch(vids[v][start:start + T].unsqueeze(0))
        finally:
            del vae.encode
        row = cache.window(v, start, T)
        b = cached.prepare_batch(dict(first_frame=vids[v][start:start + 1], index=torch.tensor([row])))
        for k in ("sigmas", "timesteps", "added_time_ids"):
            assert torch.equal(a[k], b[k]), (seed, k)
        (mean, logvar), = seen
        r = (rel(cache.mean[row:row + T], mean[:T]), rel(2 * cache.std[row:row + T].log(), logvar[:T]),
             rel(cache.embed[row:row + 1], encode_image(vids[v][start:start + 1].cuda(), enc).float()))
        print("cached vs uncached rel-L2 (mean, logvar, embed):", r)
        assert r[0] <= 2e-2 and r[1] <= 2e-2 and r[2] <= 2e-2, r


COMMON = ["--tiny", "--seed", "7", "--width", "128", "--height", "128", "--num_frames", "3", "--learning_rate", "1e-3", "--lr_scheduler",
          "constant_with_warmup", "--lr_warmup_steps", "2", "--use_ema", "--num_validation_steps", "2", "--cache_videos", "3"]


def test_example_builds_loads_checkpoints_and_resumes(tmp_path, capsys):
    import train_svd_amd as ex
    out, cdir = str(tmp_path / "run"), str(tmp_path / "cache")
    args = COMMON + ["--output_dir", out, "--latent_cache", cdir]
    r = ex.main(args + ["--max_train_steps", "3", "--checkpointing_steps", "2", "--validation_steps", "2"])
    assert r["global_step"] == 3 and r["train_loss"] == r["train_loss"] and r["train_loss"] > 0
    assert "Built a latent cache of 18 frames in 3 videos" in capsys.readouterr().out
    assert sorted(os.listdir(cdir)) == ["latent_cache.safetensors", "meta.json"]
    assert sorted(os.listdir(os.path.join(out, "checkpoint-2"))) == ["optimizer.bin", "random_states_0.pkl", "scaler.pt", "scheduler.bin",
                                                                     "unet", "unet_ema"]
    assert sorted(os.listdir(os.path.join(out, "validation_images"))) == ["step_1_val_img_0.gif", "step_2_val_img_0.gif"]
    stamp = os.path.getmtime(os.path.join(cdir, "latent_cache.safetensors"))
    r2 = ex.main(args + ["--max_train_steps", "4", "--checkpointing_steps", "100", "--validation_steps", "100", "--resume_from_checkpoint", "latest"])
    assert r2["global_step"] == 4 and r2["train_loss"] == r2["train_loss"] and r2["train_loss"] > 0
    text = capsys.readouterr().out
    assert "Built a latent cache" not in text and "Latent cache" in text                # the second run loads
    assert os.path.getmtime(os.path.join(cdir, "latent_cache.safetensors")) == stamp
    # a cache of another resolution is refused, not trained from
    with pytest.raises(ValueError):
        ex.main(COMMON[:3] + ["--width", "64", "--height", "128"] + COMMON[7:] + ["--output_dir", out, "--latent_cache", cdir, "--max_train_steps", "1"])


def test_captured_cached_loop_equals_eager_and_serves_a_new_window_per_replay(tmp_path, monkeypatch):
    """The captured conditioner graph reads `index` on the device: consecutive replays read different rows and leave different
    targets, and the captured run ends on the eager (--no_graph) run's loss bit for bit."""
    import train_svd_amd as ex
    from svd_xtend_amd.loop import TrainLoop
    cdir = str(tmp_path / "cache")
    quiet = COMMON + ["--latent_cache", cdir, "--max_train_steps", "4", "--checkpointing_steps", "100", "--validation_steps", "100"]
    log, produce = [], TrainLoop._produce

    def spy(self, j, clip):
        produce(self, j, clip)
        if self.cond_graph is not None:
            log.append((self._index.clone(), self._cond_out["target"].clone(), clip["index"].clone()))
    monkeypatch.setattr(TrainLoop, "_produce", spy)
    a = ex.main(quiet + ["--output_dir", str(tmp_path / "graph")])
    assert len(log) == 3                                                                    # steps 2, 3, 4 came from replays
    for dev_idx, _, host_idx in log:
        assert torch.equal(dev_idx.cpu(), host_idx)
    pairs = [(x, y) for x, y in zip(log, log[1:]) if not torch.equal(x[0], y[0])]
    assert pairs, [l[0].tolist() for l in log]                                              # consecutive iterations, different windows
    for x, y in pairs:
        assert not torch.equal(x[1], y[1])
    n = len(log)
    b = ex.main(quiet + ["--output_dir", str(tmp_path / "eager"), "--no_graph"])
    assert len(log) == n                                                                    # the eager run replays nothing
    assert a["train_loss"] == b["train_loss"], (a, b)
