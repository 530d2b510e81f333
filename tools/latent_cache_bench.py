"""TrainLoop.step with and without a latent cache, same process, alternating.

    python tools/latent_cache_bench.py [--frames 14 --height 320 --width 512 --dtype fp16] [--reps 5 --steps 20] [--out profiles/latent_cache.json]

Two trainers of the same geometry (bench.py's model and initialisation), the same frozen towers, the same synthetic videos: the uncached
loop gets a window's T pixel frames per iteration (bench.py's `real_loop`), the cached loop the window's first frame and its cache row.
Both run their captured graphs.  After a warm-up the two loops alternate, `--reps` times `--steps` iterations each; an iteration ends in
the loss read on the host, so the host clock around a block measures finished device work.  Also timed, by device events, nothing beside
them: each loop's conditioners (the replay of its captured conditioner graph), a one-frame and a T + 1-frame VAE encode, the CLIP embed,
the cache build (host clock), the weights' fingerprint inside it, and the build's encoder calls per frame.  Prints one JSON line; nothing here falls back to a CPU."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=14)
    ap.add_argument("--height", type=int, default=320)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "bf16"])
    ap.add_argument("--reps", type=int, default=5, help="alternations")
    ap.add_argument("--steps", type=int, default=20, help="iterations of each loop per alternation")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--videos", type=int, default=4)
    ap.add_argument("--tiny", action="store_true", help="debug: tiny topologies")
    ap.add_argument("--optimizer", default="default", choices=["default", "beside", "after"],
                    help="both loops: the captured optimizer beside or after the next clip's conditioners (TrainLoop(overlap_optimizer=...)); default: "
                         "each loop's own default (beside without a cache, after with one)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import bench
    from svd_xtend_amd.clip import CLIPVisionModelWithProjection, encode_image
    from svd_xtend_amd.latent_cache import LatentCache, towers_fingerprint
    from svd_xtend_amd.loop import TrainLoop
    from svd_xtend_amd.train import Trainer
    from svd_xtend_amd.unet import UNetSpatioTemporalConditionModel
    from svd_xtend_amd.vae import AutoencoderKLTemporalDecoder
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device: this tool measures on the GPU only")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dt = torch.float16 if args.dtype == "fp16" else torch.bfloat16
    T, H, W = args.frames, args.height, args.width
    ucfg, vcfg, ccfg = {}, {}, {}
    if args.tiny:
        ucfg = dict(block_out_channels=(64, 128, 128, 128), addition_time_embed_dim=32, projection_class_embeddings_input_dim=96,
                    cross_attention_dim=64, num_attention_heads=(1, 2, 2, 2))
        vcfg = dict(block_out_channels=(64, 128, 128, 128), layers_per_block=1)
        ccfg = dict(hidden_size=320, intermediate_size=640, projection_dim=64, num_hidden_layers=2, num_attention_heads=4, image_size=56, patch_size=14)

    def trainer():
        with torch.device(dev):
            model = UNetSpatioTemporalConditionModel(**ucfg)
        bench.init_weights_(model, seed=1234)
        return Trainer(model, dtype=dt, lr=1e-5)

    with torch.device(dev):
        vae, enc = AutoencoderKLTemporalDecoder(**vcfg), CLIPVisionModelWithProjection(**ccfg)
    bench.init_weights_(vae, seed=4321)
    bench.init_weights_(enc, seed=4322)
    for m in (vae, enc):
        m.requires_grad_(False)
        m.prepare(dt)

    def timed(fn, n=5):
        """ms per call by device events, after one warm-up call"""
        fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n

    g = torch.Generator().manual_seed(777)
    length = T + 6
    videos = [torch.rand(length, 3, H, W, generator=g) * 2 - 1 for _ in range(args.videos)]
    LatentCache.build(vae, enc, videos[:1])                                   # warm the towers' shapes
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cache = LatentCache.build(vae, enc, videos)
    torch.cuda.synchronize()
    build_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    towers_fingerprint(vae, enc)                                              # part of every build and every checked load: weights to the host + SHA-256
    fingerprint_ms = (time.perf_counter() - t0) * 1e3

    windows = [(v, (3 * v) % (length - T + 1)) for v in range(args.videos)]
    clips = [videos[v][s:s + T].unsqueeze(0).contiguous().pin_memory() for v, s in windows]
    items = [dict(first_frame=videos[v][s:s + 1].contiguous().pin_memory(), index=torch.tensor([cache.window(v, s, T)]).pin_memory()) for v, s in windows]
    ov = dict(default=None, beside=True, after=False)[args.optimizer]
    loops = {"uncached": (TrainLoop(trainer(), vae, enc, conditioning_dropout_prob=0.1, seed=99, overlap_optimizer=ov), clips),
             "cached": (TrainLoop(trainer(), vae, enc, conditioning_dropout_prob=0.1, seed=99, overlap_optimizer=ov, latent_cache=cache, num_frames=T), items)}
    its = {k: 1 for k in loops}
    losses = {k: [] for k in loops}

    def run(name, n):
        loop, feed = loops[name]
        for _ in range(n):
            losses[name].append(loop.step(feed[its[name] % len(feed)]))
            its[name] += 1

    for name, (loop, feed) in loops.items():
        loop.start(feed[0])
        run(name, args.warmup)
    blocks = {k: [] for k in loops}
    for _ in range(args.reps):
        for name in loops:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(name, args.steps)
            torch.cuda.synchronize()
            blocks[name].append((time.perf_counter() - t0) * 1e3 / args.steps)

    # the conditioners alone: what the loop queues per micro-batch (copy in, draws, replay of the captured conditioner graph, copy out)
    cond = {name: timed(lambda loop=loop, feed=feed: loop._produce(0, feed[1]), n=10) for name, (loop, feed) in loops.items()}
    pix = clips[0].to(dev).to(torch.float32)[0]
    frames = torch.cat([pix, pix[:1]])
    with torch.no_grad():
        enc_ms = {"vae_encode_1_frame": timed(lambda: vae.encode(frames[:1]).latent_dist, n=10),
                  f"vae_encode_{T + 1}_frames": timed(lambda: vae.encode(frames).latent_dist),
                  "clip_embed_1_frame": timed(lambda: encode_image(frames[:1], enc), n=10)}
        x = videos[0].to(dev)                                                 # what LatentCache.build does with one video, per frame
        enc_ms["cache_build_encoders_per_frame"] = timed(lambda: (vae.encode(x).latent_dist, encode_image(x, enc)), n=3) / x.shape[0]

    med = {k: statistics.median(v) for k, v in blocks.items()}
    spread = {k: max(v) - min(v) for k, v in blocks.items()}
    out = {"geometry": f"{T} frames {W}x{H}, batch 1, {args.dtype}", "tiny": args.tiny, "overlap_optimizer": {k: loop.overlap_optimizer for k, (loop, _) in loops.items()}, "reps": args.reps, "steps_per_block": args.steps,
           "ms_per_iteration_blocks": blocks, "ms_per_iteration_median": med, "ms_per_iteration_spread": spread,
           "gain_ms": med["uncached"] - med["cached"], "gain_beyond_spread": med["uncached"] - med["cached"] > max(spread.values()),
           "conditioners_ms_alone": cond, "encoders_ms_alone": enc_ms, "cache_build_ms": build_ms, "towers_fingerprint_ms": fingerprint_ms,
           "cache_frames": cache.n_frames, "cache_bytes": 4 * (cache.mean.numel() + cache.std.numel() + cache.embed.numel()),
           "losses_finite": {k: all(l == l and abs(l) != float("inf") for l in v) for k, v in losses.items()},
           "exec": {k: "hipgraph" if loop.graphed is not None and loop.cond_graph is not None else "eager" for k, (loop, _) in loops.items()}}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
