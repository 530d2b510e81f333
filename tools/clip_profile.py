"""Cost of gradient-norm clipping (Trainer(max_grad_norm=...)) on the benched configuration's trainable buffer.

    python tools/clip_profile.py --kernels [--kernel-reps 20]      # the two clip launches beside svdx_check_finite over the same buffer
    python tools/clip_profile.py --step [--reps 5 --steps 30]   # GraphedStep with clipping on and off, same process, alternating

--kernels issues, `--kernel-reps` times, svdx_check_finite (GradScaler's full inf check: one 16-byte-per-lane read of the buffer, the same access
pattern), svdx_grad_sumsq_spans and svdx_grad_clip_coef over the flat gradient buffer of the benched model (bench.py's defaults: 397.6 M
trainable floats, its span table); each launch is bracketed by events, and the run is meant to be wrapped in
`rocprofv3 --kernel-trace --stats` for the kernel times proper.  --step captures the step twice on one Trainer -- the optimizer graph with
and without the two launches -- and replays the graphs alternately.  Prints one line per measurement and a JSON summary (--out)."""
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


def build(args):
    import bench
    from svd_xtend_amd.train import Trainer
    from svd_xtend_amd.unet import UNetSpatioTemporalConditionModel
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    with torch.device(dev):
        model = UNetSpatioTemporalConditionModel()
    bench.init_weights_(model, seed=1234)
    tr = Trainer(model, dtype=torch.float16 if args.dtype == "fp16" else torch.bfloat16, lr=1e-5, max_grad_norm=args.max_grad_norm)
    batch = bench.make_batch(1, args.frames, args.height // 8, args.width // 8, model.config.cross_attention_dim, seed=123, dev=dev)
    return tr, batch, dev


def kernels(args, tr, dev):
    k, n = tr.rt.k, tr.n_flat
    g = tr.g_flat
    gen = torch.Generator(device=dev).manual_seed(1)
    g[:n].normal_(generator=gen)
    st0 = tr.opt_state.clone()
    st = st0.clone()                            # scratch state, reset before every launch: the trainer's own is not touched
    n_spans = tr.clip_spans.shape[0]
    launches = {
        "svdx_check_finite": lambda: k.check_finite(g, n, st),
        "svdx_grad_sumsq_spans": lambda: k.grad_sumsq_spans(g, tr.clip_spans, n_spans, tr.clip_partial),
        "svdx_grad_clip_coef": lambda: k.grad_clip_coef(tr.clip_partial, tr.clip_spans, n_spans, tr.n_clip_tensors, tr.max_grad_norm, 1.0,
                                                        st, tr.clip_out, param_mode=tr.param_mode),
    }
    times = {name: [] for name in launches}
    for name, f in launches.items():            # warm-up
        f()
    torch.cuda.synchronize()
    for _ in range(args.kernel_reps):
        for name, f in launches.items():
            st.copy_(st0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1))
    out = {"n_floats": n, "n_spans": n_spans, "n_tensors": tr.n_clip_tensors, "grad_norm": float(tr.clip_out[0])}
    for name, ts in times.items():
        med = statistics.median(ts)
        out[name] = {"median_ms": med, "min_ms": min(ts), "max_ms": max(ts)}
        bw = ""
        if name != "svdx_grad_clip_coef":       # the two passes over the buffer
            out[name]["TBps_at_median"] = n * 4 / (med * 1e-3) / 1e12
            bw = f"  ({n * 4 / (med * 1e-3) / 1e12:.2f} TB/s over {n * 4 / 1e9:.2f} GB)"
        print(f"{name:24s} median {med * 1e3:8.1f} us  min {min(ts) * 1e3:8.1f}  max {max(ts) * 1e3:8.1f}{bw}", flush=True)
    out["sumsq_over_check_finite"] = out["svdx_grad_sumsq_spans"]["median_ms"] / out["svdx_check_finite"]["median_ms"]
    print(f"sum of squares / check_finite (event medians): {out['sumsq_over_check_finite']:.3f}", flush=True)
    return out


def step(args, tr, batch):
    from svd_xtend_amd.train import GraphedStep
    graphs = {}
    for cfg in ("off", "on"):
        saved = tr.clip_spans
        if cfg == "off":
            tr.clip_spans = None                # optimizer_step issues exactly the launches of a Trainer without max_grad_norm
        try:
            for _ in range(2):
                tr.step(batch)
            torch.cuda.synchronize()
            graphs[cfg] = GraphedStep(tr, batch)
            graphs[cfg]()
            torch.cuda.synchronize()
        finally:
            tr.clip_spans = saved
        print(f"# captured clipping {cfg}: loss {float(tr.loss_slot.cpu()):.6f}", flush=True)
    for c in graphs:                            # settle clocks
        for _ in range(10):
            graphs[c]()
    torch.cuda.synchronize()
    res = {c: [] for c in graphs}
    for rep in range(args.reps):
        for c in graphs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                graphs[c]()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) / args.steps * 1e3
            res[c].append(ms)
            print(f"[clipping {c}] rep {rep}: {ms:.3f} ms/step", flush=True)
    st = tr.opt_state.cpu().tolist()
    print(f"# after the timed replays: loss {float(tr.loss_slot.cpu()):.6f}, optimizer steps {st[0]:.0f}, loss scale {st[1]:g}, "
          f"grad_norm {float(tr.clip_out.cpu()[0]):.4f}", flush=True)
    med = {c: statistics.median(v) for c, v in res.items()}
    out = {"ms_per_step": res, "median": med, "delta_median_ms": med["on"] - med["off"],
           "spread_off_ms": max(res["off"]) - min(res["off"]), "spread_on_ms": max(res["on"]) - min(res["on"])}
    print(f"# median on - off: {out['delta_median_ms']:+.3f} ms (spread off {out['spread_off_ms']:.3f}, on {out['spread_on_ms']:.3f})", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--frames", type=int, default=14)
    ap.add_argument("--height", type=int, default=320)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--dtype", default="fp16")
    ap.add_argument("--max-grad-norm", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not (args.kernels or args.step):
        raise SystemExit("--kernels and / or --step")
    tr, batch, dev = build(args)
    out = {}
    if args.kernels:
        out["kernels"] = kernels(args, tr, dev)
    if args.step:
        out["step"] = step(args, tr, batch)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
