"""Step time with trainable convolutions (profiles/conv_wgrad.md, measurement 2): the captured c2 step (B = 1, 14 frames, 512 x 320) with
--trainable temporal_transformer_block,@conv beside the default set, alternating in one process.  --trace-steps N instead replays the
first configuration N times and exits (every model is built and stepped before the first capture: on this runtime ATen kernels launched
after a graph's replay leave its later replays non-finite, tools/ab_inproc.py; a non-finite loss after the timed replays is an error): the run `rocprofv3 --kernel-trace --stats` wraps for the weight-gradient bucket split.

    python tools/conv_wgrad_step.py [--steps 20] [--reps 3] [--lr 1e-5] [--dtype fp16] [--trace-steps 0] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETS = {"conv": ("temporal_transformer_block", "@conv"), "default": "temporal_transformer_block"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "bf16"])
    ap.add_argument("--lr", type=float, default=1e-5)
    ap.add_argument("--trace-steps", type=int, default=0)
    ap.add_argument("--sets", default="conv,default")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bench
    from svd_xtend_amd.train import GraphedStep, Trainer
    from svd_xtend_amd.unet import UNetSpatioTemporalConditionModel
    dev = torch.device("cuda", 0)
    dt = torch.float16 if args.dtype == "fp16" else torch.bfloat16
    # every model is built and stepped eagerly BEFORE the first capture: on this runtime ATen kernels launched after a graph replay leave
    # that graph's later replays with a non-finite loss (tools/ab_inproc.py has the same rule), and building a model is all ATen
    trainers, graphs, info = {}, {}, {}
    for name in args.sets.split(","):
        with torch.device(dev):
            model = UNetSpatioTemporalConditionModel()
        bench.init_weights_(model, seed=1234)
        tr = Trainer(model, dtype=dt, lr=args.lr, trainable=SETS[name])
        batch = bench.make_batch(1, 14, 40, 64, model.config.cross_attention_dim, seed=123, dev=dev)
        for _ in range(2):
            tr.step(batch)
        torch.cuda.synchronize()
        trainers[name] = (tr, batch)
    for name, (tr, batch) in trainers.items():
        graphs[name] = (GraphedStep(tr, batch), tr)
        info[name] = dict(trainable_params=int(sum(p.numel() for p in tr.params)), lr=args.lr)
    torch.cuda.synchronize()
    if args.trace_steps:
        for _ in range(args.trace_steps):
            for gs, _ in graphs.values():
                gs()
        torch.cuda.synchronize()
        return
    res = {n: [] for n in graphs}
    for n, (gs, _) in graphs.items():
        for _ in range(5):
            gs()
    torch.cuda.synchronize()
    for rep in range(args.reps):
        for n, (gs, _) in graphs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                gs()
            torch.cuda.synchronize()
            res[n].append((time.perf_counter() - t0) / args.steps * 1e3)
            print(f"[{n}] rep {rep}: {res[n][-1]:.3f} ms/step", flush=True)
    for n, (gs, tr) in graphs.items():
        st = tr.opt_state.cpu().tolist()
        info[n].update(ms_per_step=res[n], median_ms=statistics.median(res[n]), loss_after=float(tr.loss_slot.cpu()), opt_steps=st[0], loss_scale=st[1])
        print(f"# {n}: median {info[n]['median_ms']:.3f} ms/step, loss {info[n]['loss_after']:.6f}, optimizer steps {st[0]:.0f}, loss scale {st[1]:g}")
    if args.out:
        with open(args.out, "w") as f:
            json.dump(info, f, indent=1)
    bad = [n for n in info if not (info[n]["loss_after"] == info[n]["loss_after"] and abs(info[n]["loss_after"]) < 1e30)]
    if bad:
        raise SystemExit(f"non-finite loss after the timed replays of {bad}: their timings are void")


if __name__ == "__main__":
    main()
