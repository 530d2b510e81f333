"""Cost of the GroupNorm affine gradients (profiles/gn_affine.md).

kernel: the GroupNorm backward shapes of the c2 step (the distinct svdx_gn_bwd_stats signatures tests/census.py records for configuration
c2: B = 1, 14 frames, 512 x 320) -- svdx_gn_bwd_stats_affine + the reducing launch of its partial rows beside the frozen
svdx_gn_bwd_stats, alternating in one process, device events, every shape warmed; the frozen launch is timed twice per round (A, B) and
|median A - median B| is the spread; the affine launch is also timed alone (partial rows left for a later reduction, as the step
queues them).  Yardstick per shape: frozen time x (bytes(dy) + bytes(x) + bytes(partial rows written and read)) /
(bytes(dy) + bytes(x)) + spread.

step: the captured c2 step with "@norm" beside its counterpart without, alternating in one process (tools/conv_wgrad_step.py's method).

    python tools/gn_affine_bench.py kernel [--rounds 30] [--dtype fp16] [--out FILE.json]
    python tools/gn_affine_bench.py step [--steps 20] [--reps 3] [--sets default,norm,conv,conv_norm] [--out FILE.json]
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

# (n_s, rows, C, silu, launches per c2 step): census.census("c2"), entry gn_bwd_stats, merged over eps
C2_SHAPES = [
    (1, 560, 1280, 1, 14), (1, 2240, 1280, 1, 10), (1, 8960, 640, 1, 10), (1, 35840, 320, 1, 8),
    (14, 40, 1280, 0, 1), (14, 40, 1280, 1, 11), (14, 40, 2560, 1, 3),
    (14, 160, 640, 1, 1), (14, 160, 1280, 0, 5), (14, 160, 1280, 1, 6), (14, 160, 1920, 1, 1), (14, 160, 2560, 1, 2),
    (14, 640, 320, 1, 1), (14, 640, 640, 0, 5), (14, 640, 640, 1, 6), (14, 640, 960, 1, 1), (14, 640, 1280, 1, 1), (14, 640, 1920, 1, 1),
    (14, 2560, 320, 0, 4), (14, 2560, 320, 1, 6), (14, 2560, 640, 1, 2), (14, 2560, 960, 1, 1),
]
SETS = {"default": "temporal_transformer_block", "norm": ("temporal_transformer_block", "@norm"),
        "conv": ("temporal_transformer_block", "@conv"), "conv_norm": ("temporal_transformer_block", "@conv", "@norm")}


def kernel(args):
    from svd_xtend_amd import kernels as K
    k = K.backend()
    dev = torch.device("cuda", 0)
    dt = torch.float16 if args.dtype == "fp16" else torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(5)
    rows_out = []
    for n_s, rows, C, silu, count in C2_SHAPES:
        M = n_s * rows
        x = (1.5 * torch.randn(M, C, generator=g, device=dev) + 0.5).to(dt)
        dy = torch.randn(M, C, generator=g, device=dev).to(dt)
        gamma = 1 + 0.3 * torch.randn(C, generator=g, device=dev)
        beta = 0.3 * torch.randn(C, generator=g, device=dev)
        nst = K.GN_REPLICAS * n_s * 32 * K.GN_STAT_FLOATS
        stats, bst = torch.zeros(nst, device=dev), torch.zeros(nst, device=dev)
        k.gn_stats(x, stats, n_s, rows, C, 32, prezeroed=1)
        nblk = K.gn_bwd_blocks(n_s, rows, C, 32)
        partial = torch.empty(nblk * 2 * C, device=dev)
        dg, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)

        def frozen():
            k.gn_bwd_stats(dy, x, stats, gamma, beta, bst, n_s, rows, C, 32, 1e-6, silu, prezeroed=1)

        def affine():           # the launch + the reducing launch of its own partial rows (in the step: a share of one table-driven launch)
            k.gn_bwd_stats_affine(dy, x, stats, gamma, beta, bst, dg, db, partial, n_s, rows, C, 32, 1e-6, silu, prezeroed=1, defer_reduce=False)

        def affine_only():      # the statistics launch alone: the partial rows stay for a reducing launch the step shares among ~100 norms
            k.gn_bwd_stats_affine(dy, x, stats, gamma, beta, bst, dg, db, partial, n_s, rows, C, 32, 1e-6, silu, prezeroed=1, defer_reduce=True)
        t = {"A": [], "affine": [], "B": [], "alone": []}
        for _ in range(5):
            frozen(), affine()
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for name, fn in (("A", frozen), ("affine", affine), ("B", frozen), ("alone", affine_only)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                t[name].append(e0.elapsed_time(e1) * 1e3)
        a, b, f, alone = (statistics.median(t[n]) for n in ("A", "B", "affine", "alone"))
        frozen_us, spread = min(a, b), abs(a - b)
        op_bytes = 2 * M * C * x.element_size()
        part_bytes = 2 * nblk * 2 * C * 4
        yard = frozen_us * (op_bytes + part_bytes) / op_bytes + spread
        rows_out.append(dict(n_s=n_s, rows=rows, C=C, silu=silu, count=count, partial_rows=nblk, frozen_us=frozen_us, spread_us=spread, affine_us=f, affine_alone_us=alone,
                             yardstick_us=yard, ratio=f / yard, extra_bytes_frac=part_bytes / op_bytes))
        r = rows_out[-1]
        print(f"({n_s:2d}, {rows:5d}, {C:4d}) silu={silu} x{count:2d}: frozen {frozen_us:7.2f} us (spread {spread:5.2f})  affine+reduce {f:7.2f} us (launch alone {alone:6.2f})  "
              f"partial rows {nblk:4d} (+{100 * r['extra_bytes_frac']:.1f} % bytes)  yardstick {yard:7.2f} us  ratio {r['ratio']:.2f}", flush=True)
    tot_f = sum(r["frozen_us"] * r["count"] for r in rows_out)
    tot_a = sum(r["affine_us"] * r["count"] for r in rows_out)
    print(f"# over the {sum(r['count'] for r in rows_out)} launches of a c2 step: frozen {tot_f / 1e3:.3f} ms, affine + own reduce {tot_a / 1e3:.3f} ms")
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(shapes=rows_out, step_frozen_ms=tot_f / 1e3, step_affine_ms=tot_a / 1e3), f, indent=1)


def step(args):
    import bench
    from svd_xtend_amd.train import GraphedStep, Trainer
    from svd_xtend_amd.unet import UNetSpatioTemporalConditionModel
    dev = torch.device("cuda", 0)
    dt = torch.float16 if args.dtype == "fp16" else torch.bfloat16
    # every model is built and stepped eagerly BEFORE the first capture (tools/conv_wgrad_step.py, tools/ab_inproc.py have the same rule)
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
        print(f"[{name}] built, {sum(p.numel() for p in tr.params)} trainable elements", flush=True)
    for name, (tr, batch) in trainers.items():
        graphs[name] = (GraphedStep(tr, batch), tr)
        info[name] = dict(trainable_params=int(sum(p.numel() for p in tr.params)), lr=args.lr)
    torch.cuda.synchronize()
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
    for a, b in (("norm", "default"), ("conv_norm", "conv")):
        if a in info and b in info:
            print(f"# {a} - {b}: {info[a]['median_ms'] - info[b]['median_ms']:+.3f} ms/step")
    if args.out:
        with open(args.out, "w") as f:
            json.dump(info, f, indent=1)
    bad = [n for n in info if not (info[n]["loss_after"] == info[n]["loss_after"] and abs(info[n]["loss_after"]) < 1e30)]
    if bad:
        raise SystemExit(f"non-finite loss after the timed replays of {bad}: their timings are void")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernel", "step"])
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "bf16"])
    ap.add_argument("--lr", type=float, default=1e-5)
    ap.add_argument("--sets", default="default,norm,conv,conv_norm")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    kernel(args) if args.what == "kernel" else step(args)


if __name__ == "__main__":
    main()
