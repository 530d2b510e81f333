"""Cost of the gather in the convolution weight gradient (profiles/conv_wgrad.md, measurement 1): svdx_gemm_tn_gather + svdx_conv_wgrad_finalize
against svdx_gemm_tn on a MATERIALISED [R, taps * cin] operand (built with torch indexing, outside the timed window), same split_k and
tile, for c2's stride-1 3x3 and temporal convolutions at the 64x40 and 32x20 levels.  The two alternate in one process; medians over the
rounds, and the plain kernel's own max - min spread.

    python tools/conv_wgrad_bench.py [--rounds 7] [--iters 20] [--dtype fp16] [--out FILE.json]

Counters (where the gathered kernel's extra time goes): `--pmc-run` issues, per shape, PMC_N launches of the gathered kernel and then PMC_N
of the plain one and nothing else from the library; run it under `rocprofv3 --pmc <one pass> --output-format csv -d DIR -- ...`, a run of
its own per pass (the passes of tools/stall_pmc.py), then `--pmc-report DIR [DIR ...]` joins the passes: per shape and kernel, averages
over the launches after the first two.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, B = 14, 1
# (label, kind, h, w, cin, cout): the ResNet halves of c2 (B = 1, 14 frames, 512 x 320 pixels) at its two upper levels
SHAPES = [("64x40 3x3 320->320", "3x3", 40, 64, 320, 320), ("64x40 3x3 640->320", "3x3", 40, 64, 640, 320),
          ("64x40 3x3 960->320", "3x3", 40, 64, 960, 320), ("64x40 t3 320->320", "t3", 40, 64, 320, 320),
          ("32x20 3x3 320->640", "3x3", 20, 32, 320, 640), ("32x20 3x3 640->640", "3x3", 20, 32, 640, 640),
          ("32x20 3x3 1280->640", "3x3", 20, 32, 1280, 640), ("32x20 t3 640->640", "t3", 20, 32, 640, 640)]


def gathered_operand(x, g, R):
    """[R, taps * cin]: the A operand svdx_gemm forms from x [source rows, >= cin] for the gather g (3x3 at stride 1 | 2 with optional `ups`,
    or the temporal mode), by torch indexing; a tap outside the image is zeros."""
    from svd_xtend_amd import kernels as K
    m = torch.arange(R, device=x.device)
    cols = []
    if g.mode == K.GATHER_TEMPORAL3:
        pp, tt, b = m % g.hw, (m // g.hw) % g.t, m // (g.hw * g.t)
        for dt in (-1, 0, 1):
            ts = tt + dt
            cols.append(((b * g.t + ts.clamp(0, g.t - 1)) * g.hw + pp, (ts >= 0) & (ts < g.t)))
    else:
        xo, yo, n = m % g.wo, (m // g.wo) % g.ho, m // (g.wo * g.ho)
        hs, ws = g.hi >> g.ups, g.wi >> g.ups
        for dy in range(3):
            for dx in range(3):
                ys, xs = yo * g.stride + dy - 1, xo * g.stride + dx - 1
                ok = (ys >= 0) & (ys < g.hi) & (xs >= 0) & (xs < g.wi)
                cols.append(((n * hs + (ys.clamp(0, g.hi - 1) >> g.ups)) * ws + (xs.clamp(0, g.wi - 1) >> g.ups), ok))
    return torch.cat([x[row, :g.cin] * ok[:, None].to(x.dtype) for row, ok in cols], 1)


PMC_N = 6


def pmc_report(dirs):
    import csv
    import glob
    from collections import defaultdict
    cnt = defaultdict(lambda: defaultdict(float))             # (shape index, "gather" | "plain") -> counter -> mean
    for d in dirs:
        rows = defaultdict(dict)
        for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                i = int(r["Dispatch_Id"])
                rows[i]["name"] = r["Kernel_Name"]
                rows[i][r["Counter_Name"]] = rows[i].get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
        ids = [i for i in sorted(rows) if "gemm_tn_kernel" in rows[i]["name"]]
        if len(ids) != 2 * PMC_N * len(SHAPES):
            print(f"{d}: {len(ids)} TN dispatches, expected {2 * PMC_N * len(SHAPES)}", file=sys.stderr)
        for s in range(len(SHAPES)):
            for j, which in enumerate(("gather", "plain")):
                sel = ids[(2 * s + j) * PMC_N + 2:(2 * s + j + 1) * PMC_N]
                for i in sel:
                    for k, v in rows[i].items():
                        if k != "name":
                            cnt[(s, which)][k] += v / len(sel)
    keys = ("SQ_WAIT_ANY", "SQ_WAIT_INST_ANY", "SQ_ACTIVE_INST_ANY", "SQ_ACTIVE_INST_VALU")
    print("| shape | kernel | wave cycles (M quad-cycles) | busy cycles (M) | parked at a wait / barrier | issue stall | issuing | issuing VALU | VALU per MFMA | SALU per MFMA | VMEM per MFMA | MFMA busy |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for s, shape in enumerate(SHAPES):
        for which in ("gather", "plain"):
            c = cnt[(s, which)]
            wc, mf = c.get("SQ_WAVE_CYCLES", 0.0), c.get("SQ_INSTS_MFMA", 0.0)
            frac = [f"{c[k] / wc:.3f}" if wc and k in c else "--" for k in keys]
            per = [f"{c[k] / mf:.2f}" if mf and k in c else "--" for k in ("SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_VMEM")]
            busy = f"{c['SQ_VALU_MFMA_BUSY_CYCLES'] / (1024 * c['GRBM_GUI_ACTIVE'] / 8):.3f}" if c.get("GRBM_GUI_ACTIVE") and "SQ_VALU_MFMA_BUSY_CYCLES" in c else "--"
            print(f"| {shape[0]} | {which} | {wc / 1e6:.2f} | {c.get('SQ_BUSY_CYCLES', 0.0) / 1e6:.2f} | " + " | ".join(frac + per) + f" | {busy} |")
    print("raw:", json.dumps({f"{SHAPES[s][0]} {w}": dict(v) for (s, w), v in sorted(cnt.items())}))


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3          # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "bf16"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--pmc-run", action="store_true")
    ap.add_argument("--pmc-report", nargs="+", default=None, metavar="DIR")
    args = ap.parse_args()
    if args.pmc_report:
        return pmc_report(args.pmc_report)
    from svd_xtend_amd import kernels as K
    from svd_xtend_amd import ops
    k = K.backend()
    dt = torch.float16 if args.dtype == "fp16" else torch.bfloat16
    dev = torch.device("cuda")
    rows = []
    for label, kind, h, w, cin, cout in SHAPES:
        taps = 3 if kind == "t3" else 9
        R, Kd = B * T * h * w, taps * cin
        g = K.Gather(K.GATHER_TEMPORAL3, n_img=B, cin=cin, t=T, hw=h * w, lda=cin) if kind == "t3" else \
            K.Gather(K.GATHER_CONV3X3, n_img=B * T, hi=h, wi=w, ho=h, wo=w, cin=cin, stride=1, lda=cin)
        gen = torch.Generator(device=dev).manual_seed(R + Kd)
        x = torch.randn(R, cin, device=dev, generator=gen).to(dt)
        dy = torch.randn(R, cout, device=dev, generator=gen).to(dt)
        aeff = gathered_operand(x, g, R).contiguous()
        sk, stages = ops._tn_gather_formula(R, cout, Kd)
        slabs, cs = torch.empty(sk, cout, Kd, device=dev), torch.empty(sk, cout, device=dev)
        slabs2, cs2 = torch.empty(sk, cout, Kd, device=dev), torch.empty(sk, cout, device=dev)
        wg, bg = torch.empty(cout, cin, taps, device=dev), torch.empty(cout, device=dev)
        flat, bflat = torch.empty(cout, Kd, device=dev), torch.zeros(cout, device=dev)
        runs = {
            "gather": lambda: k.gemm_tn_gather(dy, x, slabs, R, cout, cout, Kd, g, out_mode=K.OUT_F32_SLAB, split_k=sk, a_colsum=cs, stages=stages),
            "finalize": lambda: k.conv_wgrad_finalize(slabs, sk, cout * Kd, Kd, wg, cout, cin, cin, taps, alpha=1.0, store=True, colsum_slabs=cs,
                                                      colsum_ld=cout, b_grad=bg),
            "plain": lambda: k.gemm_tn(dy, aeff, slabs2, R, cout, Kd, cout, Kd, Kd, out_mode=K.OUT_F32_SLAB, split_k=sk, a_colsum=cs2, stages=stages),
            "plain_finalize": lambda: k.gemm_finalize(slabs2, sk, cout * Kd, flat, cout, Kd, Kd, accumulate_f32=2, dtype=dt, colsum_slabs=cs2,
                                                      colsum_out=bflat),
        }
        runs["gather+finalize"] = lambda: (runs["gather"](), runs["finalize"]())
        if args.pmc_run:
            for name in ("gather", "plain"):
                for _ in range(PMC_N):
                    runs[name]()
            torch.cuda.synchronize()
            continue
        for fn in runs.values():                         # warm up every launch
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        # same numbers either way: the finalized gradient against the plain kernel's slabs reduced on the host side
        ref = slabs2.sum(0).view(cout, taps, cin).permute(0, 2, 1)
        err = float((wg - ref).abs().max() / ref.abs().max())
        assert err < 1e-5, (label, err)
        t = {name: [] for name in runs}
        for _ in range(args.rounds):
            for name in ("plain", "gather+finalize", "plain_finalize", "gather", "finalize"):
                t[name].append(timed(runs[name], args.iters))
        med = {name: statistics.median(v) for name, v in t.items()}
        spread = max(t["plain"]) - min(t["plain"])
        row = dict(shape=label, R=R, N=cout, K=Kd, split_k=sk, stages=stages, us=med, plain_spread_us=spread,
                   passes=med["gather+finalize"] <= med["plain"] + spread, rel_err_vs_plain=err)
        rows.append(row)
        print(json.dumps(row), flush=True)
    print("\n| shape | R | N x K | split_k | plain gemm_tn | its spread | gather | finalize | gather + finalize | plain + gemm_finalize | within bar |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        u = r["us"]
        print(f"| {r['shape']} | {r['R']} | {r['N']} x {r['K']} | {r['split_k']} | {u['plain']:.1f} | {r['plain_spread_us']:.1f} | {u['gather']:.1f} | "
              f"{u['finalize']:.1f} | {u['gather+finalize']:.1f} | {u['plain'] + u['plain_finalize']:.1f} | {'yes' if r['passes'] else 'NO'} |")
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
