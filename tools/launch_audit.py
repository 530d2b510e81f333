"""Launches per C-ABI entry (and per call site) of ONE steady-state optimizer step, counted on the CPU emulation of the kernels
(tests/emul.py) with the tiny topology -- same block structure and call graph as the full model, so a launch that should not be there
shows up without a GPU.  (It found config 5 re-casting its frozen feed-forward weights after every step: 128 launches.)

    python tools/launch_audit.py [--lora-rank 64 | --trainable temporal_transformer_block,@conv,@norm] [--sites small_linear,outer_acc]

TEST-SIDE tool: imports tests/emul.py.  A launch is a call at depth 0 of emul.record -- one the host issued, not one an emulation makes
on itself (the singles under a *_batch entry, gemm_tn under gemm_tn_gather, tattn_fwd under tsa_fwd).
"""
import argparse
import collections
import os
import sys
import traceback

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lora-rank", type=int, default=0)
    ap.add_argument("--trainable", default="", help="comma-separated Trainer(trainable=...) rules, e.g. temporal_transformer_block,@conv,@norm")
    ap.add_argument("--sites", default="", help="comma-separated entries whose call sites are listed")
    args = ap.parse_args()
    import emul
    from svd_xtend_amd import kernels as K
    from svd_xtend_amd.train import Trainer
    be = emul.EmuBackend()
    log = emul.record(be)                         # depth 0 = a launch; what an emulation calls on itself (depth >= 1) is not one
    log.on = False
    sites = collections.Counter()

    def with_site(name, f):
        def w(*a, **kw):
            n, st = len(log), traceback.extract_stack(limit=5)[:-1]
            try:
                return f(*a, **kw)
            finally:
                if len(log) > n and log[n][1] == 0:
                    sites[(name,) + tuple(f"{s.name}:{s.lineno}" for s in st[-3:])] += 1
        return w
    for name in filter(None, args.sites.split(",")):
        setattr(be, name, with_site(name, getattr(be, name)))
    K._set_backend_for_tests(be)
    import e2e_checks
    orig, n = Trainer.step, [0]

    def step(self, *a, **kw):
        n[0] += 1
        log.on = n[0] == 2                        # the second step: packing and caches are behind us
        try:
            return orig(self, *a, **kw)
        finally:
            log.on = False
    Trainer.step = step
    if args.trainable:
        import selection_checks as sc
        which = tuple(args.trainable.split(","))
        ref = sc.oracle_step(which)               # (for its seeded weights and batch)
        tr = sc.make_trainer(ref, which, torch.float32, torch.device("cpu"))
        for _ in range(2):
            tr.step(sc.step_batch(ref, "cpu"))
    else:
        e2e_checks.run_steps(dev=torch.device("cpu"), dtype=torch.float32, steps=2, lora_r=args.lora_rank)
    cnt = collections.Counter(e[len("svdx_"):] for e in log.names(depth=0))
    for k, v in cnt.most_common():
        print(f"{v:6d}  {k}")
    print(f"{sum(cnt.values()):6d}  total")
    for k, v in sites.most_common():
        print(f"{v:6d}  {' <- '.join(k)}")


if __name__ == "__main__":
    main()
