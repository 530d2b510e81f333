"""The trainable convolutions at FULL size (c2: B = 1, 14 frames, 512 x 320, the 1.5 B-parameter topology), where the tiny-topology tests
do not reach.  One forward + backward sweep with `temporal_transformer_block,@conv`, during which EVERY ConvOp.bwd_dw call -- 3x3 at
stride 1 and 2, `ups`, conv_in (padded input channels), conv_out (cout 4 at N = 8), the temporal convolutions with their folded alpha, the
1x1 shortcuts -- is compared against out_scale * dy^T Aeff computed by torch from the materialised operand (fp32 matmul of the same 16-bit
values); then optimizer steps, after each of which every re-packed w / wd is compared bit for bit with ConvOp.pack's torch statements
and the loss, the skip flag and the first non-finite tensor (if any) are reported.

    python tools/conv_wgrad_fullsize.py [--steps 6] [--lr 1e-5] [--dtype fp16] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--lr", type=float, default=1e-5)
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "bf16"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bench
    from conv_wgrad_bench import gathered_operand
    from svd_xtend_amd import ops
    from svd_xtend_amd.train import Trainer
    from svd_xtend_amd.unet import UNetSpatioTemporalConditionModel
    dev = torch.device("cuda", 0)
    dt = torch.float16 if args.dtype == "fp16" else torch.bfloat16
    with torch.device(dev):
        model = UNetSpatioTemporalConditionModel()
    bench.init_weights_(model, seed=1234)
    tr = Trainer(model, dtype=dt, lr=args.lr, trainable=("temporal_transformer_block", "@conv"))
    batch = bench.make_batch(1, 14, 40, 64, model.config.cross_attention_dim, seed=123, dev=dev)
    rt = tr.rt
    names = {id(op): n for n, op in conv_names(model)}
    report, orig = [], ops.ConvOp.bwd_dw

    def checked(self, rt_, dy, x, n_img, h, w, T=0, lddy=None):
        orig(self, rt_, dy, x, n_img, h, w, T=T, lddy=lddy)
        if not self.trainable:
            return
        rt_.flush_deferred()                                   # (a 1x1 shortcut's reducing launch may be queued)
        lddy = lddy or self.cout_p
        if self.kind == "1x1":
            M = x.shape[0]
            aeff = x[:, :self.cin]
        else:
            ho, wo = self.out_hw(h, w)
            M = n_img * T * h * w if self.kind == "t3" else n_img * ho * wo
            g = self._gather(n_img, ho if self.ups else h, wo if self.ups else w, ho, wo, self.cin_p, self.cin_p, T=T, hw=h * w) if self.kind != "t3" \
                else self._gather(n_img, 0, 0, 0, 0, self.cin_p, self.cin_p, T=T, hw=h * w)
            aeff = gathered_operand(x, g, M)[:, :self.taps * self.cin_p].view(M, self.taps, self.cin_p)[:, :, :self.cin]
        d = dy[:M, :self.cout].float()
        ref = self.out_scale * (d.t() @ aeff.reshape(M, -1).float()).view(self.cout, self.taps, self.cin).permute(0, 2, 1)
        got = self.w_grad.view(self.cout, self.cin, self.taps)
        refb = self.out_scale * d.sum(0)
        scale = float(ref.abs().max()) + 1e-30
        row = dict(conv=names.get(id(self), "?"), kind=self.kind, stride=self.stride, ups=bool(self.ups), cin=self.cin, cout=self.cout, R=M,
                   alpha=self.out_scale, w_err=float((got - ref).abs().max()) / scale, w_max=scale,
                   b_err=float((self.b_grad - refb).abs().max()) / (float(refb.abs().max()) + 1e-30), finite=bool(torch.isfinite(got).all()))
        report.append(row)
    ops.ConvOp.bwd_dw = checked
    tr.zero_grad()
    tr.forward_backward(**batch)
    ops.ConvOp.bwd_dw = orig
    torch.cuda.synchronize()
    worst = {}
    for r in report:
        key = f"{r['kind']} s{r['stride']}{' ups' if r['ups'] else ''}"
        if key not in worst or r["w_err"] > worst[key]["w_err"]:
            worst[key] = r
    print(f"# {len(report)} weight-gradient calls checked against the materialised path; worst per kind (error / largest |reference| of the tensor):")
    for key, r in sorted(worst.items()):
        print(f"  {key:10s} {r['conv']:60s} cin {r['cin']:5d} cout {r['cout']:5d} R {r['R']:6d} alpha {r['alpha']:.3f}  weight {r['w_err']:.2e}  bias {r['b_err']:.2e}")
    special = [r for r in report if r["conv"] in ("conv_in", "conv_out")]
    for r in special:
        print(f"  {r['conv']:10s} cin {r['cin']} cout {r['cout']}  weight {r['w_err']:.2e}  bias {r['b_err']:.2e}")
    bad = [r for r in report if not (r["w_err"] < 2e-3 and r["b_err"] < 2e-3 and r["finite"])]
    print(f"# calls beyond 2e-3: {len(bad)}", bad[:5])
    tr.optimizer_step()
    steps = []
    for s in range(args.steps):
        pack_bad = check_packs(model, rt, ops)
        tr.step(batch)
        torch.cuda.synchronize()
        st = tr.opt_state.cpu().tolist()
        loss = float(tr.loss_slot.cpu())
        steps.append(dict(step=s + 2, loss=loss, skipped=st[7], opt_steps=st[0], loss_scale=st[1], repack_mismatches=pack_bad))
        print(f"# step {s + 2}: loss {loss:.6f} skipped {st[7]:.0f} optimizer steps {st[0]:.0f} loss scale {st[1]:g} re-pack mismatches {pack_bad}", flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(calls=report, steps=steps, lr=args.lr), f, indent=1)


def conv_names(model):
    out = [("conv_in", model.cin_op), ("conv_out", model.cout_op)]
    for name, m in model.named_modules():
        for attr in ("c1", "c2", "sc", "op"):
            op = m.__dict__.get(attr)
            if op is not None and op.__class__.__name__ == "ConvOp":
                out.append((f"{name}.{attr}", op))
    return out


def check_packs(model, rt, ops):
    """every trainable convolution's w / wd against ConvOp.pack's torch statements on the current master: number of tensors that differ"""
    bad = 0
    for op in model._conv_ops:
        if not op.trainable:
            continue
        W = op.weight.data * op.out_scale if op.out_scale != 1.0 else op.weight.data
        w4 = W.reshape(op.cout, op.cin, op.taps)
        wp = torch.zeros(op.cout, op.taps, op.cin_p, dtype=torch.float32, device=W.device)
        wp[:, :, :op.cin] = w4.permute(0, 2, 1)
        bad += int(not torch.equal(wp.to(rt.dt).view(-1), op.w.view(-1)))
        if op.wd is not None:
            src = w4.flip(2) if (op.kind in ("3x3", "t3") and op.stride == 1) else w4
            wd = torch.zeros(op.cin, op.taps, op.cout_p, dtype=torch.float32, device=W.device)
            wd[:, :, :op.cout] = src.permute(1, 2, 0)
            bad += int(not torch.equal(wd.to(rt.dt).view(-1), op.wd.view(-1)))
    return bad


if __name__ == "__main__":
    main()
