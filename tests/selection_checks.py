"""A selection of the tiny topology (Trainer(trainable=...): substrings, "@conv", "@norm"), one optimizer step, against the CPU oracle:
the oracle's step and its cache, the product's step on any installed backend (tests/emul.py's emulation on the CPU, the library on the
device), the eager / captured / launch-plan runs and their bit comparison.  What is particular to one family of trainable tensors (its
selections, its assert_step_parity) stays in that family's checks module.  TEST INFRASTRUCTURE."""
import torch

STEP_GEOM = (1, 3, 16, 16)            # B, T, h, w
# the project's bars on the cosine of a gradient tensor against the oracle (e2e_checks.assert_parity)
COS_BAR = {False: 0.9995, True: 0.995}
_STEP_REFS = {}


def oracle_names(orc, which):
    """the rule of train.select_trainable, RESTATED for the oracle (torch's own nn.Conv2d / nn.Conv3d / nn.GroupNorm modules): the
    assert_step_parity functions hold the product's selection against it, so it must not call select_trainable"""
    rules = [which] if isinstance(which, str) else list(which)
    pick = set()
    if "@conv" in rules:
        pick |= {id(p) for m in orc.modules() if isinstance(m, (torch.nn.Conv2d, torch.nn.Conv3d)) for p in m.parameters()}
    if "@norm" in rules:
        pick |= {id(p) for m in orc.modules() if isinstance(m, torch.nn.GroupNorm) for p in m.parameters()}
    subs = [r for r in rules if r not in ("@conv", "@norm")]
    return [n for n, p in orc.named_parameters() if id(p) in pick or any(r in n for r in subs)]


def gn_names(orc_or_model):
    return sorted(f"{mn}.{pn}" for mn, m in orc_or_model.named_modules() if isinstance(m, torch.nn.GroupNorm) for pn, _ in m.named_parameters())


def oracle_step(which, seed=3, lr=1e-4, steps=1):
    """One torch.optim.AdamW step of the CPU oracle (fp32 autograd) with `which` trainable: loss, prediction, every gradient, the updated
    parameters and the prediction of the updated weights.  Computed once per selection and shared."""
    import copy
    from oracle.step import edm_inputs, edm_loss, make_synthetic_batch
    from oracle.unet import TINY_CONFIG, UNetSpatioTemporalConditionOracle, scaled_init_
    key = (tuple([which] if isinstance(which, str) else which), seed, lr, steps)
    if key in _STEP_REFS:
        return _STEP_REFS[key]
    cfg = TINY_CONFIG
    B, T, h, w = STEP_GEOM
    orc = UNetSpatioTemporalConditionOracle(**cfg)
    scaled_init_(orc, seed)
    names = set(oracle_names(orc, which))
    for n, p in orc.named_parameters():
        p.requires_grad_(n in names)
    batch = make_synthetic_batch(B, T, h, w, seed + 1, cross_dim=cfg["cross_attention_dim"])
    opt = torch.optim.AdamW([p for p in orc.parameters() if p.requires_grad], lr=lr, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8)
    sd0 = copy.deepcopy(orc.state_dict())
    unet_in, ts, ehs, ids, noisy, sig = edm_inputs(batch)
    pred = orc(unet_in, ts, ehs, added_time_ids=ids).sample
    loss = edm_loss(pred, noisy, batch["latents"], sig)
    loss.backward()
    grads = {n: p.grad.clone() for n, p in orc.named_parameters() if p.grad is not None}
    opt.step()
    params_after = {n: p.detach().clone() for n, p in orc.named_parameters() if p.requires_grad}
    with torch.no_grad():
        pred_after = orc(unet_in, ts, ehs, added_time_ids=ids).sample
    params_after2 = None
    if steps == 2:                                 # a second torch.optim.AdamW step on the same batch
        opt.zero_grad()
        edm_loss(orc(unet_in, ts, ehs, added_time_ids=ids).sample, noisy, batch["latents"], sig).backward()
        opt.step()
        params_after2 = {n: p.detach().clone() for n, p in orc.named_parameters() if p.requires_grad}
    _STEP_REFS[key] = dict(params_after2=params_after2, sd0=sd0, batch=batch, inputs=(unet_in, ts, ehs, ids, noisy), loss=float(loss.detach()), pred=pred.detach(),
                           pred_after=pred_after, lr=lr, grads=grads, params_after=params_after, names=sorted(names), traj=None)
    return _STEP_REFS[key]


def make_trainer(ref, which, dtype, dev, lr=None, **kw):
    from oracle.unet import TINY_CONFIG
    from svd_xtend_amd.train import Trainer
    from svd_xtend_amd.unet import UNetSpatioTemporalConditionModel
    m = UNetSpatioTemporalConditionModel(**TINY_CONFIG)
    m.load_state_dict(ref["sd0"], strict=True)
    m.to(dev)
    return Trainer(m, dtype=dtype, lr=lr or ref["lr"], trainable=which, **kw)


def step_batch(ref, dev):
    unet_in, ts, ehs, ids, noisy = (t.to(dev) for t in ref["inputs"])
    b = ref["batch"]
    return dict(unet_in=unet_in, timesteps=ts, ehs=ehs, added_time_ids=ids, noisy_latents=noisy, target=b["latents"].to(dev),
                sigmas=b["sigmas"].to(dev))


def product_step(ref, which, dtype, dev):
    """the same step through Trainer(trainable=which): what e2e_checks.compare / assert_parity read"""
    tr = make_trainer(ref, which, dtype, dev)
    m, b = tr.model, step_batch(ref, dev)
    with torch.no_grad():
        pred0 = m(b["unet_in"], b["timesteps"], b["ehs"], b["added_time_ids"]).sample.float().cpu()
    tr.zero_grad()
    tr.forward_backward(**b)
    loss = float(tr.last_loss())
    scale = float(tr.opt_state[1])
    grads = {n: (p.grad.detach().float().cpu() / scale) for n, p in m.named_parameters() if p.requires_grad}
    tr.optimizer_step()
    params = {n: p.detach().float().cpu() for n, p in m.named_parameters() if p.requires_grad}
    with torch.no_grad():
        pred = m(b["unet_in"], b["timesteps"], b["ehs"], b["added_time_ids"]).sample.float().cpu()
    return dict(loss=loss, grads=grads, params_after=params, pred=pred0, pred_after=pred, state=tr.opt_state.cpu().tolist(), trainer=tr)


def run_mode(ref, which, mode: str, steps: int = 3, dtype=torch.float16, lr: float = 1e-3):
    """`steps` optimizer steps on the device, eager (`Trainer.step`), as the captured step (train.GraphedStep: its warm-up pass is step 1)
    or as the launch plan recorded during that capture (svdx_plan_replay): masters, moments, loss and the packed convolution weights."""
    from svd_xtend_amd.train import GraphedStep
    tr = make_trainer(ref, which, dtype, "cuda", lr=lr)
    batch = step_batch(ref, "cuda")
    if mode == "eager":
        for _ in range(steps):
            tr.step(batch)
    else:
        gs = GraphedStep(tr, batch, record_plan=mode == "plan")
        for _ in range(steps - 1):
            gs.replay_plan() if mode == "plan" else gs()
    torch.cuda.synchronize()
    packed = [op for op in tr.model._conv_ops if op.trainable]
    return dict(p=tr.p_flat.clone(), m=tr.m_flat.clone(), v=tr.v_flat.clone(), loss=float(tr.loss_slot.cpu()), state=tr.opt_state.cpu().tolist(),
                w=[op.w.clone() for op in packed], wd=[op.wd.clone() for op in packed if op.wd is not None])


def assert_same_bits(a, b, what, min_packed=0):
    """two run_mode results agree bit for bit; min_packed: at least so many packed (trainable) convolution weights were compared"""
    assert a["loss"] == b["loss"] and a["state"] == b["state"], (what, a["loss"], b["loss"])
    for k in ("p", "m", "v"):
        assert torch.equal(a[k], b[k]), (what, k, float((a[k] - b[k]).abs().max()))
    assert len(a["w"]) == len(b["w"]) >= min_packed and all(torch.equal(x, y) for x, y in zip(a["w"], b["w"])), (what, "packed w")
    assert all(torch.equal(x, y) for x, y in zip(a["wd"], b["wd"])), (what, "packed wd")
