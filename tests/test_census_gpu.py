"""Every launch of the train step on the MI355X (`-m gpu`): each distinct signature of the launch census of configurations 2, 2 + clipping,
5 (both parameter-dtype modes) and 4 (tests/census.py) through HipBackend on operands rebuilt from the signature, judged element by element
against the float64 reference (tests/ref64.py) computed on the device.  A signature several configurations share runs once.  What this
covers is every launch ALONE at its real shape, pitch, aliasing and feature combination; the composition of the launches stays with the
oracle tests (tests/test_e2e_gpu.py)."""
import collections
import time

import pytest
import torch

import census
import ref64
from svd_xtend_amd import kernels as K

pytestmark = pytest.mark.gpu

_SEEN = {}
_WORST = collections.defaultdict(float)


@pytest.fixture(scope="module")
def hip():
    return K.HipBackend()


@pytest.mark.parametrize("name", ["c2", "c2_clip", "c5", "c4"])
def test_every_launch_of_the_step_meets_float64_reference(hip, name):
    counts = collections.Counter(census.census(name))
    if name == "c5":                                    # the reference's bf16 parameter recipe: the signatures it adds (its optimizer launch)
        counts.update({s: n for s, n in census.census("c5_ref").items() if s not in counts})
    launches, distinct, checked, allowed, missing = census.coverage(counts)
    assert not missing, f"{name}: entries with neither a runner nor an allow-list entry: {missing}"
    assert sum(allowed.values()) <= census.ALLOW_FRACTION * launches, (dict(allowed), launches)
    bad, new, t0 = [], 0, time.time()
    for sig in counts:
        if sig[0] not in census.RUNNERS or sig in _SEEN:
            continue
        new += 1
        _SEEN[sig] = res = census.run_case(hip, sig, "cuda")
        for label, excess, idx in res:
            fam = census.family(sig, label)
            _WORST[fam] = max(_WORST[fam], excess)
            if not excess <= 1.0:
                bad.append(f"excess {excess:.4g} at {idx}: {label}: {census.sig_str(sig, 700)}")
        if torch.cuda.memory_reserved() > 120e9:
            torch.cuda.empty_cache()
    print(f"\n{name}: {launches} launches, {distinct} distinct signatures, {checked} checked ({new} run here, the others with an earlier "
          f"configuration), allow-listed launches {dict(allowed)} = {100.0 * sum(allowed.values()) / launches:.2f} %, {time.time() - t0:.1f} s")
    if name == "c4":
        print("worst excess (error / bound) per family, all configurations:")
        for fam, w in sorted(_WORST.items()):
            print(f"{w:10.4f}  {fam}")
    torch.cuda.empty_cache()
    assert not bad, f"{len(bad)} outputs beyond their bound:\n" + "\n".join(bad[:25])


def test_float64_reference_on_the_device_equals_the_cpu():
    """the device's float64 operators (convolutions as gathers, norms and attention through autograd) against the same functions on the CPU"""
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    cases = []
    n, h, w, ci, co = 2, 6, 8, 16, 24
    W9, W3 = r(co, 9 * ci), r(co, 3 * ci)
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    for ga, nsrc, M, W in [(K.Gather(K.GATHER_CONV3X3, n_img=n, hi=h, wi=w, ho=h, wo=w, cin=ci, stride=1, lda=ci), n * h * w, n * h * w, W9),
                           (K.Gather(K.GATHER_CONV3X3, n_img=n, hi=h, wi=w, ho=ho, wo=wo, cin=ci, stride=2, lda=ci), n * h * w, n * ho * wo, W9),
                           (K.Gather(K.GATHER_CONV3X3, n_img=n, hi=2 * h, wi=2 * w, ho=2 * h, wo=2 * w, cin=ci, stride=1, ups=1, lda=ci), n * h * w, 4 * n * h * w, W9),
                           (K.Gather(K.GATHER_CONV3X3_DGRAD2, n_img=n, hi=ho, wi=wo, ho=h, wo=w, cin=ci, lda=ci), n * ho * wo, n * h * w, W9),
                           (K.Gather(K.GATHER_CONV3X3_PAD0, n_img=n, hi=h, wi=w, ho=h - 2, wo=w - 2, cin=ci, stride=1, lda=ci), n * h * w, n * (h - 2) * (w - 2), W9),
                           (K.Gather(K.GATHER_TEMPORAL3, n_img=n, cin=ci, t=5, hw=7, lda=ci), n * 5 * 7, n * 5 * 7, W3)]:
        src = r(nsrc, ci)
        cases.append((f"gather mode {ga.mode} stride {ga.stride} ups {ga.ups}", lambda dev, src=src, W=W, ga=ga, M=M: [ref64.gather_matmul(src.to(dev), W.to(dev), ga, M)]))
    x, dy, gam, bet = r(3 * 20, 64), r(3 * 20, 64), r(64), r(64)
    cases.append(("group norm", lambda dev: list(ref64.gn_bwd(dy.to(dev), x.to(dev), gam.to(dev), bet.to(dev), 3, 20, 64, 32, 1e-6, True))
                  + [ref64.gn_fwd(x.to(dev), gam.to(dev), bet.to(dev), 3, 20, 64, 32, 1e-6, True)]))
    cases.append(("layer norm", lambda dev: list(ref64.ln_bwd(dy.to(dev), x.to(dev), gam.to(dev), 1e-5)) + list(ref64.ln_fwd(x.to(dev), gam.to(dev), bet.to(dev), 1e-5))))
    q, k, v, do = r(2, 3, 50, 64), r(2, 3, 50, 64), r(2, 3, 50, 64), r(2, 3, 50, 64)
    cases.append(("attention", lambda dev: list(ref64.attention(q.to(dev), k.to(dev), v.to(dev), 0.125)) + list(ref64.attention_bwd(q.to(dev), k.to(dev), v.to(dev), do.to(dev), 0.125))))
    pre, dh = r(30, 128), r(30, 64)
    cases.append(("geglu", lambda dev: [ref64.geglu(pre.to(dev), 64), ref64.geglu_bwd(dh.to(dev), pre.to(dev), 64)]))
    p4, sg = r(2, 3, 4, 40), r(2).abs() + 0.3
    cases.append(("edm loss", lambda dev: list(ref64.edm_loss(p4.to(dev), p4.flip(0).to(dev), p4.flip(1).to(dev), sg.to(dev), 1024.0))))
    pp, gg, mm, vv = r(500), r(500), r(500), r(500).abs()
    cases.append(("adamw", lambda dev: list(ref64.adamw_step(pp.to(dev), gg.to(dev), mm.to(dev), vv.to(dev), 1e-3, 0.9, 0.999, 1e-8, 1e-2, 3))))
    for label, fn in cases:
        for a, b in zip(fn("cpu"), fn("cuda")):
            err = float((a - b.cpu()).abs().max() / (a.abs().max() + 1e-300))
            print(f"{label}: {err:.2e}")
            assert err <= 1e-12, (label, err)
