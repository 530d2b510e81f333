"""Shared checks of the latent cache (svd_xtend_amd/latent_cache.py, svdx_latent_batch): the torch statement block that DEFINES the
kernel's result (`statements`: it lives in tests/emul.py, whose EmuBackend.latent_batch is built on it) and the kernel cases the
simulator (tests/test_latent_cache.py) and the device (tests/test_latent_cache_gpu.py) both run.  TEST INFRASTRUCTURE."""
import itertools

import torch

from emul import latent_statements as statements

SENTINEL = 12345.678
GUARD = 64                       # floats of sentinel on either side of every buffer (256 bytes: keeps the payload 16-byte aligned)
SIGMAS = (1.3e-2, 1.0, 3e2)      # the +-5 sigma range of the loop's draw exp(N(0.7, 1.6))


# ---- kernel cases ---------------------------------------------------------------------------------------------------------------
# (c, h, w, T, B, byte offset of the cache base)
SHAPES = [(4, h, w, T, B, 0) for (h, w), T, B in itertools.product(((1, 1), (3, 5), (8, 8)), (1, 3, 14), (1, 2, 3))]
SHAPES.append((3, 1, 5, 3, 2, 0))        # c * h * w = 15: the scalar path and its tail
SHAPES.append((4, 3, 5, 3, 2, 4))        # 16-byte-able sizes behind a cache base 4 bytes off: the scalar path for want of alignment
EXTRA_FRAMES = 5                          # F = T + 5
PATTERNS = ("distinct", "equal", "overlapping", "zero", "last", "minus_one", "past_end")


def first_of(pattern: str, B: int, T: int, F: int):
    last = F - T
    return dict(distinct=[(2 * b) % (last + 1) for b in range(B)], equal=[2] * B, overlapping=[min(b, last) for b in range(B)],
                zero=[0] * B, last=[last] * B, minus_one=[-1] + [1] * (B - 1), past_end=[1] * (B - 1) + [F])[pattern]


def _banded(shape, dev, fill, offset_floats=0):
    """A tensor of `shape` inside a sentinel-filled flat buffer; returns (the flat buffer, the payload view)."""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((GUARD + offset_floats + n + GUARD,), SENTINEL, dtype=fill.dtype)
    flat[GUARD + offset_floats:GUARD + offset_floats + n] = fill.reshape(-1)
    flat = flat.to(dev)
    return flat, flat[GUARD + offset_floats:GUARD + offset_floats + n].view(shape)


def make_case(shape, pattern: str, k: int, seed: int = 0):
    """Host tensors of one kernel case: randn moments and draws (so that a contracted a + b * c is visible), keep of 0 and 1 in one
    batch, sigma walking SIGMAS."""
    c, h, w, T, B, off = shape
    F = T + EXTRA_FRAMES
    g = torch.Generator().manual_seed(1000 * seed + 7 * k + 13 * T + B + h * w)
    r = lambda *s: torch.randn(*s, generator=g)          # noqa: E731
    sigma = torch.tensor([SIGMAS[(b + k) % 3] for b in range(B)], dtype=torch.float32)
    t = dict(mean=r(F, c, h, w), std=r(F, c, h, w).abs(), eps=r(B, T + 1, c, h, w), noise=r(B, T, c, h, w), cond_mean=r(B, c, h, w),
             cond_std=r(B, c, h, w).abs(), sigma=sigma, den=(sigma ** 2 + 1) ** 0.5,
             keep=torch.tensor([float((b + k) % 2) for b in range(B)], dtype=torch.float32),
             first=torch.tensor(first_of(pattern, B, T, F), dtype=torch.int64))
    return t, 0.18215


def contraction_visible(t) -> int:
    """Elements where mean + std * eps rounded ONCE (the fused multiply-add a contracting compiler emits) differs from the two-rounding
    form the statements execute, over the frames a clamped window can read."""
    T = t["noise"].shape[1]
    m, s, e = t["mean"][:T], t["std"][:T], t["eps"][0, :T]
    fused = torch.addcmul(m.double(), s.double(), e.double()).float()
    return int((fused != m + s * e).sum())


def run_case(backend, dev, shape, pattern: str, k: int):
    """One launch of `backend.latent_batch` on `dev` against the statements on the CPU: all three outputs bit for bit, every guard band
    of every input and output untouched."""
    c, h, w, T, B, off = shape
    t, scaling = make_case(shape, pattern, k)
    want = statements(t["mean"], t["std"], t["first"], t["eps"], t["noise"], t["cond_mean"], t["cond_std"], t["sigma"], t["den"], t["keep"], scaling)
    flats, dv = {}, {}
    for name, x in t.items():
        flats[name], dv[name] = _banded(tuple(x.shape), dev, x, off // 4 if name in ("mean", "std") else 0)
    out_shapes = dict(unet_in=(B, T, 2 * c, h, w), noisy=(B, T, c, h, w), target=(B, T, c, h, w))
    for name, s in out_shapes.items():
        flats[name], dv[name] = _banded(s, dev, torch.full(s, SENTINEL))
    if off:
        assert dv["mean"].data_ptr() % 16 == off
    backend.latent_batch(dv["mean"], dv["std"], dv["first"], dv["eps"], dv["noise"], dv["cond_mean"], dv["cond_std"], dv["sigma"], dv["den"],
                         dv["keep"], scaling, dv["unet_in"], dv["noisy"], dv["target"])
    if dev != "cpu":
        torch.cuda.synchronize()
    for name, ref in zip(("unet_in", "noisy", "target"), want):
        got = dv[name].cpu()
        assert torch.equal(got, ref), (shape, pattern, name, int((got != ref).sum()), float((got - ref).abs().max()))
    for name, flat in flats.items():
        f = flat.cpu()
        lo = GUARD + (off // 4 if name in ("mean", "std") else 0)
        sent = torch.tensor(SENTINEL, dtype=f.dtype)
        assert bool((f[:lo] == sent).all()) and bool((f[-GUARD:] == sent).all()), (shape, pattern, name, "guard band written")
    for name, x in t.items():                                  # the inputs themselves are read-only
        assert torch.equal(dv[name].cpu(), x), (shape, pattern, name, "input modified")
