"""Shared checks of the convolution weight gradient (svdx_gemm_tn_gather, svdx_conv_wgrad_finalize, svdx_conv_pack): the kernel cases,
their float64 reference (autograd through the float64 convolutions of tests/ref64.py), the error bound, and the runners the simulator
(tests/test_conv_wgrad.py) and the device (tests/test_conv_wgrad_gpu.py) both use.  The emulation of the three entries is
emul.EmuBackend's; the step against the oracle is selection_checks.py's.  TEST INFRASTRUCTURE."""
from typing import NamedTuple

import torch

import ref64
from census import _ratio, ulp_of
from selection_checks import COS_BAR
from svd_xtend_amd import kernels as K

SENTINEL = 77.0                  # exact in fp16, bf16 and fp32
GUARD = 64                       # elements of sentinel on either side of every buffer (>= 128 bytes: the payload stays 16-byte aligned)
DT = {"f16": torch.float16, "bf16": torch.bfloat16}


class Case(NamedTuple):
    """One convolution.  3x3: n_img images of h x w source pixels (`ups`: stored at h x w, read through nearest x2), stride 1 | 2;
    t3: n_img clips of T frames of hw = h * w pixels.  cin / cout real channels, cin_p / cout_p the padded counts the GEMM sees
    (cout_p = the row pitch of dY and the N of the launch)."""
    name: str
    kind: str
    n_img: int
    h: int
    w: int
    cin: int
    cin_p: int
    cout: int
    cout_p: int
    stride: int = 1
    ups: int = 0
    T: int = 0
    alpha: float = 1.0


CASES = [
    Case("3x3_s1_5x3_borders", "3x3", 3, 5, 3, 64, 64, 64, 64),                                    # R = 45 < one 64-row tile: every border
    Case("3x3_s1_8x8_c320", "3x3", 2, 8, 8, 320, 320, 320, 320, alpha=0.37),                       # taps straddle the 128-column tiles; N = 2.5 tiles
    Case("3x3_s2_5x3", "3x3", 2, 5, 3, 64, 64, 64, 64, stride=2),
    Case("3x3_s2_8x8", "3x3", 2, 8, 8, 64, 64, 64, 64, stride=2, alpha=-1.75),
    Case("3x3_ups_4x4", "3x3", 2, 4, 4, 64, 64, 64, 64, ups=1),
    Case("3x3_conv_in_cin8", "3x3", 1, 8, 8, 8, 64, 64, 64),                                       # padded input channels dropped
    Case("3x3_conv_out_cout4", "3x3", 1, 8, 8, 64, 64, 4, 64),                                     # padded output channels dropped
    Case("3x3_s1_16x16_split8", "3x3", 2, 16, 16, 64, 64, 64, 64),                                 # R = 512: eight row tiles, split_k up to 8
] + [Case(f"t3_T{T}_c64", "t3", 2, 5, 3, 64, 64, 64, 64, T=T, alpha=0.625 if T == 3 else 1.0) for T in (1, 2, 3, 14)] \
  + [Case(f"t3_T{T}_c320", "t3", 2, 5, 3, 320, 320, 320, 320, T=T) for T in (1, 2, 3, 14)]
BY_NAME = {c.name: c for c in CASES}


def taps_of(c: Case) -> int:
    return 3 if c.kind == "t3" else 9


def out_hw(c: Case):
    if c.ups:
        return 2 * c.h, 2 * c.w
    if c.stride == 2:
        return (c.h - 1) // 2 + 1, (c.w - 1) // 2 + 1
    return c.h, c.w


def rows_of(c: Case) -> int:
    ho, wo = out_hw(c)
    return c.n_img * c.T * c.h * c.w if c.kind == "t3" else c.n_img * ho * wo


def src_rows_of(c: Case) -> int:
    return c.n_img * (c.T if c.kind == "t3" else 1) * c.h * c.w


def gather_of(c: Case, cin: int, lda: int) -> K.Gather:
    if c.kind == "t3":
        return K.Gather(K.GATHER_TEMPORAL3, n_img=c.n_img, cin=cin, t=c.T, hw=c.h * c.w, lda=lda)
    ho, wo = out_hw(c)
    return K.Gather(K.GATHER_CONV3X3, n_img=c.n_img, hi=ho if c.ups else c.h, wi=wo if c.ups else c.w, ho=ho, wo=wo, cin=cin, stride=c.stride,
                    ups=c.ups, lda=lda)


def splits_of(c: Case):
    """the split_k of {1, 2, 4, 8} the row tiles allow (no slice without rows: the entry's own argument check)"""
    rt = (rows_of(c) + 63) // 64
    return [s for s in (1, 2, 4, 8) if s == 1 or -(-rt // s) * (s - 1) < rt]


# ---- operands and the float64 reference ---------------------------------------------------------------------------------------------
def operands(c: Case, dt: torch.dtype, seed: int = 0):
    """(x [source rows, cin_p], dy [R, cout_p]) in `dt`, randn -- the PADDED channels too (the finalize has to drop them) -- and the
    float values an accumulating launch finds in the gradients (c0_w [cout, cin, taps], c0_b [cout])."""
    g = torch.Generator().manual_seed(97 * seed + 13 * len(c.name) + rows_of(c) + c.cin_p)
    x = torch.randn(src_rows_of(c), c.cin_p, generator=g).to(dt)
    dy = torch.randn(rows_of(c), c.cout_p, generator=g).to(dt)
    return x, dy, torch.randn(c.cout, c.cin, taps_of(c), generator=g), torch.randn(c.cout, generator=g)


@torch.enable_grad()
def _dw64(c: Case, x, dy):
    """d/dW of sum(dy * conv(x, W)) through ref64.gather_matmul in float64, in the parameter's layout [cout, cin, taps]"""
    taps = taps_of(c)
    W = torch.zeros(c.cout, taps * c.cin, dtype=torch.float64, requires_grad=True)
    y = ref64.gather_matmul(x[:, :c.cin].contiguous(), W, gather_of(c, c.cin, c.cin), rows_of(c))
    (dW,) = torch.autograd.grad(y, W, ref64.d(dy[:, :c.cout]))
    return dW.view(c.cout, taps, c.cin).permute(0, 2, 1).contiguous()


def reference(c: Case, x, dy):
    """float64: (dW, S = sum |dy| |x|, in-image products per element) [cout, cin, taps]; (db, sum |dy|) [cout]; not yet times alpha"""
    dW = _dw64(c, x, dy)
    S = _dw64(c, x.abs(), dy.abs())
    cnt = _dw64(c, torch.ones_like(x), torch.ones_like(dy))
    d = ref64.d(dy[:, :c.cout])
    return dW, S, cnt, d.sum(0), d.abs().sum(0)


def bounds(c: Case, ref, nsplit: int, c0_w=None, c0_b=None):
    """Per element: the census' svdx_gemm_tn bound 0.5 ulp_fp32(ref) + (k_acc + 1) 2^-23 S, k_acc = the in-image products + the slabs
    added + one rounding for alpha (+ one for the value an accumulating launch adds to).  -> (ref_w, bound_w, ref_b, bound_b)"""
    dW, S, cnt, db, Sb = ref
    a = float(torch.tensor(c.alpha, dtype=torch.float32))            # the float the binding passes
    vw, Sw, kw = a * dW, abs(a) * S, cnt + nsplit + 1
    vb, Sbb, kb = a * db, abs(a) * Sb, rows_of(c) + nsplit + 1
    if c0_w is not None:
        vw, Sw, kw = vw + ref64.d(c0_w), Sw + ref64.d(c0_w).abs(), kw + 1
        vb, Sbb, kb = vb + ref64.d(c0_b), Sbb + ref64.d(c0_b).abs(), kb + 1
    bw = 0.5 * ulp_of(vw, torch.float32) + (kw + 1) * 2.0 ** -23 * Sw
    bb = 0.5 * ulp_of(vb, torch.float32) + (kb + 1) * 2.0 ** -23 * Sbb
    return vw, bw, vb, bb


def significant(ref, bound, cnt=None) -> float:
    """fraction of the reference elements that exceed 10 x their bound: a kernel that drops a tap, or writes zeros, cannot pass then.
    DELIBERATE DEPARTURE from the rule as first worded ("at least 95 % of a case's reference elements"): with cnt -- the in-image products
    per element -- an element WITHOUT any product (the outer taps of a one-frame clip, T = 1: two thirds of that case) is a structural
    zero and is left out of the fraction.  This loosens nothing: no bound is widened, and such an element's bound is that of an empty sum
    (half the smallest fp32 subnormal), so only an exact zero passes there; the 95 % must hold over every other element."""
    big = ref.abs() > 10 * bound
    return float((big if cnt is None else big[cnt > 0]).double().mean())


_REF_CACHE = {}


def case_reference(c: Case, dt: torch.dtype):
    """operands and reference of a case, computed once per (case, dtype) and shared by the tests that need them (never modified)"""
    key = (c, dt)
    if key not in _REF_CACHE:
        x, dy, c0_w, c0_b = operands(c, dt)
        _REF_CACHE[key] = (x, dy, c0_w, c0_b, reference(c, x, dy))
    return _REF_CACHE[key]


# ---- buffers between guard bands ------------------------------------------------------------------------------------------------------
def banded(fill: torch.Tensor, dev):
    """`fill` inside a sentinel-filled flat buffer on `dev`: (flat, payload view of fill's shape)"""
    n = fill.numel()
    flat = torch.full((2 * GUARD + n,), SENTINEL, dtype=fill.dtype)
    flat[GUARD:GUARD + n] = fill.reshape(-1)
    flat = flat.to(dev)
    return flat, flat[GUARD:GUARD + n].view(fill.shape)


def bands_intact(flats) -> None:
    for name, flat in flats.items():
        lo, hi = flat[:GUARD].cpu().float(), flat[-GUARD:].cpu().float()            # (the bands alone: a pitched buffer holds gigabytes between them)
        assert bool((lo == SENTINEL).all()) and bool((hi == SENTINEL).all()), f"{name}: guard band written"


def pitched(fill: torch.Tensor, ld: int, dev):
    """the rows of `fill` at a pitch of `ld` elements inside a zeroed, sentinel-banded flat buffer on `dev` (allocated there: only the
    rows are touched): (flat, strided view of fill's shape)"""
    rows, cols = fill.shape
    n = (rows - 1) * ld + cols
    flat = torch.zeros(2 * GUARD + n, dtype=fill.dtype, device=dev)
    flat[:GUARD] = SENTINEL
    flat[-GUARD:] = SENTINEL
    view = torch.as_strided(flat, (rows, cols), (ld, 1), GUARD)
    view.copy_(fill.to(dev))
    return flat, view


def run_case(be, dev, c: Case, dt: torch.dtype, split_k: int, store: bool, slab: bool = True, stages: int = 0, verbose: bool = False, ld_dy: int = 0):
    """svdx_gemm_tn_gather + svdx_conv_wgrad_finalize of one case on `dev` against the float64 reference, per element; every buffer
    between guard bands, the operands unchanged.  ld_dy: the pitch of dY's rows where it is not cout_p (tests/reach_checks.py).
    slab=False (split_k 1): the kernel's own store mode (SVDX_OUT_F32) feeds the finalize,
    its column sums accumulate into a zeroed row, and its non-finite flag stays down.  -> worst error / bound (weight, bias)."""
    x, dy, c0_w, c0_b, ref = case_reference(c, dt)
    taps, R, N, Kd = taps_of(c), rows_of(c), c.cout_p, taps_of(c) * c.cin_p
    vw, bw, vb, bb = bounds(c, ref, split_k, None if store else c0_w, None if store else c0_b)
    assert significant(vw, bw, ref[2]) >= 0.95 and significant(vb, bb) >= 0.95, (c.name, significant(vw, bw, ref[2]), significant(vb, bb))
    nan = float("nan")
    flats, dv = {}, {}
    for name, t in (("x", x), ("dy", dy), ("slabs", torch.full((split_k, N, Kd), nan)),
                    ("cs", torch.full((split_k, N), nan) if slab else torch.zeros(1, N)),
                    ("w_grad", torch.full_like(c0_w, nan) if store else c0_w), ("b_grad", torch.full_like(c0_b, nan) if store else c0_b),
                    ("found", torch.zeros(4))):
        flats[name], dv[name] = pitched(t, ld_dy, dev) if (name == "dy" and ld_dy) else banded(t, dev)
    g = gather_of(c, c.cin_p, c.cin_p)
    if slab:
        be.gemm_tn_gather(dv["dy"], dv["x"], dv["slabs"], R, N, ld_dy or c.cout_p, Kd, g, out_mode=K.OUT_F32_SLAB, split_k=split_k, a_colsum=dv["cs"], stages=stages)
    else:
        assert split_k == 1
        be.gemm_tn_gather(dv["dy"], dv["x"], dv["slabs"], R, N, ld_dy or c.cout_p, Kd, g, out_mode=K.OUT_F32, a_colsum=dv["cs"], stages=stages, found_inf=dv["found"][0:1])
    be.conv_wgrad_finalize(dv["slabs"], split_k, N * Kd, Kd, dv["w_grad"], c.cout, c.cin, c.cin_p, taps, alpha=c.alpha, store=store,
                           colsum_slabs=dv["cs"], colsum_ld=N, b_grad=dv["b_grad"], found_inf=dv["found"][1:2])
    if str(dev) != "cpu":
        torch.cuda.synchronize()
    rw = _ratio(dv["w_grad"].cpu(), vw, bw)
    rb = _ratio(dv["b_grad"].cpu(), vb, bb)
    worst = (float(rw.max()), float(rb.max()))
    if verbose:
        print(f"{c.name} {dt} split_k={split_k} store={store} slab={slab}: worst error / bound weight {worst[0]:.3f} bias {worst[1]:.3f}")
    assert worst[0] <= 1.0 and worst[1] <= 1.0, (c.name, dt, split_k, store, worst, int((rw > 1).sum()), int((rb > 1).sum()))
    assert bool((dv["found"].cpu() == 0).all()), "non-finite flag raised on finite gradients"
    bands_intact(flats)
    assert torch.equal(dv["x"].cpu(), x) and torch.equal(dv["dy"].cpu(), dy), "operand modified"
    return worst


def sweep_case(be, dev, c: Case, dt: torch.dtype, verbose: bool = False):
    """every split_k the case allows, store and add alternating, plus the kernel's own store mode"""
    for i, sk in enumerate(splits_of(c)):
        run_case(be, dev, c, dt, sk, store=i % 2 == 0, verbose=verbose)
        if sk == max(splits_of(c)):
            run_case(be, dev, c, dt, sk, store=i % 2 == 1, stages=3 if sk > 1 else 0, verbose=verbose)
    run_case(be, dev, c, dt, 1, store=True, slab=False, verbose=verbose)


# ---- svdx_conv_pack against ConvOp.pack ----------------------------------------------------------------------------------------------
# (kind, stride, cout, cin, cin_p, cout_p): flipped (3x3 / t3 at stride 1) and unflipped (stride 2, 1x1) data-gradient forms, padded channels
PACK_SHAPES = [("3x3", 1, 64, 64, 64, 64), ("3x3", 2, 64, 64, 64, 64), ("t3", 1, 64, 64, 64, 64), ("3x3", 1, 40, 8, 64, 64),
               ("3x3", 1, 4, 72, 128, 64), ("t3", 1, 24, 40, 64, 32), ("1x1", 1, 72, 40, 64, 128)]


def run_pack(dev, dt: torch.dtype, shape, out_scale: float, need_dx: bool = True):
    """`ConvOp.refresh` (svdx_conv_pack through the installed backend) on fresh, banded w / wd against `ConvOp.pack`'s torch statements on
    the same master: torch.equal, the padded lanes zero, the guard bands and the master untouched."""
    from svd_xtend_amd import ops
    kind, stride, cout, cin, cin_p, cout_p = shape
    g = torch.Generator().manual_seed(cout * 131 + cin + int(out_scale * 100))
    wshape = dict([("3x3", (cout, cin, 3, 3)), ("t3", (cout, cin, 3, 1, 1)), ("1x1", (cout, cin, 1, 1))])[kind]
    weight = torch.nn.Parameter(torch.randn(*wshape, generator=g).to(dev), requires_grad=False)
    bias = torch.nn.Parameter(torch.randn(cout, generator=g).to(dev), requires_grad=False)
    rt = ops.Runtime(dt, torch.device(dev))
    op = ops.ConvOp(weight, bias, kind, stride=stride, cin_pad=cin_p, cout_pad=cout_p)
    op.pack(rt, need_dx=need_dx, out_scale=out_scale)
    want_w, want_wd, want_b = op.w, op.wd, op.b.clone()
    flats = {}
    flats["master"], master = banded(weight.data.cpu(), dev)
    weight.data = master
    flats["w"], op.w = banded(torch.full(tuple(want_w.shape), 3.0, dtype=dt), dev)
    if need_dx:
        flats["wd"], op.wd = banded(torch.full(tuple(want_wd.shape), 3.0, dtype=dt), dev)
    if out_scale != 1.0:
        flats["b"], op.b = banded(torch.full((cout,), 3.0), dev)
    op.refresh(rt)
    if str(dev) != "cpu":
        torch.cuda.synchronize()
    assert torch.equal(op.w, want_w), (shape, out_scale, int((op.w != want_w).sum()))
    assert not need_dx or torch.equal(op.wd, want_wd), (shape, out_scale, int((op.wd != want_wd).sum()))
    assert torch.equal(op.b, want_b)
    taps = op.taps
    assert bool((op.w.view(cout, taps, cin_p)[:, :, cin:] == 0).all())
    assert not need_dx or bool((op.wd.view(cin, taps, cout_p)[:, :, cout:] == 0).all())
    bands_intact(flats)
    assert torch.equal(master.cpu().view(-1), flats["master"].cpu()[GUARD:-GUARD])


# ---- one optimizer step of the tiny topology with trainable convolutions (selection_checks.py), against the CPU oracle -------------------
CONV_AND_TEMPORAL = ("temporal_transformer_block", "@conv")


def assert_step_parity(key, ref, got, bf16=False):
    """e2e_checks.assert_parity (loss, the cosine of EVERY trainable tensor's gradient at the project's 0.9995 / 0.995 bars, the updated
    parameters, pred_after: the forward through the re-packed weights) + the selection itself; the convolution tensors include both temporal
    conv2's, whose gradient carries the folded (1 - sigmoid(mix_factor))."""
    import e2e_checks
    assert sorted(got["grads"]) == ref["names"], (key, set(got["grads"]) ^ set(ref["names"]))
    conv = [n for n in ref["names"] if ".conv" in n or n.startswith("conv_")]
    assert any("temporal_res_block.conv2.weight" in n for n in conv) and "conv_in.weight" in conv and "conv_out.bias" in conv
    for n in conv:
        c = e2e_checks.cosine(got["grads"][n], ref["grads"][n])
        assert c >= COS_BAR[bf16], (key, n, c)
    r = e2e_checks.compare(ref, got)
    e2e_checks.assert_parity(key, r, bf16=bf16)
    return r
