"""Every launch of the passes around the train step on the MI355X (`-m gpu`): each distinct signature of the VAE encode / decode, the CLIP
image path, the sampler's batch-2 UNet forward, weight packing and the EMA update (tests/census.py: COND_GPU) through HipBackend on
operands rebuilt from the signature, judged element by element against the float64 reference (tests/ref64.py) computed on the device.
A pass runs at the smallest geometries that reach the dispatch classes of the real workload, plus the signatures of the real geometry
whose class they do not reach (tests/test_census_cond.py asserts the union is complete).  A signature several parts share runs once.
Then all 65536 bit patterns of both 16-bit types through both activations of svdx_act_rows."""
import collections
import time

import pytest
import torch

import census
from svd_xtend_amd import kernels as K

pytestmark = pytest.mark.gpu

_SEEN = {}
# parts that take longer than about 10 s in one piece (the float64 temporal convolutions over 655360 rows): dealt into this many tests
SPLIT = {"decode_1x4x40x64": 4}
PARTS = [(what, name) for what in ("vae_encode", "vae_decode", "clip_image", "sampler_fwd", "pack", "ema")
         for name in census.COND_GPU[what] + ((census.COND_REAL[what],) if what in ("vae_encode", "vae_decode") else ())]
CASES = [(what, name, i, SPLIT.get(name, 1)) for what, name in PARTS for i in range(SPLIT.get(name, 1))]


def _deal(sigs, pieces):
    """the signatures in `pieces` lists of about equal cost: largest first, each to the list that has least so far.  Cost = seconds x 1e11,
    roughly, from profiles/census_cond_gpu.txt: the float64 reference of a GEMM is M N K multiply-adds; through the temporal gather it is a
    float64 conv1d over M / T short sequences, whose time goes with M (N + 128); everything else is small."""
    def cost(s):
        a = census.sig_args(s)
        if s[0] != "gemm":
            return 1
        g = a["gather"]
        return a["M"] * (a["N"] + 128) * 4000 if g is not None and g.mode == K.GATHER_TEMPORAL3 else a["M"] * a["N"] * a["K"] // 7
    out, load = [[] for _ in range(pieces)], [0] * pieces
    for s in sorted(sigs, key=lambda s: (-cost(s), repr(s))):
        i = load.index(min(load))
        out[i].append(s)
        load[i] += cost(s)
    return out


@pytest.fixture(scope="module")
def hip():
    return K.HipBackend()


@pytest.mark.parametrize("what,name,piece,pieces", CASES, ids=[f"{n}-{i + 1}of{k}" if k > 1 else n for _, n, i, k in CASES])
def test_every_launch_of_the_pass_meets_float64_reference(hip, what, name, piece, pieces):
    counts = census.cond_gpu_signatures(what)[name]
    launches, distinct, checked, allowed, missing = census.coverage(counts)
    assert not missing, f"{name}: entries with neither a runner nor an allow-list entry: {missing}"
    if name in census.COND_GPU[what]:                   # (a whole pass: the real geometry's part here is a selection of its signatures)
        assert sum(allowed.values()) <= census.ALLOW_FRACTION * launches, (dict(allowed), launches)
    mine = _deal(sorted((s for s in counts if s[0] in census.RUNNERS), key=repr), pieces)[piece]
    bad, new, worst, t0 = [], 0, collections.defaultdict(float), time.time()
    for sig in mine:
        if sig in _SEEN:
            continue
        new += 1
        t1 = time.time()
        _SEEN[sig] = res = census.run_case(hip, sig, "cuda")
        if time.time() - t1 > 1.0:
            print(f"\n{time.time() - t1:.1f} s: {census.sig_str(sig, 300)}")
        for label, excess, idx in res:
            fam = census.family(sig, label)
            worst[fam] = max(worst[fam], excess)
            if not excess <= 1.0:
                bad.append(f"excess {excess:.4g} at {idx}: {label}: {census.sig_str(sig, 700)}")
        if torch.cuda.memory_reserved() > 120e9:
            torch.cuda.empty_cache()
    print(f"\n{name}{f' piece {piece + 1} of {pieces}' if pieces > 1 else ''}: {launches} launches, {distinct} distinct signatures, {len(mine)} in "
          f"this test ({new} run here, the others with an earlier part), allow-listed launches {dict(allowed)}, {time.time() - t0:.1f} s")
    print("worst excess (error / bound) per family:")
    for fam, w in sorted(worst.items()):
        print(f"{w:10.4f}  {fam}")
    torch.cuda.empty_cache()
    assert not bad, f"{len(bad)} outputs beyond their bound:\n" + "\n".join(bad[:25])


@pytest.mark.parametrize("act", [0, 1], ids=["gelu", "quick_gelu"])
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_activation_at_every_16_bit_input(hip, dt, act):
    """one launch over all 65536 bit patterns: finite inputs within the derived bound of census.act_bound, NaN / infinite inputs in the
    reference's class"""
    res = census.run_act_exhaustive(hip, dt, act, "cuda")
    for label, excess, idx in res:
        print(f"{dt} act {act}: excess {excess:.4f} at bit pattern {idx}: {label}")
    assert all(e <= 1.0 for _, e, _ in res), res
