"""The train step's launches at geometries beyond the two benchmarked, on the MI355X (`-m gpu`): every distinct signature of the six edge
geometries of tests/census.py (GEOM_EDGE: latents down to 8x8 -- attention over 64, 16, 4 and 1 keys, 1x1 and 2x2 convolutions, one
pixel per frame --, a 3x5 deepest level, batches of 2 and 3, 1, 16 and 17 frames) and one signature for every dispatch class of the
geometry grid (GEOM_GRID) that neither those nor the step's own configurations reach, through HipBackend on operands rebuilt from the
signature, judged element by element against the float64 reference (tests/ref64.py) computed on the device.  The bounds are the census's
derived ones.  tests/test_census_geom.py asserts on the CPU that this selection reaches every dispatch class of the grid; the grid
samples an unbounded domain, so a geometry outside it may still reach a class that nothing runs.  The dispatch class holds how far the
operands reach in memory (census.reach_key): batch 2 of config 4 puts A, or C and the GEGLU operand, of four GEMM classes and A of one
gemm_tn class beyond 2^31 bytes, where svdx_gemm / svdx_gemm_tn take other code; those run here at their real shape (M = 460800).

The host-only recording of the geometries sits in a module-scoped fixture; the signatures of a part are dealt into pieces of about
equal cost so that each test takes a few seconds.  profiles/census_geom_gpu.txt has what was measured."""
import collections
import time

import pytest
import torch

import census
from svd_xtend_amd import kernels as K

pytestmark = pytest.mark.gpu

# part -> pieces.  A signature costs about 12 ms whatever it is (operands, launch, judging) plus its float64 reference, which the cost
# model of `_deal` puts at 5e11 units a second: the pieces come to 2 - 3 s each (profiles/census_geom_gpu.txt); the seven signatures of
# "grid_reach" (M = 460800, operands of 2.2 GiB) get a piece each (profiles/reach_gpu.txt)
PIECES = collections.OrderedDict([("e_1x1x8x8", 2), ("e_3x5x8x24", 4), ("e_1x14x24x40", 3), ("e_2x16x16x8", 7), ("e_1x17x16x24", 4),
                                  ("e_2x14x40x64", 3), ("grid", 13), ("grid_reach", 7)])
CASES = [(name, i, k) for name, k in PIECES.items() for i in range(k)]
_SEEN = {}
_WORST = collections.defaultdict(float)
_TIMES = collections.OrderedDict()


def _cost(s):
    """float64 reference of a GEMM: M N K multiply-adds (through the temporal gather a conv1d over short sequences, whose time goes with
    M (N + 128)); of the spatial attention: the S x S score matrices of every head; plus the fixed cost of any signature"""
    a = census.sig_args(s)
    fixed = 6 * 10 ** 9
    if s[0] == "gemm":
        g = a["gather"]
        if a["out_mode"] == K.OUT_F32_SLAB:          # one reference per slice, each a float64 convolution of all images with the masked weight
            return fixed + a["split_k"] * (a["N"] * a["K"] * 90 * (g.n_img if g is not None else 1) + a["M"] * a["N"] * a["K"] // 7)
        return fixed + (a["M"] * (a["N"] + 128) * 4000 if g is not None and g.mode == K.GATHER_TEMPORAL3 else a["M"] * a["N"] * a["K"] // 7)
    if s[0] == "gemm_tn":
        return fixed + a["R"] * a["N"] * a["K"] // 7
    if s[0] in ("attn_fwd", "attn_bwd_dkv", "attn_bwd_dq"):
        return fixed + a["nb"] * a["heads"] * a["S"] * a["S"] * 64
    return fixed


def _deal(sigs, pieces):
    out, load = [[] for _ in range(pieces)], [0] * pieces
    for s in sorted(sigs, key=lambda s: (-_cost(s), repr(s))):
        i = load.index(min(load))
        out[i].append(s)
        load[i] += _cost(s)
    return out


@pytest.fixture(scope="module")
def hip():
    return K.HipBackend()


@pytest.fixture(scope="module")
def recorded():
    """{part: [pieces of signatures]}: the host-only recording (no kernel runs), once for the module.  A signature several parts share
    belongs to the first."""
    t0 = time.time()
    parts = census.geom_gpu_signatures()
    assert list(parts) == list(PIECES), (list(parts), list(PIECES))
    taken, dealt, counts = set(), {}, {}
    for name, c in parts.items():
        launches, distinct, checked, allowed, missing = census.coverage(c)
        assert not missing, f"{name}: entries with neither a runner nor an allow-list entry: {missing}"
        mine = sorted((s for s in c if s[0] in census.RUNNERS and s not in taken), key=repr)
        taken.update(mine)
        dealt[name], counts[name] = _deal(mine, PIECES[name]), (distinct, len(mine))
    _TIMES["recording fixture"] = time.time() - t0
    print(f"\nrecording: {len(census.GEOM_EDGE)} edge and {len(census.GEOM_GRID)} grid geometries in {_TIMES['recording fixture']:.1f} s; "
          f"{len(taken)} signatures to run: " + ", ".join(f"{n} {m} (of {d} distinct)" for n, (d, m) in counts.items()))
    return dealt


@pytest.mark.parametrize("name,piece,pieces", CASES, ids=[f"{n}-{i + 1}of{k}" for n, i, k in CASES])
def test_every_launch_of_the_geometry_meets_float64_reference(hip, recorded, name, piece, pieces):
    mine = recorded[name][piece]
    bad, t0 = [], time.time()
    for sig in mine:
        assert sig not in _SEEN
        t1 = time.time()
        _SEEN[sig] = res = census.run_case(hip, sig, "cuda")
        if time.time() - t1 > 1.0:
            print(f"\n{time.time() - t1:.1f} s: {census.sig_str(sig, 300)}")
        for label, excess, idx in res:
            fam = census.family(sig, label)
            _WORST[fam] = max(_WORST[fam], excess)
            if not excess <= 1.0:
                bad.append(f"excess {excess:.4g} at {idx}: {label}: {census.sig_str(sig, 700)}")
        if torch.cuda.memory_reserved() > 120e9:
            torch.cuda.empty_cache()
    torch.cuda.empty_cache()
    _TIMES[f"{name} {piece + 1}/{pieces}"] = time.time() - t0
    print(f"\n{name} piece {piece + 1} of {pieces}: {len(mine)} signatures, {time.time() - t0:.1f} s")
    if (name, piece + 1) == (CASES[-1][0], CASES[-1][2]):
        print(f"{len(_SEEN)} signatures in all; time per part: " + ", ".join(f"{k} {v:.1f} s" for k, v in _TIMES.items()))
        print("worst excess (error / bound) per family, all parts:")
        for fam, w in sorted(_WORST.items()):
            print(f"{w:10.4f}  {fam}")
    assert not bad, f"{len(bad)} outputs beyond their bound:\n" + "\n".join(bad[:25])
