"""The launch census of the train step at geometries beyond the two benchmarked (tests/census.py: GEOM_EDGE, GEOM_GRID, GEOM_TINY) on the
CPU (`-m "not gpu"`): that what the GPU test runs reaches every dispatch class of the grid, that every entry launched has a runner, the
tiny topology at the edge geometries through the emulation and through the HIP sources on the simulator, the model's refusal of the
batch sizes its time-context ordering cannot serve, and the checker against faults planted at edge signatures.

GEOM_GRID samples an unbounded domain (any multiple of 8 for the latent's sides, any frame count, any batch size): a geometry outside
it may still reach a dispatch class that nothing runs.  How far the operands reach in memory is part of the class: the signatures of the
grid and of GEOM_REACH with an operand of 2^31 bytes or more are tabulated with the kernel they take, none of them is one the library
would refuse, and each of the grid's runs on the GPU at its own reach; tests/test_reach.py pins the line itself at small shapes."""
import collections
import os
import sys

import pytest
import torch

import census
import emul
from svd_xtend_amd import kernels as K

FULL = os.environ.get("SVDX_SIM_FULL") == "1"

# dispatch classes of GEOM_GRID that nothing on the GPU reaches: class -> reason.  Empty.
UNCOVERED = {}


def _run_all(be, sigs):
    bad, worst = [], collections.defaultdict(float)
    for sig in sigs:
        for label, excess, idx in census.run_case(be, sig):
            fam = census.family(sig, label)
            worst[fam] = max(worst[fam], excess)
            if not excess <= 1.0:
                bad.append(f"excess {excess:.3g} at {idx}: {label}: {census.sig_str(sig)}")
    return bad, worst


def _cost(sig):
    a = census.sig_args(sig)
    n = 1
    for k in ("M", "N", "K", "n", "rows", "C", "R", "S", "nb", "F"):
        if isinstance(a.get(k), int):
            n *= max(a[k], 1)
    return n


# ---- the tables ----------------------------------------------------------------------------------------------------------------------------
def test_geometry_tables_are_what_they_say():
    assert len(census.GEOM_EDGE) == 6 and all(c[0] == "svd" for c in census.GEOM_EDGE.values())
    grid = {(c[1], c[2], c[3]) for c in census.GEOM_GRID.values()}
    full = [g for g, dt, r in grid if r == 0]
    lora = [g for g, dt, r in grid if r == 64]
    # fp16 full: 2 x 5 x 5 less B = 2 at 8x8 and 24x40 (refused: odd deepest level); bf16 LoRA 64: 2 x 2 x 3 less the same
    assert len(full) == 50 - 10 and len(lora) == 12 - 4, (len(full), len(lora))
    assert all(not census.geom_refused(B, h, w) for (B, T, h, w) in full + lora)
    assert census.geom_refused(2, 8, 8) and census.geom_refused(2, 24, 40) and not census.geom_refused(2, 32, 32)
    # a geometry another table records is listed under that table's name: one recording
    assert {"c2", "e_1x1x8x8", "e_1x14x24x40", "e_2x14x40x64"} <= set(census.GEOM_GRID)
    assert not set(census.CONFIGS) & (set(census.GEOM_EDGE) | set(census.GEOM_TINY))
    # the tiny edge set: a 1x1 deepest level, a non-power-of-two one, B = 2 and 3, T = 1, T on both sides of 16
    tiny = [c[1] for c in census.GEOM_TINY.values()]
    assert any(h == 8 and w == 8 for _, _, h, w in tiny) and any((h // 8) * (w // 8) == 15 for _, _, h, w in tiny)
    assert {1, 2, 3} <= {B for B, _, _, _ in tiny} and {1, 16, 17} <= {T for _, T, _, _ in tiny}


def test_gpu_signatures_reach_every_dispatch_class_of_the_grid():
    parts = census.geom_gpu_signatures()
    run = {census.dispatch_class(s) for c in parts.values() for s in c}
    step = {census.dispatch_class(s) for n in census.STEP_GPU for s in census.census(n)}
    grid = {}
    for n in census.GEOM_GRID:
        for s in census.census(n):
            grid.setdefault(census.dispatch_class(s), s)
    edge = {census.dispatch_class(s) for n in census.GEOM_EDGE for s in census.census(n)}
    missing = [k for k in grid if k not in run and k not in step and k not in UNCOVERED]
    print(f"dispatch classes: the step's own configurations {len(step)}, the {len(census.GEOM_GRID)} grid geometries {len(grid)} "
          f"({len(grid.keys() - step)} of them new), the edge geometries {len(edge)} ({len(edge - step)} new); "
          f"grid classes run at an edge geometry {len((grid.keys() - step) & edge)}, at a grid signature of their own {len(parts['grid'])}")
    print("signatures per part: " + ", ".join(f"{n} {len(c)}" for n, c in parts.items()))
    per = collections.Counter(k[0] for k in grid.keys() - step)
    print(f"new classes by entry: {dict(per)}")
    assert not missing, "\n".join(census.sig_str(grid[k], 500) for k in missing[:20])
    assert not UNCOVERED
    # what the issue names: the unfused GEGLU pair, colsum, tsa_fwd with the row vector grouped by rv_mod, slab splits of 3, 5 and 8
    entries = {s[0] for c in parts.values() for s in c}
    assert {"geglu_fwd", "geglu_bwd", "colsum"} <= entries
    assert any(s[0] == "tsa_fwd" and census.sig_args(s)["rv_mod"] > 1 for c in parts.values() for s in c)
    splits = {census.sig_args(s)["split_k"] for c in parts.values() for s in c if s[0] == "gemm" and census.sig_args(s)["out_mode"] == K.OUT_F32_SLAB}
    assert {3, 5, 8} <= splits, splits
    # batch 2 at the benchmark geometry runs what c2 does not
    c2 = census.census("c2")
    assert parts["e_2x14x40x64"] and not any(s in c2 for s in parts["e_2x14x40x64"])
    # extents the dispatch class does not describe
    S = {census.sig_args(s)["S"] for s in parts["e_1x1x8x8"] if s[0] == "attn_fwd"}
    assert S == {64, 16, 4, 1}, S
    assert {census.sig_args(s)["S"] for s in parts["e_1x14x24x40"] if s[0] == "attn_fwd"} == {960, 240, 60, 15}
    assert any(s[0] == "tattn_fwd" and census.sig_args(s)["HW"] == 1 for s in parts["e_1x1x8x8"])


# ---- how far the operands reach ------------------------------------------------------------------------------------------------------------
def _quoted(entry, **kw):
    """whether some signature of batch 2 of config 4 (full and LoRA) has these arguments"""
    return [s for n in ("g_2x25x72x128_full", "g_2x25x72x128_lora") for s in census.census(n)
            if s[0] == entry and all(census.sig_args(s)[k] == v for k, v in kw.items())]


def _reaching():
    """[(geometry, signature)] of the grid and GEOM_REACH with an operand of 2^31 bytes or more, each signature once"""
    out, seen = [], set()
    for n in list(census.GEOM_GRID) + list(census.GEOM_REACH):
        for s in sorted(census.census(n), key=repr):
            if s[0] in census.RUNNERS and s not in seen and max(census.reach(s).values(), default=0) >= census.REACH_2G:
                seen.add(s)
                out.append((n, s))
    return out


def test_signatures_that_reach_2_gib_and_the_kernel_they_take():
    """(the table profiles/reach_gpu.txt keeps)"""
    rows = _reaching()
    print(f"{len(rows)} signatures of the grid and of {list(census.GEOM_REACH)} with an operand of 2^31 bytes or more:")
    for n, s in rows:
        big = {k: f"{v / 2 ** 30:.2f} GiB" for k, v in census.reach(s).items() if v >= census.REACH_2G}
        print(f"  {n}: {census.reach_key(s)} {big} -> {census.gemm_kernel_taken(s) or 'the same kernel'}: {census.sig_str(s, 260)}")
    taken = {s: census.gemm_kernel_taken(s) for _, s in rows}
    dgrad = _quoted("gemm", M=460800, N=320, K=2560, variant=16)
    assert dgrad and all(census.reach(s)["A"] >= census.REACH_2G and taken[s] == "gemm_kernel (64-bit pointers)" for s in dgrad)
    for epi, N, aux in ((K.EPI_GEGLU_FWD, 2560, "aux_out"), (K.EPI_GEGLU_BWD, 1280, "aux_in")):
        fused = _quoted("gemm", M=460800, N=N, K=320, variant=26, epilogue=epi)
        assert fused and all(taken[s] == "tile kernel (buffer descriptors)" and census.reach(s)["C"] >= census.REACH_2G and
                             census.reach(s)["A"] < census.REACH_2G and aux in census.reach(s) for s in fused), (epi, fused)
    tn = _quoted("gemm_tn", R=460800, N=2560, K=320, lda=2560)
    assert tn and all(census.reach(s)["A"] >= census.REACH_2G and taken[s] == "gemm_tn kernel, flat staging" for s in tn)
    # GEOM_REACH is what reaches 2^32 bytes: through both GEMM entries
    assert {s[0] for n, s in rows if n in census.GEOM_REACH and max(census.reach(s).values()) >= census.REACH_4G} == {"gemm", "gemm_tn"}
    assert not any(max(census.reach(s).values()) >= census.REACH_4G for n, s in rows if n in census.GEOM_GRID)


def test_no_recorded_launch_is_one_the_library_would_refuse():
    """from the conditions of the entry points (census.gemm_kernel_taken): the dual, GroupNorm-statistics and fused-GEGLU forms of svdx_gemm
    with A or B of 2 GiB, svdx_tsa_fwd and svdx_gemm_tn_gather beyond their limits.  The host's own fallbacks (ops.gemm_act's `gn_fits`, the
    unfused path of unet.py's temporal block) are why none is recorded."""
    n_judged, refused = 0, []
    for n in list(census.GEOM_GRID) + list(census.GEOM_REACH):
        for s in census.census(n):
            verdict = census.gemm_kernel_taken(s) if s[0] in ("gemm", "gemm_tn", "gemm_tn_gather", "tsa_fwd") else None
            n_judged += verdict is not None
            if verdict is not None and verdict.startswith("refused"):
                refused.append(f"{n}: {verdict}: {census.sig_str(s, 300)}")
    print(f"{n_judged} recorded gemm / gemm_tn / gemm_tn_gather / tsa_fwd signatures judged")
    assert n_judged > 1000 and not refused, "\n".join(refused[:20])
    # the conditions themselves, at the line: one step below is served, the line is refused
    sig = _quoted("gemm", M=460800, N=320, K=2560, variant=16)[0]

    def with_args(s, **kw):
        return (s[0], tuple((k, kw.get(k, v)) for k, v in s[1]))
    assert census.gemm_kernel_taken(with_args(sig, M=419430)) == "tile kernel (buffer descriptors)"          # 419430 * 2560 * 2 = 2^31 - 2560
    assert census.gemm_kernel_taken(with_args(sig, M=419431)) == "gemm_kernel (64-bit pointers)"
    assert census.gemm_kernel_taken(with_args(sig, M=419431, gn=(("T", "f32", None, None, None), 1, 32))).startswith("refused: svdx_gemm_gn")
    assert census.gemm_kernel_taken(with_args(sig, M=419431, epilogue=K.EPI_GEGLU_FWD, aux_dim=160)).startswith("refused: svdx_gemm: fused")


def test_every_reach_class_of_the_grid_runs_on_the_gpu():
    """a grid signature with an operand of 2^31 bytes or more takes other code than the signature of its class with the fewest rows: the
    GPU selection (census.geom_gpu_signatures, census.STEP_GPU) holds a signature of the same class AND the same reach for each.  Reach
    is computed here from census.reach_key, not read off the dispatch class."""
    base = lambda s: (census._dispatch_class(s), census.reach_key(s))
    run = {base(s) for c in census.geom_gpu_signatures().values() for s in c} | {base(s) for n in census.STEP_GPU for s in census.census(n)}
    rows = [(n, s) for n, s in _reaching() if n in census.GEOM_GRID]
    assert len(rows) >= 7 and {s[0] for _, s in rows} == {"gemm", "gemm_tn"}
    missing = [f"{n}: {census.reach_key(s)}: {census.sig_str(s, 300)}" for n, s in rows if base(s) not in run]
    assert not missing, "grid signatures whose reach no GPU part runs:\n" + "\n".join(missing)
    assert all(census.dispatch_class(s)[-len(census.reach_key(s)):] == census.reach_key(s) for _, s in rows)


@pytest.mark.parametrize("name", sorted(census.GEOM_EDGE) + sorted(census.GEOM_TINY) + ["grid"])
def test_every_entry_launched_has_a_runner_or_is_allow_listed(name):
    names = sorted(census.GEOM_GRID) if name == "grid" else [name]
    for n in names:
        launches, distinct, checked, allowed, missing = census.coverage(census.census(n))
        print(f"{n}: {launches} launches, {distinct} distinct signatures, {checked} checked, allow-listed launches {dict(allowed)}")
        assert not missing, f"{n}: entries with neither a runner nor an allow-list entry: {missing}"
        assert sum(allowed.values()) <= census.ALLOW_FRACTION * launches, (n, dict(allowed), launches)


# ---- the model's own refusal ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo,level", [((2, 2, 8, 8), "3 is 1x1"), ((2, 2, 24, 40), "3 is 3x5"), ((3, 1, 8, 16), "0 is 8x16"), ((4, 1, 8, 16), "3 is 1x2")])
def test_batch_the_time_context_ordering_cannot_serve_is_refused_before_the_first_launch(geo, level):
    from oracle.unet import TINY_CONFIG, no_default_init
    from svd_xtend_amd.unet import UNetSpatioTemporalConditionModel
    B, T, h, w = geo
    rec = census.Recorder()
    with census._backend(rec), torch.no_grad():
        with no_default_init():
            m = UNetSpatioTemporalConditionModel(**TINY_CONFIG)
        for p in m.parameters():
            p.requires_grad_(False)
        m.prepare()
        before = rec.n_calls
        with pytest.raises(ValueError, match=f"multiple of {B}.*level {level}"):
            m(torch.empty(B, T, 8, h, w), torch.tensor(1.0), encoder_hidden_states=torch.empty(B, 1, TINY_CONFIG["cross_attention_dim"]),
              added_time_ids=torch.ones(B, 3), return_dict=False)
        assert rec.n_calls == before, "the refusal came after a launch"
        # the same batch at a geometry whose levels are all multiples of it goes through
        m(torch.empty(B, T, 8, 8 * B, 16), torch.tensor(1.0), encoder_hidden_states=torch.empty(B, 1, TINY_CONFIG["cross_attention_dim"]),
          added_time_ids=torch.ones(B, 3), return_dict=False)
        assert rec.n_calls > before


# ---- emulation and simulator at the tiny edge geometries -----------------------------------------------------------------------------------
def _tiny_sigs(name):
    sigs = [s for s in census.census(name) if s[0] in census.RUNNERS]
    if name == "t_1x1x8x8":
        # the unfused GEGLU pair, which only the real widths launch: its smallest real signatures (M = 4 rows, F = 5120)
        sigs += [s for s in census.census("e_1x1x8x8") if s[0] in ("geglu_fwd", "geglu_bwd")]
    return sigs


@pytest.mark.parametrize("name", sorted(census.GEOM_TINY))
def test_emulation_meets_float64_reference_at_every_tiny_edge_signature(name):
    sigs = _tiny_sigs(name)
    assert len(sigs) >= 250
    bad, worst = _run_all(emul.EmuBackend(), sigs)
    for fam, w in sorted(worst.items()):
        print(f"{w:8.3f}  {fam}")
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("name", sorted(census.GEOM_TINY))
def test_hip_sources_meet_float64_reference_on_simulator_at_the_tiny_edges(name):
    """the HIP sources themselves (tests/sim): the cheapest signature per (entry, feature combination, reduced extent that is an edge);
    all signatures under SVDX_SIM_FULL=1"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "sim"))
    from backend import SimBackend
    sigs = _tiny_sigs(name)
    if not FULL:
        first = {}
        for s in sorted(sigs, key=lambda s: (_cost(s), repr(s))):
            first.setdefault(census.feature_key(s), s)
        sigs = list(first.values())
    print(f"{name}: {len(sigs)} signatures on the simulator")
    bad, worst = _run_all(SimBackend(), sigs)
    for fam, w in sorted(worst.items()):
        print(f"{w:8.3f}  {fam}")
    assert not bad, "\n".join(bad[:20])


def _s1_sigs():
    sigs = [s for s in census.census("t_1x1x8x8") if s[0] in ("attn_bwd_dkv", "attn_bwd_dq") and census.sig_args(s)["S"] == 1]
    sigs += [s for s in census.census("e_1x1x8x8") if s[0] in ("attn_bwd_dkv", "attn_bwd_dq") and census.sig_args(s)["S"] == 1]
    return sorted(sigs, key=repr)


def test_attention_backward_with_one_key_passes_on_the_emulation():
    """S = 1: P = 1 and dS = P (dP - D) is exactly 0 in float64, so dq and dk are pure cancellation residue.  The parent's bound there is
    half a subnormal spacing (a bar on the row's own maximum, which is 0) and the emulation misses it by a factor of 18 to 44; the
    cancellation term of census._attn_bwd is the whole bound now.  It is derived from the operands, not from the residue: a D that
    belongs to another head is still flagged, hundreds of bounds away."""
    sigs = _s1_sigs()
    assert {s[0] for s in sigs} == {"attn_bwd_dkv", "attn_bwd_dq"} and len(sigs) >= 4
    for sig in sigs:
        ops = []
        res = census.run_case(emul.EmuBackend(), sig, operands_out=ops)
        for label, e, _ in res:
            print(f"{e:8.3f}  {label}: {census.sig_str(sig, 160)}")
        assert all(e <= 1.0 for _, e, _ in res), (res, census.sig_str(sig))
        out = ops[0]["dq"] if sig[0] == "attn_bwd_dq" else ops[0]["dk"]
        assert bool((out.float() != 0).any()), "no residue: the operands do not exercise the cancellation"
        nm = "dq" if sig[0] == "attn_bwd_dq" else "dk"
        wrong = {label: e for label, e, _ in census.run_case(Faulty("attn_bwd: D of the neighbouring row"), sig)}
        print(f"    with the neighbouring head's D: {nm} excess {wrong[nm]:.3g}")
        assert wrong[nm] > 10.0, wrong


# ---- planted faults ------------------------------------------------------------------------------------------------------------------------
class Faulty(emul.EmuBackend):
    def __init__(self, fault):
        self.fault = fault

    def attn_fwd(self, q, k, v, o, lse, nb, heads, S, ld, ld_o, scale):
        assert self.fault == "attn_fwd: last key ignored when S < 16" and 1 < S < 16
        qf, kf, vf = (self._hv(t, nb, S, heads, ld).float() for t in (q, k, v))
        s = (qf @ kf[:, :, :S - 1].transpose(2, 3)) * scale
        l = torch.logsumexp(s, -1)
        emul.V1(lse, nb * heads * S).view(nb, heads, S).copy_(l)
        self._hv(o, nb, S, heads, ld_o).copy_((torch.exp(s - l[..., None]) @ vf[:, :, :S - 1]).to(o.dtype))

    def _attn_bwd_common(self, q, k, v, d_o, lse, D, nb, heads, S, *rest):
        assert self.fault == "attn_bwd: D of the neighbouring row"
        Dn = emul.V1(D, nb * heads * S).roll(1).contiguous()                 # (with one key per head: the neighbouring head's)
        return super()._attn_bwd_common(q, k, v, d_o, lse, Dn, nb, heads, S, *rest)

    def tsa_fwd(self, x, gamma, beta, eps, wqkv, wo, bo, cvec, rv_ld, rv_rpg, rv_mod, n1, stats, qkv, o, h1, B, T, HW, *rest):
        assert self.fault == "tsa_fwd: row vector grouped as if B = 1" and rv_mod > 1
        super().tsa_fwd(x, gamma, beta, eps, wqkv, wo, bo, cvec, rv_ld, B * T * HW, 0, n1, stats, qkv, o, h1, B, T, HW, *rest)

    def gemm(self, A, B, C, M, N, Kd, lda, ldb, ldc, bias=None, rowvec=None, rv_ld=0, rv_rpg=0, rv_mod=0, res=None, ldres=0, gather=None,
             out_mode=K.OUT_ACT, alpha=1.0, split_k=1, *rest, **kw):
        if self.fault == "gemm: slab split-K, last slice not written":
            assert out_mode == K.OUT_F32_SLAB and split_k > 1
            last = torch.as_strided(C, (M, N), (N, 1), C.storage_offset() + (split_k - 1) * M * N)
            before = last.clone()
            super().gemm(A, B, C, M, N, Kd, lda, ldb, ldc, bias, rowvec, rv_ld, rv_rpg, rv_mod, res, ldres, gather, out_mode, alpha, split_k, *rest, **kw)
            last.copy_(before)
            return
        assert self.fault == "gemm: mode-1 gather at 1x1 reads the pixel where the padding is"
        g = gather
        assert g.mode == K.GATHER_CONV3X3 and (g.hi, g.wi, g.ho, g.wo, g.stride, g.ups) == (1, 1, 1, 1, 1, 0) and M == g.n_img
        wide = emul.V(A, M, g.cin, g.lda).repeat(1, 9).contiguous()          # every one of the nine taps finds the image's one pixel
        super().gemm(wide, B, C, M, N, Kd, 9 * g.cin, ldb, ldc, bias, rowvec, rv_ld, rv_rpg, rv_mod, res, ldres, None, out_mode, alpha, split_k,
                     *rest, **kw)


def _pick(names, entry, pred):
    for name in names:
        sigs = sorted((s for s in census.census(name) if s[0] == entry and pred(census.sig_args(s))), key=lambda s: (_cost(s), repr(s)))
        if sigs:
            return sigs[0]
    raise AssertionError(f"no such {entry} signature in {names}")


def _gather_1x1(a):
    g = a["gather"]
    return g is not None and g.mode == K.GATHER_CONV3X3 and (g.hi, g.wi, g.stride, g.ups) == (1, 1, 1, 0) and a["out_mode"] == K.OUT_ACT


FAULTS = {
    # fault -> (signature, the output that must be flagged)
    "attn_fwd: last key ignored when S < 16": (lambda: _pick(("t_1x1x8x8",), "attn_fwd", lambda a: a["S"] == 4), ("o", "lse")),
    "attn_bwd: D of the neighbouring row": (lambda: _pick(("t_3x5x8x24",), "attn_bwd_dq", lambda a: a["S"] == 3), ("dq",)),
    "gemm: mode-1 gather at 1x1 reads the pixel where the padding is": (lambda: _pick(("t_1x1x8x8",), "gemm", _gather_1x1), ("C",)),
    "tsa_fwd: row vector grouped as if B = 1": (lambda: _pick(("t_3x5x8x24", "t_2x16x8x16"), "tsa_fwd", lambda a: a["rv_mod"] > 1),
                                                ("h1 (from the o it wrote)",)),
    "gemm: slab split-K, last slice not written": (lambda: _pick(("t_1x1x8x8", "t_3x5x8x24"), "gemm",
                                                                 lambda a: a["out_mode"] == K.OUT_F32_SLAB and a["split_k"] > 1), None),
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_checker_notices_fault_planted_at_an_edge_signature(fault):
    """numeric perturbations of a correct CPU result (nothing runs on a GPU): the clean emulation passes, the faulty one is flagged at
    the output the fault reaches"""
    pick, names = FAULTS[fault]
    sig = pick()
    a = census.sig_args(sig)
    if names is None:
        names = (f"slab {a['split_k'] - 1}",)
    clean = census.run_case(emul.EmuBackend(), sig)
    assert all(e <= 1.0 for _, e, _ in clean), clean
    res = census.run_case(Faulty(fault), sig)
    flagged = [(label, e) for label, e, _ in res if not e <= 1.0]
    print(f"{fault}: {census.sig_str(sig, 260)}")
    for label, e in flagged:
        print(f"    flagged: {label}: excess {e:.3g}")
    assert flagged, f"the checker let '{fault}' through: {res}"
    assert {label for label, _ in flagged} >= set(names[:1]), (flagged, names)
    assert {label for label, _ in flagged} <= set(names) | {l for l, _, _ in res if "rounding" in l}, (flagged, names)
