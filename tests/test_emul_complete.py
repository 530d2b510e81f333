"""CPU (`-m "not gpu"`): tests/emul.py's EmuBackend emulates every launching entry of kernels.HipBackend with the same signature, so the
one emulation the shared fixtures install can run any step the product can -- here clipping, "@conv" and "@norm" in one."""
import inspect
import math

import torch

import emul
import gn_affine_checks as ga
import selection_checks as sc
from svd_xtend_amd import kernels as K

# HipBackend's public functions that launch nothing the emulation has to compute
NOT_ENTRIES = {"last_error", "wall_clock_khz", "stamp", "plan_begin", "plan_end"}


def _public(cls):
    return {n: f for n, f in inspect.getmembers(cls, inspect.isfunction) if not n.startswith("_")}


def test_emulation_has_every_entry_with_the_same_signature():
    """the names, the count of parameters and which of them have defaults (not their names: K / Kd, silu / silu_, opt_state / st differ,
    which is why the census calls positionally)"""
    hip, emu = _public(K.HipBackend), _public(emul.EmuBackend)
    assert set(hip) - NOT_ENTRIES == set(emu), (sorted(set(hip) - NOT_ENTRIES - set(emu)), sorted(set(emu) - set(hip)))
    for name, f in emu.items():
        a, b = (list(inspect.signature(g).parameters.values()) for g in (hip[name], f))
        assert [p.default is p.empty for p in a] == [p.default is p.empty for p in b], (name, a, b)


def test_one_emulation_runs_clipping_convolutions_and_norms_in_one_step(emu_backend):
    rec = emul.record(K._backend)
    ref = sc.oracle_step(ga.ALL_THREE)
    tr = sc.make_trainer(ref, ga.ALL_THREE, torch.float16, torch.device("cpu"), max_grad_norm=1.0)
    tr.step(sc.step_batch(ref, "cpu"))
    assert math.isfinite(float(tr.last_loss())) and math.isfinite(float(tr.grad_norm))
    launches = set(rec.names(depth=0))
    assert {"svdx_gemm_tn_gather", "svdx_gn_bwd_stats_affine", "svdx_grad_sumsq_spans", "svdx_grad_clip_coef"} <= launches
    # the default set: its launches are the depth-0 calls among the ga.PARENT_DEFAULT_LAUNCHES calls of every depth
    tr = sc.make_trainer(ref, "temporal_transformer_block", torch.float16, torch.device("cpu"))
    rec.clear()
    tr.step(sc.step_batch(ref, "cpu"))
    assert len(rec.names(depth=0)) == ga.DEFAULT_LAUNCHES and len(rec) == ga.PARENT_DEFAULT_LAUNCHES[0], (len(rec.names(depth=0)), len(rec))
