"""Data-parallel path with trainable GroupNorm affines on CPU: 2 processes over gloo (127.0.0.1), emulated kernels.  The affine
gradients of the ResNet norms and of conv_norm_out lie outside the per-block buckets, in the spans the gradient sum reduces as "the
rest"; a transformer model's `norm` lies inside its block's bucket, which starts its reduction when the block reports.  After the sum every rank holds, for
every GroupNorm tensor, the sum of the two ranks' single-rank gradients (AdamW's grad_mul = 1 / world makes it their mean), under both
schedules of the sum, and the replicas stay bitwise identical through an optimizer step."""
import os
import sys

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
WHICH = ("temporal_transformer_block", "@norm")


def _setup():
    for p in (ROOT, HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    import emul
    from svd_xtend_amd import kernels
    kernels._set_backend_for_tests(emul.EmuBackend())


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(2)
    _setup()
    import selection_checks as sc
    import test_conv_wgrad_dp as base
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from svd_xtend_amd.train import Trainer
    res = {}
    for overlap in (True, False):
        tr = Trainer(base._make(0), dtype=torch.float32, lr=1e-3, trainable=WHICH)
        tr.overlap = overlap
        assert tr.world == world and tr.rt.found_inf is None           # several ranks: the SUM is tested, by the full pass
        tr.zero_grad()
        tr.forward_backward(**base._batch(100 + rank))                 # rank-distinct data
        res[overlap] = dict(local=tr.g_flat.clone())
        tr.finish_grads()
        res[overlap]["summed"] = tr.g_flat.clone()
        tr.optimizer_step()
        res[overlap]["p"] = tr.p_flat.clone()
    gn = set(sc.gn_names(tr.model))
    named = [(n, p) for n, p in tr.model.named_parameters() if p.requires_grad]
    assert [n for n, _ in named] == tr.names
    norm = [(n, o, p.numel()) for (n, p), o in zip(named, tr.offsets) if n in gn]
    assert len(norm) == 210
    torch.save(dict(res=res, norm=norm, rest=tr._rest, buckets=sorted(tr._buckets.values())), os.path.join(out, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_sum_of_groupnorm_gradients_is_the_sum_of_the_single_rank_gradients(tmp_path):
    port = 33500 + os.getpid() % 2000
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0 = torch.load(tmp_path / "r0.pt", weights_only=False)
    r1 = torch.load(tmp_path / "r1.pt", weights_only=False)
    # the single-rank gradients: as the one-collective schedule left them (with buckets, a block's slice may already be summed when the
    # sweep returns -- the 16 transformer models' `norm` lie inside their block's bucket, final when the block reports)
    la, lb = r0["res"][False]["local"], r1["res"][False]["local"]
    assert not torch.equal(la, lb)
    in_bucket = 0
    for overlap in (True, False):
        a, b = r0["res"][overlap], r1["res"][overlap]
        assert torch.equal(a["summed"], b["summed"]) and torch.equal(a["p"], b["p"])
        for name, off, n in r0["norm"]:
            want = la[off:off + n] + lb[off:off + n]                          # two addends: the order of the sum cannot matter
            assert float(want.abs().max()) > 0, name
            assert torch.equal(a["summed"][off:off + n], want), (overlap, name)
            if ".attentions." in name:
                assert any(lo <= off and off + n <= hi for lo, hi in r0["buckets"]), name
                in_bucket += overlap
            else:
                assert any(lo <= off and off + n <= hi for lo, hi in r0["rest"]), name
                assert not any(lo < off + n and off < hi for lo, hi in r0["buckets"]), name
    assert in_bucket == 32
    assert torch.equal(r0["res"][True]["summed"], r0["res"][False]["summed"])
