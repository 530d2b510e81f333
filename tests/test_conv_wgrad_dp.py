"""Data-parallel path with trainable convolutions on CPU: 2 processes over gloo (127.0.0.1), emulated kernels.  The convolution
gradients lie outside the per-block buckets, in the spans the gradient sum reduces as "the rest": after the sum every rank holds, for
every convolution tensor, the sum of the two ranks' single-rank gradients (AdamW's grad_mul = 1 / world makes it their mean), under both
schedules of the sum, and the replicas stay bitwise identical through an optimizer step."""
import os
import sys

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
WHICH = ("temporal_transformer_block", "@conv")


def _setup():
    for p in (ROOT, HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    import emul
    from svd_xtend_amd import kernels
    kernels._set_backend_for_tests(emul.EmuBackend())


def _make(seed):
    from oracle.unet import TINY_CONFIG, UNetSpatioTemporalConditionOracle, scaled_init_
    from svd_xtend_amd.unet import UNetSpatioTemporalConditionModel
    orc = UNetSpatioTemporalConditionOracle(**TINY_CONFIG)
    scaled_init_(orc, seed)
    m = UNetSpatioTemporalConditionModel(**TINY_CONFIG)
    m.load_state_dict(orc.state_dict(), strict=True)
    return m


def _batch(seed):
    from oracle.step import edm_inputs, make_synthetic_batch
    b = make_synthetic_batch(1, 2, 16, 16, seed, cross_dim=64)
    unet_in, ts, ehs, ids, noisy, _ = edm_inputs(b)
    return dict(unet_in=unet_in, timesteps=ts, ehs=ehs, added_time_ids=ids, noisy_latents=noisy, target=b["latents"],
                sigmas=b["sigmas"])


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(2)
    _setup()
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from svd_xtend_amd.train import Trainer
    res = {}
    for overlap in (True, False):
        tr = Trainer(_make(0), dtype=torch.float32, lr=1e-3, trainable=WHICH)
        tr.overlap = overlap
        assert tr.world == world and tr.rt.found_inf is None           # several ranks: the SUM is tested, by the full pass
        tr.zero_grad()
        tr.forward_backward(**_batch(100 + rank))                      # rank-distinct data
        if overlap:
            assert tr._pending                                         # the blocks' buckets are on their way; the convolutions are not in them
        res[overlap] = dict(local=tr.g_flat.clone())
        tr.finish_grads()
        res[overlap]["summed"] = tr.g_flat.clone()
        tr.optimizer_step()
        res[overlap]["p"] = tr.p_flat.clone()
    conv = [(n, o, p.numel()) for (n, p), o in zip([(n, p) for n, p in tr.model.named_parameters() if p.requires_grad], tr.offsets) if p.ndim > 2]
    assert [n for n, p in tr.model.named_parameters() if p.requires_grad] == tr.names and len(conv) > 20
    torch.save(dict(res=res, conv=conv, rest=tr._rest, buckets=sorted(tr._buckets.values())), os.path.join(out, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_sum_of_conv_gradients_is_the_sum_of_the_single_rank_gradients(tmp_path):
    port = 31500 + os.getpid() % 2000
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0 = torch.load(tmp_path / "r0.pt", weights_only=False)
    r1 = torch.load(tmp_path / "r1.pt", weights_only=False)
    for overlap in (True, False):
        a, b = r0["res"][overlap], r1["res"][overlap]
        assert torch.equal(a["summed"], b["summed"]) and torch.equal(a["p"], b["p"])
        assert not torch.equal(a["local"], b["local"])
        for name, off, n in r0["conv"]:
            want = a["local"][off:off + n] + b["local"][off:off + n]          # two addends: the order of the sum cannot matter
            assert float(want.abs().max()) > 0, name
            assert torch.equal(a["summed"][off:off + n], want), (overlap, name)
            assert any(lo <= off and off + n <= hi for lo, hi in r0["rest"]), name
            assert not any(lo < off + n and off < hi for lo, hi in r0["buckets"]), name
    assert torch.equal(r0["res"][True]["summed"], r0["res"][False]["summed"])
