"""world_size-2 check (gloo, CPU, the emulator build of the kernels) of the dynamic loss scale under data parallelism: the finite check of
FlatAdam.step() reads the REDUCED arena, after the all-reducer's join, so an inf in ONE rank's local gradient raises the flag on every rank --
nothing besides the gradients is exchanged."""
import os
import tempfile

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_distributed_gloo import _free_port

STEPS, BAD_STEP, BAD_RANK = 3, 2, 1


def _worker(rank, world, port, outdir, emu_lib):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from riders_amd import _lib, engine, rcnet_main
    from riders_amd.optim import DynamicLossScale, FlatAdam
    from riders_amd.parallel import GradientAllReducer
    from tests.test_host_logic import _TwoStage, _toy_batch, _toy_loss
    _lib._install_for_tests(emu_lib)      # TEST INFRA: host build of the kernel sources
    engine.set_compute_dtype("fp32")
    torch.manual_seed(100 + rank)
    model = _TwoStage(); model.train()
    opt = FlatAdam(list(model.parameters()), lr=1e-2)
    scaler = DynamicLossScale(init_scale=1024.0, growth_interval=2)
    red = GradientAllReducer(opt, stages={"head_done": list(model.head.parameters()) + list(model.out.parameters())}, bucket_bytes=1 << 10)
    red.broadcast_parameters(0)
    trace = []
    for step in range(1, STEPS + 1):
        x, label, valid = _toy_batch(10 * step + rank)      # this rank's shard
        before = opt.flat_param.clone()
        rcnet_main.staged_gradients(lambda: _toy_loss(model, x, label, valid), opt, None, scaler)
        if step == BAD_STEP and rank == BAD_RANK:
            opt.flat_grad[7] = float("inf")                 # this rank's LOCAL gradient, before the exchange
        red.reduce()
        opt.step()
        trace.append(dict(stats=scaler.stats(), moved=not torch.equal(before, opt.flat_param), local_bad=step == BAD_STEP and rank == BAD_RANK))
    sd = opt.state_dict()
    dist.barrier()
    dist.destroy_process_group()
    torch.save(dict(trace=trace, final=opt.flat_param.clone(), state=scaler._state.clone(), skipped=opt.skipped_steps(),
                    steps=sorted(set(int(v["step"]) for v in sd["state"].values()))), os.path.join(outdir, "r%d.pt" % rank))


def test_dynamic_loss_scale_world2_one_rank_overflows(emu_lib_path):
    ctx = mp.get_context("spawn")
    port = _free_port()
    with tempfile.TemporaryDirectory() as outdir:
        procs = [ctx.Process(target=_worker, args=(r, 2, port, outdir, emu_lib_path)) for r in range(2)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(timeout=600)
            assert p.exitcode == 0, "worker exit code %s" % p.exitcode
        res = [torch.load(os.path.join(outdir, "r%d.pt" % r)) for r in range(2)]
    for r in range(2):
        moved = [t["moved"] for t in res[r]["trace"]]
        assert moved == [s != BAD_STEP for s in range(1, STEPS + 1)], "rank %d: steps that changed the parameters %s" % (r, moved)
        assert res[r]["skipped"] == 1 and res[r]["steps"] == [STEPS - 1], (r, res[r]["skipped"], res[r]["steps"])
        stats = [t["stats"] for t in res[r]["trace"]]
        assert [s["scale"] for s in stats] == [1024.0, 512.0, 512.0] and [s["growth_tracker"] for s in stats] == [1, 0, 1], stats
        assert [s["skipped"] for s in stats] == [0, 1, 1] and all(s["found_inf"] == 0 for s in stats), stats
    assert [t["local_bad"] for t in res[0]["trace"]] == [False] * STEPS      # rank 0 never saw an inf of its own
    assert torch.equal(res[0]["state"], res[1]["state"]), "the ranks' scaler states differ"
    assert torch.equal(res[0]["final"].view(torch.int32), res[1]["final"].view(torch.int32)), "the ranks' parameters differ"
    assert bool(torch.isfinite(res[0]["final"]).all())
