"""world_size-2 check (gloo, CPU, the emulator build of the kernels) of FlatAdam.set_grad_clip under data parallelism: the norm pass of
FlatAdam.step() reads the REDUCED arena, after the all-reducer's join, with grad_scale = 1 / world folded in, so both ranks form the same norm
and coefficient -- the norm of the averaged gradient -- without exchanging anything more; under a dynamic loss scale the same pass raises the
flag, so an inf in ONE rank's local gradient skips the step on both."""
import os
import tempfile

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_distributed_gloo import _free_port

STEPS, BAD_STEP, BAD_RANK, MAX_NORM = 3, 2, 1, 0.05


def _worker(rank, world, port, outdir, emu_lib, dynamic):
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
    opt.set_grad_clip(MAX_NORM)
    scaler = DynamicLossScale(init_scale=1024.0, growth_interval=2) if dynamic else 1.0
    red = GradientAllReducer(opt, stages={"head_done": list(model.head.parameters()) + list(model.out.parameters())}, bucket_bytes=1 << 10)
    red.broadcast_parameters(0)
    trace = []
    for step in range(1, STEPS + 1):
        x, label, valid = _toy_batch(10 * step + rank)      # this rank's shard
        before = opt.flat_param.clone()
        rcnet_main.staged_gradients(lambda: _toy_loss(model, x, label, valid), opt, None, scaler)
        if dynamic and step == BAD_STEP and rank == BAD_RANK:
            opt.flat_grad[7] = float("inf")                 # this rank's LOCAL gradient, before the exchange
        red.reduce()
        summed = opt.flat_grad.clone()                      # the ranks' gradients summed: a single process would average exactly these
        inv = 1.0 / scaler.get_scale() if dynamic else 1.0
        touched = opt.touched_indices()
        opt.step()
        trace.append(dict(clip=opt._clip_state.clone(), stats=opt.clip_stats(), moved=not torch.equal(before, opt.flat_param), summed=summed, inv=inv,
                          touched=touched, scaler=scaler.stats() if dynamic else None))
    dist.barrier()
    dist.destroy_process_group()
    torch.save(dict(trace=trace, final=opt.flat_param.clone(), offsets=opt.offsets, numels=[p.numel() for p in opt.params],
                    skipped=opt.skipped_steps()), os.path.join(outdir, "r%d.pt" % rank))


def _run(emu_lib_path, dynamic):
    ctx = mp.get_context("spawn")
    port = _free_port()
    with tempfile.TemporaryDirectory() as outdir:
        procs = [ctx.Process(target=_worker, args=(r, 2, port, outdir, emu_lib_path, dynamic)) for r in range(2)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(timeout=600)
            assert p.exitcode == 0, "worker exit code %s" % p.exitcode
        return [torch.load(os.path.join(outdir, "r%d.pt" % r)) for r in range(2)]


def _single_process_norm(t, offsets, numels, dt):
    """torch's clip_grad_norm_ in one process on the average of the ranks' unscaled gradients (the written slots only)"""
    avg = t["summed"].to(dt) * (0.5 * t["inv"])
    ps = []
    for i in t["touched"]:
        p = torch.nn.Parameter(torch.zeros(numels[i], dtype=dt))
        p.grad = avg[offsets[i]:offsets[i] + numels[i]].clone()
        ps.append(p)
    return torch.nn.utils.clip_grad_norm_(ps, MAX_NORM, foreach=False).detach()


def _common(res, dynamic):
    from tests.parity_cases_glue import _check
    for k in range(STEPS):
        a, b = res[0]["trace"][k], res[1]["trace"][k]
        assert torch.equal(a["clip"], b["clip"]), "step %d: the ranks' clip states differ: %s / %s" % (k + 1, a["stats"], b["stats"])
        assert a["stats"]["passes"] == k + 1
        if dynamic and k + 1 == BAD_STEP:
            assert a["stats"]["nonfinite"] == 1 and not a["moved"] and not b["moved"], (a["stats"], a["moved"], b["moved"])
            continue
        assert a["moved"] and b["moved"]
        t64 = _single_process_norm(a, res[0]["offsets"], res[0]["numels"], torch.float64)
        t32 = _single_process_norm(a, res[0]["offsets"], res[0]["numels"], torch.float32)
        assert abs(float(t64) / MAX_NORM - 1.0) > 0.01
        got = a["clip"][0:1].view(torch.float32)
        _check("world 2, step %d: total_norm" % (k + 1), got, t64.reshape(1), t32.reshape(1))
        coef = lambda t, dt: torch.clamp(torch.tensor(MAX_NORM, dtype=dt) / (t + 1e-6), max=1.0).reshape(1)      # noqa: E731
        _check("world 2, step %d: coef" % (k + 1), a["clip"][1:2].view(torch.float32), coef(t64, torch.float64), coef(t32, torch.float32))
    assert res[0]["trace"][0]["stats"]["clipped"] == 1      # MAX_NORM is below the first step's norm: the run does clip
    assert torch.equal(res[0]["final"].view(torch.int32), res[1]["final"].view(torch.int32)), "the ranks' parameters differ"
    assert bool(torch.isfinite(res[0]["final"]).all())


def test_grad_clip_world2_same_norm_on_both_ranks(emu_lib_path):
    _common(_run(emu_lib_path, False), False)


def test_grad_clip_world2_dynamic_scale_one_rank_overflows(emu_lib_path):
    res = _run(emu_lib_path, True)
    _common(res, True)
    for r in range(2):
        assert res[r]["skipped"] == 1, (r, res[r]["skipped"])
        stats = [t["scaler"] for t in res[r]["trace"]]
        assert [s["scale"] for s in stats] == [1024.0, 512.0, 512.0] and [s["skipped"] for s in stats] == [0, 1, 1], stats
        assert all(s["found_inf"] == 0 for s in stats), stats
