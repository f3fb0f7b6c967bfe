"""Parity tests proper: HIP kernels on a real MI355X, called through the C ABI (libriders_hip.so), against the
oracle and against golden vectors produced by the reference.  fp32 path: <= 1e-3 relative (north_star); index
outputs bit-exact."""
import pytest

from tests import parity_cases as P

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", range(len(P.CONV_CASES)))
def test_conv(gpu, case):
    P.conv_case(gpu, P.CONV_CASES[case])


@pytest.mark.parametrize("case", range(len(P.PATCH_CONV_CASES)))
def test_patch_conv(gpu, case):
    with P.force_patch_conv():
        P.conv_case(gpu, P.PATCH_CONV_CASES[case])


def test_patch_conv_decoder_and_bf16(gpu):
    with P.force_patch_conv():
        P.decoder_block_case(gpu, cin=32, cskip=32, cout=32)
        P.decoder_block_case(gpu, cin=256, cskip=128, cout=256, hs=(7, 3), hv=(15, 6), N=6)
        P.bf16_exact_conv_case(gpu, cin=64, cout=64, k=3, s=1, H=9, W=19, N=1)
        P.bf16_exact_conv_case(gpu, cin=32, cout=128, k=3, s=1, N=1, up=((4, 3), (17, 6)), cin2=32)
        P.bf16_exact_conv_case(gpu, cin=16, cout=16, k=3, s=1, H=17, W=9, N=1)
        P.bf16_exact_conv_case(gpu, cin=16, cout=16, k=3, s=1, N=1, up=((4, 3), (9, 17)), cin2=16)
        P.bf16_exact_conv_case(gpu, cin=64, cout=8, k=3, s=1, H=8, W=5, N=2)
        P.bf16_exact_conv_case(gpu, cin=32, cout=64, k=3, s=1, H=12, W=17, N=1)     # 64 output channels: weights in LDS
        P.bf16_exact_conv_case(gpu, cin=16, cout=48, k=3, s=1, H=9, W=10, N=2)
    # persistent narrow-layer kernel with many tiles per block (1024 blocks): 3300+ tiles, ragged edges, upsample + concat
    P.bf16_exact_conv_case(gpu, cin=16, cout=16, k=3, s=1, N=12, up=((60, 25), (121, 50)), cin2=16)
    P.bf16_exact_conv_case(gpu, cin=16, cout=1, k=3, s=1, H=130, W=100, N=24)
    P.conv_case(gpu, dict(cin=16, cout=16, k=3, s=1, H=120, W=100, N=24, bn=True))
    P.bf16_exact_conv_case(gpu, cin=64, cout=128, k=3, s=1, H=80, W=72, N=4)     # routed to the patch kernel by block count
    P.conv_case(gpu, dict(cin=64, cout=64, k=3, s=1, H=64, W=96, N=4, bn=True))


def test_upsample_fused_dgrad(gpu):
    P.upsample_fused_dgrad_cases(gpu)
    # RC-Net's deconv0 / deconv1 geometry, routed by block count: 60x25 -> 120x50 (64 -> 32) and 120x50 -> 240x100 (32 -> 16), 24 RoIs
    P.bf16_exact_conv_case(gpu, cin=32, cout=16, k=3, s=1, N=24, up=((120, 50), (240, 100)))
    P.bf16_exact_conv_case(gpu, cin=64, cout=32, k=3, s=1, N=24, up=((60, 25), (120, 50)))


def test_grad_add_in_data_gradient_epilogue(gpu):
    P.grad_add_cases(gpu)


def test_frag_conv(gpu):
    P.frag_conv_cases(gpu)


def test_frag32_conv(gpu):
    P.frag32_cases(gpu)


def test_wgrad_fit(gpu):
    P.wgrad_fit_cases(gpu)


def test_up2_on_source(gpu):
    P.up2_cases(gpu)


def test_bn_head_fused(gpu):
    P.bn_head_cases(gpu)


def test_bn_bwd_sums_in_dgrad_epilogue(gpu):
    P.bn_bwd_fused_cases(gpu)
    # RC-Net sizes, routed by block count (no hooks): RoI maps as pixel runs across images, encoder maps as 2-D tiles
    P.bf16_exact_conv_case(gpu, cin=256, cout=128, k=3, s=1, H=30, W=12, N=40)
    P.bf16_exact_conv_case(gpu, cin=128, cout=64, k=3, s=1, N=24, up=((30, 12), (60, 25)), cin2=0)
    P.bf16_exact_conv_case(gpu, cin=64, cout=64, k=3, s=1, H=62, W=77, N=4)
    P.conv_case(gpu, dict(cin=64, cout=64, k=3, s=1, H=64, W=96, N=4, bn=True))
    P.conv_case(gpu, dict(cin=128, cout=128, k=3, s=1, H=15, W=6, N=60, bn=True))


def test_lazy_batchnorm_is_bit_identical(gpu):
    """Consumer-side BatchNorm apply (engine.LazyAct): forward / weight-gradient staging of the 3x3 kernels and the fused apply + add +
    activation give the bits of the separate rd_affine_act pass -- small shapes on every kernel route, then RC-Net's own layer sizes."""
    P.lazy_bn_cases(gpu)
    P.lazy_bn_rcnet_geometry_case(gpu)


def test_decoder_block(gpu):
    P.decoder_block_case(gpu)
    P.decoder_block_case(gpu, cin=16, cskip=0, cout=16, hs=(5, 4), hv=(10, 8))
    P.decoder_block_case(gpu, cin=256, cskip=128, cout=256, hs=(7, 3), hv=(15, 6), N=6)


def test_resnet_block(gpu):
    P.resnet_block_case(gpu)
    P.resnet_block_case(gpu, cin=16, cout=16, stride=1)
    P.resnet_block_case(gpu, cin=64, cout=128, stride=2)


def test_linear_attention(gpu):
    P.linear_attention_case(gpu)
    P.linear_attention_case(gpu, N=1, L=7, S=30)
    P.linear_attention_case(gpu, N=64, L=21, S=21)


def test_golden_attention(gpu):
    P.golden_attention_case(gpu)


def test_transformer(gpu):
    P.transformer_case(gpu)
    P.transformer_case(gpu, N=5, n_layers=4)


def test_roi_pool_compact_argmax(gpu):
    P.roi_pool_compact_case(gpu)


def test_roi_pool(gpu):
    P.roi_pool_case(gpu)


def test_roi_pool_known_answers(gpu):
    P.roi_pool_kat_case(gpu)


def test_maxpool(gpu):
    P.maxpool_case(gpu)


def test_labels_loss(gpu):
    P.labels_loss_case(gpu)


def test_scatter_crops(gpu):
    P.scatter_crops_case(gpu)


def test_batch_transforms(gpu):
    P.transforms_case(gpu)


def test_batch_transforms_noise_and_both_flips(gpu):
    P.transforms_all_case(gpu)


def test_projection_scatter(gpu):
    P.projection_case(gpu)


def test_lidar_interpolation(gpu):
    P.interpolation_case(gpu, big=True)
    P.interpolator_case(gpu, big=True)


def test_fp16_build(gpu):
    P.fp16_cases(gpu)


def test_config4_fp16_high_res(gpu):
    P.config4_case(gpu)


def test_inference_driver(gpu):
    P.inference_driver_case(gpu)


def test_adam(gpu):
    P.adam_case(gpu)


def test_resnet_encoder_golden(gpu):
    P.resnet_encoder_case(gpu)


def test_decoder_golden(gpu):
    P.decoder_case(gpu, "small")
    P.decoder_case(gpu, "zju")


def test_rcnet_end_to_end_golden(gpu):
    P.rcnet_e2e_case(gpu)


def test_rcnet_full_size_fp32_vs_oracle(gpu):
    P.rcnet_fullsize_oracle_case(gpu)


def test_rcnet_config3_per_rank_geometry(gpu):
    P.rcnet_config3_rank_case(gpu)


def test_rcnet_config1_bf16_vs_fp32(gpu):
    P.rcnet_fullsize_bf16_case(gpu)


def test_rcnet_round5_routes_on_vs_off(gpu):
    P.rcnet_round5_routes_case(gpu)


def test_rcnet_full_size_bf16_vs_rounding_oracle(gpu):
    P.rcnet_fullsize_bf16_oracle_case(gpu)


def test_native_library_loaded(gpu):
    """The GPU tests must have run on libriders_hip.so (no silent fallback)."""
    import os
    from riders_amd import _lib
    assert not _lib.ALLOW_HOST_POINTERS
    maps = open("/proc/self/maps").read()
    assert os.path.join("riders_amd", "libriders_hip.so") in maps


def test_bf16_throughput_mode(gpu):
    """bf16 activations (fp32 accumulate / parameters / statistics) are a throughput mode.  The data path is checked EXACTLY with
    integer-valued tensors (every product and partial sum representable: forward, data gradient, weight gradient, concat / upsample
    gathers must be bit-identical to the fp32 oracle); rounding behaviour is then bounded on real-valued cases: 3e-2 of max|ref| on
    the attention forward/backward, 2e-1 (max-norm, incl. weight gradients) through a 2-layer transformer, 5e-2 on end-to-end logits / loss (25 % on gradient norms)."""
    from riders_amd import engine
    P.bf16_exact_conv_case(gpu)
    P.bf16_exact_conv_case(gpu, cin=32, cout=64, k=3, s=2, H=10, W=13)
    P.bf16_exact_conv_case(gpu, cin=8, cout=1, k=3, s=1, H=6, W=5)
    P.bf16_exact_conv_case(gpu, cin=16, cout=16, k=3, s=1, N=1, up=((4, 3), (9, 6)), cin2=8)
    P.bf16_exact_conv_case(gpu, cin=3, cout=32, k=7, s=2, H=14, W=12, N=1)
    P.bf16_exact_conv_case(gpu, cin=128, cout=128, k=1, s=1, H=5, W=1, N=2)
    P.bf16_exact_conv_case(gpu, cin=64, cout=128, k=3, s=1, H=40, W=36, N=2)     # 128-pixel tiles, several blocks
    engine.set_compute_dtype("bf16")
    try:
        P.linear_attention_case(gpu, tol=3e-2)
        P.transformer_case(gpu, tol=2e-1)
        P.rcnet_e2e_case(gpu, tol=5e-2)
    finally:
        engine.set_compute_dtype("fp32")


def test_bf16_layers_match_rounding_emulation(gpu):
    """bf16 throughput mode, layer / block level, against the oracle with the SAME rounding points (oracle/precision.py: stored
    activations, packed dense weights and the gradients of those tensors rounded to bf16).  Max-norm 1e-2 (2.5 bf16 ulp) on outputs, input
    gradients and parameter gradients (measured: relative L2 1e-5 .. 2.4e-3) -- the bound on every bf16 kernel of the RC-Net path; the
    end-to-end numbers of the mode are in test_rcnet_config1_bf16_vs_fp32."""
    with P.bf16_mode():
        P.conv_case(gpu, dict(cin=16, cout=16, k=3, s=1, H=40, W=50, N=4, bn=True), tol=1e-2)
        P.conv_case(gpu, dict(cin=64, cout=32, k=3, s=1, H=30, W=25, N=4, bn=True), tol=1e-2)
        P.conv_case(gpu, dict(cin=128, cout=128, k=3, s=2, H=31, W=39, N=2, bn=True), tol=1e-2)
        P.conv_case(gpu, dict(cin=3, cout=32, k=7, s=2, H=40, W=36, N=2, bn=True, no_input_grad=True), tol=1e-2)
        P.conv_case(gpu, dict(cin=256, cout=128, k=3, s=1, H=30, W=12, N=6, bn=True), tol=1e-2)
        P.decoder_block_case(gpu, cin=64, cskip=32, cout=32, hs=(15, 12), hv=(30, 25), N=4, tol=1e-2)
        # wide layers on the 15x6 maps (R = 48 RoIs): relative L2 2e-3 .. 3e-3, max-norm 1.4e-2 at ~5 sigma of the rounding noise
        P.decoder_block_case(gpu, cin=256, cskip=128, cout=256, hs=(7, 3), hv=(15, 6), N=48, tol=2.5e-2)
        P.resnet_block_case(gpu, cin=64, cout=128, stride=2, tol=1e-2)
        P.resnet_block_case(gpu, cin=32, cout=32, stride=1, tol=1e-2)


def test_graphed_step_matches_eager(gpu):
    """The step replayed from a hipGraph (driven by engine.StepTape; split at the stage marks only when an all-reducer is attached) reproduces the eager autograd step
    (same kernels, same order; the only run-to-run freedom is the fp32 atomic order of the ROI-pool scatter-add), and constructing the
    graphed step trains nothing: its warm-up passes leave weights, Adam state, BatchNorm statistics and counters untouched."""
    import torch
    from riders_amd import rcnet_main
    from riders_amd.optim import FlatAdam
    cfg = dict(rcnet_main.ZJU_CONFIG, patch_size=[64, 32], total_points_sampled=4)
    batch = rcnet_main.synthetic_batch(2, 64, 96, cfg, seed=5, device=gpu)
    losses, finals = {}, {}
    for mode in ("eager", "graph"):
        torch.manual_seed(0)
        model = rcnet_main.build_model(gpu, cfg)
        model.train()
        opt = FlatAdam(model.parameters(), lr=1e-3)
        if mode == "eager":
            step = lambda: rcnet_main.train_step(model, opt, batch, cfg)  # noqa: E731
        else:
            p0 = opt.flat_param.clone()
            rm0 = model.encoder.encoder_image.conv1.batch_norm.running_mean.clone()
            step = rcnet_main.GraphedTrainStep(model, opt, batch, cfg, warmup=2)
            assert len(step.graphs) == 1 and step.tags == [None]      # no all-reducer: nothing to interleave, one graph
            assert torch.equal(opt.flat_param, p0) and opt.step_count == 0
            assert torch.equal(model.encoder.encoder_image.conv1.batch_norm.running_mean, rm0)
            assert int(model.encoder.state_dict()["encoder_image.conv1.batch_norm.num_batches_tracked"]) == 0
        losses[mode] = [float(step()) for _ in range(3)]
        finals[mode] = opt.flat_param.clone()
        nbt = int(model.encoder.state_dict()["encoder_image.conv1.batch_norm.num_batches_tracked"])
        assert nbt == 3, (mode, nbt)
    for a, b in zip(losses["eager"], losses["graph"]):
        assert abs(a - b) <= 1e-3 * abs(a), losses  # atomics-order noise amplified by Adam's normalised first steps
    assert losses["eager"][2] != losses["eager"][0]


def test_graphed_step_survives_zero_grad_between_replays(gpu):
    """The reference loop calls optimizer.zero_grad() before every backward (rcnet_main.py:353-359).  A replay fills the gradient arena
    without passing the gradient allocator, so the optimizer's written-slot flags must be restored by the graphed step itself: every
    replay has to move the parameters exactly as without the zero_grad() calls."""
    import torch
    from riders_amd import rcnet_main
    from riders_amd.optim import FlatAdam
    cfg = dict(rcnet_main.ZJU_CONFIG, patch_size=[64, 32], total_points_sampled=4)
    batch = rcnet_main.synthetic_batch(2, 64, 96, cfg, seed=5, device=gpu)
    finals = []
    for zero in (False, True):
        torch.manual_seed(0)
        model = rcnet_main.build_model(gpu, cfg)
        model.train()
        opt = FlatAdam(model.parameters(), lr=1e-3)
        step = rcnet_main.GraphedTrainStep(model, opt, batch, cfg, warmup=1)
        p0 = opt.flat_param.clone()
        for _ in range(3):
            if zero:
                opt.zero_grad()
            step()
        assert not torch.equal(opt.flat_param, p0) and opt.step_count == 3, zero
        finals.append(opt.flat_param.clone())
    # only the fp32 atomic order of the small-map RoI-pool scatter differs between the runs; Adam's normalised first steps turn a sign
    # flip of a near-zero gradient into 2 lr per step, so the bound is a few lr relative to the largest weight (measured 1.2e-3)
    rel = float((finals[0] - finals[1]).abs().max() / finals[0].abs().max())
    assert rel <= 1e-2, rel
    moved = float((finals[1] - p0).abs().max())
    assert moved >= 2e-3, moved      # three Adam steps at lr 1e-3 really happened with zero_grad() in between


def test_staged_step_reports_buckets_in_backward_order(gpu):
    """Single-GPU check of the overlap plumbing (N > 1 itself cannot run on a 1-GPU box): with the all-reducer attached, a
    replayed step hands the decoder bucket over after the first graph, the transformer + point-MLP bucket after the second, and
    reduce() issues the image-encoder rest; together they tile the gradient arena exactly once."""
    import torch
    from riders_amd import rcnet_main
    from riders_amd.optim import FlatAdam
    from riders_amd.parallel import GradientAllReducer, rcnet_stages
    cfg = dict(rcnet_main.ZJU_CONFIG, patch_size=[64, 32], total_points_sampled=4)
    batch = rcnet_main.synthetic_batch(2, 64, 96, cfg, seed=5, device=gpu)
    torch.manual_seed(0)
    model = rcnet_main.build_model(gpu, cfg)
    model.train()
    opt = FlatAdam(model.parameters(), lr=1e-3)
    red = GradientAllReducer(opt, stages=rcnet_stages(model))
    try:
        step = rcnet_main.GraphedTrainStep(model, opt, batch, cfg, reducer=red, warmup=1)
        assert len(step.graphs) == 3 and step.tags == ["decoder_done", "attention_done", None]      # split at the stage marks
        assert red.log == []                       # no collective during warm-up / capture
        order = []
        orig = red.on_stage
        red.on_stage = lambda tag: (order.append(tag), orig(tag))[1]
        step()
        assert order == ["decoder_done", "attention_done"]
        eager_log = []
        red.on_stage = orig
        rcnet_main.train_step(model, opt, batch, cfg, red)     # eager autograd path: the same marks fire from the backward itself
        spans = sorted((s, e) for _, s, e in red.log[-3:])
        assert spans[0][0] == 0 and spans[-1][1] == opt.numel and all(a[1] == b[0] for a, b in zip(spans, spans[1:])), spans
        assert [t for t, _, _ in red.log[-3:]] == ["decoder_done", "attention_done", None]
    finally:
        red.close()


def test_step_with_rccl_collectives_matches_plain_step(gpu):
    """The N > 1 code path on one rank (a 1-GPU box cannot run more): an RCCL process group of size 1, the stage-bucketed asynchronous
    all-reduces issued between the replayed graphs, reduce() before Adam.  A sum over one rank is the identity, so the losses must follow
    the plain graphed step's."""
    import os
    import torch
    import torch.distributed as dist
    from riders_amd import rcnet_main
    from riders_amd.optim import FlatAdam
    from riders_amd.parallel import GradientAllReducer, rcnet_stages
    cfg = dict(rcnet_main.ZJU_CONFIG, patch_size=[64, 32], total_points_sampled=4)
    batch = rcnet_main.synthetic_batch(2, 64, 96, cfg, seed=5, device=gpu)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")
    dist.init_process_group(backend="nccl", rank=0, world_size=1, device_id=torch.device(gpu))
    try:
        losses, modes = {}, {}
        # rccl: one graph per stage, the stage's bucket started between two replays; rccl_rs_ag: reduce_scatter + all_gather per bucket instead of
        # one all-reduce.  (One graph with external stage events is not available: torch-rocm raises "External events are disallowed in rocm".)
        # c_abi / c_abi_rs_ag (round 5): the library's own communicator (rd_comm_init / rd_allreduce_bucket on its communication stream): the
        # collectives are CAPTURED, forward + backward + exchange are ONE graph
        from riders_amd.parallel import RcclComm
        comm = RcclComm()
        assert comm.world == 1 and comm.pending() == 0
        probe = torch.arange(1000, dtype=torch.float32, device=gpu)
        for md in (0, 1):
            comm.all_reduce(probe, md)
        assert comm.pending() == 2
        comm.join(probe)
        torch.cuda.synchronize()
        assert comm.pending() == 0 and torch.equal(probe.cpu(), torch.arange(1000, dtype=torch.float32))      # a sum over one rank
        for mode in ("plain", "rccl", "rccl_rs_ag", "c_abi", "c_abi_rs_ag"):
            torch.manual_seed(0)
            model = rcnet_main.build_model(gpu, cfg)
            model.train()
            opt = FlatAdam(model.parameters(), lr=1e-3)
            red = GradientAllReducer(opt, stages=rcnet_stages(model), mode="rs_ag" if mode.endswith("rs_ag") else "all_reduce",
                                     comm=comm if mode.startswith("c_abi") else None) if mode != "plain" else None
            try:
                if red is not None:
                    red.broadcast_parameters(0)
                step = rcnet_main.GraphedTrainStep(model, opt, batch, cfg, reducer=red, warmup=1)
                losses[mode] = [float(step()) for _ in range(3)]
                modes[mode] = len(step.graphs)
                if red is not None:
                    assert red.collective and opt.grad_scale == 1.0
                    assert [t for t, _, _ in red.log][:2] == ["decoder_done", "attention_done"], red.log      # the stage buckets go first, in backward order
            finally:
                if red is not None:
                    red.close()
        assert modes == {"plain": 1, "rccl": 3, "rccl_rs_ag": 3, "c_abi": 1, "c_abi_rs_ag": 1}, modes
        for m in ("rccl", "rccl_rs_ag", "c_abi", "c_abi_rs_ag"):
            for a, b in zip(losses["plain"], losses[m]):
                assert abs(a - b) <= 1e-3 * abs(a), (m, losses)
        assert losses["c_abi"][0] == losses["plain"][0], losses      # the first forward is bit-identical (later steps differ in the last digits: fp32 L2 atomics in the small-map RoI backward)
        # the eager step (torch.autograd + stage hooks) through the same transport
        torch.manual_seed(0)
        model = rcnet_main.build_model(gpu, cfg)
        model.train()
        opt = FlatAdam(model.parameters(), lr=1e-3)
        red = GradientAllReducer(opt, stages=rcnet_stages(model), comm=comm)
        try:
            red.broadcast_parameters(0)
            eager = [float(rcnet_main.train_step(model, opt, batch, cfg, red)) for _ in range(3)]
            assert comm.pending() == 0 and [t for t, _, _ in red.log][:2] == ["decoder_done", "attention_done"]
        finally:
            red.close()
        for a, b in zip(losses["plain"], eager):
            assert abs(a - b) <= 1e-3 * abs(a), (eager, losses)
        torch.cuda.synchronize()
        comm.close()
    finally:
        # quiesce before the group goes away: drop the captured graphs / reducer, drain the device and the communicator (one run in ~15 of the
        # round-4 build aborted inside destroy_process_group with the NCCL watchdog thread still polling)
        import gc
        step = red = model = opt = None
        gc.collect()
        torch.cuda.synchronize()
        dist.barrier()
        torch.cuda.synchronize()
        dist.destroy_process_group()


def test_bf16_wgrad_transpose_read(gpu):
    """bf16 weight gradient of narrow 3x3 layers through the LDS transpose read (rd_wgrad3x3.hip), bit-exact on integer data."""
    P.bf16_exact_conv_case(gpu, cin=16, cout=1, k=3, s=1, H=9, W=20, N=1)
    P.bf16_exact_conv_case(gpu, cin=16, cout=32, k=3, s=1, H=8, W=33, N=1)
    P.bf16_exact_conv_case(gpu, cin=32, cout=24, k=3, s=1, H=11, W=16, N=2)
    P.bf16_exact_conv_case(gpu, cin=64, cout=32, k=3, s=1, H=9, W=17, N=1)
    # wide layers: (64-channel input slice) x (32-channel output slice) blocks, concat boundary inside a slice, partial last output slice
    P.bf16_exact_conv_case(gpu, cin=128, cout=64, k=3, s=1, H=17, W=16, N=1)
    P.bf16_exact_conv_case(gpu, cin=96, cout=40, k=3, s=1, N=1, up=((5, 7), (15, 14)), cin2=32)
    P.bf16_exact_conv_case(gpu, cin=192, cout=16, k=3, s=1, H=8, W=14, N=2)
    with P.force_patch_conv(g8=1):
        P.bf16_exact_conv_case(gpu, cin=16, cout=16, k=3, s=1, H=40, W=50, N=2)
        P.bf16_exact_conv_case(gpu, cin=16, cout=16, k=3, s=1, N=2, up=((13, 9), (27, 64)), cin2=16)
    # full persistent grid (1024 blocks, several tiles each) at a slice of the ROI-resolution shapes
    P.bf16_exact_conv_case(gpu, cin=16, cout=16, k=3, s=1, H=240, W=100, N=12)
    P.bf16_exact_conv_case(gpu, cin=16, cout=16, k=3, s=1, N=12, up=((120, 50), (240, 100)), cin2=16)
    P.bf16_exact_conv_case(gpu, cin=64, cout=32, k=3, s=1, H=120, W=50, N=12)


def test_grouped_linear_wgrad(gpu):
    """rd_linear_wgrad_batch: bit-exact bf16 (transpose-read MFMA operands) and 1e-3 fp32 against the oracle, LoFTR-sized token counts."""
    P.bf16_exact_conv_case(gpu, cin=64, cout=192, k=1, s=1, H=9, W=7, N=3, cin2=64)
    P.bf16_exact_conv_case(gpu, cin=128, cout=64, k=1, s=1, H=41, W=17, N=1)
    P.bf16_exact_conv_case(gpu, cin=128, cout=256, k=1, s=1, H=240, W=21, N=1, cin2=128)
    P.conv_case(gpu, dict(cin=128, cout=64, k=1, s=1, H=13, W=11, N=2, bn=False, act=None))
    P.conv_case(gpu, dict(cin=64, cout=128, k=1, s=1, H=30, W=23, N=1, bn=True))
    # ragged edge tiles: channel counts that are multiples of the 16-byte vector only
    P.bf16_exact_conv_case(gpu, cin=24, cout=144, k=1, s=1, H=9, W=7, N=2)
    P.bf16_exact_conv_case(gpu, cin=64, cout=40, k=1, s=1, H=11, W=5, N=1, cin2=24)
    P.conv_case(gpu, dict(cin=36, cout=100, k=1, s=1, H=13, W=11, N=2, bn=True))
    P.conv_case(gpu, dict(cin=128, cout=128, k=1, s=1, H=240, W=21, N=1, bn=False, act=None))


def test_pack_batch(gpu):
    P.pack_batch_case(gpu)


def test_loftr_unfused_path(gpu):
    """The per-op LoFTR path (separate projection / attention / LayerNorm launches) stays covered now that eligible layers run fused."""
    from riders_amd import engine
    engine.set_fused_loftr(False)
    try:
        P.golden_attention_case(gpu)
        P.transformer_case(gpu)
    finally:
        engine.set_fused_loftr(True)


def test_bn_generic_channel_counts(gpu):
    """BatchNorm / activation passes for channel counts whose 16-byte vector count does not divide 256 (EfficientNet-Lite3 widths)."""
    P.conv_case(gpu, dict(cin=24, cout=40, k=1, s=1, H=13, W=11, N=2, bn=True))
    P.conv_case(gpu, dict(cin=16, cout=144, k=1, s=1, H=9, W=10, N=2, bn=True))
    P.conv_case(gpu, dict(cin=8, cout=232, k=3, s=1, H=6, W=7, N=1, bn=True))
    P.conv_case(gpu, dict(cin=8, cout=288, k=1, s=1, H=9, W=18, N=2, bn=True))     # > 256 channels: short per-block pixel ranges in the backward reduce
    P.conv_case(gpu, dict(cin=8, cout=816, k=1, s=1, H=5, W=7, N=1, bn=True))
    P.conv_case(gpu, dict(cin=16, cout=1392, k=1, s=1, H=9, W=18, N=4, bn=True))


def test_stem_padded_channels(gpu):
    """3-channel stems without an input gradient run zero-padded to one 16-byte vector (rd_pad_channels / rd_conv_pack_weights_padded /
    rd_unpad_weight_grad): forward, BatchNorm and the weight gradient must match the oracle on the original 3-channel weights."""
    P.conv_case(gpu, dict(cin=3, cout=32, k=7, s=2, H=20, W=18, N=2, bn=True, no_input_grad=True))
    P.conv_case(gpu, dict(cin=3, cout=32, k=3, s=2, H=15, W=14, N=1, bn=True, no_input_grad=True))
    P.conv_case(gpu, dict(cin=5, cout=16, k=3, s=1, H=9, W=11, N=2, bn=False, act=None, no_input_grad=True))


def test_roi_pool_gather_backward(gpu):
    P.roi_pool_stress_case(gpu)


def test_roi_pool_tile_backward_is_reproducible(gpu):
    P.roi_pool_tile_deterministic_case(gpu)


def test_direct_pointwise_conv(gpu):
    """1x1 layers with a short K axis through conv1x1_direct_kernel (pixel fragments straight from memory, weights in registers)."""
    with P.force_direct_1x1():
        P.conv_case(gpu, dict(cin=24, cout=144, k=1, s=1, H=13, W=11, N=2, bn=True))             # fp32: two k-steps, two channel blocks
        P.conv_case(gpu, dict(cin=16, cout=40, k=1, s=1, H=9, W=15, N=1, bn=False, act=None))    # fp32: one k-step
        P.bf16_exact_conv_case(gpu, cin=24, cout=144, k=1, s=1, H=13, W=11, N=2)                  # bf16: one k-step
        P.bf16_exact_conv_case(gpu, cin=48, cout=288, k=1, s=1, H=7, W=19, N=1)                   # bf16: two k-steps, three channel blocks
        P.bf16_exact_conv_case(gpu, cin=64, cout=8, k=1, s=1, H=10, W=13, N=1)
    P.bf16_exact_conv_case(gpu, cin=32, cout=192, k=1, s=1, H=144, W=192, N=2)   # routed by pixel count (55 K pixels)


def test_bf16_hardware_rounding_is_rne(gpu):
    """The kernels round fp32 -> bf16 with gfx950's v_cvt_pk_bf16_f32 (rd_common.h: f32_to_bf16 / pack_bf16x2); the emulator and the
    oracle use the integer round-to-nearest-even sequence.  Bit-exact on ties, denormals, infinities and the largest finite values."""
    import torch
    from riders_amd import engine
    g = torch.Generator().manual_seed(5)
    bits = torch.randint(-2**31, 2**31 - 1, (1 << 16,), dtype=torch.int64, generator=g).to(torch.int32)
    x = bits.view(torch.float32)
    x = x[torch.isfinite(x)]
    ties = (torch.arange(0x3f80, 0x3f80 + 512, dtype=torch.int32) << 16 | 0x8000).view(torch.float32)       # exactly half way
    above = (torch.arange(0x3f80, 0x3f80 + 512, dtype=torch.int32) << 16 | 0x8001).view(torch.float32)
    below = (torch.arange(0x3f80, 0x3f80 + 512, dtype=torch.int32) << 16 | 0x7fff).view(torch.float32)
    edge = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), 3.3895314e38, -3.3895314e38, 3.4028235e38, 1e-40, -1e-40, 1.1754944e-38,
                         9.1835e-41, 65504.0, 1.0, -1.0], dtype=torch.float32)
    x = torch.cat([x, ties, -ties, above, below, edge])
    if x.numel() % 8:
        x = x[: x.numel() - x.numel() % 8]
    xd = x.to(gpu)
    out = engine.cast(xd, torch.bfloat16)
    ref = x.to(torch.bfloat16)
    assert torch.equal(out.cpu().view(torch.int16), ref.view(torch.int16)), "fp32 -> bf16 rounding differs from round-to-nearest-even"


def test_roi_pool_gather_rcnet_geometry(gpu):
    P.roi_pool_gather_rcnet_geometry_case(gpu)


def test_wgrad_reduce_batch(gpu):
    P.wgrad_reduce_batch_case(gpu)


def test_streaming_weight_gradient_of_few_channel_layers(gpu):
    P.tiny_wgrad_cases(gpu)


def test_config4_per_rank_batch(gpu):
    P.config4_b8_case(gpu)


def test_point_mlp(gpu):
    P.point_mlp_case(gpu)


@pytest.mark.gpu
def test_stem_kernel(gpu):
    """conv_stem_kernel on small cases (RD_CONV_STEM_MIN_M=0) and at RC-Net's stem size through the default routing."""
    P.stem_kernel_cases(gpu)
    P.conv_case(gpu, dict(cin=3, cout=32, k=7, s=2, H=372, W=816, N=1, bn=True, no_input_grad=True))


@pytest.mark.gpu
def test_stride2_dgrad_parity_classes(gpu):
    P.stride2_dgrad_cases(gpu)
    P.bf16_exact_conv_case(gpu, cin=64, cout=128, k=3, s=2, H=93, W=204, N=1)      # RC-Net's 64 -> 128 stage at one image


@pytest.mark.gpu
def test_skinny_linear(gpu):
    P.skinny_linear_cases(gpu)



def test_rcnet_ntu_geometry_fp32_vs_oracle(gpu):
    """the reference's other RC-Net geometry (patch 150x50, K = 40, B = 4) -- nothing is specialised to the ZJU shapes"""
    P.rcnet_ntu_geometry_case(gpu)


def test_rcnet_bf16_trains_like_fp32(gpu):
    """150 optimisation steps, bf16 against fp32 against fp32's own sensitivity"""
    P.rcnet_bf16_convergence_case(gpu)


def test_integration_aliasing_block_against_the_hip_library(gpu):
    """INTEGRATION.md section 1's aliasing block + an unchanged-caller loop, two steps, losses vs the oracle"""
    from riders_amd import _lib
    assert _lib.load()._name.endswith("libriders_hip.so")
    P.integration_aliasing_case(gpu)


def test_graphed_step_load_batch_feeds_new_data(gpu):
    """a loop over real data puts `step.load_batch(batch)` in front of the replay.  Two different batches through ONE
    captured step must give the losses of the eager step on those batches (same weights trajectory), and a wrong shape is refused."""
    import pytest as _pt
    import torch
    from riders_amd import engine, rcnet_main
    from riders_amd.optim import FlatAdam
    cfg = dict(rcnet_main.ZJU_CONFIG, patch_size=[64, 32], total_points_sampled=4)
    batches = [rcnet_main.synthetic_batch(2, 64, 96, cfg, seed=s_, device=gpu) for s_ in (5, 6, 7)]
    losses = {}
    for mode in ("eager", "graph"):
        torch.manual_seed(0)
        model = rcnet_main.build_model(gpu, cfg)
        model.train()
        opt = FlatAdam(model.parameters(), lr=1e-3)
        engine.set_deterministic_roi_pool(True)
        try:
            if mode == "eager":
                losses[mode] = [float(rcnet_main.train_step(model, opt, b, cfg)) for b in batches]
            else:
                static = tuple(t_.clone() for t_ in batches[0])
                step = rcnet_main.GraphedTrainStep(model, opt, static, cfg, warmup=1)
                out = []
                for b in batches:
                    step.load_batch(b)
                    out.append(float(step()))
                losses[mode] = out
                with _pt.raises(ValueError):
                    step.load_batch(tuple(t_[:1] for t_ in b))
        finally:
            engine.set_deterministic_roi_pool(False)
    for a, b in zip(losses["eager"], losses["graph"]):
        assert abs(a - b) <= 1e-4 * abs(a), losses
    assert len(set(losses["graph"])) == 3


def _unchanged_loop(model_step, steps):
    return [model_step(i) for i in range(steps)]


def test_autograph_rcnet_unchanged_loop_matches_eager(gpu):
    """engine.set_autograph(True): the unchanged-caller loop (torch.autograd + torch.optim.Adam + loss.item(), RCNet/rcnet_main.py:342-359) with the
    model's forward region captured on its second call and replayed afterwards must reproduce the eager loop: same losses, same parameters,
    same BatchNorm buffers / counters -- over batches that CHANGE between steps -- and gradient accumulation without zero_grad keeps torch's
    semantics.  The region is captured once and replayed."""
    import torch
    from riders_amd import engine, rcnet_main
    cfg = dict(rcnet_main.ZJU_CONFIG, patch_size=[64, 32], total_points_sampled=4)
    batches = [rcnet_main.synthetic_batch(2, 64, 96, cfg, seed=20 + i, device=gpu) for i in range(5)]
    res = {}
    for mode in ("eager", "autograph"):
        engine.set_autograph(mode == "autograph")
        engine.set_deterministic_roi_pool(True)
        try:
            torch.manual_seed(0)
            model = rcnet_main.build_model(gpu, cfg)
            model.train()
            opt = torch.optim.Adam(model.parameters(), lr=1e-3)
            losses = []
            for i, b in enumerate(batches):
                loss = rcnet_main.forward_loss(model, b, cfg)
                if i != 3:                      # step 3 accumulates on top of step 2's gradients (no zero_grad)
                    opt.zero_grad()
                loss.backward()
                opt.step()
                losses.append(loss.item())
            sd = {k: v.detach().clone() for k, v in list(model.encoder.state_dict().items()) + list(model.decoder.state_dict().items())}
            res[mode] = (losses, sd, engine.autograph_stats() if mode == "autograph" else None)
        finally:
            engine.set_autograph(False)
            engine.set_deterministic_roi_pool(False)
    (le, sde, _), (la, sda, st) = res["eager"], res["autograph"]
    assert st["captured"] - 0 >= 1 and st["replayed"] >= 4, st
    for a, b in zip(le, la):
        assert abs(a - b) <= 1e-5 * abs(a), (le, la)
    for k in sde:
        if sde[k].is_floating_point():
            d = float((sde[k] - sda[k]).abs().max()), float(sde[k].abs().max())
            assert d[0] <= 1e-4 * max(d[1], 1e-3), (k, d)
        else:
            assert torch.equal(sde[k], sda[k]), k      # num_batches_tracked


def test_autograph_sml_unchanged_loop_matches_eager(gpu):
    """the same for the Scale Map Learner's loop (train_zju.py:353-392): pre-step, model.forward captured / replayed, compute_loss, torch.optim.Adam"""
    import contextlib
    import io
    import torch
    from riders_amd import engine, sml_main
    batches = [sml_main.synthetic_batch(2, 64, 96, seed=40 + i, device=gpu) for i in range(4)]
    res = {}
    for mode in ("eager", "autograph"):
        engine.set_autograph(mode == "autograph")
        try:
            torch.manual_seed(0)
            with contextlib.redirect_stdout(io.StringIO()):
                model = sml_main.build_model(gpu)
            model.train()
            opt = torch.optim.Adam(model.parameters(), lr=1e-4)
            orr = sml_main.make_outlier_removal()
            losses = []
            for b in batches:
                loss = sml_main.forward_loss(model, b, outlier=orr)
                opt.zero_grad()
                loss.backward()
                opt.step()
                losses.append(loss.item())
            res[mode] = (losses, {k: v.detach().clone() for k, v in model.state_dict().items()}, engine.autograph_stats())
        finally:
            engine.set_autograph(False)
    (le, sde, _), (la, sda, st) = res["eager"], res["autograph"]
    assert st["captured"] >= 1 and st["replayed"] >= 3, st
    for a, b in zip(le, la):
        assert abs(a - b) <= 1e-5 * abs(a), (le, la)
    for k in sde:
        if sde[k].is_floating_point():
            d = float((sde[k] - sda[k]).abs().max()), float(sde[k].abs().max())
            assert d[0] <= 1e-4 * max(d[1], 1e-3), (k, d)
        else:
            assert torch.equal(sde[k], sda[k]), k


def test_autograph_other_shapes_and_eval_take_the_right_path(gpu):
    """A captured region must not be replayed for anything it was not captured for: a batch of another size runs eagerly (and is captured on its
    own second call), a validation forward under no_grad in between is eager and sees the trained BatchNorm statistics, and going back to the
    first geometry replays its entry again.  Losses against the all-eager loop."""
    import torch
    from riders_amd import engine, rcnet_main
    cfg = dict(rcnet_main.ZJU_CONFIG, patch_size=[64, 32], total_points_sampled=4)
    sizes = [2, 2, 2, 1, 1, 2, 1, 2]
    batches = [rcnet_main.synthetic_batch(b, 64, 96, cfg, seed=60 + i, device=gpu) for i, b in enumerate(sizes)]
    res = {}
    for mode in ("eager", "autograph"):
        engine.set_autograph(mode == "autograph")
        engine.set_deterministic_roi_pool(True)
        try:
            torch.manual_seed(0)
            model = rcnet_main.build_model(gpu, cfg)
            model.train()
            opt = torch.optim.Adam(model.parameters(), lr=1e-3)
            out = []
            for i, b in enumerate(batches):
                loss = rcnet_main.forward_loss(model, b, cfg)
                opt.zero_grad(); loss.backward(); opt.step()
                out.append(loss.item())
                if i == 4:      # a validation pass in the middle of training
                    model.eval()
                    with torch.no_grad():
                        out.append(float(rcnet_main.forward_loss(model, batches[0], cfg)))
                    model.train()
            res[mode] = (out, engine.autograph_stats())
        finally:
            engine.set_autograph(False)
            engine.set_deterministic_roi_pool(False)
    (le, _), (la, st) = res["eager"], res["autograph"]
    for a, b in zip(le, la):
        assert abs(a - b) <= 1e-5 * abs(a), (le, la)
    assert st["captured"] >= 2 and st["eager"] >= 2, st      # two geometries, each: first call eager, second captured


def test_pointwise_gemm_kernel(gpu):
    P.pw_gemm_cases(gpu)


def test_bn_one_launch_wide_layers(gpu):
    P.bn_slab_cases(gpu)


@pytest.mark.parametrize("case", [c["name"] for c in P.ROUTE_CASES])
def test_conv_block_routes(gpu, case):
    """The emulator's route table (tests/test_emu_ops.py) against the real library: the same launch sequences, the same oracle comparison."""
    P.route_case(gpu, next(c for c in P.ROUTE_CASES if c["name"] == case))
