"""RC-Net training / inference harness on MI355X: the counterpart of the reference's RCNet/rcnet_main.py for the
hot path (train step body :272-359, forward_output :435-487) plus the synthetic ZJU-shape batch generator that
restates the tensor contract of data/datasets.py:170-288.  File I/O, TensorBoard and the
augmentation transforms are out of scope.
"""
import ctypes
import os

import torch
import torch.distributed

from . import engine
from .networks import boxes_to_rois
from .optim import DynamicLossScale
from .rcnet_model import RCNetModel

# RCNet/train_rcnet_zju.py:28-65
ZJU_CONFIG = dict(
    patch_size=[240, 100], total_points_sampled=30, batch_size=4,
    input_channels_image=3, input_channels_depth=3,
    encoder_type=['rcnet', 'batch_norm'], n_filters_encoder_image=[32, 64, 128, 128, 128],
    n_neurons_encoder_depth=[32, 64, 128, 128, 128],
    decoder_type=['multiscale', 'batch_norm'], n_filters_decoder=[256, 128, 64, 32, 16],
    weight_initializer='kaiming_uniform', activation_func='leaky_relu',
    learning_rate=2e-4, w_positive_class=2.5, max_distance_correspondence=0.5, set_invalid_to_negative_class=False,
)


def build_model(device, cfg=ZJU_CONFIG):
    return RCNetModel(cfg['input_channels_image'], cfg['input_channels_depth'], cfg['patch_size'], cfg['encoder_type'],
                      cfg['n_filters_encoder_image'], cfg['n_neurons_encoder_depth'], cfg['decoder_type'],
                      cfg['n_filters_decoder'], cfg['weight_initializer'], cfg['activation_func'], device=device)


def synthetic_batch(batch_size, height=256, width=512, cfg=ZJU_CONFIG, seed=1234, device='cpu'):
    """The tuple RCNetTrainingDataset.__getitem__ returns, batched (data/datasets.py:288):
    image (B,3,H+ph,W+pw) fp32 0..255 edge-padded; radar_points (B,K,3) = (x+pad_x, y+pad_y, z);
    bounding_boxes (B,K,4) = (x-pad_x, y-pad_y, x+pad_x, y+pad_y) in padded coords; ground truth crops
    (B,K,1,ph,pw) cut from a zero-padded synthetic dense depth with ~50% invalid pixels."""
    g = torch.Generator().manual_seed(seed)
    ph, pw = cfg['patch_size']
    pad_y, pad_x = ph // 2, pw // 2
    K = cfg['total_points_sampled']
    B = batch_size
    img = torch.randint(0, 256, (B, 3, height, width), generator=g).float()
    img = torch.nn.functional.pad(img, (pad_x, pad_x, pad_y, pad_y), mode='replicate')
    x = torch.randint(0, width, (B, K), generator=g).float()
    y = torch.randint(0, height, (B, K), generator=g).float()
    z = torch.rand((B, K), generator=g) * 98.5 + 1.5
    pts = torch.stack([x + pad_x, y + pad_y, z], dim=-1)
    boxes = torch.stack([pts[..., 0] - pad_x, pts[..., 1] - pad_y, pts[..., 0] + pad_x, pts[..., 1] + pad_y], dim=-1)
    depth = torch.rand((B, 1, height, width), generator=g) * 98.5 + 1.5
    depth = depth * (torch.rand((B, 1, height, width), generator=g) > 0.5).float()
    # make a share of pixels agree with the radar depth so that positives exist
    depth = torch.nn.functional.pad(depth, (pad_x, pad_x, pad_y, pad_y))
    crops = torch.empty((B, K, 1, ph, pw))
    for b in range(B):
        for k in range(K):
            xs, ys = int(pts[b, k, 0]) - pad_x, int(pts[b, k, 1]) - pad_y
            c = depth[b, :, ys:ys + ph, xs:xs + pw].clone()
            m = (torch.rand(c.shape, generator=g) < 0.05) & (c > 0)
            c[m] = z[b, k] + 0.25
            crops[b, k] = c
    return tuple(t.to(device) for t in (img, pts, boxes, crops))


def prepare_batch(batch):
    """Device-side batch preparation of the train loop (rcnet_main.py:283-340): /255 normalise (rcnet_transforms.py:258),
    flatten points and crops, per-image box list -> ROI rows."""
    image, radar_point, boxes, gt = batch
    image = engine.as_nchw(engine.nchw_to_nhwc(image, scale=1.0 / 255.0))
    B, K = radar_point.shape[0], radar_point.shape[1]
    radar_point = radar_point.reshape(B * K, radar_point.shape[2])
    gt = gt.reshape(B * K, gt.shape[2], gt.shape[3], gt.shape[4])
    rois = boxes_to_rois(boxes)
    return image, radar_point, rois, gt


def scaled_backward(loss, optimizer, loss_scale):
    """loss.backward() with the loss scale of the fp16 mode (the seed gradient is the scale; Adam divides it out again): a float is the static
    scale, an optim.DynamicLossScale seeds the backward with its device word, which the optimizer's step then adjusts (torch.amp.GradScaler's rule).
    Several ranks: the step's finite check reads the reduced arena, after the all-reducer's join, so the ranks decide alike."""
    if isinstance(loss_scale, DynamicLossScale):
        optimizer.loss_scale = loss_scale
        loss.backward(loss_scale.scale_tensor.view(loss.shape))
        return
    optimizer.loss_scale = float(loss_scale)
    if loss_scale == 1.0:
        loss.backward()
    else:
        loss.backward(torch.full_like(loss, float(loss_scale)))


def train_step(model, optimizer, batch, cfg=ZJU_CONFIG, reducer=None, loss_scale=1.0):
    """One optimisation step (rcnet_main.py:294-359).  Returns the loss as a device tensor (no host sync)."""
    loss = forward_loss(model, batch, cfg)
    optimizer.zero_grad()
    scaled_backward(loss, optimizer, loss_scale)
    if reducer is not None:
        reducer.reduce()
    optimizer.step()
    return loss


def _scatter(crops, pts, ph, pw, H, W, response_thr):
    depth = torch.empty((1, H, W), dtype=torch.float32, device=crops.device)
    resp = torch.empty((1, H, W), dtype=torch.float32, device=crops.device)
    engine._chk(engine.L().rd_scatter_crops(engine._p(crops), engine._p(pts), engine._p(depth), engine._p(resp), crops.shape[0], ph, pw,
                                            H, W, ctypes.c_float(response_thr), engine.rd_of(crops), engine._stream(crops)),
                "rd_scatter_crops")
    return depth, resp


def forward_crops(model, image, radar_points, bounding_boxes_list):
    """First half of rcnet_main.py:435-487: edge-pad, one forward over all N points -> (crops (N,1,ph,pw) sigmoid responses, points)."""
    ph, pw = model.input_patch_size_image
    pad_y, pad_x = ph // 2, pw // 2
    image = torch.nn.functional.pad(image, (pad_x, pad_x, pad_y, pad_y), mode='replicate')  # data prep, as the reference
    if radar_points.dim() == 3:
        radar_points = torch.squeeze(radar_points, dim=0)
    pts = radar_points.contiguous().float()
    crops = model.forward(image=image, point=pts, bounding_boxes=bounding_boxes_list, return_logits=False)
    return crops, pts, (image.shape[-2] - 2 * pad_y, image.shape[-1] - 2 * pad_x)


def forward_output(model, image, radar_points, bounding_boxes_list, response_thr=0.5, device=None):
    """rcnet_main.py:435-487: edge-pad, one forward over all N points, threshold, integer paste, confidence-weighted
    mean depth; zero where nothing responds.  image (1,3,H,W) already normalised; radar_points (N,3) in padded coords."""
    ph, pw = model.input_patch_size_image
    crops, pts, (H, W) = forward_crops(model, image, radar_points, bounding_boxes_list)
    return _scatter(crops, pts, ph, pw, H, W, response_thr)


def points_to_boxes(radar_points, patch_size):
    """run_rcnet_zju.py:221-234: (N,3) radar points in image coordinates -> (points shifted into the padded image, RoI rows
    (0, x - pad_x, y - pad_y, x + pad_x, y + pad_y)); one launch instead of the reference's per-point Python loop."""
    pad_x, pad_y = patch_size[1] // 2, patch_size[0] // 2
    pts = radar_points.reshape(-1, radar_points.shape[-1]).contiguous().float()
    N = pts.shape[0]
    out = torch.empty_like(pts)
    rois = torch.empty((N, 5), dtype=torch.float32, device=pts.device)
    engine._chk(engine.L().rd_points_to_rois(engine._p(pts), engine._p(out), engine._p(rois), N, float(pad_x), float(pad_y), 0,
                                             engine._stream(pts)), "rd_points_to_rois")
    return out, rois


def fuse_with_retry(crops, pts, ph, pw, H, W, response_thr=0.5, thr_step=0.05):
    """run_rcnet_zju.py:250-264: fuse the crops (rcnet_main.py:460-485); while the fused depth sums to zero lower the threshold by 0.05."""
    thr = response_thr
    total = torch.empty(1, dtype=torch.float64, device=crops.device)
    while True:
        depth, resp = _scatter(crops, pts, ph, pw, H, W, thr)
        engine._chk(engine.L().rd_sum_f32(engine._p(depth), depth.numel(), engine._p(total), engine._stream(depth)), "rd_sum_f32")
        if float(total) != 0.0:
            return depth, resp, thr
        if thr < -1.0:
            raise RuntimeError("fuse_with_retry: no radar point responds at any threshold (no points?)")
        thr = thr - thr_step


def run_frame(model, image, radar_points, response_thr=0.5, thr_step=0.05):
    """One frame of run_rcnet_zju.py:204-266: box construction (:221-234), /255 normalisation (transforms, :236-240), forward_output
    (:242-248) and the retry loop (:250-264) that lowers the response threshold by 0.05 while the fused depth map is all zeros.
    The reference re-runs the whole network per retry; the crops do not depend on the threshold, so only the scatter is repeated here.
    image (1,3,H,W) 0..255, radar_points (N,3) or (1,N,3) image coordinates.  Returns (depth (H,W) fp32, response (H,W), threshold)."""
    ph, pw = model.input_patch_size_image
    pts, rois = points_to_boxes(radar_points, (ph, pw))
    img = engine.as_nchw(engine.nchw_to_nhwc(image.float(), scale=1.0 / 255.0, dtype=torch.float32))
    with torch.no_grad():
        crops, pts, (H, W) = forward_crops(model, img, pts, rois)
        depth, resp, thr = fuse_with_retry(crops, pts, ph, pw, H, W, response_thr, thr_step)
    return depth[0], resp[0], thr


_no_response_flags = {}     # device -> sticky int32 word of rd_frame_thresholds (a frame without a positive in-image response)


def _no_response_flag(dev):
    f = _no_response_flags.get(str(dev))
    if f is None:
        if dev.type == 'cuda' and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("fuse_frames: the first call on a device allocates and zeroes its sticky flag word; make one call before capturing "
                               "(a fill inside the capture would clear the flag on every replay)")
        f = _no_response_flags[str(dev)] = torch.zeros(1, dtype=torch.int32, device=dev)
    return f


def check_no_response():
    """Host-side check of rd_frame_thresholds' sticky flag (synchronises: the one host read of the frame-batch path; call it where the host
    waits anyway, e.g. after the maps of a batch were copied back, as engine.check_roi_overflow): raises, once, if a frame fused since the
    last check had no positive response inside the image -- the case in which the reference's retry loop never ends and fuse_with_retry
    raises.  Such a frame has retries == -1 and all-zero maps; the other frames of its batch are unaffected."""
    bad = [k for k, f in _no_response_flags.items() if int(f.cpu()[0])]
    for k in bad:
        _no_response_flags[k].zero_()
    if bad:
        raise RuntimeError("riders_amd: a frame had no positive response inside the image at any threshold (no radar points, or every crop "
                           "pasted outside the image): its retries entry is -1 and its maps are zero")


def fuse_frames(crops, pts, frame_start, ph, pw, H, W, response_thr=0.5, thr_step=0.05):
    """The fusion of F frames (rcnet_main.py:460-485) with the threshold retry of run_rcnet_zju.py:250-264 decided on the device: three launches in
    one chain (in-image maxima, threshold per frame, scatter) and no host read, so the call can be captured in a hipGraph.
    crops (R,1,ph,pw) or (R,ph,pw) responses of all frames, frame-major; pts (R,3) in padded coordinates; frame_start: int32 DEVICE tensor (F+1,),
    ascending, frame_start[0] = 0, frame_start[F] = R.  -> depth (F,H,W), response (F,H,W), thr (F,) float32, retries (F,) int32, all on the device.
    For every frame depth / response / thr equal fuse_with_retry on the frame's slice, bit for bit.  Precondition, as in the reference: radar
    depths are positive (z > 0; the dataset's range filter guarantees it), so "the fused depth sums to zero" means "no response passed the
    threshold".  A frame without any positive in-image response gets retries = -1, zero maps, thr = response_thr, and raises the sticky flag
    check_no_response() reads."""
    R = int(crops.shape[0])
    F = int(frame_start.numel()) - 1
    if F < 0 or frame_start.dtype != torch.int32 or frame_start.device != crops.device:
        raise ValueError("fuse_frames: frame_start must be an int32 tensor of F + 1 entries on the crops' device")
    dev = crops.device
    crops = crops if crops.is_contiguous() else crops.contiguous()
    pts = pts if (pts.dtype == torch.float32 and pts.is_contiguous()) else pts.contiguous().float()
    if crops.numel() != R * ph * pw or tuple(pts.shape) != (R, 3):
        raise ValueError("fuse_frames: crops %s / points %s do not describe %d patches of %d x %d" % (tuple(crops.shape), tuple(pts.shape), R, ph, pw))
    lib = engine.L()
    depth = torch.empty((F, H, W), dtype=torch.float32, device=dev)
    resp = torch.empty((F, H, W), dtype=torch.float32, device=dev)
    rmax = torch.empty(F, dtype=torch.float32, device=dev)
    thr = torch.empty(F, dtype=torch.float32, device=dev)
    retries = torch.empty(F, dtype=torch.int32, device=dev)
    if F == 0:
        return depth, resp, thr, retries
    ws = torch.empty(int(lib.rd_frame_thresholds_ws_bytes(R)) // 4, dtype=torch.float32, device=dev)
    flag = _no_response_flag(dev)
    st = engine._stream(frame_start)
    engine._chk(lib.rd_frame_thresholds(engine._p(crops), engine._p(pts), engine._p(frame_start), R, F, ph, pw, H, W, float(response_thr),
                                        float(thr_step), engine._p(ws), engine._p(rmax), engine._p(thr), engine._p(retries), engine._p(flag),
                                        engine.rd_of(crops), st), "rd_frame_thresholds")
    engine._chk(lib.rd_scatter_crops_frames(engine._p(crops), engine._p(pts), engine._p(frame_start), engine._p(thr), engine._p(depth),
                                            engine._p(resp), R, F, ph, pw, H, W, engine.rd_of(crops), st), "rd_scatter_crops_frames")
    return depth, resp, thr, retries


def run_frames(model, images, radar_points, response_thr=0.5, thr_step=0.05):
    """run_rcnet_zju.py:204-266 for F frames in ONE network forward and one fuse_frames: box construction per frame into slices of one RoI tensor
    (each frame's batch index), /255 normalisation, forward over all R = sum N_f points, fusion with the retry threshold decided on the device.
    images (F,3,H,W) 0..255; radar_points: list of F tensors (N_f,3) in image coordinates, N_f may differ (the list lengths are host knowledge;
    frame_start is built from them and uploaded once).  The model is in eval mode: BatchNorm's running statistics make a frame's result
    independent of its batch mates.  -> (depth (F,H,W), response (F,H,W), thr (F,), retries (F,)) on the device, without a host read: call
    check_no_response() where the host waits anyway.  data_utils.quantize_depth takes the (F,H,W) depth as it is.
    Measured (tools/bench_infer.py -> profiles/infer_frames.txt, DESIGN.md "Inference over frame batches"): at F = 1 within the spread of a run_frame
    loop, 3.4 x / 4.9 x / 6.1 x its frames/s at F = 4 / 8 / 16 in bf16 (1.9 x / 2.0 x / 2.1 x in fp32) -- prefer this path whenever frames can be
    batched; run_frame stays as it is."""
    ph, pw = model.input_patch_size_image
    pad_x, pad_y = pw // 2, ph // 2
    F = int(images.shape[0])
    if len(radar_points) != F:
        raise ValueError("run_frames: %d point tensors for %d frames" % (len(radar_points), F))
    dev = images.device
    per_frame = [p.reshape(-1, p.shape[-1]) for p in radar_points]
    starts = [0]
    for p in per_frame:
        starts.append(starts[-1] + int(p.shape[0]))
    R = starts[-1]
    frame_start = torch.tensor(starts, dtype=torch.int32).to(dev)
    pts = torch.empty((R, 3), dtype=torch.float32, device=dev)
    rois = torch.empty((R, 5), dtype=torch.float32, device=dev)
    lib = engine.L()
    for f, p in enumerate(per_frame):
        n = int(p.shape[0])
        if n == 0:
            continue
        p = p if (p.dtype == torch.float32 and p.is_contiguous() and p.device == dev) else p.to(dev).contiguous().float()
        engine._chk(lib.rd_points_to_rois(engine._p(p), engine._p(pts[starts[f]:]), engine._p(rois[starts[f]:]), n, float(pad_x), float(pad_y), f,
                                          engine._stream(pts)), "rd_points_to_rois")
    H, W = int(images.shape[-2]), int(images.shape[-1])
    with torch.no_grad():
        if R > 0:
            img = engine.as_nchw(engine.nchw_to_nhwc(images.float(), scale=1.0 / 255.0, dtype=torch.float32))
            crops, pts, _ = forward_crops(model, img, pts, rois)
        else:
            crops = torch.empty((0, 1, ph, pw), dtype=torch.float32, device=dev)
        return fuse_frames(crops, pts, frame_start, ph, pw, H, W, response_thr, thr_step)


def forward_loss(model, batch, cfg=ZJU_CONFIG):
    """Label build + forward + masked BCE of one step (rcnet_main.py:294-352) -> loss tensor."""
    image, radar_point, rois, gt = prepare_batch(batch)
    label, valid = engine.rcnet_labels(gt, radar_point, cfg['max_distance_correspondence'], cfg['set_invalid_to_negative_class'])
    logits = model.forward(image, radar_point, rois, return_logits=True)
    loss, _ = model.compute_loss(logits=logits, ground_truth=label, validity_map=valid, w_positive_class=cfg['w_positive_class'])
    return loss


def compute_gradients(model, optimizer, batch, cfg=ZJU_CONFIG, loss_scale=1.0):
    """Forward + loss + backward of one step (everything of rcnet_main.py:294-358 except the optimizer) through torch.autograd,
    as an unchanged training script would run it."""
    loss = forward_loss(model, batch, cfg)
    optimizer.zero_grad()
    scaled_backward(loss, optimizer, loss_scale)
    return loss


def staged_gradients(fwd_loss, optimizer, on_stage=None, loss_scale=1.0):
    """The same step on ONE engine tape driven from this thread (engine.StepTape, no torch.autograd): the backward stops at every
    stage mark and calls `on_stage(tag)`, which is where GraphedStep ends one hipGraph capture and begins the next.  The stage hooks
    registered with the engine (the all-reducer's) fire at the same marks."""
    optimizer.zero_grad()
    dynamic = isinstance(loss_scale, DynamicLossScale)
    optimizer.loss_scale = loss_scale if dynamic else float(loss_scale)
    st = engine.StepTape()
    loss = st.forward(fwd_loss)
    st.seed(loss, loss_scale.scale_tensor if dynamic else loss_scale)      # the device word itself: a replay reads the scale of that moment
    while True:
        tag = st.backward_stage()
        if tag is None:
            break
        if on_stage is not None:
            on_stage(tag)
    st.finish()
    return loss


class GraphedStep(object):
    """The launch-bound part of a step (forward + loss + backward: ~1100 small kernel launches for RC-Net) captured once into
    hipGraphs and replayed per step; the RCCL gradient all-reduce and the fused Adam launch stay eager.  With an all-reducer the capture
    is SPLIT at the model's stage marks: after the graph of a stage has been enqueued the all-reducer starts that stage's bucket on the
    communication stream, so the exchange overlaps the replay of the remaining backward graphs.  Without one it is a single graph.
    `fwd_loss()` runs forward + loss on static device tensors and returns the loss tensor; `on_replay(n)` keeps host-side bookkeeping
    (BatchNorm num_batches_tracked counters) in step with replays; `buffers` are tensors the forward updates in place (BatchNorm running
    statistics): the warm-up passes needed before a capture are undone on them, so constructing a GraphedStep trains nothing."""

    def __init__(self, fwd_loss, optimizer, reducer=None, warmup=2, on_replay=None, buffers=(), loss_scale=1.0):
        self.opt, self.reducer, self.on_replay = optimizer, reducer, on_replay
        assert engine._timer["t"] is None, "kernel timing and graph capture are exclusive"
        buffers = list(buffers)
        hooks, engine._stage_hooks[:] = list(engine._stage_hooks), []      # no collectives during warm-up / capture
        try:
            saved = [b.clone() for b in buffers]
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(warmup):
                    staged_gradients(fwd_loss, optimizer, None, loss_scale)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            with torch.no_grad():
                for b, s_ in zip(buffers, saved):
                    b.copy_(s_)
            self.graphs, self.tags = [], []
            pool = torch.cuda.graph_pool_handle()
            state = {}
            # The library's own collectives (parallel.RcclComm: rd_allreduce_bucket on its communication stream) are stream operations and
            # are CAPTURED: forward + backward + every bucket's exchange + the final join are one graph, the fork / join of the communication
            # stream are graph edges (round 5; replaces the per-stage graphs below for that transport).
            self.captured_comm = reducer is not None and getattr(reducer, "comm", None) is not None
            if self.captured_comm:      # RCCL sets up channels / buffers lazily on a communicator's first collective: not inside a capture
                warm = torch.zeros(256, dtype=torch.float32, device=optimizer.flat_grad.device)
                reducer.comm.all_reduce(warm)
                reducer.comm.join(warm)
                torch.cuda.synchronize()
            # With an all-reducer the capture is SPLIT at the stage marks (one graph per stage; measured 5 % slower than one graph at one rank
            # before any wire time).  ONE graph with an external event recorded at each mark (an event-record node the communication side could
            # wait on) was built in round 4 and cannot run: torch-rocm 2.10 raises "External events are disallowed in rocm" for
            # torch.cuda.Event(external=True) under capture, and an event recorded behind torch's back on a capturing stream is not something
            # that can be validated on a 1-GPU pool (a mis-ordered wait would all-reduce unfinished gradients silently).
            def begin():
                state["g"] = torch.cuda.CUDAGraph()
                # thread_local whenever a communicator lives in this process: RCCL's proxy thread and torch.distributed's NCCL watchdog thread
                # (event queries) touch the runtime while this thread captures; in the default global mode such a call invalidates the
                # capture or aborts the process (seen once in ~15 runs of the one-rank RCCL test in round 4, and again in round 5)
                relaxed = reducer is not None or (torch.distributed.is_available() and torch.distributed.is_initialized())
                state["ctx"] = torch.cuda.graph(state["g"], pool=pool, **({"capture_error_mode": "thread_local"} if relaxed else {}))
                state["ctx"].__enter__()

            def end(tag):
                state["ctx"].__exit__(None, None, None)
                self.graphs.append(state["g"])
                self.tags.append(tag)

            def boundary(tag):
                end(tag)
                begin()

            begin()
            try:
                # without an all-reducer there is nothing to interleave: one graph (each extra graph launch costs ~1 % of an RC-Net step)
                if self.captured_comm:
                    self.loss = staged_gradients(fwd_loss, optimizer, reducer.on_stage, loss_scale)
                    reducer.reduce()      # the remaining buckets + the join, inside the capture
                else:
                    self.loss = staged_gradients(fwd_loss, optimizer, boundary if reducer is not None else None, loss_scale)
            except BaseException:
                state["ctx"].__exit__(None, None, None)
                raise
            end(None)
            # a replay writes the gradient arena without passing the optimizer's gradient allocator: remember what the capture pass touched
            self.touched = optimizer.touched_indices() if hasattr(optimizer, "touched_indices") else None
            if self.touched is not None and not self.touched:
                raise RuntimeError("GraphedStep: the captured backward wrote no parameter gradient")
        finally:
            engine._stage_hooks[:] = hooks
        if on_replay is not None:
            on_replay(-(warmup + 1))  # neither the warm-up passes (undone) nor the capture pass (not executed) were training steps

    def load_batch(self, batch):
        """Copy a new batch into the static tensors the captured step reads (same shapes / dtypes; device-to-device or host-to-device copies on the
        current stream, ordered before the next replay).  This is the one line a training loop adds in front of `step()` when it feeds real data:
        `step.load_batch(next(loader)); loss = step()`."""
        static = getattr(self, "static_batch", None)
        if static is None:
            raise RuntimeError("this GraphedStep was built from a closure, not from a batch: there are no static input tensors to load into")
        if len(static) != len(batch):
            raise ValueError("load_batch: %d tensors, the captured step reads %d" % (len(batch), len(static)))
        for dst, src in zip(static, batch):
            if tuple(dst.shape) != tuple(src.shape):
                raise ValueError("load_batch: shape %s does not match the captured %s (a hipGraph replays fixed shapes)" % (tuple(src.shape), tuple(dst.shape)))
            if src.is_cuda:
                engine.dev_copy(dst, src)      # a kernel, not a hipMemcpyAsync, in front of the replay (engine.dev_copy)
            else:
                dst.copy_(src, non_blocking=True)

    def __call__(self):
        for g, tag in zip(self.graphs, self.tags):
            g.replay()
            if tag is not None and self.reducer is not None:
                self.reducer.on_stage(tag)
        if self.on_replay is not None:
            self.on_replay(+1)
        if self.reducer is not None and not self.captured_comm:
            self.reducer.reduce()
        if self.touched is not None:      # the replay filled these slots, whatever zero_grad() calls happened since the capture
            self.opt.mark_touched(self.touched)
        self.opt.step()
        return self.loss


class GraphedTrainStep(GraphedStep):
    """RC-Net training step with forward+backward replayed from hipGraphs (inputs: the static tensors of `batch`)."""

    def __init__(self, model, optimizer, batch, cfg=ZJU_CONFIG, reducer=None, warmup=2, loss_scale=1.0):
        nets = [RCNetModel._unwrap(model.encoder), RCNetModel._unwrap(model.decoder)]
        bn = [m for net in nets for m in net.modules() if getattr(m, 'use_batch_norm', False) and hasattr(m, '_nbt_pending')]

        def bump(delta):
            for m in bn:
                if m._bn_counts():      # per BatchNorm: only layers that run in training mode count a batch
                    m._nbt_pending += delta
        buffers = [b for net in nets for b in net.buffers() if b.is_floating_point()]
        self.static_batch = tuple(batch)
        super().__init__(lambda: forward_loss(model, batch, cfg), optimizer, reducer, warmup, bump, buffers, loss_scale)
