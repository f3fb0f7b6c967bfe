"""Device-agnostic cases of RC-Net inference over frame batches (riders_amd/csrc/rd_infer.hip, rcnet_main.fuse_frames / run_frames): run on the
GPU (tests/test_gpu_infer.py) and under the fiber emulator (tests/test_emu_infer.py).  The oracles are the single-frame path that was there
before (rd_scatter_crops, rcnet_main.fuse_with_retry -- bit-exact), the REFERENCE's own forward_output results (fixture g10) and
oracle.rcnet.forward_output run in the reference's retry loop."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import rcnet as O
from tests.parity_cases import close, leaves, load, t


def _i32(a, dev):
    return torch.tensor(list(a), dtype=torch.int32).to(dev)


def _frames(dev, crops, pts, frame_start, thr, patch, H, W):
    """rd_scatter_crops_frames through the C ABI -> (depth, response) numpy (F,H,W)"""
    from riders_amd import engine
    F = len(frame_start) - 1
    depth = torch.full((F, H, W), -7.0, dtype=torch.float32, device=dev)
    resp = torch.full((F, H, W), -7.0, dtype=torch.float32, device=dev)
    fs, th = _i32(frame_start, dev), torch.tensor(thr, dtype=torch.float32).to(dev)
    rc = engine.L().rd_scatter_crops_frames(engine._p(crops), engine._p(pts), engine._p(fs), engine._p(th), engine._p(depth), engine._p(resp),
                                            crops.shape[0], F, patch[0], patch[1], H, W, engine.rd_of(crops), engine._stream(depth))
    assert rc == 0, engine.L().rd_last_error_string()
    return depth.cpu().numpy(), resp.cpu().numpy()


def _single(dev, crops, pts, thr, patch, H, W):
    """the parent kernel on one frame's slice -> (depth, response) numpy (H,W)"""
    from riders_amd import engine
    depth = torch.full((1, H, W), -3.0, dtype=torch.float32, device=dev)
    resp = torch.full((1, H, W), -3.0, dtype=torch.float32, device=dev)
    n = crops.shape[0]
    rc = engine.L().rd_scatter_crops(engine._p(crops) if n else None, engine._p(pts) if n else None, engine._p(depth), engine._p(resp), n, patch[0],
                                     patch[1], H, W, ctypes.c_float(thr), engine.rd_of(crops), engine._stream(depth))
    assert rc == 0
    return depth.cpu().numpy()[0], resp.cpu().numpy()[0]


def _points(rng, n, patch, H, W):
    """n radar points with fractional coordinates inside the H x W image, in PADDED coordinates, z in 1.5 .. 100"""
    x = rng.uniform(0.0, W - 0.01, n) + patch[1] // 2
    y = rng.uniform(0.0, H - 0.01, n) + patch[0] // 2
    return np.stack([x, y, rng.uniform(1.5, 100.0, n)], axis=1).astype(np.float32)


def scatter_frames_exact_case(dev):
    """rd_scatter_crops_frames against rd_scatter_crops per frame, np.array_equal on both maps: patch (16,8); maps 20x28 and 37x45 (no multiple of
    the tile); F = 4 frames of N = (1, 0, 7, 2 * chunk + 3) points (an empty frame, and one that crosses the chunk capacity twice); fractional
    coordinates; fp32, bf16 and fp16 crops; a different threshold per frame, one above every response (all-zero maps) and one <= 0."""
    from riders_amd import engine
    chunk = int(engine.L().rd_scatter_frames_chunk())
    assert chunk > 0
    patch = (16, 8)
    counts = (1, 0, 7, 2 * chunk + 3)
    fs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    R = int(fs[-1])
    for H, W in ((20, 28), (37, 45)):
        rng = np.random.RandomState(H * 100 + W)
        crops32 = t(rng.uniform(0.0, 1.0, (R, patch[0], patch[1])).astype(np.float32))
        pts = t(_points(rng, R, patch, H, W), dev)
        for dt in (torch.float32, torch.bfloat16, torch.float16):
            crops = crops32.to(dt).to(dev)
            for thr in ((0.4, 0.5, 1.5, 0.55), (1.5, 0.3, -0.25, 0.0)):
                depth, resp = _frames(dev, crops, pts, fs, thr, patch, H, W)
                for f in range(4):
                    d1, r1 = _single(dev, crops[fs[f]:fs[f + 1]], pts[fs[f]:fs[f + 1]], thr[f], patch, H, W)
                    what = "%dx%d %s frame %d thr %g" % (H, W, dt, f, thr[f])
                    assert np.array_equal(resp[f], r1), what + ": response differs from rd_scatter_crops"
                    assert np.array_equal(depth[f], d1), what + ": depth differs from rd_scatter_crops"
                    if counts[f] == 0 or thr[f] > 1.0:
                        assert not depth[f].any() and not resp[f].any(), what + ": maps must be zero"
                    else:
                        assert resp[f].any(), what + ": nothing fused"


def scatter_frames_reference_case(dev):
    """Fixture g10 (the REFERENCE's forward_output results) used as two frames with thresholds 0.5 and thr2: support set exact, depth within 1e-5,
    response within 1e-6 (scatter_crops_case's bounds)."""
    g = load("g10_forward_output")
    patch, H, W = (64, 32), 64, 96
    n = g["crops"].shape[0]
    crops = t(np.concatenate([g["crops"], g["crops"]]), dev)
    pts = t(np.concatenate([g["pts"], g["pts"]]), dev)
    depth, resp = _frames(dev, crops, pts, (0, n, 2 * n), (0.5, float(g["thr2"][0])), patch, H, W)
    for f, (dk, rk) in enumerate((("depth", "resp"), ("depth2", "resp2"))):
        assert np.array_equal(depth[f] != 0, g[dk].reshape(H, W) != 0), "support set differs (frame %d)" % f
        close(depth[f], g[dk].reshape(H, W), 1e-5, "frames scatter depth"); close(resp[f], g[rk].reshape(H, W), 1e-6, "frames scatter response")


def _threshold_frames():
    """Five frames, patch (16,8) on 20x28: in-image maxima 0.62 (no retry), float32(0.45) (= (float)t_1: one retry and stop), 0.07 (nine retries), a
    frame whose largest values lie in the part of its patch that falls into the padded border (0.9 above, 0.8 left) with 0.33 on image pixel (0,0)
    (four retries; the border values would give none), and a frame of all-zero crops."""
    patch, H, W = (16, 8), 20, 28
    rng = np.random.RandomState(5)
    counts = (2, 3, 2, 1, 2)
    fs = np.concatenate([[0], np.cumsum(counts)])
    R = int(fs[-1])
    crops = rng.uniform(0.001, 0.06, (R, patch[0], patch[1])).astype(np.float32)
    pts = _points(rng, R, patch, H, W)
    pts[:, 0] = np.clip(pts[:, 0], 4 + patch[1] // 2, W - 4 + patch[1] // 2 - 0.5)      # the first three frames' patches lie inside the image
    pts[:, 1] = np.clip(pts[:, 1], 8 + patch[0] // 2, H - 8 + patch[0] // 2 - 0.5)
    crops[fs[0] + 1, 3, 2] = 0.62
    crops[fs[1] + 2, 15, 7] = np.float32(0.45)
    crops[fs[2], 0, 0] = 0.07
    c = fs[3]
    pts[c, 0], pts[c, 1] = 1.5 + patch[1] // 2, 2.25 + patch[0] // 2      # x0 = 1, y0 = 2: crop pixel (cr, cc) lands on image pixel (cr - 6, cc - 3)
    crops[c, 2, 5] = 0.9
    crops[c, 10, 1] = 0.8
    crops[c, 6, 3] = 0.33
    crops[fs[4]:] = 0.0
    return patch, H, W, fs, crops, pts, (0, 1, 9, 4, -1)


def thresholds_case(dev):
    """fuse_frames' thresholds, retries and maps against (a) fuse_with_retry per frame (float(thr[f]) == np.float32(its threshold), maps bit-exact) and
    (b) oracle.forward_output run in the reference's loop (same threshold, same number of retries, exact support set, depth within 1e-5), as
    inference_driver_case does; the all-zero frame gives retries -1 and zero maps, check_no_response() raises once and is quiet afterwards, and the
    other frames are what they are without it.  The same frames with bf16 crops against fuse_with_retry."""
    from riders_amd import rcnet_main
    patch, H, W, fs, crops_np, pts_np, want_retries = _threshold_frames()
    pad_y, pad_x = patch[0] // 2, patch[1] // 2
    rcnet_main._no_response_flags.clear()
    rcnet_main.check_no_response()      # nothing fused yet: quiet
    for dt in (torch.float32, torch.bfloat16):
        crops, pts = t(crops_np).to(dt).to(dev), t(pts_np, dev)
        depth, resp, thr, retries = rcnet_main.fuse_frames(crops, pts, _i32(fs, dev), patch[0], patch[1], H, W, 0.5, 0.05)
        assert thr.dtype == torch.float32 and retries.dtype == torch.int32 and thr.device == crops.device
        depth, resp, thr, retries = depth.cpu().numpy(), resp.cpu().numpy(), thr.cpu().numpy(), retries.cpu().numpy()
        print("thresholds (%s): thr %s retries %s" % (dt, thr.tolist(), retries.tolist()))
        for f in range(4):
            sl = slice(int(fs[f]), int(fs[f + 1]))
            d1, r1, thr_py = rcnet_main.fuse_with_retry(crops[sl], pts[sl], patch[0], patch[1], H, W, 0.5, 0.05)
            assert float(thr[f]) == np.float32(thr_py), (f, float(thr[f]), thr_py)
            assert np.array_equal(depth[f], d1.cpu().numpy()[0]) and np.array_equal(resp[f], r1.cpu().numpy()[0]), "frame %d: maps differ from fuse_with_retry" % f
            if dt != torch.float32:
                continue
            assert int(retries[f]) == want_retries[f], (f, retries.tolist())
            rthr, n = 0.5, 0
            while True:
                rd_, _ = O.forward_output(t(crops_np[sl])[:, None], t(pts_np[sl]), patch, (H + 2 * pad_y, W + 2 * pad_x), rthr)
                if float(rd_.sum()) != 0:
                    break
                rthr -= 0.05
                n += 1
            assert float(thr[f]) == np.float32(rthr) and int(retries[f]) == n, (f, float(thr[f]), rthr, int(retries[f]), n)
            assert np.array_equal(depth[f] != 0, rd_.numpy().reshape(H, W) != 0), "frame %d: support set differs from the reference loop's" % f
            close(depth[f], rd_.reshape(H, W), 1e-5, "frame %d depth after retry" % f)
        assert int(retries[4]) == -1 and float(thr[4]) == np.float32(0.5), (retries.tolist(), thr.tolist())
        assert not depth[4].any() and not resp[4].any(), "a frame without a response must give zero maps"
        with pytest.raises(RuntimeError):
            rcnet_main.check_no_response()
        rcnet_main.check_no_response()      # reported once
    # without the all-zero frame: the same four frames, and nothing to report
    crops, pts = t(crops_np[:fs[4]], dev), t(pts_np[:fs[4]], dev)
    d4, r4, t4, n4 = rcnet_main.fuse_frames(crops, pts, _i32(fs[:5], dev), patch[0], patch[1], H, W, 0.5, 0.05)
    assert np.array_equal(n4.cpu().numpy(), np.array(want_retries[:4], np.int32))
    rcnet_main.check_no_response()


def entry_refusals_case(dev):
    """What the two entry points refuse (negative return, rd_last_error_string set): step <= 0, a non-finite start, start / step above 4096, odd
    patch sizes, F < 0, null pointers with R > 0.  F = 0 is accepted and launches nothing."""
    from riders_amd import engine
    lib = engine.L()
    patch, H, W = (16, 8), 20, 28
    crops, pts = torch.zeros((2, 16, 8), device=dev), t(np.array([[10, 12, 3], [11, 13, 4]], np.float32), dev)
    fs = _i32((0, 2), dev)
    ws = torch.empty(int(lib.rd_frame_thresholds_ws_bytes(2)) // 4, dtype=torch.float32, device=dev)
    rmax, thr, ret, flag = (torch.zeros(1, dtype=d, device=dev) for d in (torch.float32, torch.float32, torch.int32, torch.int32))
    out, out2 = torch.zeros((1, H, W), device=dev), torch.zeros((1, H, W), device=dev)
    st = engine._stream(out)

    def thresholds(start=0.5, step=0.05, ph=patch[0], pw=patch[1], F=1, c=crops, w=ws):
        return lib.rd_frame_thresholds(engine._p(c), engine._p(pts), engine._p(fs), 2, F, ph, pw, H, W, start, step, engine._p(w), engine._p(rmax),
                                       engine._p(thr), engine._p(ret), engine._p(flag), 0, st)

    def scatter(ph=patch[0], pw=patch[1], F=1, c=crops):
        return lib.rd_scatter_crops_frames(engine._p(c), engine._p(pts), engine._p(fs), engine._p(thr), engine._p(out), engine._p(out2), 2, F, ph,
                                           pw, H, W, 0, st)
    for bad in (dict(step=0.0), dict(step=-0.05), dict(start=float("inf")), dict(start=float("nan")), dict(start=500.0, step=0.1), dict(ph=15),
                dict(pw=7), dict(F=-1), dict(c=None), dict(w=None)):
        assert thresholds(**bad) < 0 and lib.rd_last_error_string(), bad
    for bad in (dict(ph=15), dict(pw=7), dict(F=-1), dict(c=None)):
        assert scatter(**bad) < 0 and lib.rd_last_error_string(), bad
    assert thresholds(F=0) == 0 and scatter(F=0) == 0
    assert thresholds() == 0 and scatter() == 0
    assert int(ret.cpu()[0]) == -1 and int(flag.cpu()[0]) == 1      # all-zero crops: flagged in the caller's word


def run_frames_case(dev, tol=1e-3):
    """run_frames end to end: patch (64,32), F = 3 frames of 64x96, N = (3, 1, 5), fp32.  The four outputs equal fuse_with_retry applied per frame to
    slices of the same batched forward's crops, bit for bit; the crops agree with oracle.rcnet_forward(training=False) run frame by frame within the
    fp32 parity gate (1e-3 of max|ref|); quantize_depth takes the (F,H,W) depth."""
    from riders_amd import data_utils, engine, rcnet_main
    cfg = dict(rcnet_main.ZJU_CONFIG, patch_size=[64, 32])
    ph, pw = cfg['patch_size']
    pad_y, pad_x = ph // 2, pw // 2
    H, W, counts = 64, 96, (3, 1, 5)
    torch.manual_seed(0)
    model = rcnet_main.build_model(dev, cfg)
    model.eval()
    sd_e, sd_d = leaves(model.encoder.state_dict()), leaves(model.decoder.state_dict())
    rng = np.random.RandomState(11)
    images = t(rng.randint(0, 256, (3, 3, H, W)).astype(np.float32))
    raw = [t(np.stack([rng.uniform(0, W - 0.01, n), rng.uniform(0, H - 0.01, n), rng.uniform(1.5, 100.0, n)], axis=1).astype(np.float32)) for n in counts]
    rcnet_main._no_response_flags.clear()
    seen = {}
    keep = rcnet_main.fuse_frames

    def spy(crops, pts, frame_start, *a, **k):      # the crops / points / frame_start of the batched forward, as run_frames hands them over
        seen.update(crops=crops, pts=pts, fs=frame_start)
        return keep(crops, pts, frame_start, *a, **k)
    rcnet_main.fuse_frames = spy
    try:
        depth, resp, thr, retries = rcnet_main.run_frames(model, images.to(dev), [p.to(dev) for p in raw], 0.9, 0.05)
    finally:
        rcnet_main.fuse_frames = keep
    assert tuple(depth.shape) == (3, H, W) and tuple(resp.shape) == (3, H, W) and tuple(thr.shape) == (3,) and retries.dtype == torch.int32
    fs = seen["fs"].cpu().numpy()
    assert fs.tolist() == [0, 3, 4, 9]
    rcnet_main.check_no_response()      # a sigmoid response is positive: every frame has one
    crops, pts = seen["crops"], seen["pts"]
    assert tuple(crops.shape) == (9, 1, ph, pw) and crops.dtype == torch.float32
    for f in range(3):
        sl = slice(int(fs[f]), int(fs[f + 1]))
        d1, r1, thr_py = rcnet_main.fuse_with_retry(crops[sl].contiguous(), pts[sl], ph, pw, H, W, 0.9, 0.05)
        assert float(thr[f]) == np.float32(thr_py), (f, float(thr[f]), thr_py)
        assert np.array_equal(depth[f].cpu().numpy(), d1.cpu().numpy()[0]), "frame %d: depth differs from fuse_with_retry" % f
        assert np.array_equal(resp[f].cpu().numpy(), r1.cpu().numpy()[0]), "frame %d: response differs from fuse_with_retry" % f
        # the reference per frame: one image, its own points and boxes
        p = raw[f].clone(); p[:, 0] += pad_x; p[:, 1] += pad_y
        assert np.array_equal(pts[sl].cpu().numpy(), p.numpy()), "frame %d: shifted points" % f
        boxes = torch.stack([p[:, 0] - pad_x, p[:, 1] - pad_y, p[:, 0] + pad_x, p[:, 1] + pad_y], dim=-1)
        img = torch.nn.functional.pad(images[f:f + 1] / 255.0, (pad_x, pad_x, pad_y, pad_y), mode='replicate')
        with torch.no_grad():
            ref = torch.sigmoid(O.rcnet_forward(img, p, [boxes], sd_e, sd_d, cfg['patch_size'], False))
        close(crops[sl], ref, tol, "frame %d crops against the oracle" % f)
    print("run_frames: thr %s retries %s" % (thr.cpu().tolist(), retries.cpu().tolist()))
    q = data_utils.quantize_depth(depth)
    assert q.shape == (3, H, W) and q.dtype == np.uint16
    assert np.array_equal(q[1], data_utils.quantize_depth(depth[1]))
