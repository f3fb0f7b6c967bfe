"""RC-Net inference over frame batches on the device: the cases of tests/parity_cases_infer.py against libriders_hip.so, and the proof that
fuse_frames reads nothing back -- it is captured into a hipGraph (a synchronising call fails a capture) and replayed on new data."""
import numpy as np
import pytest
import torch

from tests import parity_cases_infer as I

pytestmark = pytest.mark.gpu


def test_scatter_frames_equals_scatter_crops(gpu):
    I.scatter_frames_exact_case(gpu)


def test_scatter_frames_reference_fixture(gpu):
    I.scatter_frames_reference_case(gpu)


def test_frame_thresholds(gpu):
    I.thresholds_case(gpu)


def test_entry_refusals(gpu):
    I.entry_refusals_case(gpu)


def test_run_frames(gpu):
    I.run_frames_case(gpu)


def test_fuse_frames_is_capturable(gpu):
    """fuse_frames inside torch.cuda.graph: a linear chain of three launches, no parallel branches.  New crops and points are copied into the captured
    inputs, the graph is replayed, and the four outputs equal an eager fuse_frames on the same data."""
    from riders_amd import engine, rcnet_main
    patch, H, W, fs, crops_np, pts_np, want = I._threshold_frames()
    fs4 = I._i32(fs[:5], gpu)      # the four frames that have a response
    R = int(fs[4])
    rcnet_main._no_response_flags.clear()
    static_crops, static_pts = I.t(crops_np[:R], gpu), I.t(pts_np[:R], gpu)
    args = (fs4, patch[0], patch[1], H, W, 0.5, 0.05)
    eager1 = [o.clone() for o in rcnet_main.fuse_frames(static_crops, static_pts, *args)]      # also allocates the sticky flag outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = rcnet_main.fuse_frames(static_crops, static_pts, *args)
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(outs, eager1):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
    assert outs[3].cpu().tolist() == list(want[:4])
    # new data: other responses and other points, same shapes
    rng = np.random.RandomState(23)
    crops2 = I.t(rng.uniform(0.0, 0.3, crops_np[:R].shape).astype(np.float32), gpu)
    pts2 = I.t(I._points(rng, R, patch, H, W), gpu)
    eager2 = [o.clone() for o in rcnet_main.fuse_frames(crops2, pts2, *args)]
    engine.dev_copy(static_crops, crops2)      # a kernel in front of the replay, as GraphedStep.load_batch copies
    engine.dev_copy(static_pts, pts2)
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(outs, eager2):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
    assert not np.array_equal(eager1[0].cpu().numpy(), eager2[0].cpu().numpy())
    assert (eager2[3].cpu().numpy() > 0).all()      # responses below 0.3: every frame retried
    rcnet_main.check_no_response()
