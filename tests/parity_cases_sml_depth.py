"""Parity cases for the Scale-Map-Learner options 'midas-small-depth' and ground-truth dilation (see tests/parity_cases.py for how case functions
are used by the emulator and GPU twins): rd_sml_depth_head_fwd / _bwd, rd_maxpool_dilate, their refusals, MidasNet_small_depth against the
reference's own outputs (fixture g21, tests/golden/make_golden_sml_depth.py) and, on the GPU, the training / validation step.

Harness as tests/parity_cases_glue.py (imported, not copied): every kernel through the C ABI, every buffer a kernel writes a `Buf` with sentinels on
both sides, outputs prefilled with NaN, inputs checked unchanged.  The three kernels do no rounding arithmetic beyond one fp32 addition, so the
comparisons are bit for bit: the head against a numpy float32 restatement on the stored `out`, the dilation against torch.nn.MaxPool2d on the CPU.
"""
import contextlib
import io

import numpy as np
import torch

from oracle import sml as OS
from tests.golden.fill import fill_state_dict, rand_array
from tests.parity_cases import TOL, close, load, t
from tests.parity_cases_adam_groups import _Count
from tests.parity_cases_bn import DT, _nanbuf
from tests.parity_cases_glue import BF16, F16, F32, Buf, _bits, _call, _E, _exact, _P, _refused, _rs, _S

HEAD_N = (1, 255, 257, 4099, 12288)
HEAD_BOUNDS = ((5.0, 1.0 / 255.0), (10.0, -1.0), (-1.0, 0.25), (-1.0, -1.0))
HEAD_DTYPES = (F32, BF16, F16)
# (shape, k): one pixel; odd sizes; window larger than the image; a row longer than a workgroup (and W % 4 == 0: the vector form with 5 halo
# columns); several rows of vectors with k = 7; the copy
DILATE_CASES = (((1, 1, 1, 1), 3), ((2, 1, 5, 7), 3), ((1, 1, 2, 3), 5), ((1, 1, 3, 300), 5), ((2, 1, 12, 16), 7), ((2, 1, 12, 16), 1))
MIN_PRED, MAX_PRED = 0.2, 255.0      # the fixture's clamps (make_golden_sml_depth.py says why not 0.1)


# ---------------------------------------------------------------------------------------------------------------- 1. head
def _ulp_neighbours(v, dtype):
    """(one ulp below, v, one ulp above) of v rounded to `dtype`, as fp32 values"""
    x = torch.tensor([v], dtype=torch.float32).to(dtype)
    b = _bits(x)
    step = 1 if float(x) > 0 else -1      # sign-magnitude: a larger bit pattern is a larger magnitude
    return [float((b + s).view(dtype).float()) for s in (-step, 0, step)]


def _head_restated(out32, dpred, hi, lo):
    """numpy float32 restatement of the head on the stored values -> (pred, pass mask)"""
    hi, lo, one, zero = np.float32(hi), np.float32(lo), np.float32(1.0), np.float32(0.0)
    s = one + out32
    assert s.dtype == np.float32
    p = np.where(s > zero, s, zero)
    over = (p > hi) if hi > 0 else np.zeros(p.shape, bool)
    under = (p < lo) if lo > 0 else np.zeros(p.shape, bool)
    pred = p.copy()
    pred[over] = hi
    if lo > 0:
        pred[pred < lo] = lo
    return pred, (s > zero) & ~over & ~under, over, under


def _head_one(dev, dtype, n, hi, lo, off=0):
    hi, lo = float(np.float32(hi)), float(np.float32(lo))
    rs = _rs("depth_head", str(dtype), n, hi, lo, off)
    out = torch.from_numpy((2.5 * rs.standard_normal(n)).astype(np.float32)).to(dtype).float()
    planted = [-1.0, -1.5, -3.0] + _ulp_neighbours(-1.0, dtype)
    for b in (hi, lo):
        if b > 0:
            planted += _ulp_neighbours(float(np.float32(b) - np.float32(1.0)), dtype)
    pos = rs.permutation(n)[:len(planted)]
    for i, v in zip(pos, planted):
        out[int(i)] = v
    assert torch.equal(out.to(dtype).float(), out)
    dpred = torch.from_numpy(rs.standard_normal(n).astype(np.float32))
    pred, keep, over, under = _head_restated(out.numpy(), dpred.numpy(), hi, lo)
    what = "sml_depth_head %s n=%d hi=%g lo=%g off=%d" % (dtype, n, hi, lo, off)
    if n >= 255:
        assert keep.any() and (~keep).any() and (hi <= 0 or over.any()) and (lo <= 0 or under.any()), what + ": a branch is not exercised"
        # the planted neighbours fall on both sides of each comparison
        assert (pred == 0).any() or lo > 0
    O, DP = Buf(dev, n, dtype, out, off=off), Buf(dev, n, F32, dpred, off=off)
    PR, DO = Buf(dev, n, F32, torch.full((n,), float("nan")), off=off), Buf(dev, n, dtype, torch.full((n,), float("nan")), off=off)
    _call("rd_sml_depth_head_fwd", _P(O.v), _P(PR.v), n, hi, lo, DT[dtype], _S(O.v))
    _exact(what + " pred", PR.v, torch.from_numpy(pred))
    _call("rd_sml_depth_head_bwd", _P(O.v), _P(DP.v), _P(DO.v), n, hi, lo, DT[dtype], _S(O.v))
    want = torch.where(torch.from_numpy(keep), dpred, torch.zeros(n)).to(dtype)      # dpred rounded to out's type, or 0
    _exact(what + " dout", DO.v, want)
    PR.check(what); DO.check(what)
    O.check(what, unchanged=True); DP.check(what, unchanged=True)


def head_case(dev, dtypes=HEAD_DTYPES):
    """rd_sml_depth_head_fwd / _bwd: sizes x clamp bounds x the type of `out`; out = -1, below -1, hi - 1 and lo - 1 planted with their neighbours one
    ulp either side; and one misaligned call (every pointer 4 or 2 bytes off a 16-byte boundary: the all-scalar form)"""
    for dt in dtypes:
        for n in HEAD_N:
            for hi, lo in HEAD_BOUNDS:
                _head_one(dev, dt, n, hi, lo)
        _head_one(dev, dt, 257, 5.0, 0.25, off=1)


# ---------------------------------------------------------------------------------------------------------------- 2. dilation
def _dilate_one(dev, shape, k, off=0):
    N, _, H, W = shape
    rs = _rs("dilate", shape, k, off)
    x = torch.from_numpy((rs.uniform(0.5, 80.0, shape) * (rs.uniform(size=shape) < 0.5)).astype(np.float32))      # about half zeros, as ground truth
    ref = torch.nn.MaxPool2d(kernel_size=k, stride=1, padding=k // 2)(x)
    assert ref.shape == x.shape
    n = x.numel()
    what = "maxpool_dilate %s k=%d off=%d" % (shape, k, off)
    X, Y = Buf(dev, n, F32, x, off=off), Buf(dev, n, F32, torch.full((n,), float("nan")), off=off)
    _call("rd_maxpool_dilate", _P(X.v), _P(Y.v), N, H, W, k, _S(X.v))
    _exact(what, Y.v, ref.reshape(-1))
    Y.check(what); X.check(what, unchanged=True)


def dilate_case(dev):
    """rd_maxpool_dilate against torch.nn.MaxPool2d(k, 1, k // 2) on the CPU, bit for bit; the W % 4 == 0 shape once more from a misaligned
    pointer (the one-output-per-thread form on a width the vector form would take)"""
    for shape, k in DILATE_CASES:
        _dilate_one(dev, shape, k)
    _dilate_one(dev, (2, 1, 12, 16), 3, off=1)
    x = torch.zeros((2, 1, 6, 8)); x[0, 0, 2, 3] = 7.0; x[1, 0, 0, 0] = 2.0
    y = _E().dilate_max(x.to(dev), 3).cpu()
    assert torch.equal(y, torch.nn.MaxPool2d(3, 1, 1)(x)) and int((y > 0).sum()) == 9 + 4


# ---------------------------------------------------------------------------------------------------------------- 3. refusals
def refusals_case(dev):
    """null pointers, a bad dtype, a negative size, an even or out-of-range k and x aliasing y are refused on the host: nothing is written"""
    n = 64
    X, G = Buf(dev, n, F32, torch.ones(n)), Buf(dev, n, F32, torch.ones(n))
    Y, D = _nanbuf(dev, n, F32), _nanbuf(dev, n, F32)
    s = _S(X.v)
    _refused("rd_sml_depth_head_fwd", "sml_depth_head_fwd: null pointer", None, _P(Y.v), n, 5.0, 0.25, 0, s)
    _refused("rd_sml_depth_head_fwd", "sml_depth_head_fwd: null pointer", _P(X.v), None, n, 5.0, 0.25, 0, s)
    _refused("rd_sml_depth_head_fwd", "sml_depth_head_fwd: bad dtype", _P(X.v), _P(Y.v), n, 5.0, 0.25, 3, s)
    _refused("rd_sml_depth_head_fwd", "sml_depth_head_fwd: bad dtype", _P(X.v), _P(Y.v), n, 5.0, 0.25, -1, s)
    _refused("rd_sml_depth_head_fwd", "sml_depth_head_fwd: negative size", _P(X.v), _P(Y.v), -1, 5.0, 0.25, 0, s)
    _refused("rd_sml_depth_head_bwd", "sml_depth_head_bwd: null pointer", None, _P(G.v), _P(D.v), n, 5.0, 0.25, 0, s)
    _refused("rd_sml_depth_head_bwd", "sml_depth_head_bwd: null pointer", _P(X.v), None, _P(D.v), n, 5.0, 0.25, 0, s)
    _refused("rd_sml_depth_head_bwd", "sml_depth_head_bwd: null pointer", _P(X.v), _P(G.v), None, n, 5.0, 0.25, 0, s)
    _refused("rd_sml_depth_head_bwd", "sml_depth_head_bwd: bad dtype", _P(X.v), _P(G.v), _P(D.v), n, 5.0, 0.25, 7, s)
    _refused("rd_sml_depth_head_bwd", "sml_depth_head_bwd: negative size", _P(X.v), _P(G.v), _P(D.v), -5, 5.0, 0.25, 0, s)
    _refused("rd_maxpool_dilate", "maxpool_dilate: null pointer", None, _P(Y.v), 1, 8, 8, 3, s)
    _refused("rd_maxpool_dilate", "maxpool_dilate: null pointer", _P(X.v), None, 1, 8, 8, 3, s)
    for k in (0, 2, 4, 32, 33, -3):
        _refused("rd_maxpool_dilate", "maxpool_dilate: kernel size must be odd in 1..31", _P(X.v), _P(Y.v), 1, 8, 8, k, s)
    for geo in ((-1, 8, 8), (1, -8, 8), (1, 8, -8)):
        _refused("rd_maxpool_dilate", "maxpool_dilate: negative size", _P(X.v), _P(Y.v), *geo, 3, s)
    _refused("rd_maxpool_dilate", "maxpool_dilate: x must not alias y", _P(X.v), _P(X.v), 1, 8, 8, 3, s)
    for b in (Y, D):
        b.check("refused", unchanged=True)
    for b in (X, G):
        b.check("refusals", unchanged=True)
    # the Python layer: a model type this port does not have, an even dilation size
    from riders_amd import sml_main
    for bad in ("dpt-large", "midas"):
        try:
            sml_main.build_model(torch.device("cpu"), dict(sml_main.ZJU_SML_CONFIG, model_type=bad))
        except NotImplementedError:
            pass
        else:
            raise AssertionError("build_model accepted model_type %r" % bad)
    for k, want in ((-1, 0), (0, 0), (1, 0), (3, 3), (7, 7)):
        assert sml_main.gt_dilation_kernel_size(dict(ground_truth_dilation_kernel_size=k)) == want
    assert sml_main.gt_dilation_kernel_size({}) == 0
    try:
        sml_main.gt_dilation_kernel_size(dict(ground_truth_dilation_kernel_size=4))
    except ValueError:
        pass
    else:
        raise AssertionError("an even ground_truth_dilation_kernel_size was accepted")


# ---------------------------------------------------------------------------------------------------------------- 4. the network
def _names(a):
    return bytes(a).decode().split("\n") if len(a) else []


_ORACLE = {}      # in_channels -> (g64, g32): the float64 / fp32 oracle gradients, computed once and shared (never modified)


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _oracle_grads(in_channels, B, H, W):
    if in_channels in _ORACLE:
        return _ORACLE[in_channels]
    from riders_amd.midas.midas_net_custom import MidasNet_small_depth

    def run(dt):
        # SMLOracle computes d * relu(1 + out) with the same clamps: with d = ones it is MidasNet_small_depth exactly
        o = OS.SMLOracle(in_channels=in_channels, min_pred=MIN_PRED, max_pred=MAX_PRED).to(dt)
        o.load_state_dict({k: (v.to(dt) if v.is_floating_point() else v) for k, v in fill_state_dict(_quiet(
            MidasNet_small_depth, device='cpu', min_pred=MIN_PRED, max_pred=MAX_PRED, in_channels=in_channels), "g9.sml").items()})
        o.train()
        xo = t(rand_array("g9.x", (B, in_channels, H, W), 1.0)).to(dt).requires_grad_()
        po = o(xo, torch.ones((B, 1, H, W), dtype=dt))
        (po * t(rand_array("g9.w", po.shape, 1.0)).to(dt)).sum().backward()
        gr = {k: p.grad for k, p in o.named_parameters()}
        gr["x"] = xo.grad
        return gr
    # one thread, whatever the host has: see parity_cases_sml.sml_net_case
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        _ORACLE[in_channels] = (run(torch.float64), run(torch.float32))
    finally:
        torch.set_num_threads(threads)
    return _ORACLE[in_channels]


def sml_depth_net_case(dev, in_channels=3, tol=TOL, forward_only=False):
    """Full MidasNet_small_depth forward / backward against the REFERENCE's own outputs (fixture g21), as parity_cases_sml.sml_net_case does for
    g9: same tolerances, same conditioning-aware gradient bound.  in_channels = 3 is what train_zju.py passes, 2 the class default (the stem then
    runs through the channel-padding route of engine.conv_block).
    forward_only (the emulator twin): the key list, the train-mode prediction, the two running statistics and the checkpoint exchange; the
    backward and the eval-mode forward are left to the GPU twin.  Under the emulator one forward at this size takes minutes and the backward
    several times that (measured: 226 s for the forward alone), on top of a CPU suite that already runs for an hour."""
    from riders_amd.midas.midas_net_custom import MidasNet_small_depth
    g = load("g21_sml_depth")
    pre = "" if in_channels == 3 else "c%d." % in_channels
    m = _quiet(MidasNet_small_depth, device=dev, min_pred=MIN_PRED, max_pred=MAX_PRED, in_channels=in_channels)
    assert tuple(m.first[0].weight.shape) == (3, in_channels, 3, 3)
    fill_state_dict(m, "g9.sml")
    assert list(m.state_dict().keys()) == _names(g["state_keys"]) and len(m.state_dict()) == 489
    B, H, W = 2, 64, 96
    x = t(rand_array("g9.x", (B, in_channels, H, W), 1.0), dev).requires_grad_()
    m.train()
    pred = m.forward(x, None)
    assert tuple(pred.shape) == (B, 1, H, W) and pred.dtype == torch.float32
    ref = t(g[pre + "pred"])
    hi, lo = np.float32(1.0 / MIN_PRED), np.float32(1.0 / MAX_PRED)
    assert int((ref == hi).sum()) >= 8 and int((ref == lo).sum()) >= 8, "the fixture does not reach both clamps"
    close(pred, ref, tol, "g21 pred (in_channels=%d)" % in_channels)
    if forward_only:
        return _net_state_checks(dev, m, g, tol)
    (pred * t(rand_array("g9.w", pred.shape, 1.0), dev)).sum().backward()
    g64, g32 = _oracle_grads(in_channels, B, H, W)

    def cond(k):
        return float((g32[k].double() - g64[k]).abs().max() / max(float(g64[k].abs().max()), 1e-30))
    close(x.grad, g64["x"], max(4 * tol, 3 * cond("x")), "g21 dx (in_channels=%d)" % in_channels)
    close(g32["x"], g[pre + "dx"], max(4 * tol, 3 * cond("x")), "oracle vs reference dx (in_channels=%d)" % in_channels)
    none = set(_names(g["none_keys"]))
    num = den = num32 = 0.0
    for k, p in m.named_parameters():
        if k in none:
            assert p.grad is None, k
            continue
        ref = g64[k]
        num += float((p.grad.detach().cpu().double() - ref).pow(2).sum())
        num32 += float((g32[k].double() - ref).pow(2).sum())
        den += float(ref.pow(2).sum())
        if float(ref.abs().max()) < 1e-12:
            continue
        close(p.grad, ref, max(4 * tol, 50 * cond(k)), "g21 grad " + k)
    gerr, gcond = (num / den) ** 0.5, (num32 / den) ** 0.5
    print("g21 in_channels=%d: global gradient error %.3e (fp32 oracle vs fp64: %.3e)" % (in_channels, gerr, gcond))
    assert gerr <= max(2e-3, 3 * gcond), "global gradient error %.3e vs fp32-oracle %.3e" % (gerr, gcond)
    if in_channels != 3:
        return
    assert _names(g["grad_keys"]) == [k for k, p in m.named_parameters() if k not in none]
    m.eval()
    with torch.no_grad():
        # `d` is ignored, whatever it holds: the train-mode forward above had None, this one a map of threes (a head that multiplied by it would be 3 x off)
        close(m.forward(x.detach(), torch.full((B, 1, H, W), 3.0, device=dev)), g["pred_eval"], tol, "g21 eval pred")
    m.train()
    _net_state_checks(dev, m, g, tol)


def _net_state_checks(dev, m, g, tol):
    """after ONE train-mode forward of the in_channels = 3 model: the two running statistics g9 stores; then a checkpoint of the scale-map model loads"""
    from riders_amd.midas.midas_net_custom import MidasNet_small_videpth
    sd = m.state_dict()
    close(sd["first.1.running_mean"], g["rm_first"], tol, "first BN running mean")
    close(sd["pretrained.layer1.1.running_var"], g["rv_stem"], tol, "stem BN running var")
    assert int(sd["first.1.num_batches_tracked"]) == 1
    # a checkpoint of the scale-map model loads (same 489 keys), and save / load round-trip
    v = _quiet(MidasNet_small_videpth, device='cpu', min_pred=0.1, max_pred=255.0, in_channels=3)
    fill_state_dict(v, "g21.other")
    m.load_state_dict(v.state_dict())
    assert all(torch.equal(a.cpu(), b) for a, b in zip(m.state_dict().values(), v.state_dict().values()))


# ---------------------------------------------------------------------------------------------------------------- 5. step level (GPU)
def _cfg(**kw):
    from riders_amd import sml_main
    return dict(sml_main.ZJU_SML_CONFIG, **kw)


def _setup(dev, cfg):
    from riders_amd import sml_main
    from riders_amd.optim import FlatAdam
    torch.manual_seed(0)
    m = _quiet(sml_main.build_model, dev, cfg)
    fill_state_dict(m, "g9.sml")
    m.train()
    return m, FlatAdam(m.parameters(), lr=cfg['learning_rate'])


def train_step_case(dev, steps=3, tol=TOL):
    """sml_main.train_step with model_type 'midas-small-depth' and ground_truth_dilation_kernel_size 3, three steps at B = 2, 64 x 96; each step's
    loss against the same step built from torch on the host: MaxPool2d on the resized ground truth, the project's outlier removal, then the
    project's compute_loss on the dilated map with the prediction the model gives in that step (tolerance: the existing SML step test's 1e-3)."""
    from riders_amd import engine, sml_main
    from riders_amd.loss import compute_loss
    from riders_amd.midas.midas_net_custom import MidasNet_small_depth
    cfg = _cfg(model_type='midas-small-depth', ground_truth_dilation_kernel_size=3)
    batch = sml_main.synthetic_batch(2, 64, 96, seed=21, device=dev)
    m, opt = _setup(dev, cfg)
    assert type(m) is MidasNet_small_depth
    orr = sml_main.make_outlier_removal(cfg)
    image, mono, sparse_depth, gt, sparse_gt, rcnet = batch
    hw = sml_main.net_size(64, 96)
    pool = torch.nn.MaxPool2d(kernel_size=3, stride=1, padding=1)
    gt_r, sgt_r = sml_main.nearest_resize(gt, *hw), sml_main.nearest_resize(sparse_gt, *hw)
    gt_dil = pool(gt_r.cpu()).to(dev)
    assert int((gt_dil != gt_r).sum()) > 0, "the dilation changes nothing on this batch"
    gi = orr.remove_outliers(gt_dil)
    losses = []
    for step in range(steps):
        with torch.no_grad():
            x, d, _ = sml_main.prepare_inputs(image, mono, sparse_depth, rcnet, hw, cfg)
            m_bn = {k: v.clone() for k, v in m.state_dict().items()}
            pred = m.forward(x, d)           # train mode: the step's own prediction (the BatchNorm buffers are put back below)
            m.load_state_dict(m_bn)
            ref, _ = compute_loss(image=1.0 / d, output_depth=1.0 / pred, gt_interp=gi, gt_sparse=sgt_r, loss_func=cfg['loss_func'],
                                  w_smoothness=cfg['w_smoothness'], sobel_filter_size=cfg['sobel_filter_size'], validity_map_loss_smoothness=None,
                                  w_lidar_loss=cfg['w_lidar_loss'], w_edge=cfg['w_edge'], invalid_map_gt=None, w_unsupervised=0.0)
            plain, _ = compute_loss(image=1.0 / d, output_depth=1.0 / pred, gt_interp=orr.remove_outliers(gt_r), gt_sparse=sgt_r,
                                    loss_func=cfg['loss_func'], w_smoothness=cfg['w_smoothness'], sobel_filter_size=cfg['sobel_filter_size'],
                                    validity_map_loss_smoothness=None, w_lidar_loss=cfg['w_lidar_loss'], w_edge=cfg['w_edge'], invalid_map_gt=None, w_unsupervised=0.0)
        loss = float(sml_main.train_step(m, opt, batch, cfg, outlier=orr).detach())
        print("step %d: loss %.8g, host restatement %.8g, without dilation %.8g" % (step, loss, float(ref), float(plain)))
        assert np.isfinite(loss) and abs(loss - float(ref)) <= tol * abs(float(ref)), (step, loss, float(ref))
        assert abs(float(plain) - float(ref)) > 3 * tol * abs(float(ref)), "the comparison cannot tell the dilated map from the plain one"
        losses.append(loss)
    assert len(set(losses)) == steps, losses      # the parameters move
    engine.set_param_grad_allocator(None)


def graphed_step_case(dev, steps=3):
    """GraphedTrainStep against the eager train_step for the new model with dilation: losses and parameters bit-identical over three replays on the
    captured batch and three more after load_batch of another batch."""
    from riders_amd import engine, sml_main
    cfg = _cfg(model_type='midas-small-depth', ground_truth_dilation_kernel_size=3)
    b1 = sml_main.synthetic_batch(2, 64, 96, seed=3, device=dev)
    b2 = sml_main.synthetic_batch(2, 64, 96, seed=4, device=dev)
    m, opt = _setup(dev, cfg)
    orr = sml_main.make_outlier_removal(cfg)
    eager = [float(sml_main.train_step(m, opt, b, cfg, outlier=orr).detach()) for b in (b1,) * steps + (b2,) * steps]
    assert all(np.isfinite(eager)), eager
    p_eager = [p.detach().clone() for p in m.parameters()]
    bufs_eager = {k: v.detach().clone() for k, v in m.state_dict().items()}
    engine.set_param_grad_allocator(None)
    m2, opt2 = _setup(dev, cfg)
    step = sml_main.GraphedTrainStep(m2, opt2, tuple(b.clone() for b in b1), cfg, outlier=sml_main.make_outlier_removal(cfg), warmup=1)
    graphed = [float(step().detach()) for _ in range(steps)]
    step.load_batch(b2)
    graphed += [float(step().detach()) for _ in range(steps)]
    print("eager", eager, "graphed", graphed)
    assert graphed == eager, (graphed, eager)
    for a, b in zip(p_eager, m2.parameters()):
        assert torch.equal(a, b.detach())
    for k, v in m2.state_dict().items():
        if v.is_floating_point():
            assert torch.equal(v, bufs_eager[k]), k
    del step
    engine.set_param_grad_allocator(None)


def validate_case(dev):
    """sml_main.validate_batch takes the new model: finite metrics, a depth map of the frame size, predictions inside the clamps"""
    from riders_amd import sml_main
    cfg = _cfg(model_type='midas-small-depth')
    m, _ = _setup(dev, cfg)
    m.eval()
    batch = sml_main.synthetic_batch(2, 60, 80, seed=21, device=dev)
    got = sml_main.validate_batch(m, batch, cfg)
    assert tuple(got["depth"].shape) == (2, 1, 60, 80) and bool(torch.isfinite(got["depth"]).all())
    for k in ("count", "mae", "rmse", "imae", "irmse", "abs_rel", "sq_rel", "delta1"):
        assert got[k].shape == (2,) and np.isfinite(got[k]).all(), (k, got[k])
    assert (got["count"] > 0).all()


class _AllCounts(object):
    """calls of every entry point of the C ABI, by name (tests.parity_cases_adam_groups._Count per name)"""

    def __init__(self):
        from riders_amd import _lib
        self.cs = [_Count(n) for n in sorted(_lib.parse_header())]

    def __enter__(self):
        for c in self.cs:
            c.__enter__()
        return self

    def __exit__(self, *exc):
        for c in reversed(self.cs):
            c.__exit__(None, None, None)

    def dict(self):
        return dict((c.name, c.n) for c in self.cs if c.n)


def default_launches_case(dev):
    """With both new keys absent forward_loss calls the library exactly as it did before they existed: the same entry points the same number of
    times as with the defaults spelled out, none of the three new ones; the dilation adds one rd_maxpool_dilate and nothing else; the new model
    trades rd_sml_head_fwd for rd_sml_depth_head_fwd and nothing else."""
    from riders_amd import engine, sml_main
    batch = sml_main.synthetic_batch(2, 64, 96, seed=21, device=dev)
    absent = dict(sml_main.ZJU_SML_CONFIG)
    assert 'model_type' not in absent and 'ground_truth_dilation_kernel_size' not in absent

    def count(cfg):
        m, _ = _setup(dev, cfg)
        orr = sml_main.make_outlier_removal(cfg)
        with torch.no_grad():
            sml_main.forward_loss(m, batch, cfg, orr)      # warm: packed operands, lazily allocated buffers
            with _AllCounts() as c:
                loss = sml_main.forward_loss(m, batch, cfg, orr)
        assert bool(torch.isfinite(loss))
        return c.dict()
    base = count(absent)
    new = ("rd_sml_depth_head_fwd", "rd_sml_depth_head_bwd", "rd_maxpool_dilate")
    assert not any(n in base for n in new), base
    assert base.get("rd_sml_head_fwd") == 1 and base.get("rd_outlier_removal") == 1, base
    print("forward_loss, default configuration: %d calls of %d entry points" % (sum(base.values()), len(base)))
    assert count(_cfg(model_type='midas-small', ground_truth_dilation_kernel_size=-1)) == base
    assert count(_cfg(ground_truth_dilation_kernel_size=1)) == base
    assert count(_cfg(ground_truth_dilation_kernel_size=3)) == dict(base, rd_maxpool_dilate=1)
    want = dict(base, rd_sml_depth_head_fwd=1)
    del want["rd_sml_head_fwd"]
    assert count(_cfg(model_type='midas-small-depth')) == want
    engine.set_param_grad_allocator(None)
