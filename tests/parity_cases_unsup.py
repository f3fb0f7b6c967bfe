"""Unsupervised SML loss term (utils/loss.py:65-70, 83-88, 101-106) and the masked on-device median it needs: parity cases shared by the emulator
and GPU suites (see tests/parity_cases.py for how these are used).  The yardsticks are torch.median on the CPU, the REFERENCE's own loss values /
gradients (fixtures g18_loss_unsup_*, tests/golden/make_golden_unsup.py) and a torch restatement of the term validated against those fixtures."""
import ctypes

import numpy as np
import torch
import torch.nn.functional as F

from oracle import sml as OS
from tests.golden.fill import rand_array
from tests.parity_cases import close, load, t

KEYS = ('loss', 'loss_supervised', 'loss_lidar', 'loss_smoothness', 'loss_edge', 'loss_unsupervised')
# fixture tag -> (loss_func, w_smoothness, w_edge); all with w_unsupervised 0.7, w_lidar_loss 1.5, Sobel size 5
FIXTURES = {"l1": ("l1", 0.2, 0.0), "l2": ("l2", 0.2, 0.0), "smoothl1": ("smoothl1", 0.2, 0.0), "edge_only": ("l1", 0.0, 0.35),
            "smoothl1_edge": ("smoothl1", 0.2, 0.5)}
W_UNSUP, W_LIDAR, FS = 0.7, 1.5, 5
# phi' is a sign for 'l1' and branches at |d| = 1 for 'smoothl1': an element within fp32 rounding (~1e-6 on u and t) of a branch point could flip
# and move its gradient entry by ~1 % of the map's maximum while staying inside the tolerance of a max-norm.  Inputs keep 100 x that distance.
MARGIN = 1e-4


def g7_inputs():
    """image, gt_interp, gt_sparse of fixture g7 (tests/parity_cases_sml.py loss_case) and the raw prediction."""
    N, H, W = 2, 24, 32
    image = rand_array("g7.img", (N, 1, H, W), 20.0, lo=0.05)
    gi = rand_array("g7.gi", (N, 1, H, W), 30.0, lo=0.0); gi[rand_array("g7.gim", gi.shape, 1.0, lo=0.0) < 0.3] = 0
    gs = rand_array("g7.gs", (N, 1, H, W), 30.0, lo=0.0); gs[rand_array("g7.gsm", gs.shape, 1.0, lo=0.0) < 0.9] = 0
    pred = rand_array("g7.pred", (N, 1, H, W), 20.0, lo=0.05)
    return image, gi, gs, pred


def unsup_d(pred, image, mask):
    """d = o / median(o) - I / median(I) over the mask, in fp32 torch arithmetic as the reference computes it (numpy in, numpy out)."""
    o, im = t(pred)[t(mask)], t(image)[t(mask)]
    return (o / torch.median(o) - im / torch.median(im)).numpy()


def margins(pred, image, mask):
    d = np.abs(unsup_d(pred, image, mask).astype(np.float64))
    return float(d.min()), float(np.abs(d - 1.0).min())


def nudge(pred, image, mask):
    """Deterministically move the prediction pixels whose d lies within MARGIN of a branch point of phi' (0, or +-1) until none does."""
    pred = pred.copy()
    idx = np.flatnonzero(mask.reshape(-1))
    for _ in range(200):
        d = np.abs(unsup_d(pred, image, mask).astype(np.float64))
        bad = (d < MARGIN) | (np.abs(d - 1.0) < MARGIN)
        if not bad.any():
            return pred
        flat = pred.reshape(-1)
        flat[idx[bad]] = flat[idx[bad]] * np.float32(1.001) + np.float32(1e-3)
    raise AssertionError("nudge did not converge")


def unsup_restated(pred, image, mask, loss_func):
    """The reference's unsupervised term restated in torch (utils/loss.py:65-70 and its 'l2' / 'smoothl1' twins)."""
    term = {'l1': F.l1_loss, 'l2': F.mse_loss, 'smoothl1': F.smooth_l1_loss}[loss_func]
    o, im = pred[mask], image[mask]
    return term(o / torch.median(o), im / torch.median(im))


def restated_loss(image, pred, gi, gs, mask, loss_func, w_smooth, w_edge, w_unsup, fs=FS, w_lidar=W_LIDAR):
    """total and loss_info: the oracle's compute_loss (which has no unsupervised term) plus the restated term"""
    loss, info = OS.compute_loss(image, pred, gi, gs, w_smooth, fs, torch.ones_like(image), w_lidar, w_edge, loss_func)
    lu = unsup_restated(pred, image, mask, loss_func)
    info = dict(info, loss_unsupervised=lu)
    info['loss'] = loss + w_unsup * lu
    return info['loss'], info


def _hip_loss(dev, image, pred, gi, gs, mask, loss_func, w_smooth, w_edge, w_unsup, fs=FS, w_lidar=W_LIDAR):
    from riders_amd.loss import compute_loss
    p = t(pred, dev).requires_grad_()
    m = None if mask is None else (mask.to(dev) if torch.is_tensor(mask) else t(mask, dev))
    loss, info = compute_loss(image=t(image, dev), output_depth=p, gt_interp=t(gi, dev), gt_sparse=t(gs, dev), loss_func=loss_func,
                              w_smoothness=w_smooth, sobel_filter_size=fs, validity_map_loss_smoothness=torch.ones_like(t(image, dev)),
                              w_lidar_loss=w_lidar, w_edge=w_edge, invalid_map_gt=m, w_unsupervised=w_unsup)
    loss.backward()
    return loss.detach().cpu(), {k: float(info[k].detach() if torch.is_tensor(info[k]) else info[k]) for k in KEYS}, p.grad.detach().cpu()


def _check_info(got, ref, tol, what):
    for k in KEYS:
        a, b = float(got[k]), float(ref[k])
        print("%s %-18s hip %.8g ref %.8g" % (what, k, a, b))
        assert abs(a - b) <= tol * max(abs(b), 1e-3), (what, k, a, b)


# ---------------------------------------------------------------------------------------------------------------------------- 1. selection
def masked_median(dev, x0, x1, mask_bool=None, mask_le0=None):
    """rd_masked_median through the C ABI -> (m0, m1, n, nan flag) as python floats"""
    from riders_amd import engine
    lib = engine.L()
    a, b = t(np.ascontiguousarray(x0, np.float32), dev), t(np.ascontiguousarray(x1, np.float32), dev)
    n = a.numel()
    mu8 = None if mask_bool is None else t(np.ascontiguousarray(mask_bool, np.bool_), dev).view(torch.uint8)
    mf = None if mask_le0 is None else t(np.ascontiguousarray(mask_le0, np.float32), dev)
    scratch = torch.empty(lib.rd_masked_median_bytes(n), dtype=torch.uint8, device=dev)
    out = torch.empty(4, dtype=torch.float32, device=dev)
    engine._chk(lib.rd_masked_median(engine._p(a), engine._p(b), engine._p(mu8), engine._p(mf), n, engine._p(scratch), engine._p(out), engine._stream(a)),
                "rd_masked_median")
    return out.cpu().numpy()


def _same(got, want):
    """== on the values; either sign of zero passes for a zero (the key order separates -0 from +0, torch does not); NaN matches NaN"""
    got, want = np.float32(got), np.float32(want)
    if np.isnan(want):
        return bool(np.isnan(got))
    return bool(got == want)


def selection_case(dev):
    rs = np.random.RandomState(18)
    cases = []
    for n in (1, 2, 3, 4, 5, 64, 257):      # tiny, even and odd n: the mask selects the first n of 300 elements
        x = rs.randn(300).astype(np.float32) * 7
        m = np.zeros(300, bool); m[rs.permutation(300)[:n]] = True
        cases.append(("n=%d" % n, x, rs.randn(300).astype(np.float32), m))
    shape = (4, 1, 97, 161)                 # 62468 elements: many blocks, not a multiple of the vector width or of the block size
    for dens in (0.01, 0.6, 1.0):
        x = (rs.rand(*shape).astype(np.float32) * 60 + 2)
        cases.append(("dens=%.2f" % dens, x, rs.randn(*shape).astype(np.float32) * 3, rs.rand(*shape) < dens))      # second array: negative values
    x = np.round(rs.randn(*shape) * 4) .astype(np.float32) * np.float32(0.25)
    cases.append(("duplicates", x, np.round(rs.rand(*shape) * 8).astype(np.float32) * np.float32(0.25), rs.rand(*shape) < 0.6))
    cases.append(("all equal", np.full(shape, 3.5, np.float32), np.full(shape, -0.0, np.float32), rs.rand(*shape) < 0.6))
    x = rs.randn(*shape).astype(np.float32); x[rs.rand(*shape) < 0.3] = np.inf; x[rs.rand(*shape) < 0.3] = -np.inf
    y = rs.randn(*shape).astype(np.float32); y[rs.rand(*shape) < 0.6] = np.inf
    cases.append(("inf", x, y, rs.rand(*shape) < 0.6))
    x = (rs.randint(-2000, 2000, shape).astype(np.float32) * np.float32(1e-42)).astype(np.float32)      # denormals of both signs (and zeros)
    y = (rs.randint(1, 5000, shape).astype(np.float32) * np.float32(1e-43)).astype(np.float32)
    cases.append(("denormals", x, y, rs.rand(*shape) < 0.6))
    x = rs.randn(*shape).astype(np.float32) - 50
    cases.append(("negative", x, -np.abs(rs.randn(*shape).astype(np.float32)) * 1e-3, rs.rand(*shape) < 0.6))
    for name, x, y, m in cases:
        assert x.dtype == np.float32 and y.dtype == np.float32
        want = (float(torch.median(t(x)[t(m)])), float(torch.median(t(y)[t(m)])))
        gt = np.where(m, 0.0, 1.0).astype(np.float32)      # a ground-truth map that is <= 0 exactly on the mask (zeros; negatives below)
        gt[m & (rs.rand(*m.shape) < 0.5)] = -2.0
        for form, kw in (("bool", dict(mask_bool=m)), ("le0", dict(mask_le0=gt))):
            got = masked_median(dev, x, y, **kw)
            assert _same(got[0], want[0]) and _same(got[1], want[1]), (name, form, got, want)
            assert got[2] == m.sum() and got[3] == 0.0, (name, form, got)
        # unaligned views take the scalar path: same answer
        if x.size > 300:
            xs, ys, ms = x.reshape(-1)[1:], y.reshape(-1)[1:], m.reshape(-1)[1:]
            buf = np.zeros(xs.size + 1, np.float32); buf2 = np.zeros(xs.size + 1, np.float32)
            buf[1:] = xs; buf2[1:] = ys
            want_s = (float(torch.median(t(xs.copy())[t(ms.copy())])), float(torch.median(t(ys.copy())[t(ms.copy())])))
            got = _median_offset(dev, buf, buf2, ms)
            assert _same(got[0], want_s[0]) and _same(got[1], want_s[1]), (name, "offset", got, want_s)
    # a NaN among the selected values -> NaN (never a finite number), in the array that holds it; an unselected NaN changes nothing
    x = rs.randn(*shape).astype(np.float32); y = rs.randn(*shape).astype(np.float32)
    m = rs.rand(*shape) < 0.6
    sel, uns = np.argwhere(m)[7], np.argwhere(~m)[3]
    x[tuple(sel)] = np.nan; y[tuple(uns)] = np.nan
    got = masked_median(dev, x, y, mask_bool=m)
    assert np.isnan(got[0]) and got[3] == 1.0, got
    assert _same(got[1], float(torch.median(t(y)[t(m)]))), got
    assert bool(torch.isnan(torch.median(t(x)[t(m)])))
    # an empty mask -> NaN, n = 0
    got = masked_median(dev, x, y, mask_bool=np.zeros(shape, bool))
    assert np.isnan(got[0]) and np.isnan(got[1]) and got[2] == 0.0, got


def _median_offset(dev, buf, buf2, ms):
    """the arrays start 4 bytes into an allocation (and the bool mask 1 byte into its own): the kernels' scalar path"""
    from riders_amd import engine
    lib = engine.L()
    A, B = t(buf, dev), t(buf2, dev)
    mb = np.zeros(ms.size + 1, bool); mb[1:] = ms
    Mt = t(mb, dev).view(torch.uint8)
    n = buf.size - 1
    scratch = torch.empty(lib.rd_masked_median_bytes(n), dtype=torch.uint8, device=dev)
    out = torch.empty(4, dtype=torch.float32, device=dev)
    vp = lambda x, off: ctypes.c_void_p(x.data_ptr() + off)  # noqa: E731
    engine._chk(lib.rd_masked_median(vp(A, 4), vp(B, 4), vp(Mt, 1), None, n, engine._p(scratch), engine._p(out), engine._stream(A)), "rd_masked_median")
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------- 2. the reference's fixtures
def fixture_case(dev, tol=1e-4):
    """HIP loss with w_unsupervised = 0.7 vs the REFERENCE's own values and gradient (fixtures g18_loss_unsup_*), g7's inputs with
    invalid_map_gt = gt_interp <= 0; then the torch restatement against the same fixtures (it is the yardstick of larger_maps_case)."""
    image, gi, gs, _ = g7_inputs()
    mask = gi <= 0
    assert int(mask.sum()) == 468
    for tag, (lf, ws, we) in FIXTURES.items():
        g = load("g18_loss_unsup_" + tag)
        pred = g["pred"]
        m0, m1 = margins(pred, image, mask)
        print("fixture %s: min|d| %.3e, min||d|-1| %.3e" % (tag, m0, m1))
        assert m0 >= MARGIN and m1 >= MARGIN, (tag, m0, m1)
        ref = dict(zip(KEYS, g["loss"]))
        for form, mk in (("bool", mask), ("le0", gi)):      # the public bool mask, and the ground-truth map under the rule <= 0
            _, info, dpred = _hip_loss(dev, image, pred, gi, gs, mk, lf, ws, we, W_UNSUP)
            _check_info(info, ref, tol, "fixture %s (%s)" % (tag, form))
            close(dpred, g["dpred"], 10 * tol, "unsup dpred %s (%s)" % (tag, form))
        pr = t(pred).requires_grad_()
        lo, io = restated_loss(t(image), pr, t(gi), t(gs), t(mask), lf, ws, we, W_UNSUP)
        lo.backward()
        _check_info({k: float(io[k].detach()) for k in KEYS}, ref, tol, "restatement %s" % tag)
        close(pr.grad, g["dpred"], 10 * tol, "restatement dpred " + tag)
    # the median element carries the largest gradient of the map (issue: 2.3e-2 against ~1.5e-4 elsewhere): the comparison above sees that path
    g = load("g18_loss_unsup_l1")
    o = g["pred"][mask]
    at = np.abs(g["dpred"][mask][o == np.float32(torch.median(t(o)))]).max()
    assert at > 10 * np.median(np.abs(g["dpred"][mask])), at


# -------------------------------------------------------------------------------------------------------- 3. larger maps, ties, w_u = 0, errors
def larger_maps_case(dev, tol=1e-4):
    rs = np.random.RandomState(1803)
    shape = (4, 1, 96, 160)
    image = (rs.rand(*shape) * 19 + 1).astype(np.float32)
    gi = (rs.rand(*shape) * 30).astype(np.float32); gi[rs.rand(*shape) < 0.6] = 0      # mask density 0.6
    gs = (rs.rand(*shape) * 30).astype(np.float32); gs[rs.rand(*shape) < 0.9] = 0
    mask = gi <= 0
    pred = nudge((rs.rand(*shape) * 19 + 1).astype(np.float32), image, mask)
    m0, m1 = margins(pred, image, mask)
    print("larger maps: n %d, min|d| %.3e, min||d|-1| %.3e" % (mask.sum(), m0, m1))
    assert m0 >= MARGIN and m1 >= MARGIN
    for lf, ws, we in (("l1", 0.2, 0.0), ("smoothl1", 0.0, 0.35), ("l2", 0.2, 0.5)):
        _, info, dpred = _hip_loss(dev, image, pred, gi, gs, mask, lf, ws, we, 0.7)
        pr = t(pred).requires_grad_()
        lo, io = restated_loss(t(image), pr, t(gi), t(gs), t(mask), lf, ws, we, 0.7)
        lo.backward()
        _check_info(info, {k: float(io[k].detach()) for k in KEYS}, tol, "larger %s" % lf)
        close(dpred, pr.grad, 10 * tol, "larger maps dpred " + lf)
    # tied medians: a quantised prediction (multiples of 0.25) -- torch spreads the median's gradient evenly over the c ties
    image7, gi7, gs7, pred7 = g7_inputs()
    mask7 = gi7 <= 0
    pq = (np.round(pred7 * 4) / 4).astype(np.float32)
    o = pq[mask7]
    c = int((o == np.float32(torch.median(t(o)))).sum())
    assert c >= 3, c
    m0, _ = margins(pq, image7, mask7)      # 'l1' below: only the distance to d = 0 matters
    assert m0 >= MARGIN, m0
    _, info, dpred = _hip_loss(dev, image7, pq, gi7, gs7, mask7, "l1", 0.2, 0.0, 0.7)
    pr = t(pq).requires_grad_()
    lo, io = restated_loss(t(image7), pr, t(gi7), t(gs7), t(mask7), "l1", 0.2, 0.0, 0.7)
    lo.backward()
    _check_info(info, {k: float(io[k].detach()) for k in KEYS}, tol, "ties c=%d" % c)
    close(dpred, pr.grad, 10 * tol, "tied medians dpred")
    # w_unsupervised = 0 with a mask given == the call without a mask, bitwise
    la, ia, da = _hip_loss(dev, image7, pred7, gi7, gs7, mask7, "l1", 0.2, 0.35, 0.0)
    lb, ib, db = _hip_loss(dev, image7, pred7, gi7, gs7, None, "l1", 0.2, 0.35, 0.0)
    assert torch.equal(la, lb) and torch.equal(da, db) and ia == ib and ia['loss_unsupervised'] == 0.0
    # an empty mask: the term and the total are NaN (the reference's median / mean over nothing), the term adds no gradient
    _, ie, de = _hip_loss(dev, image7, pred7, gi7, gs7, np.zeros_like(mask7), "l1", 0.2, 0.0, 0.7)
    _, i0, d0 = _hip_loss(dev, image7, pred7, gi7, gs7, None, "l1", 0.2, 0.0, 0.0)
    assert np.isnan(ie['loss_unsupervised']) and np.isnan(ie['loss']) and ie['loss_supervised'] == i0['loss_supervised']
    assert torch.equal(de, d0)
    pr = t(pred7).requires_grad_()
    lo, _ = restated_loss(t(image7), pr, t(gi7), t(gs7), t(np.zeros_like(mask7)), "l1", 0.2, 0.0, 0.7)
    assert bool(torch.isnan(lo))
    # w_unsupervised > 0 without a mask is an error of the caller
    import pytest
    with pytest.raises(ValueError):
        _hip_loss(dev, image7, pred7, gi7, gs7, None, "l1", 0.2, 0.0, 0.7)


def dropped_mask_case(dev, tol=1e-4):
    """The caller's mask does not outlive compute_loss (train_zju.py passes the temporary `batch_gt <= 0`; sml_main.forward_loss a local): it is
    dropped, collected and its memory allocated over before backward().  The gradient must still be the fixture's -- the backward reads the mask
    again, so the tape has to keep it alive."""
    import gc
    from riders_amd.loss import compute_loss
    image, gi, gs, _ = g7_inputs()
    g = load("g18_loss_unsup_l1")
    for form in ("bool", "le0"):
        p = t(g["pred"], dev).requires_grad_()
        mask = (t(gi, dev) <= 0) if form == "bool" else t(gi, dev).clone()
        size, dtype = mask.numel(), mask.dtype
        loss, _ = compute_loss(image=t(image, dev), output_depth=p, gt_interp=t(gi, dev), gt_sparse=t(gs, dev), loss_func="l1", w_smoothness=0.2,
                               sobel_filter_size=FS, validity_map_loss_smoothness=torch.ones_like(t(image, dev)), w_lidar_loss=W_LIDAR, w_edge=0.0,
                               invalid_map_gt=mask, w_unsupervised=W_UNSUP)
        del mask
        gc.collect()
        over = [torch.full((size,), 1 if dtype == torch.bool else 7.0, dtype=dtype, device=dev) for _ in range(8)]      # same-sized blocks: "nothing selected"
        over += [torch.full((size,), 7.0, dtype=torch.float32, device=dev) for _ in range(8)]
        loss.backward()
        del over
        close(p.grad, g["dpred"], 10 * tol, "unsup dpred after the mask was dropped (%s)" % form)


def forward_loss_case(dev, net_hw=None, B=2, H=48, W=64, tol=1e-4):
    """sml_main.forward_loss with cfg['w_unsupervised'] > 0 against the torch restatement on the same batch: the mask is the resized ground truth
    <= 0 BEFORE outlier removal (train_zju.py:361 ahead of :363-367), the supervised term sees it after.  A stand-in model returns a given
    prediction, so that the loss AND its gradient with respect to the prediction are compared, one step."""
    from riders_amd import sml_main
    cfg = dict(sml_main.ZJU_SML_CONFIG, w_unsupervised=0.5)
    if net_hw is not None:
        cfg['net_hw'] = net_hw
    batch = sml_main.synthetic_batch(B, H, W, seed=11, device=dev)
    image, mono, sparse_depth, gt, sparse_gt, rcnet = batch
    hw = tuple(net_hw) if net_hw else sml_main.net_size(H, W)
    _, d, _ = sml_main.prepare_inputs(image, mono, sparse_depth, rcnet, hw, cfg)
    d_depth = (1.0 / d.cpu())
    gt_r, sgt_r = sml_main.nearest_resize(gt, *hw).cpu(), sml_main.nearest_resize(sparse_gt, *hw).cpu()
    mask = gt_r <= 0
    gi = OS.remove_outliers(gt_r, cfg['outlier_removal_kernel_size'], cfg['outlier_removal_threshold'])
    assert int(((gi <= 0) & ~mask).sum()) > 0, "outlier removal changes nothing on this batch: the case would not tell the two mask sources apart"
    # the network's output is an inverse depth: choose the depth (margins as in the fixture cases), hand its reciprocal to the loss
    rs = np.random.RandomState(5)
    depth = nudge((rs.rand(*d_depth.shape) * 19 + 1).astype(np.float32), d_depth.numpy(), mask.numpy())
    pred_c = (1.0 / t(depth)).requires_grad_()
    m0, m1 = margins((1.0 / pred_c.detach()).numpy(), d_depth.numpy(), mask.numpy())
    print("forward_loss: maps %s, n %d, min|d| %.3e, min||d|-1| %.3e" % (hw, int(mask.sum()), m0, m1))
    assert m0 >= MARGIN and m1 >= MARGIN
    lo, io = restated_loss(d_depth, 1.0 / pred_c, gi, sgt_r, mask, cfg['loss_func'], cfg['w_smoothness'], cfg['w_edge'], cfg['w_unsupervised'],
                           fs=cfg['sobel_filter_size'], w_lidar=cfg['w_lidar_loss'])
    lo.backward()

    class Given(object):
        def __init__(self):
            self.pred = pred_c.detach().to(dev).requires_grad_()

        def forward(self, x, dd):
            assert torch.equal(dd.cpu(), d.cpu())
            return self.pred
    model = Given()
    loss = sml_main.forward_loss(model, batch, cfg, sml_main.make_outlier_removal(cfg))
    loss.backward()
    a, b = float(loss.detach()), float(lo.detach())
    print("forward_loss: hip %.8g restated %.8g (unsupervised term %.8g)" % (a, b, float(io['loss_unsupervised'].detach())))
    assert abs(a - b) <= tol * max(abs(b), 1e-3), (a, b)
    close(model.pred.grad, pred_c.grad, 10 * tol, "forward_loss dpred")
    # and the comparison above can tell the mask sources apart: with the mask taken AFTER outlier removal the restated total lies outside its tolerance, 3 x over
    lo2, _ = restated_loss(d_depth, 1.0 / pred_c.detach(), gi, sgt_r, gi <= 0, cfg['loss_func'], cfg['w_smoothness'], cfg['w_edge'], cfg['w_unsupervised'],
                           fs=cfg['sobel_filter_size'], w_lidar=cfg['w_lidar_loss'])
    assert abs(float(lo2) - b) > 3 * tol * abs(b), (float(lo2), b)


# ------------------------------------------------------------------------------------------------------------------------------ 4. GPU only
def _sml_setup(dev, seed=0):
    from riders_amd import sml_main
    from riders_amd.optim import FlatAdam
    torch.manual_seed(seed)
    m = sml_main.build_model(dev)
    m.train()
    return m, FlatAdam(m.parameters(), lr=1e-4)


def graphed_step_case(dev, steps=3):
    """GraphedTrainStep with w_unsupervised = 0.5: losses and parameters after 3 steps equal the eager train_step run bit for bit (the standard
    of the existing graphed-step tests): the selection runs inside the captured step, with no host synchronisation."""
    from riders_amd import sml_main
    cfg = dict(sml_main.ZJU_SML_CONFIG, w_unsupervised=0.5)
    batch = sml_main.synthetic_batch(2, 96, 128, seed=3, device=dev)
    m, opt = _sml_setup(dev)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    orr = sml_main.make_outlier_removal(cfg)
    eager = [float(sml_main.train_step(m, opt, batch, cfg, outlier=orr).detach()) for _ in range(steps)]
    assert all(np.isfinite(eager)), eager
    p_eager = [p.detach().clone() for p in m.parameters()]
    m2, opt2 = _sml_setup(dev)
    m2.load_state_dict(sd)
    step = sml_main.GraphedTrainStep(m2, opt2, batch, cfg, outlier=sml_main.make_outlier_removal(cfg), warmup=1)
    graphed = [float(step().detach()) for _ in range(steps)]
    print("eager", eager, "graphed", graphed)
    assert graphed == eager, (graphed, eager)
    for a, b in zip(p_eager, m2.parameters()):
        assert torch.equal(a, b.detach())
    # the term is in the loss: the same step without it gives another value
    m3, opt3 = _sml_setup(dev)
    m3.load_state_dict(sd)
    assert float(sml_main.train_step(m3, opt3, batch, sml_main.ZJU_SML_CONFIG, outlier=orr).detach()) != eager[0]


def autograph_case(dev, steps=4):
    """The same under engine.set_autograph(True), the mode for UNCHANGED callers (train_zju.py:353-392: forward -> compute_loss -> loss.backward() ->
    torch.optim.Adam.step()): with the model's region captured and replayed the loop equals the plain eager loop bit for bit, the unsupervised term
    running eagerly behind the replayed forward."""
    import contextlib
    import io
    from riders_amd import engine, sml_main
    cfg = dict(sml_main.ZJU_SML_CONFIG, w_unsupervised=0.5)
    batch = sml_main.synthetic_batch(2, 96, 128, seed=3, device=dev)
    runs = []
    for auto in (False, True):
        torch.manual_seed(0)
        with contextlib.redirect_stdout(io.StringIO()):
            m = sml_main.build_model(dev)
        m.train()
        opt = torch.optim.Adam(m.parameters(), lr=1e-4)
        orr = sml_main.make_outlier_removal(cfg)
        engine.set_autograph(auto)
        try:
            losses = []
            for _ in range(steps):
                loss = sml_main.forward_loss(m, batch, cfg, orr)
                opt.zero_grad()
                loss.backward()
                opt.step()
                losses.append(loss.item())
            stats = engine.autograph_stats()
        finally:
            engine.set_autograph(False)
        runs.append((losses, [p.detach().clone() for p in m.parameters()], stats))
    (la, pa, s0), (lb, pb, sb) = runs
    print("eager", la, "autograph", lb, sb)
    assert sb["captured"] - s0["captured"] >= 1 and sb["replayed"] - s0["replayed"] >= steps - 1, (s0, sb)
    assert all(np.isfinite(la)) and la == lb, (la, lb)
    for a, b in zip(pa, pb):
        assert torch.equal(a, b)


def reproducible_case(dev):
    """Two eager runs of one step give bitwise equal gradients: the selection's atomics add integers, the sums reduce in a fixed order."""
    from riders_amd import sml_main
    cfg = dict(sml_main.ZJU_SML_CONFIG, w_unsupervised=0.5)
    batch = sml_main.synthetic_batch(2, 96, 128, seed=3, device=dev)
    grads = []
    for _ in range(2):
        m, opt = _sml_setup(dev)
        loss = sml_main.compute_gradients(m, opt, batch, cfg, sml_main.make_outlier_removal(cfg))
        grads.append((float(loss), [p.grad.detach().clone() for p in m.parameters() if p.grad is not None]))
    assert grads[0][0] == grads[1][0] and len(grads[0][1]) == len(grads[1][1]) > 0
    for a, b in zip(*[g[1] for g in grads]):
        assert torch.equal(a, b)
