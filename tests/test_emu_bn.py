"""The BatchNorm kernel family one by one under the fiber emulator (see tests/test_emu_ops.py for what these are and are not): a covering
selection of the cross products the GPU twin runs in full (tests/parity_cases_bn.py `_cover`), and the census of |mean| * rstd over every BatchNorm
layer of the two fixture networks, which is a measurement (DESIGN.md "BatchNorm parity"), not an assertion.  The census runs the forward of a
training step only: every rd_bn_finalize / rd_bn_finalize_apply call of a step is made there, and the backward triples the emulator's time."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import parity_cases_bn as B


def test_statistics_producers(emu):
    B.stats_case(emu, quick=True)
    B.report_bn()


def test_finalize(emu):
    B.finalize_case(emu, quick=True)
    B.report_bn()


def test_affine_act(emu):
    B.affine_case(emu, quick=True)
    B.report_bn()


def test_backward(emu):
    B.backward_case(emu, quick=True)
    B.report_bn()


def test_thresholds(emu):
    B.thresholds_case(emu, quick=True)
    B.report_bn()


def test_phases(emu):
    B.phases_case(emu, quick=True)
    B.report_bn()


def test_conditioning(emu):
    B.conditioning_case(emu, quick=True)
    B.report_bn()


# ---------------------------------------------------------------------------------------------------------------- census
def _floats(ptr, n):
    return np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctypes.c_float)), (n,)).astype(np.float64)


def _census(name, modules, step):
    """Run `step` with rd_bn_finalize and rd_bn_finalize_apply wrapped (here, not in the engine): after every call read the mean and rstd it
    left (host memory under the emulator) and keep max_c |mean| * rstd, keyed by the layer whose running_mean the call was given."""
    from riders_amd import engine
    lib = engine.L()
    layers = {}
    for root, mod in modules:
        for n, m in mod.named_modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                layers[m.running_mean.data_ptr()] = root + n
    seen, calls = {}, [0]

    def note(running_mean, C, mean, rstd):
        calls[0] += 1
        key = layers.get(running_mean.value if running_mean is not None else None, "(unnamed)")
        if mean is not None and rstd is not None:
            seen[key] = max(seen.get(key, 0.0), float((np.abs(_floats(mean.value, C)) * _floats(rstd.value, C)).max()))

    fin, fin_apply = lib.rd_bn_finalize, lib.rd_bn_finalize_apply

    def w_fin(*a):
        rc = fin(*a)
        if a[8]:      # training: batch statistics
            note(a[9], a[2], a[11], a[12])
        return rc

    def w_fin_apply(*a):
        rc = fin_apply(*a)
        note(a[7], a[15], a[9], a[10])
        return rc

    lib.rd_bn_finalize, lib.rd_bn_finalize_apply = w_fin, w_fin_apply
    try:
        step()
    finally:
        lib.rd_bn_finalize, lib.rd_bn_finalize_apply = fin, fin_apply
    worst = max(seen, key=seen.get)
    B.CENSUS[name] = (seen[worst], worst, calls[0], len(layers))
    for k in sorted(seen, key=seen.get, reverse=True)[:5]:
        print("bn census %s: max |mean| * rstd %.3f at %s" % (name, seen[k], k))
    B.report_bn()
    missing = sorted(set(layers.values()) - set(seen))
    assert not missing, "%s: the census saw no finalize call of %s" % (name, missing)


@pytest.mark.slow
def test_census_rcnet(emu):
    from riders_amd import engine
    from riders_amd.rcnet_model import RCNetModel
    from tests.golden.fill import fill_state_dict, rand_array
    from tests.parity_cases import load, t
    g = load("g6_rcnet_e2e")
    patch = [64, 32]
    m = RCNetModel(3, 3, patch, ['rcnet', 'batch_norm'], [32, 64, 128, 128, 128], [32, 64, 128, 128, 128],
                   ['multiscale', 'batch_norm'], [256, 128, 64, 32, 16], device=emu)
    fill_state_dict(m.encoder, "g6.enc"); fill_state_dict(m.decoder, "g6.dec")
    Bn, K, H, W = 2, 3, 64, 96
    img = F.pad(t(rand_array("g6.img", (Bn, 3, H, W), 1.0, lo=0.0)), (patch[1] // 2,) * 2 + (patch[0] // 2,) * 2, mode='replicate').to(emu)
    pts = t(g["pts"], emu).view(Bn * K, 3)
    boxes = [t(b, emu) for b in g["boxes"]]
    gt = rand_array("g6.gt", (Bn * K, 1, patch[0], patch[1]), 1.0, lo=0.0) * 30.0
    gt[rand_array("g6.gtm", gt.shape, 1.0, lo=0.0) < 0.5] = 0.0
    label, valid = engine.rcnet_labels(t(gt, emu), pts, 0.5)

    def step():
        m.train()
        logits = m.forward(img, pts, boxes, return_logits=True)
        m.compute_loss(logits, label, valid, 2.5)

    _census("RC-Net", (("encoder.", m.encoder), ("decoder.", m.decoder)), step)


@pytest.mark.slow
def test_census_sml(emu):
    from riders_amd.midas.midas_net_custom import MidasNet_small_videpth
    from tests.golden.fill import fill_state_dict, rand_array
    from tests.parity_cases import t
    m = MidasNet_small_videpth(device=emu, min_pred=0.1, max_pred=255.0, in_channels=3)
    fill_state_dict(m, "g9.sml")
    Bn, H, W = 2, 64, 96
    x = t(rand_array("g9.x", (Bn, 3, H, W), 1.0), emu).requires_grad_()
    d = t(rand_array("g9.d", (Bn, 1, H, W), 0.3, lo=0.05) + np.float32(0.02), emu)

    def step():
        m.train()
        m.forward(x, d)

    _census("SML", (("", m),), step)
