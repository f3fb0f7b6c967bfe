"""Frozen BatchNorm at the engine and module level, device-agnostic (the GPU twin runs them on an MI355X, the emulator twin under the fiber
emulator): layers that normalise with their running statistics -- through `bn.eval()` under a parent in .train(), or through the sticky mark of
riders_amd.freeze_batch_norm -- forward AND backward against the oracle with training=False, in fp32.  Every case also checks what frozen means
for the buffers: running_mean / running_var bit-unchanged, num_batches_tracked not counted.

Tolerances are those of the training-mode cases these are built from (tests/parity_cases.py, tests/parity_cases_sml.py): TOL relative to
max|ref| for outputs, input gradients and the Conv2d-family parameter gradients; 2 x TOL for the EfficientNet blocks' parameter gradients, as
effnet_block_case; for the mixed-mode RC-Net step TOL on logits and loss and 5 x TOL relative L2 per module, as rcnet_fullsize_oracle_case."""
import torch

import riders_amd
from oracle import effnet_lite3_torch as OE
from oracle import rcnet as O
from tests.golden.fill import fill_state_dict, rand_array
from tests.parity_cases import TOL, _lazy_both, _lazy_module_run, _module_grads, close, compare_param_grads, force_patch_conv, leaves, q, t
from tests.parity_cases_sml import _run_tape


def _bns(m):
    return riders_amd.engine._bn_modules(m)


def _running(m):
    sd = m.state_dict() if isinstance(m, torch.nn.Module) else {**{"e." + k: v for k, v in m.encoder.state_dict().items()},
                                                                **{"d." + k: v for k, v in m.decoder.state_dict().items()}}
    return {k: v.detach().clone() for k, v in sd.items() if "running_" in k or "num_batches_tracked" in k}


def _assert_frozen(m, before, what):
    """running statistics bit-unchanged, no batch counted (state_dict() flushes the host-side counters)"""
    after = _running(m)
    assert before.keys() == after.keys() and len(before) > 0
    for k in before:
        assert torch.equal(before[k], after[k]), "%s: %s changed under frozen BatchNorm" % (what, k)
        if "num_batches_tracked" in k:
            assert int(after[k]) == 0, (what, k)


def _assert_trained(m, before, what, count=1):
    after = _running(m)
    for k in before:
        if "num_batches_tracked" in k:
            assert int(after[k]) == count, (what, k, int(after[k]))
        else:
            assert not torch.equal(before[k], after[k]), "%s: %s did not move in training mode" % (what, k)


def _grads(m):
    return [p.grad for p in m.parameters() if p.grad is not None]


# ---------------------------------------------------------------------------------------------------------------- Conv2d
CONV_CASES = [dict(cin=16, cout=32, k=3, s=1, N=2, H=9, W=11), dict(cin=3, cout=32, k=7, s=2, N=2, H=9, W=11, no_input_grad=True)]


def conv_case(dev, c, tol=TOL):
    """net_utils.Conv2d with its BatchNorm frozen: forward, dx, gamma / beta / weight gradients against O.conv_bn_act(training=False)"""
    from riders_amd import net_utils
    m = net_utils.Conv2d(c["cin"], c["cout"], c["k"], c["s"], 'kaiming_uniform', net_utils.activation_func('leaky_relu'), True).to(dev)
    tag = "frozen.conv.%d.%d.%d" % (c["cin"], c["cout"], c["k"])
    sd = leaves(fill_state_dict(m, tag))
    x = t(rand_array(tag + ".x", (c["N"], c["cin"], c["H"], c["W"]), 1.0))
    xr = x.clone().requires_grad_()
    ref = O.conv_bn_act(xr, sd, "", c["s"], use_bn=True, act=True, training=False)
    w = t(rand_array(tag + ".w", ref.shape, 1.0))
    (ref * w).sum().backward()
    xd = x.to(dev)
    if not c.get("no_input_grad"):
        xd.requires_grad_()
    assert riders_amd.freeze_batch_norm(m) == 1
    m.train()
    before = _running(m)
    out = m(xd)
    close(out, ref, tol, tag + " fwd")
    (out * w.to(dev)).sum().backward()
    if not c.get("no_input_grad"):
        close(xd.grad, xr.grad, tol, tag + " dx")
    assert compare_param_grads(m, sd, tol) == 3
    _assert_frozen(m, before, tag)


# ---------------------------------------------------------------------------------------------------------------- ResNetBlock, the idiom, the mark
def _resblk(dev):
    from riders_amd import net_utils
    m = net_utils.ResNetBlock(16, 32, 2, 'kaiming_uniform', net_utils.activation_func('leaky_relu'), True).to(dev)
    sd = leaves(fill_state_dict(m, "frozen.resblk"))
    x = t(rand_array("frozen.resblk.x", (2, 16, 9, 11), 1.0))
    return m, sd, x


def _resblk_step(dev, m, x, w):
    for p in m.parameters():
        p.grad = None
    xd = x.clone().to(dev).requires_grad_()      # (a clone: on the emulator's device .to() returns x itself, whose .grad would accumulate)
    out = m(xd)
    (out * w.to(dev)).sum().backward()
    return out, xd.grad


def resnet_block_case(dev, tol=TOL):
    """ResNetBlock 16 -> 32, stride 2 (the residual tail: fused apply + add + activation, projection shortcut).  (a) bn.eval() on every
    BatchNorm module with the block in .train() -- the standard idiom -- and (b) freeze_batch_norm(block) followed by block.train() give outputs
    and gradients bit-identical to each other and equal to O.resnet_block(training=False); thawing restores training behaviour."""
    m, sd, x = _resblk(dev)
    xr = x.clone().requires_grad_()
    ref = O.resnet_block(xr, sd, "", 2, training=False)
    w = t(rand_array("frozen.resblk.w", ref.shape, 1.0))
    (ref * w).sum().backward()
    res = {}
    for how in ("idiom", "mark"):
        m, _, _ = _resblk(dev)
        if how == "idiom":
            m.train()
            for b in _bns(m):
                b.eval()
        else:
            assert riders_amd.freeze_batch_norm(m) == 2
            m.train()      # the mark is sticky: .train() does not thaw
            assert all(b.training for b in _bns(m))
        before = _running(m)
        out, dx = _resblk_step(dev, m, x, w)
        close(out, ref, tol, "frozen resnet block (%s) fwd" % how)
        close(dx, xr.grad, tol, "frozen resnet block (%s) dx" % how)
        assert compare_param_grads(m, sd, tol) == 7      # three convolution weights, two (gamma, beta) pairs
        _assert_frozen(m, before, "resnet block (%s)" % how)
        res[how] = [v.detach().cpu().clone() for v in [out, dx] + _grads(m)]
    assert len(res["idiom"]) == len(res["mark"]) == 9
    for i, (a, b) in enumerate(zip(res["idiom"], res["mark"])):
        assert torch.equal(a, b), "bn.eval() and freeze_batch_norm differ in tensor %d" % i
    # thaw (m is the marked block): batch statistics again, the running statistics move, one batch counted
    riders_amd.freeze_batch_norm(m, False)
    before = _running(m)
    xr2 = x.clone().requires_grad_()
    ref_t = O.resnet_block(xr2, leaves(fill_state_dict(_resblk(dev)[0], "frozen.resblk")), "", 2, training=True)
    out, _ = _resblk_step(dev, m, x, w)
    close(out, ref_t, tol, "thawed resnet block fwd")
    _assert_trained(m, before, "thawed resnet block")


def affine_false_case(dev):
    """freeze_batch_norm(affine=False): gamma / beta get no gradient and keep their values' state_dict entries; dx and the weight gradients are
    bit-identical to the affine=True run; only the launch without sums runs.  Thawing restores requires_grad."""
    from riders_amd import engine
    res = {}
    for affine in (True, False):
        m, _, x = _resblk(dev)
        keys = list(m.state_dict().keys())
        riders_amd.freeze_batch_norm(m, True, affine=affine)
        m.train()
        w = t(rand_array("frozen.resblk.w", (2, 32, 5, 6), 1.0))
        for k in engine.lazy_counts:
            engine.lazy_counts[k] = 0
        out, dx = _resblk_step(dev, m, x, w)
        c = dict(engine.lazy_counts)
        assert list(m.state_dict().keys()) == keys
        bn_par = [p for b in _bns(m) for p in (b.weight, b.bias)]
        if affine:
            assert all(p.grad is not None for p in bn_par)
            assert c["bn_frozen_sums"] == 2 and c["bn_frozen"] == 0, c
        else:
            assert all(p.grad is None and not p.requires_grad for p in bn_par)
            assert c["bn_frozen_sums"] == 0 and c["bn_frozen"] > 0, c
        convs = [m.conv1.conv.weight, m.conv2.conv.weight, m.projection.conv.weight]
        res[affine] = [v.detach().cpu().clone() for v in [out, dx] + [p.grad for p in convs]]
        if not affine:
            riders_amd.freeze_batch_norm(m, False)
            assert all(p.requires_grad for p in bn_par)
    for i, (a, b) in enumerate(zip(res[True], res[False])):
        assert torch.equal(a, b), "affine=False changes tensor %d" % i


def refuses_untracked_case(dev):
    bn = torch.nn.BatchNorm2d(8, track_running_stats=False).to(dev)
    try:
        riders_amd.freeze_batch_norm(bn)
    except ValueError:
        return
    raise AssertionError("freeze_batch_norm accepted a BatchNorm2d without running statistics")


# ---------------------------------------------------------------------------------------------------------------- DecoderBlock
def decoder_block_case(dev, tol=TOL):
    """DecoderBlock 32 + 16 -> 16, 4x3 -> 9x6, frozen: the up-convolution's output stays virtual and is concatenated with the skip inside the
    consumer's gather; both backward paths"""
    from riders_amd import net_utils
    m = net_utils.DecoderBlock(32, 16, 16, 'kaiming_uniform', net_utils.activation_func('leaky_relu'), True, 'up').to(dev)
    sd = leaves(fill_state_dict(m, "frozen.decblk"))
    x, s = t(rand_array("frozen.decblk.x", (2, 32, 4, 3), 1.0)), t(rand_array("frozen.decblk.s", (2, 16, 9, 6), 1.0))
    xr, sr = x.clone().requires_grad_(), s.clone().requires_grad_()
    ref = O.decoder_block(xr, sr, (9, 6), sd, "", training=False)
    w = t(rand_array("frozen.decblk.w", ref.shape, 1.0))
    (ref * w).sum().backward()
    riders_amd.freeze_batch_norm(m)
    m.train()
    before = _running(m)
    xd, sdv = x.to(dev).requires_grad_(), s.to(dev).requires_grad_()
    out = m(xd, sdv)
    close(out, ref, tol, "frozen decoder block fwd")
    (out * w.to(dev)).sum().backward()
    close(xd.grad, xr.grad, tol, "frozen decoder block dx")
    close(sdv.grad, sr.grad, tol, "frozen decoder block dskip")
    assert compare_param_grads(m, sd, tol) == 6
    _assert_frozen(m, before, "decoder block")


# ---------------------------------------------------------------------------------------------------------------- depthwise blocks
def effnet_block_case(dev, kind, k, cin=16, tol=TOL):
    """InvertedResidual (with its residual: stride 1, cin == cout) / DepthwiseSeparableConv on 2 x 16 x 9 x 12, frozen, against the oracle's
    torch module in .eval(): the depthwise layer's backward (dwconv_block) and the residual route of conv_block"""
    from riders_amd.midas import efficientnet_lite3 as E
    mine = (E.InvertedResidual if kind == "ir" else E.DepthwiseSeparableConv)(cin, cin, k, 1).to(dev)
    ref = (OE.InvertedResidual if kind == "ir" else OE.DepthwiseSeparableConv)(cin, cin, k, 1)
    assert mine.has_residual
    tag = "frozen.eff.%s.%d.%d" % (kind, cin, k)
    ref.load_state_dict({kk: v.cpu() for kk, v in fill_state_dict(mine, tag).items()})
    x = t(rand_array(tag + ".x", (2, cin, 9, 12), 1.0))
    xr = x.clone().requires_grad_()
    ref.eval()
    riders_amd.freeze_batch_norm(mine)
    mine.train()
    before = _running(mine)
    yr = ref(xr)
    w = t(rand_array(tag + ".w", yr.shape, 1.0))
    (yr * w).sum().backward()
    out, (dx,), tape = _run_tape(dev, [x], lambda a: mine._fwd(a), w)
    close(out, yr, tol, tag + " fwd")
    close(dx, xr.grad, tol, tag + " dx")
    n = 0
    for (kk, p), (_, pr) in zip(mine.named_parameters(), ref.named_parameters()):
        close(tape.pgrads[id(p)], pr.grad, 2 * tol, tag + " grad " + kk)
        n += 1
    assert n == (9 if kind == "ir" else 6)
    _assert_frozen(mine, before, tag)


# ---------------------------------------------------------------------------------------------------------------- mixed mode: RC-Net
def _g6_model(dev):
    from riders_amd import rcnet_main
    cfg = dict(rcnet_main.ZJU_CONFIG, patch_size=[64, 32], total_points_sampled=3)      # the g6 fixture's geometry: 2 images of 64 x 96, K = 3
    torch.manual_seed(0)
    return rcnet_main.build_model(dev, cfg), cfg


def mixed_mode_case(dev, tol=TOL):
    """RC-Net at the g6 fixture's geometry with the encoder frozen and the decoder live: the reference is O.rcnet_encoder(training=False) into
    O.multiscale_decoder(training=True).  Loss, logits, per-module gradient L2; encoder statistics unchanged and not counted, decoder statistics
    updated and counted once."""
    from riders_amd import engine, rcnet_main
    model, cfg = _g6_model(dev)
    ph, pw = cfg['patch_size']
    sd_e, sd_d = leaves(model.encoder.state_dict()), leaves(model.decoder.state_dict())
    riders_amd.freeze_batch_norm(model.encoder)
    model.train()
    before_e, before_d = _running(model.encoder), _running(model.decoder)
    batch = rcnet_main.synthetic_batch(2, 64, 96, cfg, seed=77)
    image, pts, rois, gt = rcnet_main.prepare_batch(tuple(b.to(dev) for b in batch))
    label, valid = engine.rcnet_labels(gt, pts, 0.5)
    logits = model.forward(image, pts, rois)
    loss, _ = model.compute_loss(logits, label, valid, 2.5)
    loss.backward()
    pts_c, gt_c = batch[1].reshape(-1, 3), batch[3].reshape(-1, 1, ph, pw)
    lab_c, val_c = O.rcnet_labels(gt_c, pts_c, 0.5)
    assert torch.equal(label.cpu(), lab_c) and torch.equal(valid.cpu(), val_c)
    latent, skips = O.rcnet_encoder(batch[0] / 255.0, pts_c, [b for b in batch[2]], sd_e, cfg['patch_size'], training=False)
    ref = O.multiscale_decoder(latent, skips, cfg['patch_size'], sd_d, training=True)[-1]
    ref_loss = O.rcnet_loss(ref, lab_c, val_c, 2.5)
    ref_loss.backward()
    close(logits, ref, tol, "mixed-mode logits")
    assert abs(float(loss) - float(ref_loss)) <= tol * abs(float(ref_loss)), (float(loss), float(ref_loss))
    got = _module_grads(model)
    for name, mod, sd, pref in (("encoder_image", model.encoder.encoder_image, sd_e, "encoder_image."), ("attention", model.encoder.attention, sd_e, "attention."),
                                ("encoder_depth", model.encoder.encoder_depth, sd_e, "encoder_depth."), ("decoder", model.decoder, sd_d, "")):
        r = torch.cat([sd[pref + k].grad.reshape(-1) for k, p in mod.named_parameters() if p.grad is not None])
        err = float((got[name] - r).norm() / r.norm())
        print("mixed mode %s gradient: relative L2 error %.3e" % (name, err))
        assert err <= 5 * tol, "mixed-mode %s gradient: relative L2 error %.3e" % (name, err)
    _assert_frozen(model.encoder, before_e, "frozen encoder")
    _assert_trained(model.decoder, before_d, "live decoder")


# ---------------------------------------------------------------------------------------------------------------- virtual outputs
def _frozen(m):
    riders_amd.freeze_batch_norm(m)
    return m


def _decoder_chain(cw=32):
    from riders_amd import networks
    lat = t(rand_array("lazy.lat", (2, 2 * cw, 2, 1), 1.0))
    skips = [t(rand_array("lazy.sk%d" % i, (2, c_, h_, w_), 1.0)) for i, (c_, h_, w_) in enumerate(((16, 32, 16), (cw // 2, 16, 8), (cw // 2, 7, 4), (cw, 4, 2)))]
    mk = lambda: networks.MultiScaleDecoder(2 * cw, 1, 1, [cw, cw // 2, cw // 2, 16, 16], [cw, cw // 2, cw // 2, 16, 0], 'kaiming_uniform', 'leaky_relu',      # noqa: E731
                                            'linear', True, 'up')
    return mk, lat, skips


def lazy_case(dev, tol=TOL):
    """The decoder chain of lazy_bn_cases (fp32), frozen: with every block's output virtual (set_lazy_bn(2)) and with none (0) the results are
    bit-identical (bn_head and up2_on_source pinned off, as _lazy_both pins them) -- the frozen backward recomputes the activation's argument
    from y.  With bn_head on, the layer in front of the fused head receives a HeadGrad, writes it out, and agrees with the oracle."""
    from riders_amd import engine
    mk, lat, skips = _decoder_chain()
    with force_patch_conv():
        c = _lazy_both(_lazy_module_run(dev, lambda: _frozen(mk()), [lat] + skips, lambda m, x, *s: m(x, list(s), (64, 32))[-1]))
        assert c["fwd_fused"] >= 8 and c["bn_frozen_sums"] == 10 and c["bn_frozen"] == 0, c
    # bn_head on (the default): the frozen head layer against the oracle
    m = mk().to(dev)
    sd = leaves(fill_state_dict(m, "lazy"))
    xs = [lat] + skips
    xr = [x.clone().requires_grad_() for x in xs]
    ref = O.multiscale_decoder(xr[0], xr[1:], (64, 32), sd, training=False)[-1]
    w = t(rand_array("lazy.w", tuple(ref.shape), 1.0))
    (ref * w).sum().backward()
    riders_amd.freeze_batch_norm(m)
    m.train()
    for k in engine.lazy_counts:
        engine.lazy_counts[k] = 0
    xd = [x.to(dev).requires_grad_() for x in xs]
    out = m(xd[0], xd[1:], (64, 32))[-1]
    (out * w.to(dev)).sum().backward()
    c = dict(engine.lazy_counts)
    if engine.head_route(16):
        assert c["head_fused"] == 1 and c["head_unfused_bwd"] == 1, c      # fused forward, HeadGrad materialised for the frozen layer
    close(out, ref, tol, "frozen decoder chain fwd (bn_head on)")
    for i, (a, b) in enumerate(zip(xd, xr)):
        close(a.grad, b.grad, tol, "frozen decoder chain dx %d" % i)
    compare_param_grads(m, sd, tol)


# ---------------------------------------------------------------------------------------------------------------- autograph (GPU only)
def autograph_case(dev):
    """engine.set_autograph(True) at g6 geometry: three eager-autograd steps in training mode, freeze_batch_norm(model.encoder), three more.
    Parameters and running statistics are bit-identical to the same six steps with autograph off, and the freeze leads to one more captured
    region (the graph key carries the BatchNorm-mode signature) instead of a replay of the training-mode graph."""
    from riders_amd import engine, rcnet_main
    res = {}
    for mode in ("eager", "autograph"):
        engine.set_autograph(mode == "autograph")
        engine.set_deterministic_roi_pool(True)
        try:
            model, cfg = _g6_model(dev)
            batches = [rcnet_main.synthetic_batch(2, 64, 96, cfg, seed=60 + i, device=dev) for i in range(6)]
            model.train()
            opt = torch.optim.Adam(model.parameters(), lr=1e-3)
            caps = []
            for i, b in enumerate(batches):
                if i == 3:
                    riders_amd.freeze_batch_norm(model.encoder)
                loss = rcnet_main.forward_loss(model, b, cfg)
                opt.zero_grad()
                loss.backward()
                opt.step()
                caps.append(engine.autograph_stats()["captured"])
            sd = {k: v.detach().clone() for k, v in list(model.encoder.state_dict().items()) + list(model.decoder.state_dict().items())}
            res[mode] = (sd, caps)
        finally:
            engine.set_autograph(False)
            engine.set_deterministic_roi_pool(False)
    (sde, _), (sda, caps) = res["eager"], res["autograph"]
    assert caps[2] - caps[0] == 1 and caps[5] - caps[2] == 1, caps      # one capture before the freeze, exactly one more after it
    for k in sde:
        assert torch.equal(sde[k], sda[k]), "autograph differs from eager in " + k
