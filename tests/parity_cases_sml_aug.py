"""Cases for the Scale-Map-Learner batch augmentation (riders_amd/utv_dataset.py, rd_sml_augment_geom / rd_sml_augment_noise), run by the emulator
twin (tests/test_emu_sml_aug.py) and the GPU twin (tests/test_gpu_sml_aug.py); see tests/parity_cases.py for how case functions are used.

References.  Fixture g19 holds what the REFERENCE's UTV_dataset returned for eight tiny samples under np.random.seed(123) (flip and radar noise
on, written by tests/golden/make_golden_sml_aug.py): draw order and the un-cropped path are compared with it bit for bit.  The crop path's
resize is cv2 arithmetic that the build image cannot run, so it is compared with the float64 restatement below (`_taps64`, `_resize64`) of the
rule the kernel documents: per output pixel |error| <= 8 * 2^-24 * max|taps with a non-zero weight| -- the rounding of 1.f - f, two products
and one add in each of the two passes, a derived bound, not a measured one.  The noise pass is compared bit for bit with numpy's
`radar[radar > 0] += noise` on a float32 array.  Kernels are called through the C ABI on guarded buffers (parity_cases_glue.Buf): outputs are
NaN-prefilled, and sentinels and inputs must come back bit-identical."""
import math
import os
import struct
import zlib

import numpy as np
import torch

from tests.parity_cases_glue import F32, Buf, _bits, _call, _E, _exact, _P, _rs, _S

HERE = os.path.dirname(os.path.abspath(__file__))
NAN = float("nan")
MAPS = ("mono", "radar", "gt", "sparse_gt", "rcnet")
NOISE = [-0.01, 0.01]      # train_zju.py:455: (mean, sigma) as np.random.normal is handed them
_fix = {}


def fixture():
    if not _fix:
        _fix.update(np.load(os.path.join(HERE, "golden", "g19_sml_augment.npz")))
    return _fix


# ---------------------------------------------------------------------------------------------------------------- files of the fixture
def _png_rgb8(px):
    h, w, _ = px.shape
    rows = np.zeros((h, 1 + 3 * w), dtype=np.uint8)
    rows[:, 1:] = px.reshape(h, 3 * w)
    chunk = lambda tag, data: struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)      # noqa: E731
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(rows.tobytes(), 6))
            + chunk(b"IEND", b""))


def write_files(root):
    """the fixture's decoded inputs as the PNG files the dataset reads -> {name: [paths]}"""
    from riders_amd import data_utils
    g = fixture()
    paths = {k: [] for k in ("image",) + MAPS}
    for n in range(g["image"].shape[0]):
        for name in paths:
            p = os.path.join(str(root), "%s_%d.png" % (name, n))
            with open(p, "wb") as f:
                f.write(_png_rgb8(g["image"][n]) if name == "image" else data_utils.encode_png16(g["in_" + name][n]))
            paths[name].append(p)
    return paths


def dataset(paths, **kw):
    from riders_amd import UTV_dataset
    return UTV_dataset(paths["image"], paths["mono"], paths["radar"], paths["gt"], paths["sparse_gt"], rcnet_paths=paths["rcnet"], **kw)


def _depth(words):
    return words.astype(np.float32) / np.float32(256.0)


def recorded_flags(n):
    """(flip, noise) of fixture sample n, read off the reference's outputs"""
    g = fixture()
    flip = not np.array_equal(g["out_gt"][n], _depth(g["in_gt"][n]))
    radar = _depth(g["in_radar"][n])
    return flip, not np.array_equal(g["out_radar"][n], radar[:, ::-1] if flip else radar)


# ---------------------------------------------------------------------------------------------------------------- float64 restatement
def _taps64(src, dst):
    """the documented table rule, element by element -> first taps, second taps (clamped into the window), weights f as Python floats"""
    scale = 1.0 / (dst / src)
    first, second, frac = [], [], []
    for d in range(dst):
        f = np.float32((d + 0.5) * scale - 0.5)
        s = int(math.floor(float(f)))
        f = np.float32(f - np.float32(s))
        if s < 0:
            s, f = 0, np.float32(0)
        if s >= src - 1:
            s, f = src - 1, np.float32(0)
        first.append(s); second.append(min(s + 1, src - 1)); frac.append(float(f))
    return np.array(first), np.array(second), np.array(frac, dtype=np.float64)


def _resize64(win, H, W):
    """window (nh, nw) -> (H, W) in float64: horizontal pass, then vertical pass; and max|tap| over the taps with a non-zero weight"""
    nh, nw = win.shape
    x1, x2, fx = _taps64(nw, W)
    y1, y2, fy = _taps64(nh, H)
    win = win.astype(np.float64)
    hp = win[:, x1] * (1.0 - fx) + win[:, x2] * fx
    out = hp[y1] * (1.0 - fy)[:, None] + hp[y2] * fy[:, None]
    a = np.abs(win)
    wx2, wy2 = (fx != 0)[None, :], (fy != 0)[:, None]
    top = np.maximum(a[y1][:, x1], a[y1][:, x2] * wx2)
    bot = np.maximum(a[y2][:, x1], a[y2][:, x2] * wx2) * wy2
    return out, np.maximum(top, bot)


def _expected(plane, row, crop_hw):
    """one (H, W) plane through the parameter row -> (float64 expectation, per-pixel bound; bound None: exact)"""
    H, W = plane.shape
    out, bound = plane.astype(np.float64), None
    if row[0]:
        nh, nw = crop_hw
        x0, y0 = int(row[1]), int(row[2])
        out, m = _resize64(plane[y0:y0 + nh, x0:x0 + nw], H, W)
        bound = 8.0 * 2.0 ** -24 * m
    if row[3]:
        out = out[:, ::-1]
        bound = None if bound is None else bound[:, ::-1]
    return out, bound


# ---------------------------------------------------------------------------------------------------------------- 1. draw order (host)
def _replay(radar_count, random_shape, hw, rcnet_thr=None):
    """np.random replayed by hand in the reference's order (data/UTV_dataset.py:183-217, :76, :86, :102) from the CURRENT state ->
    params row, noise vector.  radar_count(params) -> n"""
    row = np.zeros(8, dtype=np.float32)
    if rcnet_thr is not None:
        np.random.choice(rcnet_thr)
    if random_shape is not None:
        if np.random.random() > 0.2:
            d_h, d_w = hw[0] - random_shape[0], hw[1] - random_shape[1]
            x = np.random.randint(low=0, high=d_w)
            y = d_h // 2
            if np.random.rand() <= 0.30:
                y = np.random.randint(low=0, high=d_h)
            row[:3] = (1.0, x, y)
    if np.random.random() > 0.5:
        row[3] = 1.0
    noise = np.zeros(0)
    if np.random.random() > 0.5:
        row[4] = 1.0
        noise = np.random.normal(NOISE[0], NOISE[1], (radar_count(row),))
    return row, noise


def draw_order_fixture_case(root):
    """Under the fixture's seed __getitem__ makes the reference's decisions: the recorded (flip, noise) flags; the noise vectors bit for bit -- as
    float64 vectors against np.random replayed by hand, and through the only form the reference recorded them in, its float32 radar output:
    (float32)(flipped input + noise) equals it bit for bit, and output - flipped input, the vector recovered in float64, is the drawn one up to
    that one rounding (half an ulp of the output); the arrays returned are the un-augmented inputs."""
    g = fixture()
    paths = write_files(root)
    N = g["image"].shape[0]
    ds = dataset(paths, random_flip=True, rondom_radar_noise=NOISE)
    np.random.seed(int(g["seed"][0]))
    samples = [ds[n] for n in range(N)]
    np.random.seed(int(g["seed"][0]))
    combos = set()
    for n, s in enumerate(samples):
        image, mono, radar, gt, sgt, rcnet, row, noise = s
        assert image.shape == (3,) + g["image"].shape[1:3] and image.dtype == np.float32
        assert np.array_equal(image, np.transpose(g["image"][n].astype(np.float64) / 255.0, (2, 0, 1)).astype(np.float32)), "image %d" % n
        for name, a in zip(MAPS[:4], (mono, radar, gt, sgt)):
            assert a.dtype == np.float32 and np.array_equal(a, _depth(g["in_" + name][n])), (name, n)
        want_rcnet = _depth(g["in_rcnet"][n]) if g["in_rcnet"][n].any() else radar      # :188-190
        assert np.array_equal(rcnet, want_rcnet) and rcnet is not radar
        flip, noisy = recorded_flags(n)
        positives = int((radar > 0).sum())
        if positives:
            assert (bool(row[3]), bool(row[4])) == (flip, noisy), (n, row, flip, noisy)
            combos.add((flip, noisy))
        else:
            assert bool(row[3]) == flip and noise.size == 0      # (no positive pixel: the noise coin leaves no trace in the outputs)
        assert row[0] == 0 and not row[5:].any()
        want_row, want_noise = _replay(lambda r: positives, None, radar.shape)
        assert np.array_equal(row, want_row), (n, row, want_row)
        assert noise.dtype == np.float64 and np.array_equal(noise.view(np.int64), want_noise.view(np.int64)), "noise vector of sample %d" % n
        base = radar[:, ::-1] if row[3] else radar
        valid = base > 0
        out = g["out_radar"][n]
        if row[4]:
            assert noise.size == positives
            assert np.array_equal((base[valid].astype(np.float64) + noise).astype(np.float32).view(np.int32), out[valid].view(np.int32)), n
            recovered = out[valid].astype(np.float64) - base[valid].astype(np.float64)
            assert np.all(np.abs(recovered - noise) <= np.spacing(np.abs(out[valid])).astype(np.float64) / 2), n
        assert np.array_equal(out[~valid], base[~valid])
    assert combos == {(False, False), (False, True), (True, False), (True, True)}, combos


def draw_order_crop_case(root):
    """Hand-written cases for the crop draws on the fixture's files (12 x 20, random_shape (8, 14): d_height 4, d_width 6): the crop coin,
    randint(0, d_width), the ALWAYS-drawn 0.30 coin with randint(0, d_height) on a hit and the centred y_start on a miss, then flip and noise
    coins and the normal() draw of n values, n = positive pixels of the cropped-and-resized radar -- checked against np.random replayed in the
    test and against the float64 restatement's count.  A random_rcnet_thr list draws np.random.choice first.  d_width == 0 raises ValueError."""
    g = fixture()
    paths = write_files(root)
    shape, hw = (8, 14), g["in_radar"].shape[1:]
    seen = set()

    def count(n):
        def f(row):
            if not row[0]:
                return int((g["in_radar"][n] > 0).sum())
            x0, y0 = int(row[1]), int(row[2])
            out, _ = _resize64(_depth(g["in_radar"][n])[y0:y0 + shape[0], x0:x0 + shape[1]], *hw)
            return int((out > 0).sum())
        return f
    for seed in range(12):
        for n in (0, 3, 5):
            ds = dataset(paths, random_shape=shape, random_flip=True, rondom_radar_noise=NOISE)
            np.random.seed(seed)
            row, noise = ds[n][6:]
            state = np.random.get_state()[1].copy()
            np.random.seed(seed)
            want_row, want_noise = _replay(count(n), shape, hw)
            assert np.array_equal(row, want_row), (seed, n, row, want_row)
            assert np.array_equal(noise.view(np.int64), want_noise.view(np.int64)), (seed, n, noise.size, want_noise.size)
            assert np.array_equal(state, np.random.get_state()[1]), "the dataset left np.random in another state than the replay"
            np.random.seed(seed)      # which branches this seed took
            crop = np.random.random() > 0.2
            hit = None
            if crop:
                np.random.randint(low=0, high=6)
                hit = np.random.rand() <= 0.30
                if not hit:
                    assert row[2] == 2, "a missed 0.30 coin centres the window: y_start = d_height // 2"
            seen.add((crop, hit))
    assert seen == {(False, None), (True, True), (True, False)}, seen
    # the rcnet threshold draw comes first (the path keeps its file: 'rcnet_0.x' -> 'rcnet_0.x')
    thr_paths = dict(paths, rcnet=[os.path.join(str(root), "rcnet_0.5_%d.png" % n) for n in range(len(paths["rcnet"]))])
    for a, b in zip(paths["rcnet"], thr_paths["rcnet"]):
        with open(a, "rb") as src, open(b, "wb") as dst:
            dst.write(src.read())
    ds = dataset(thr_paths, random_flip=True, rondom_radar_noise=NOISE, random_rcnet_thr=[0.5])
    np.random.seed(7)
    row, noise = ds[1][6:]
    np.random.seed(7)
    want_row, want_noise = _replay(count(1), None, hw, rcnet_thr=[0.5])
    assert np.array_equal(row, want_row) and np.array_equal(noise, want_noise)
    # d_width == 0: np.random.randint(0, 0) raises, as in the reference
    seed = next(s for s in range(20) if np.random.RandomState(s).random_sample() > 0.2)
    ds = dataset(paths, random_shape=(8, 20), random_flip=True)
    np.random.seed(seed)
    try:
        ds[0]
    except ValueError:
        pass
    else:
        raise AssertionError("d_width == 0 did not raise ValueError")


# ---------------------------------------------------------------------------------------------------------------- 2. fixture parity
def fixture_parity_case(dev, root):
    """collate + augment on the fixture's files under its seed equals the reference's outputs EXACTLY: torch.equal on image, mono, gt, sparse gt
    and rcnet, bit-equal radar.  No overflow is reported."""
    from riders_amd import utv_dataset as U
    g = fixture()
    ds = dataset(write_files(root), random_flip=True, rondom_radar_noise=NOISE)
    np.random.seed(int(g["seed"][0]))
    batch, params, noise, offsets = ds.collate([ds[n] for n in range(len(ds))])
    assert tuple(batch[0].shape) == (len(ds), 3, 12, 20) and all(tuple(t.shape) == (len(ds), 1, 12, 20) for t in batch[1:])
    assert tuple(params.shape) == (len(ds), 8) and offsets.dtype == torch.int32 and noise.dtype == torch.float64 and int(offsets[-1]) == noise.numel()
    out = ds.augment(batch, params, noise, offsets, device=dev)
    U.check_noise_overflow()
    assert torch.equal(out[0].cpu(), torch.from_numpy(np.ascontiguousarray(np.transpose(g["out_image"], (0, 3, 1, 2))))), "image"
    for i, name in enumerate(MAPS):
        want = torch.from_numpy(g["out_" + name])[:, None]
        assert torch.equal(out[i + 1].cpu(), want), name
    assert torch.equal(_bits(out[2].cpu()), _bits(torch.from_numpy(g["out_radar"])[:, None])), "radar bits"
    # without rcnet paths the returned rcnet is the augmented radar
    ds2 = dataset(write_files(root), random_flip=True, rondom_radar_noise=NOISE)
    ds2.rcnet_paths = None
    np.random.seed(int(g["seed"][0]))
    b2, p2, n2, o2 = ds2.collate([ds2[n] for n in range(len(ds2))])
    assert b2[5] is None
    out2 = ds2.augment(b2, p2, n2, o2, device=dev)
    assert out2[5] is out2[2] and torch.equal(_bits(out2[2].cpu()), _bits(out[2].cpu()))


# ---------------------------------------------------------------------------------------------------------------- 3. geometry kernel, direct
def _planes(B, H, W, densities, key):
    """image in [0,1), five maps with the given density of positive pixels (depths 0.5 .. 60, multiples of 1/256 as load_depth gives)"""
    rs = _rs("sml_aug", key, B, H, W)
    image = torch.from_numpy(rs.random_sample((B, 3, H, W)).astype(np.float32))
    maps = []
    for k in range(5):
        dens = np.asarray(densities[k], dtype=np.float64).reshape(-1, 1, 1, 1) * np.ones((B, 1, 1, 1))
        depth = np.floor((0.5 + 59.5 * rs.random_sample((B, 1, H, W))) * 256.0) / 256.0
        maps.append(torch.from_numpy(np.where(rs.random_sample((B, 1, H, W)) < dens, depth, 0.0).astype(np.float32)))
    return [image] + maps


def _nan(dev, n):
    return Buf(dev, n, F32, torch.full((n,), NAN))


def _device_tables(dev, crop_hw, H, W):
    """(xtab, ytab) as the kernel takes them, from the module's host rule"""
    from riders_amd import utv_dataset as U
    tabs = []
    for src, dst in ((crop_hw[1], W), (crop_hw[0], H)):
        s, f = U.bilinear_taps(src, dst)
        s64, _, f64 = _taps64(src, dst)      # the module's table is the documented rule
        assert np.array_equal(s, s64) and np.array_equal(f.astype(np.float64), f64) and f.dtype == np.float32
        tabs.append(torch.from_numpy(np.stack([s.astype(np.float32), f], axis=1).copy()).to(dev))
    return tabs


def _geom(dev, planes, rows, crop_hw, with_rcnet=True, off=0):
    """one rd_sml_augment_geom call on guarded buffers -> list of output tensors (B,C,H,W) on the host; inputs and sentinels checked"""
    B, _, H, W = planes[0].shape
    use = planes if with_rcnet else planes[:5]
    IN = [Buf(dev, t.numel(), F32, t, off=off) for t in use]
    OUT = [_nan(dev, t.numel()) for t in use]
    P = Buf(dev, B * 8, F32, torch.from_numpy(np.asarray(rows, dtype=np.float32)))
    xt = yt = None
    if crop_hw is not None:
        xt, yt = _device_tables(dev, crop_hw, H, W)
    ptr = lambda bufs: [_P(b.v) for b in bufs] + [None] * (6 - len(bufs))      # noqa: E731
    _call("rd_sml_augment_geom", *(ptr(IN) + ptr(OUT) + [B, H, W, _P(P.v), _P(xt), _P(yt)] + (list(crop_hw) if crop_hw else [0, 0]) + [_S(IN[0].v)]))
    what = "sml_augment_geom B=%d %dx%d crop=%s rows=%s" % (B, H, W, crop_hw, np.asarray(rows)[:, :5].tolist())
    for b in IN + [P]:
        b.check(what, unchanged=True)
    for b in OUT:
        b.check(what)
    return [o.cpu().view(t.shape) for o, t in zip(OUT, use)], what


def _check_geom(outs, planes, rows, crop_hw, what):
    for k, got in enumerate(outs):
        g = got.numpy()
        assert np.isfinite(g).all(), what + ": plane %d has unwritten pixels" % k
        for b in range(g.shape[0]):
            for c in range(g.shape[1]):
                want, bound = _expected(planes[k][b, c].numpy(), rows[b], crop_hw)
                if bound is None:
                    assert np.array_equal(g[b, c].view(np.int32), want.astype(np.float32).view(np.int32)), "%s: plane %d sample %d is not the exact copy" % (what, k, b)
                else:
                    err = np.abs(g[b, c].astype(np.float64) - want)
                    assert np.all(err <= bound), "%s: plane %d sample %d error %.3e over the bound %.3e" % (what, k, b, float((err - bound).max()), float(bound.max()))


def _row(crop=None, flip=False, noise=False):
    return [0 if crop is None else 1, 0 if crop is None else crop[0], 0 if crop is None else crop[1], 1 if flip else 0, 1 if noise else 0, 0, 0, 0]


GEOM_SHAPES = ((6, 10), (7, 13), (40, 67), (8, 16), (40, 68))      # W % 4 != 0 and odd H: one pixel per item; the last two: 16-byte vectors


def _crops(H, W):
    """crop sizes per shape: d_width = 1, and a window well inside both ways"""
    return ((H - 2, W - 1), (max(1, (2 * H) // 3), max(1, (3 * W) // 5)))


def geometry_case(dev):
    """rd_sml_augment_geom directly: B = 3 with mixed rows; no crop -> exact copies / flips; crops at x_start 0 and d_width - 1, y_start 0 and
    d_height - 1 (both clamps of both tables fire: asserted) against the float64 restatement within the derived bound; rcnet NULL; a view off
    the 16-byte grid (the one-pixel form on a W that has vectors); equal in / out pointers are refused with a negative code, nothing written."""
    E = _E()
    for H, W in GEOM_SHAPES:
        planes = _planes(3, H, W, [1.0, 0.3, 0.7, 0.1, 0.4], "geom")
        # no crop table at all: the crop flag is not looked at
        rows = [_row(flip=True), _row(), _row(flip=True, noise=True)]
        outs, what = _geom(dev, planes, rows, None)
        _check_geom(outs, planes, rows, None, what)
        for nh, nw in _crops(H, W):
            dh, dw = H - nh, W - nw
            for src, dst in ((nw, W), (nh, H)):
                s1, _, f = _taps64(src, dst)
                if src < dst:
                    assert f[0] == 0 and s1[0] == 0 and s1[-1] == src - 1 and f[-1] == 0 and (f != 0).any(), "both clamps fire"
            sets = [[_row(crop=(0, 0), flip=True), _row(crop=(dw - 1 if dw > 1 else 0, dh - 1), noise=True), _row(flip=True)],
                    [_row(), _row(crop=(dw - 1 if dw > 1 else 0, 0), flip=True), _row(crop=(0, dh - 1))]]
            for i, rows in enumerate(sets):
                outs, what = _geom(dev, planes, rows, (nh, nw), with_rcnet=(i == 0))
                _check_geom(outs, planes, rows, (nh, nw), what)
        if W % 4 == 0:
            rows = [_row(crop=(0, 1), flip=True), _row(flip=True), _row()]
            outs, what = _geom(dev, planes, rows, _crops(H, W)[1], off=1)
            _check_geom(outs, planes, rows, _crops(H, W)[1], what + " misaligned")
    # identity window: the resize of the whole plane is the plane
    planes = _planes(2, 6, 12, [1.0, 0.3, 0.7, 0.1, 0.4], "identity")
    rows = [_row(crop=(0, 0)), _row(crop=(0, 0), flip=True)]
    outs, what = _geom(dev, planes, rows, (6, 12))
    for got, src in zip(outs, planes):
        _exact(what + " identity", got[0], src[0])
        _exact(what + " identity flipped", got[1], torch.flip(src[1], dims=[-1]))
    # aliasing: refused, negative code, nothing written
    lib = E.L()
    B, H, W = 2, 6, 12
    IN = [Buf(dev, t.numel(), F32, t) for t in planes]
    OUT = [_nan(dev, t.numel()) for t in planes]
    P = Buf(dev, B * 8, F32, torch.zeros(B * 8))
    for bad in ([2, 2], [0, 3], None):      # radar_out = radar; gt_out = image; two equal outputs
        ins, outs_ = [_P(b.v) for b in IN], [_P(b.v) for b in OUT]
        if bad is None:
            outs_[1] = outs_[4]
        else:
            outs_[bad[1]] = ins[bad[0]]
        rc = lib.rd_sml_augment_geom(*(ins + outs_ + [B, H, W, _P(P.v), None, None, 0, 0, _S(IN[0].v)]))
        assert rc < 0, "aliasing %s returned %d" % (bad, rc)
        assert lib.rd_last_error_string().decode().startswith("sml_augment_geom: output")
        for b in IN + OUT:
            b.check("sml_augment_geom aliasing refusal", unchanged=True)
    rc = lib.rd_sml_augment_geom(*([_P(b.v) for b in IN] + [_P(b.v) for b in OUT] + [B, H, W, _P(P.v), None, None, 7, 12, _S(IN[0].v)]))
    assert rc < 0 and "does not fit" in lib.rd_last_error_string().decode()


def count_case(dev):
    """Host count equals device mask: for every crop configuration of geometry_case, at radar densities 0, 0.02, 0.3 and 1.0 (one sample each),
    utv_dataset.count_positive_after_crop -- taps and masks only -- equals (radar_out > 0).sum() of the kernel's output, sample by sample."""
    from riders_amd import utv_dataset as U
    for H, W in GEOM_SHAPES:
        planes = _planes(4, H, W, [1.0, [0.0, 0.02, 0.3, 1.0], 0.7, 0.1, 0.4], "count")
        for nh, nw in _crops(H, W):
            dh, dw = H - nh, W - nw
            starts = [(0, 0), (dw - 1 if dw > 1 else 0, dh - 1), (0, dh - 1), (dw - 1 if dw > 1 else 0, dh // 2)]
            for shift in range(2):
                rows = [_row(crop=starts[(b + shift) % 4], flip=bool((b + shift) & 1)) for b in range(4)]
                outs, what = _geom(dev, planes, rows, (nh, nw))
                taps = (U.bilinear_taps(nw, W), U.bilinear_taps(nh, H))
                for b in range(4):
                    host = U.count_positive_after_crop(planes[2][b, 0].numpy(), int(rows[b][2]), int(rows[b][1]), (nh, nw), taps)
                    dev_n = int((outs[2][b] > 0).sum())
                    assert host == dev_n, "%s: sample %d host count %d, device mask %d" % (what, b, host, dev_n)
                assert int((outs[2][0] > 0).sum()) == 0 and int((outs[2][3] > 0).sum()) == H * W


# ---------------------------------------------------------------------------------------------------------------- 4. noise kernel, direct
def _radar(rs, H, W, kind):
    depth = (np.floor((0.5 + 59.5 * rs.random_sample((H, W))) * 256.0) / 256.0).astype(np.float32)
    if kind == "none":
        return np.zeros((H, W), np.float32)
    if kind == "all":
        return depth
    r = np.where(rs.random_sample((H, W)) < (0.3 if kind == "dense" else 0.01), depth, 0).astype(np.float32)
    if kind == "ends":
        r[0, 0], r[-1, -1] = 1.5, 2.25
    return r


def _noise_call(dev, radar, flags, noise, offsets, off=0):
    B, H, W = radar.shape
    R = Buf(dev, radar.size, F32, torch.from_numpy(radar), off=off)
    rows = np.zeros((B, 8), np.float32)
    rows[:, 4] = flags
    P = Buf(dev, B * 8, F32, torch.from_numpy(rows))
    NZ = Buf(dev, max(len(noise), 1), torch.float64, torch.from_numpy(np.asarray(noise, np.float64)) if len(noise) else None)
    OFF = Buf(dev, B + 1, torch.int32, torch.from_numpy(np.asarray(offsets, np.int32)))
    FLAG = Buf(dev, 1, torch.int32, torch.zeros(1, dtype=torch.int32))
    _call("rd_sml_augment_noise", _P(R.v), B, H, W, _P(P.v), _P(NZ.v) if len(noise) else None, _P(OFF.v), len(noise), _P(FLAG.v), _S(R.v))
    what = "sml_augment_noise B=%d %dx%d flags=%s" % (B, H, W, list(flags))
    for b in (P, NZ, OFF):
        b.check(what, unchanged=True)      # the noise buffer's canaries (and values) are intact
    R.check(what); FLAG.check(what)
    return R.cpu().numpy().reshape(B, H, W), int(FLAG.cpu()[0]), what


# H*W: 51 (below a wave) | 2680 (one ragged vector chunk) | 2747 (odd: one pixel per thread, three 1024-pixel chunks, ragged) | 9600 (three
# 4096-pixel vector chunks, ragged) | 33123 (two 32-chunk spans of the one-pixel form) | 132496 (two spans of the vector form)
NOISE_SHAPES = ((3, 17), (40, 67), (41, 67), (96, 100), (181, 183), (364, 364))


def noise_case(dev):
    """rd_sml_augment_noise directly, bit-equal to numpy's radar[radar > 0] += noise on float32: sizes as listed at NOISE_SHAPES; positives at the
    first and the last pixel, none, all, sparse and dense; B = 3 with the middle sample unflagged.  Then the argument errors the kernel handles: an
    offsets row one short -- the last positive pixel unchanged, the flag raised, the value behind the row (a NaN) never used -- and a row one
    long -- every pixel served, the flag raised."""
    for H, W in NOISE_SHAPES:
        big = H * W > 20000
        for kinds in ((("ends", "dense", "all"),) if big else (("ends", "dense", "all"), ("none", "all", "sparse"), ("all", "ends", "none"))):
            rs = _rs("noise", H, W, kinds)
            radar = np.stack([_radar(rs, H, W, k) for k in kinds])
            flags = [1, 0, 1]
            vec, offsets = [], [0]
            for b in range(3):
                if flags[b]:
                    vec.append(rs.normal(NOISE[0], NOISE[1], int((radar[b] > 0).sum())))
                offsets.append(offsets[-1] + (len(vec[-1]) if flags[b] else 0))
            noise = np.concatenate(vec)
            want = radar.copy()
            for b in range(3):
                if flags[b]:
                    want[b][want[b] > 0] += noise[offsets[b]:offsets[b + 1]]
            got, flag, what = _noise_call(dev, radar, flags, noise, offsets)
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), "%s %s: %d pixels differ" % (what, kinds, int((got != want).sum()))
            assert flag == 0, what
            assert np.array_equal(got[1], radar[1])
    for H, W, off in ((3, 17, 0), (41, 67, 0), (96, 100, 0), (40, 68, 1)):
        rs = _rs("noise short", H, W)
        radar = np.stack([_radar(rs, H, W, "dense"), _radar(rs, H, W, "ends")])
        n0, n1 = int((radar[0] > 0).sum()), int((radar[1] > 0).sum())
        noise = rs.normal(NOISE[0], NOISE[1], n0 + n1)
        # one short: the last sample's row ends one value early; the value behind it is inside the buffer, belongs to nobody and is a NaN
        short = np.concatenate([noise[:-1], [NAN]])
        got, flag, what = _noise_call(dev, radar, [1, 1], short, [0, n0, n0 + n1 - 1], off=off)
        want = radar.copy()
        want[0][want[0] > 0] += noise[:n0]
        idx = np.flatnonzero(want[1].reshape(-1) > 0)
        want[1].reshape(-1)[idx[:-1]] += noise[n0:n0 + n1 - 1]
        assert flag == 1, what + ": a row one short must raise the flag"
        assert np.isfinite(got).all(), what + ": the value behind the row was used"
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), what + ": one short"
        assert got[1, -1, -1] == radar[1, -1, -1], what + ": the last positive pixel must stay as it was"
        # rows of the right length on the same data: no flag
        got, flag, what = _noise_call(dev, radar, [1, 1], noise, [0, n0, n0 + n1], off=off)
        assert flag == 0, what
        # one long (the host counted a pixel the device does not have): every pixel served, flag raised
        got, flag, what = _noise_call(dev, radar[:1], [1], noise[:n0 + 1], [0, n0 + 1], off=off)
        want = radar[:1].copy()
        want[0][want[0] > 0] += noise[:n0]
        assert flag == 1 and np.array_equal(got.view(np.int32), want.view(np.int32)), what + ": one long"


# ---------------------------------------------------------------------------------------------------------------- 5. wrapper: out=, refusals
def _collated(B, H, W, random_shape, key):
    """a collated batch built by hand (no files): mixed rows, host-counted noise"""
    from riders_amd import utv_dataset as U
    planes = _planes(B, H, W, [1.0, 0.1, 0.7, 0.1, 0.4], key)
    rs = _rs("collated", key)
    rows, vec, offsets = [], [], [0]
    for b in range(B):
        crop = None
        if random_shape is not None and b % 2 == 0:
            crop = (int(rs.randint(0, W - random_shape[1])), int(rs.randint(0, H - random_shape[0])))
        rows.append(_row(crop=crop, flip=bool(b % 3 == 0), noise=bool(b % 2 == 0 or b == 1)))
        n = 0
        if rows[-1][4]:
            radar = planes[2][b, 0].numpy()
            n = (U.count_positive_after_crop(radar, crop[1], crop[0], random_shape, (U.bilinear_taps(random_shape[1], W), U.bilinear_taps(random_shape[0], H)))
                 if crop else int((radar > 0).sum()))
            vec.append(rs.normal(NOISE[0], NOISE[1], n))
        offsets.append(offsets[-1] + n)
    noise = torch.from_numpy(np.concatenate(vec)) if vec else torch.zeros(0, dtype=torch.float64)
    return tuple(planes), torch.tensor(rows, dtype=torch.float32), noise, torch.tensor(offsets, dtype=torch.int32)


def _raises(exc, text, fn):
    try:
        fn()
    except exc as e:
        assert text in str(e), (text, str(e))
    else:
        raise AssertionError("expected %s(%r)" % (exc.__name__, text))


def static_batch_case(dev):
    """augment(..., out=tensors) fills the given tensors with the bits the allocating call returns (crop, flip and noise mixed; 32 x 64 and a
    W without vectors); the radar equals numpy's noise on the geometry's output; wrong shapes, dtypes, counts and overlapping tensors raise; a
    short offsets row is reported once by check_noise_overflow()."""
    from riders_amd import utv_dataset as U
    for (H, W), shape in (((32, 64), (20, 48)), ((9, 14), None)):
        batch, params, noise, offsets = _collated(4, H, W, shape, "static")
        fresh = U.augment(batch, params, noise, offsets, random_shape=shape, device=dev)
        U.check_noise_overflow()
        static = tuple(torch.full_like(t, NAN).to(dev) for t in batch)
        ret = U.augment(batch, params, noise, offsets, out=static, random_shape=shape)
        U.check_noise_overflow()
        for a, b, c in zip(fresh, static, ret):
            assert c is b and torch.equal(_bits(a.cpu()), _bits(b.cpu()))
        # the radar: numpy's noise on the zero-noise geometry
        quiet = params.clone(); quiet[:, 4] = 0
        geo = U.augment(batch, quiet, torch.zeros(0, dtype=torch.float64), torch.zeros(5, dtype=torch.int32), random_shape=shape, device=dev)
        want = geo[2].cpu().numpy().copy()
        for b in range(4):
            if params[b, 4]:
                want[b][want[b] > 0] += noise.numpy()[int(offsets[b]):int(offsets[b + 1])]
        assert np.array_equal(want.view(np.int32), fresh[2].cpu().numpy().view(np.int32))
        for k in (0, 1, 3, 4, 5):
            assert torch.equal(_bits(geo[k].cpu()), _bits(fresh[k].cpu()))
        # refusals
        dbatch = tuple(t.to(dev) for t in batch)
        _raises(ValueError, "does not match", lambda: U.augment(batch, params, noise, offsets, out=tuple(t[:, :, :-1].contiguous() for t in static), random_shape=shape))
        _raises(ValueError, "out has 5", lambda: U.augment(batch, params, noise, offsets, out=static[:5], random_shape=shape))
        _raises(ValueError, "contiguous float32", lambda: U.augment(batch, params, noise, offsets, out=tuple(t.double() for t in static), random_shape=shape))
        _raises(ValueError, "overlaps", lambda: U.augment(dbatch, params, noise, offsets, out=dbatch, random_shape=shape))
        _raises(ValueError, "overlaps", lambda: U.augment(dbatch, params, noise, offsets, out=static[:2] + (dbatch[2],) + static[3:], random_shape=shape))
        _raises(ValueError, "overlaps", lambda: U.augment(dbatch, params, noise, offsets, out=static[:4] + (static[3], static[5]), random_shape=shape))
        _raises(ValueError, "do not belong", lambda: U.augment(batch, params[:3], noise, offsets, random_shape=shape, device=dev))
        if shape is not None:
            _raises(ValueError, "no random_shape", lambda: U.augment(batch, params, noise, offsets, device=dev))
        # a short row: reported, once
        bad = offsets.clone(); bad[1:] -= 1
        U.augment(batch, params, noise[:-1], bad, random_shape=shape, device=dev)
        _raises(RuntimeError, "differs from the length of its row", U.check_noise_overflow)
        U.check_noise_overflow()


def graphed_step_case(dev):
    """GPU only: a GraphedTrainStep captured at B = 2, 32 x 64 in fp32 is fed by augment(..., out=step.static_batch) -- no load_batch copy -- and
    replayed once: its loss equals the eager forward_loss on the (separately allocated) augmented batch bit for bit."""
    from riders_amd import sml_main
    from riders_amd import utv_dataset as U
    from riders_amd.optim import FlatAdam
    cfg = sml_main.ZJU_SML_CONFIG
    shape = (24, 48)
    batch, params, noise, offsets = _collated(2, 32, 64, shape, "graphed")
    torch.manual_seed(0)
    m = sml_main.build_model(dev)
    m.train()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    aug = U.augment(batch, params, noise, offsets, random_shape=shape, device=dev)
    eager = float(sml_main.forward_loss(m, aug, cfg, sml_main.make_outlier_removal(cfg)).detach())
    torch.manual_seed(0)
    m2 = sml_main.build_model(dev)
    m2.train()
    m2.load_state_dict(sd)
    opt = FlatAdam(m2.parameters(), lr=1e-4)
    step = sml_main.GraphedTrainStep(m2, opt, sml_main.synthetic_batch(2, 32, 64, seed=5, device=dev), cfg, outlier=sml_main.make_outlier_removal(cfg), warmup=1)
    ret = U.augment(batch, params, noise, offsets, out=step.static_batch, random_shape=shape)
    assert all(a is b for a, b in zip(ret, step.static_batch))
    graphed = float(step().detach())
    U.check_noise_overflow()
    print("sml augment -> static batch: eager loss %r, replayed loss %r" % (eager, graphed))
    assert np.isfinite(eager) and graphed == eager, (graphed, eager)
