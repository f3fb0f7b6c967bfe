"""Scale-Map-Learner training samples with the reference's augmentation: same class name and constructor arguments (its spellings included)
as data/UTV_dataset.py UTV_dataset (:124-225), as configured by train_zju.py:451-456 / train_ntu.py (random_flip, rondom_radar_noise;
random_shape parked in a comment there).

The reference augments every sample on the host: crop + cv2.resize back (:20-120), np.flip of six arrays (:202-209), a boolean-mask
add of np.random.normal (:212-217).  Here __getitem__ only LOADS the six arrays and DRAWS the sample's decisions, from the global np.random in
the reference's order -- np.random.choice (rcnet threshold), the crop coin `random() > 0.2`, randint(0, d_width), the always-drawn
`rand() <= 0.30` with randint(0, d_height) on a hit, the flip coin `random() > 0.5`, the noise coin `random() > 0.5` and
normal(noise[0], noise[1], n) -- and the arithmetic of a whole batch is two launches (`augment`: rd_sml_augment_geom, rd_sml_augment_noise).
A run seeded like a run of the reference makes the same decisions and, without a crop, returns the same bits (fixture g19, written by the
reference class itself).  n, the number of positive radar pixels AFTER crop and flip, is needed for the normal() draw and is computed on the
host without touching the device: the flip preserves it, and a cropped output pixel is positive iff a tap with a non-zero float32 weight lands
on a positive source pixel (depth maps are non-negative: load_depth clears z <= 0) -- a separable mask operation on the host tap tables the
kernel is handed.  Should host and device ever disagree, rd_sml_augment_noise reads nothing out of range and raises a sticky flag that
`check_noise_overflow()` reports.

cv2 is not part of the build image, so the bilinear resize is third-party arithmetic that cannot be pinned bit for bit;
it is restated (`bilinear_taps`): scale = 1 / (dst / src) in double, f = (float)((d + 0.5) * scale - 0.5), s = floor(f), f -= s, s < 0 ->
(0, 0), s >= src - 1 -> (src - 1, 0), weights 1.f - f and f, horizontal pass then vertical pass in float32, src = the crop window.

Not reproduced: with rcnet_paths=None the reference's rcnet IS its radar array, so the noise lands in both when neither crop nor flip made a
copy and in the radar alone otherwise; here the returned rcnet is always the augmented (noisy) radar tensor itself.  Multi-worker seeding is
the caller's, as in the reference.  This module imports numpy only; torch and the HIP library are touched by collate / augment.
"""
import numpy as np

from . import data_utils

N_PARAMS = 8      # (do_crop, x_start, y_start, do_flip, do_noise, 0, 0, 0): one row per sample, read by the kernels


def bilinear_taps(src, dst):
    """cv2.resize INTER_LINEAR's per-axis table restated -> (first tap int32[dst], weight of the second tap float32[dst])."""
    scale = 1.0 / (float(dst) / float(src))
    f = ((np.arange(dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f)
    f = (f - s).astype(np.float32)
    s = s.astype(np.int64)
    low, high = s < 0, s >= src - 1
    s = np.where(low, 0, np.where(high, src - 1, s))
    f = np.where(low | high, np.float32(0), f).astype(np.float32)
    return s.astype(np.int32), f


def _tap_or(mask, s, f, src, axis):
    """out[d] = mask[s[d]] | (f[d] != 0 & mask[min(s[d] + 1, src - 1)]) along `axis`: where one pass of the resize can be non-zero"""
    first = np.take(mask, s, axis=axis)
    second = np.take(mask, np.minimum(s + 1, src - 1), axis=axis)
    shape = [1, 1]
    shape[axis] = -1
    return first | (second & (f != 0).reshape(shape))


def count_positive_after_crop(radar, y_start, x_start, crop_hw, taps):
    """number of positive pixels of resize(radar[window]) without computing it (module docstring)"""
    nh, nw = crop_hw
    (sx, fx), (sy, fy) = taps
    win = radar[y_start:y_start + nh, x_start:x_start + nw] > 0
    return int(np.count_nonzero(_tap_or(_tap_or(win, sx, fx, nw, 1), sy, fy, nh, 0)))


def draw_crop(shape, crop_hw):
    """random_crop(crop_type=['horizontal', 'vertical']) :35-102 -> (x_start, y_start); raises ValueError when d_width <= 0, as randint does there"""
    d_height, d_width = shape[0] - crop_hw[0], shape[1] - crop_hw[1]
    x_start = np.random.randint(low=0, high=d_width)
    y_start = d_height // 2
    if np.random.rand() <= 0.30:
        y_start = np.random.randint(low=0, high=d_height)
    return int(x_start), int(y_start)


class UTV_dataset(object):
    """data/UTV_dataset.py:124-225 (a torch.utils.data.Dataset there; any indexable works with torch's DataLoader, `collate_fn=dataset.collate`).
    __getitem__ -> (image (3,H,W), mono (H,W), radar, gt, sparse_gt, rcnet or None, params float32[8], noise float64[n]): the UN-augmented
    float32 arrays, the sample's decisions and its noise vector (empty unless the noise coin fell)."""

    def __init__(self, image_paths, mono_pred_paths, radar_paths, gt_paths, sparse_gt_paths, rcnet_paths=None, random_shape=None,
                 random_flip=False, rondom_radar_noise=None, random_rcnet_thr=None):
        self.n_sample = len(image_paths)
        for paths in [image_paths, mono_pred_paths, radar_paths, gt_paths, sparse_gt_paths]:
            assert len(paths) == self.n_sample
        if rcnet_paths is not None:
            assert len(rcnet_paths) == self.n_sample
        self.image_paths, self.mono_pred_paths, self.radar_paths = image_paths, mono_pred_paths, radar_paths
        self.gt_paths, self.sparse_gt_paths, self.rcnet_paths = gt_paths, sparse_gt_paths, rcnet_paths
        self.random_shape = random_shape
        self.random_flip = random_flip
        self.rondom_radar_noise = rondom_radar_noise
        self.random_rcnet_thr = random_rcnet_thr
        self._taps = {}

    def __len__(self):
        return self.n_sample

    def taps(self, H, W):
        """host tap tables ((sx, fx), (sy, fy)) of the configured crop size at (H, W), computed once"""
        key = (H, W)
        if key not in self._taps:
            nh, nw = self.random_shape
            self._taps[key] = (bilinear_taps(nw, W), bilinear_taps(nh, H))
        return self._taps[key]

    def __getitem__(self, index):
        image = data_utils.load_image(self.image_paths[index], normalize=True, data_format='CHW')
        mono_pred = data_utils.load_depth(self.mono_pred_paths[index])
        if self.radar_paths[index].endswith('.npy'):      # :161-168: n x 3 (u, v, depth) -> depth_map[v, u] = depth, later rows overwrite
            points = np.load(self.radar_paths[index])
            radar = np.zeros_like(mono_pred)
            for i in range(points.shape[0]):
                radar[int(points[i, 1]), int(points[i, 0])] = points[i, 2]
        else:
            radar = data_utils.load_depth(self.radar_paths[index])
        gt = data_utils.load_depth(self.gt_paths[index])
        sparse_gt = data_utils.load_depth(self.sparse_gt_paths[index])
        image, mono_pred, radar, gt, sparse_gt = [np.ascontiguousarray(T, dtype=np.float32) for T in (image, mono_pred, radar, gt, sparse_gt)]
        rcnet = None
        if self.rcnet_paths is not None:
            if self.random_rcnet_thr is not None:             # :183-186: the path is rewritten in place, as there
                cur_thr = self.rcnet_paths[index].split('rcnet_')[-1][:3]
                rcnet_thr = np.random.choice(self.random_rcnet_thr)
                self.rcnet_paths[index] = self.rcnet_paths[index].replace(cur_thr, str(rcnet_thr))
            rcnet = data_utils.load_depth(self.rcnet_paths[index])
            if rcnet.sum() == 0:                              # :188-190
                rcnet = radar
            rcnet = np.array(rcnet, dtype=np.float32)         # (astype: a copy, also of the radar)
        H, W = mono_pred.shape
        params = np.zeros(N_PARAMS, dtype=np.float32)
        n_positive = None
        if self.random_shape is not None:
            if np.random.random() > 0.2:
                x_start, y_start = draw_crop((H, W), self.random_shape)
                params[0], params[1], params[2] = 1.0, x_start, y_start
                n_positive = lambda: count_positive_after_crop(radar, y_start, x_start, self.random_shape, self.taps(H, W))      # noqa: E731
        if self.random_flip:
            if np.random.random() > 0.5:
                params[3] = 1.0
        noise = np.zeros(0, dtype=np.float64)
        if self.rondom_radar_noise is not None:
            if np.random.random() > 0.5:
                params[4] = 1.0
                n = n_positive() if n_positive is not None else int(np.count_nonzero(radar > 0))
                noise = np.random.normal(self.rondom_radar_noise[0], self.rondom_radar_noise[1], (n,))
        return image, mono_pred, radar, gt, sparse_gt, rcnet, params, noise

    def collate(self, samples):
        return collate(samples)

    def augment(self, batch, params, noise, offsets, out=None, device=None):
        return augment(batch, params, noise, offsets, out=out, random_shape=self.random_shape, device=device)


def collate(samples):
    """list of __getitem__ results -> (batch, params, noise, offsets): batch = the six host tensors sml_main takes, image (B,3,H,W) and the
    rest (B,1,H,W) (rcnet None when the dataset has no rcnet paths), params (B,8) float32, noise = the samples' vectors back to back (float64),
    offsets int32 (B+1) into it.  `augment(*collate(samples))`."""
    import torch
    cols = list(zip(*samples))
    image = torch.from_numpy(np.stack(cols[0]))
    maps = [torch.from_numpy(np.stack(c)[:, None]) for c in cols[1:5]]
    rcnet = None if cols[5][0] is None else torch.from_numpy(np.stack(cols[5])[:, None])
    params = torch.from_numpy(np.stack(cols[6]).astype(np.float32))
    lens = [len(v) for v in cols[7]]
    noise = torch.from_numpy(np.concatenate(cols[7]).astype(np.float64)) if sum(lens) else torch.zeros(0, dtype=torch.float64)
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32))
    return (image, maps[0], maps[1], maps[2], maps[3], rcnet), params, noise, offsets


_tap_cache = {}       # (crop_h, crop_w, H, W, device) -> (xtab (W,2), ytab (H,2)) float32 on the device, uploaded once
_noise_flags = {}     # device -> sticky int32 flag of rd_sml_augment_noise


def _device_taps(crop_hw, H, W, dev):
    import torch
    key = (int(crop_hw[0]), int(crop_hw[1]), H, W, str(dev))
    if key not in _tap_cache:
        (sx, fx), (sy, fy) = bilinear_taps(key[1], W), bilinear_taps(key[0], H)
        _tap_cache[key] = tuple(torch.from_numpy(np.stack([s.astype(np.float32), f], axis=1).copy()).to(dev) for s, f in ((sx, fx), (sy, fy)))
    return _tap_cache[key]


def _noise_flag(dev):
    import torch
    f = _noise_flags.get(str(dev))
    if f is None:
        f = _noise_flags[str(dev)] = torch.zeros(1, dtype=torch.int32, device=dev)
    return f


def check_noise_overflow():
    """Host-side check of rd_sml_augment_noise's sticky flag (synchronises; call it where the host waits anyway, as engine.check_roi_overflow):
    raises, once, if a flagged sample's positive radar pixels on the device were not as many as the noise values drawn for it on the host --
    its surplus pixels were left without noise, nothing was read out of range."""
    bad = [k for k, f in _noise_flags.items() if int(f.cpu()[0])]
    for k in bad:
        _noise_flags[k].zero_()
    if bad:
        raise RuntimeError("riders_amd: rd_sml_augment_noise found a sample whose number of positive radar pixels differs from the length of its "
                           "row of noise values (host count and device mask disagree, or the offsets do not match the batch)")


def _overlap(a, b):
    lo_a, lo_b = a.data_ptr(), b.data_ptr()
    return lo_a < lo_b + b.numel() * b.element_size() and lo_b < lo_a + a.numel() * a.element_size()


def augment(batch, params, noise, offsets, out=None, random_shape=None, device=None):
    """Crop / flip / radar noise of a collated batch in two launches on the current stream -> (image, mono, radar, gt, sparse_gt, rcnet).
    Host tensors are copied to `device` (default: the device of `out`, else the current ROCm device) first.  out: six float32 tensors to write
    into -- `step.static_batch` of an sml_main.GraphedTrainStep, so that the augmentation replaces load_batch's copy instead of preceding it;
    shapes and dtypes are checked as GraphedStep.load_batch checks them, and an output that overlaps an input is refused.  Without an rcnet map
    (rcnet_paths=None) the returned rcnet is the augmented radar tensor itself and out[5] is left untouched."""
    import torch
    from . import engine
    if len(batch) != 6:
        raise ValueError("augment: %d tensors, a Scale Map Learner batch has 6" % len(batch))
    if out is not None and len(out) != 6:
        raise ValueError("augment: out has %d tensors, a Scale Map Learner batch has 6" % len(out))
    if device is None:
        if out is not None:
            device = out[0].device
        elif batch[0].is_cuda or engine._lib.ALLOW_HOST_POINTERS:
            device = batch[0].device
        else:
            device = torch.device("cuda", torch.cuda.current_device())
    dev = torch.device(device)

    def put(t, dtype):
        if t.dtype != dtype:
            raise ValueError("augment: %s tensor where %s is expected" % (t.dtype, dtype))
        t = t.to(dev, non_blocking=True)
        return t if t.is_contiguous() else t.contiguous()
    ins = [None if t is None else put(t, torch.float32) for t in batch]
    if any(t is None for t in ins[:5]):
        raise ValueError("augment: only the rcnet map may be None")
    B, C, H, W = ins[0].shape
    if C != 3:
        raise ValueError("augment: image shape %s, expected (B,3,H,W)" % (tuple(ins[0].shape),))
    for t in ins[1:]:
        if t is not None and tuple(t.shape) != (B, 1, H, W):
            raise ValueError("augment: map shape %s next to image shape %s" % (tuple(t.shape), tuple(ins[0].shape)))
    params_host = params if not params.is_cuda else None
    params, noise, offsets = put(params, torch.float32), put(noise, torch.float64), put(offsets, torch.int32)
    if tuple(params.shape) != (B, N_PARAMS) or tuple(offsets.shape) != (B + 1,) or noise.dim() != 1:
        raise ValueError("augment: params %s / offsets %s / noise %s do not belong to a batch of %d" % (tuple(params.shape), tuple(offsets.shape),
                                                                                                      tuple(noise.shape), B))
    if random_shape is None and params_host is not None and bool((params_host[:, 0] != 0).any()):
        raise ValueError("augment: a sample asks for a crop but no random_shape was given")
    if out is None:
        outs = [None if t is None else torch.empty_like(t) for t in ins]
    else:
        outs = list(out)
        if ins[5] is None:
            outs[5] = None
        for dst, src in zip(outs, ins):
            if src is None:
                continue
            if dst is None or tuple(dst.shape) != tuple(src.shape):
                raise ValueError("augment: out shape %s does not match the batch's %s (a hipGraph replays fixed shapes)" % (
                    None if dst is None else tuple(dst.shape), tuple(src.shape)))
            if dst.dtype != torch.float32 or not dst.is_contiguous() or dst.device != src.device:
                raise ValueError("augment: out tensors are contiguous float32 tensors on the batch's device")
    live_in, live_out = [t for t in ins if t is not None], [t for t in outs if t is not None]
    for i, o in enumerate(live_out):
        if any(_overlap(o, t) for t in live_in) or any(_overlap(o, t) for t in live_out[:i]):
            raise ValueError("augment: an output tensor overlaps an input or another output (the flip reads a row's far end after its near end was written)")
    lib, p_, st = engine.L(), engine._p, engine._stream(ins[0])
    xtab = ytab = None
    nh = nw = 0
    if random_shape is not None:
        nh, nw = int(random_shape[0]), int(random_shape[1])
        xtab, ytab = _device_taps((nh, nw), H, W, dev)
    engine._chk(lib.rd_sml_augment_geom(*([p_(t) for t in ins] + [p_(t) for t in outs] + [B, H, W, p_(params), p_(xtab), p_(ytab), nh, nw, st])),
                "rd_sml_augment_geom")
    engine._chk(lib.rd_sml_augment_noise(p_(outs[2]), B, H, W, p_(params), p_(noise) if noise.numel() else None, p_(offsets), noise.numel(),
                                         p_(_noise_flag(dev)), st), "rd_sml_augment_noise")
    if outs[5] is None:
        outs[5] = outs[2]
    return tuple(outs)
