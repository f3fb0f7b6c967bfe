"""Direct parity cases for the remaining kernels of rd_dwconv.hip: the depthwise forward, data gradient and weight gradient (rd_dwconv_fwd,
rd_dwconv_dgrad, rd_dwconv_wgrad, rd_dwconv_wgrad_partial + rd_dw_wgrad_finalize_batch), rd_bilinear_fwd / _bwd at ratios other than 2,
rd_sml_head_fwd / _bwd and rd_reciprocal, and the argument checks of the depthwise and bilinear entry points.  Harness and bound as
tests/parity_cases_glue.py and tests/parity_cases_bn.py (imported, not copied): every kernel through the C ABI, every buffer a kernel writes a
`Buf` with sentinels on both sides, outputs prefilled with NaN, inputs checked unchanged, references plain float64 torch on the values the kernel
receives, `_check` with torch's own fp32 CPU result of the same expression as the yardstick.  No tolerance constant is added here.

Depthwise route classes (asserted per case through rd_dwconv_stats_rows, so a routing change cannot silently empty a class):
  quad   C % 4 == 0, k in {3, 5}, s in {1, 2}: dw_run_kernel (forward; MODE 1 = the stride-1 data gradient), dw_dgrad2_kernel (stride-2 data
         gradient, both pad parities: k = 3 on an even size gives p = 0, k = 5 on an even size p = 1, odd sizes p = 1 and p = 2),
         dw_wgrad_run_kernel + dw_wgrad_finalize_tc_kernel.  C = 12 is 3 quads; C = 260 is 65 quads, which qgeom() turns into 65 channel
         chunks of one quad (QB = 1 whenever C / 4 <= 256 does not divide 256); C = 1028 (257 quads, prime) is the smallest count whose best
         geometry has a SHORT last chunk (129 chunks of 2 quads, the last of 1: the `min(QB, C / 4 - blockIdx.y * QB)` of the weight staging).
  scalar everything else: dwconv_fwd_kernel, dwconv_dgrad_kernel, dwconv_wgrad_kernel<KK = 9 / 25> with the `j < k * k` guard (k = 1, 2, 4),
         dwconv_wgrad_finalize_kernel.

quick=True (the emulator twin) runs a covering selection (`_cover`: every (class, k, s, pad parity, dtype), every channel count per k, every
geometry per stride); the GPU twin runs the cross products and one size past each launcher clamp:
  ew_grid's 4096 blocks: the scalar depthwise forward / data gradient at 2 x 300 x 300 x 6, the bilinear kernels (vector form 2 x 64 x 64 x 260
  -> 128 x 128, scalar form 2 x 300 x 300 x 3 -> 600 x 600, and the mirror of each: the backward's grid runs over the source), the head and the reciprocal at 4096 * 256 + 777 elements;
  gx of launch_dwconv_wgrad = min(512 / nchunk, ceil(units / (3 PL)), max(64, pixels / 32), rows), observed as the item.rows that
  rd_dwconv_wgrad_partial returns (WGRAD_CLAMPS holds the expected count as a literal with the arithmetic beside it):
    512 / nchunk binds at 1 x 148 x 148 x 260 (7 of 8 / 21904 / 343), ceil(units / (3 PL)) at 2 x 40 x 52 x 36 (2 of 56 / 130 / 17, also in
    the quick selection), rows at 1 x 64 x 64 x 512 (64 of 512 / 171 / 128);
    max(64, pixels / 32) can NOT bind and has no case: rows <= ceil(pixels / 64), which is <= 64 while pixels <= 4096 and <= pixels / 32 above
    that, so the `rows` clamp that follows is never the larger of the two;
  the finalize-batch grid cap of 1024 blocks: C = 2624, k = 5 (C k k / 64 = 1025).

The batch case makes 86 rd_dwconv_wgrad_partial calls: 85 cycle over five shapes, one of them scalar (item.rows == 0, dw final at once), so
that 68 items are pending -- more than DW_WGRAD_BATCH_MAX = 64 AFTER the scalar ones are taken out (70 calls would leave 56 and one launch) --
and one has 33 partial rows (the eight-rows-in-flight loop of the batch kernel steps by 32).  dw must equal rd_dwconv_wgrad's bit for bit.

Finding: the weight gradients' documented summation structure is less accurate than torch's fp32, and a correct kernel then misses _check's
bound on some data.  A block of dw_wgrad_run_kernel gives each of its PL (up to 256) pixel lanes every PL-th run of 4 pixels, and adds the lanes'
fp32 totals one after the other in fp32 before the rows go on in float64; dwconv_wgrad_kernel does the same per pixel.  On bf16 2 x 40 x 52, C = 4,
k = 5, s = 2 (one block, 256 lanes of <= 8 pixels) dw is 6.26e-5 from float64 at max|ref| 106.7 -- 5.9e-7 of it, 4.9 fp32 ulp -- where torch's
fp32 is 8.8e-6 off, so the bound is its floor, 4 ulp = 5.09e-5, and the kernel is outside it; the same shape on other random data is inside.
Nothing is wrong with the kernel and no constant is widened: as for the BatchNorm conditioning case, the fp32 yardstick of the weight gradient
is a restatement of that documented structure (`_wgrad_restated`: per-lane fp32 accumulation, lanes added in lane order in fp32, rows in
float64), written from the comments above the kernels and the launcher's arithmetic, not from what the kernels return.  Against it the same case
has kernel error 6.26e-5, restatement error 6.26e-5, bound 2.5e-4.  (The restatement turned out to reproduce the kernels' error figures to
every printed digit, on the emulator and on the MI355X.)  torch's own fp32 error on the same gradients is printed beside the table by report_dw().

Measured (relative to max|ref|, fp32 outputs; in brackets the fp32 yardstick's own error against float64: torch's fp32 CPU result, for the weight
gradients the restatement; 16-bit outputs sit within their half ulp, at most 3.8e-3):
  emulator (the covering selection): depthwise quad fwd 2.9e-7 (2.9e-7), dgrad 2.4e-7 (2.4e-7), wgrad 5.9e-7 (5.9e-7), batch 9.9e-8 (9.9e-8); scalar fwd
            2.3e-7 (2.2e-7), dgrad 2.2e-7 (2.2e-7), wgrad 2.4e-7 (2.4e-7), batch 1.8e-7 (1.8e-7); torch fp32 on the weight gradients 1.2e-6;
            bilinear vec fwd 2.5e-7 (2.6e-7), bwd 2.4e-7 (2.7e-7), scalar fwd 2.7e-7 (3.2e-7), bwd 2.3e-7 (2.3e-7); head fwd 8.0e-8 (8.0e-8),
            bwd 4.3e-8 (4.3e-8); reciprocal fwd 4.7e-8 (4.7e-8), bwd 7.8e-8 (7.8e-8)
  MI355X (the cross products and the clamp sizes): depthwise quad fwd 2.9e-7 (2.9e-7), dgrad 2.4e-7 (2.4e-7), wgrad 6.3e-7 (6.3e-7), batch 9.9e-8 (9.9e-8);
            scalar fwd 2.4e-7 (6.8e-7), dgrad 2.2e-7 (2.2e-7), wgrad 2.7e-7 (2.7e-7), batch 1.8e-7 (1.8e-7); torch fp32 on the weight gradients 4.8e-6;
            bilinear vec fwd 3.2e-6 (3.2e-6), bwd 3.4e-6 (3.4e-6), scalar fwd 7.6e-5 (7.6e-5), bwd 6.7e-5 (6.7e-5) -- the large figures are the
            sizes past the grid cap: the source coordinate is taken in fp32, by ATen as by the kernel, and at 600 columns one fp32 ulp of it
            is 3e-5 of a pixel; the 2 ... 20-pixel cases stay at 3e-7; head fwd 1.1e-7 (1.1e-7), bwd 4.3e-8 (4.3e-8); reciprocal fwd 4.8e-8 (4.8e-8),
            bwd 7.8e-8 (7.8e-8)
"""
import ctypes

import numpy as np
import torch
import torch.nn.functional as F

from tests.parity_cases import bf16_mode
from tests.parity_cases_bn import DT, _cover, _nanbuf, _same_pad
from tests.parity_cases_glue import BF16, F16, F32, MEASURED, Buf, _call, _check, _E, _exact, _P, _r, _randn, _refused, _rs, _S

DTYPES = (F32, BF16)
CLASSES = ("quad", "scalar")
QUAD_C, SCALAR_C = (4, 12, 36, 64, 256, 260, 1028), (1, 3, 6)
WIDE_C = 260                                                                      # from here on: the two small geometries only
SMALL_GEOMS = ((1, 1, 1), (1, 1, 5), (1, 2, 2), (1, 3, 2))                        # smaller than the window: every source column clamped
GEOMS = SMALL_GEOMS + ((2, 5, 9), (1, 8, 10), (2, 40, 52))                        # ragged last run of 4 columns, odd / even; several blocks
WIDE_GEOMS = ((2, 5, 9), (1, 8, 10))
SCALAR_ODD_K = ((8, 1, 1), (8, 2, 1), (8, 4, 1), (8, 3, 3))                       # (C, k, s): the KK = 9 / 25 templates with k * k < KK; stride 3
# (C, (N, H, W), k, s): 65 partial rows of one pixel lane (dwconv_wgrad_finalize_kernel strides by 64); two channel chunks with a short last one
SCALAR_WIDE = ((130, (2, 40, 52), 3, 1), (258, (2, 5, 9), 5, 2))
GROUPS = ("dw ", "bilinear ", "sml_head ", "reciprocal ")
TORCH_WGRAD = [0.0]      # torch's own fp32 error on the weight gradients, relative to max|ref| (reported only: see _wgrad_restated)


def report_dw():
    for k in sorted(MEASURED):
        if k.startswith(GROUPS):
            print("dw parity %-28s %s error %.3e   kernel error %.3e   (relative to max|ref|)" % (
                k, "restated fp32" if "wgrad" in k else "torch fp32   ", MEASURED[k][0], MEASURED[k][1]))
    print("dw parity torch fp32's own error on the weight gradients %.3e" % TORCH_WGRAD[0])


def _item():
    from riders_amd import _lib
    return _lib.DwWgradItem()


def _class_of(N, OH, OW, C, k, s):
    """the route the library takes, and the documented condition it must equal"""
    rows = _E().L().rd_dwconv_stats_rows(N, OH, OW, C, k, s)
    quad = C % 4 == 0 and k in (3, 5) and s in (1, 2)
    assert (rows > 0) == quad, "C=%d k=%d s=%d: rd_dwconv_stats_rows says %d, the documented condition says %s" % (C, k, s, rows, quad)
    return "quad" if rows > 0 else "scalar"


def _geometry(H, W, k, s, pad=None):
    """((ph, OH, total), (pw, OW, total)) of TF-SAME, or None where the two leading pads differ (the C ABI has one p).  pad: torch's symmetric
    padding instead, OH = (H + 2 pad - k) // s + 1 (engine.dwconv_block without out_hw); `total` - pad is what the last window reaches past
    the map (negative: trailing rows / columns that no window reads, which F.pad crops)"""
    if pad is not None:
        OH, OW = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
        assert OH >= 1 and OW >= 1
        return (pad, OH, (OH - 1) * s + k - H), (pad, OW, (OW - 1) * s + k - W)
    gh, gw = _same_pad(H, k, s), _same_pad(W, k, s)
    return (gh, gw) if gh[0] == gw[0] else None


# ---------------------------------------------------------------------------------------------------------------- 1. depthwise
def _dw_data(dtype, C, N, H, W, k, s, pad=None):
    (_, OH, _), (_, OW, _) = _geometry(H, W, k, s, pad)
    rs = _rs("dw", str(dtype), C, N, H, W, k, s, pad)
    return dict(x=_r(0.3 + _randn(rs, N, H, W, C), dtype), w=_r(_randn(rs, C, 1, k, k) / k, dtype), dy=_r(_randn(rs, N, OH, OW, C), dtype),
                dw0=_randn(rs, C, 1, k, k))


def _dw_ref(dt, d, k, s, H, W, pad=None):
    """y, dx (NHWC) and dw of F.conv2d(F.pad(x, TF-SAME), w, stride=s, groups=C) in dtype dt, the gradients by autograd"""
    (ph, _, th), (pw, _, tw) = _geometry(H, W, k, s, pad)
    x = d["x"].to(dt).permute(0, 3, 1, 2).contiguous().requires_grad_()
    w = d["w"].to(dt).clone().requires_grad_()
    y = F.conv2d(F.pad(x, (pw, tw - pw, ph, th - ph)), w, None, stride=s, groups=x.shape[1])
    y.backward(d["dy"].to(dt).permute(0, 3, 1, 2).contiguous())
    return y.detach().permute(0, 2, 3, 1), x.grad.permute(0, 2, 3, 1), w.grad


def _cdiv(a, b):
    return -(-a // b)


def _wgrad_geometry(cls, N, OH, OW, C):
    """(blocks along the pixels, pixel lanes per block) of the weight-gradient kernel: the launcher's arithmetic restated (rd_dwconv.hip rgeom /
    qgeom(C, 256) and the three clamps of launch_dwconv_wgrad).  The block count of the quad class is what rd_dwconv_wgrad_partial reports as
    item.rows, and every case that sees an item compares the two."""
    pixels = N * OH * OW
    rows = _E().L().rd_dw_rows(pixels, C)
    if cls == "scalar":
        cb = 1
        while cb < C and cb < 256:
            cb *= 2
        return rows, 256 // cb
    c4, best, bu = C // 4, (1, 256, C // 4), -1.0
    for nc in range(1, 257):
        qb = _cdiv(c4, nc)
        if qb <= 256:
            pl = 256 // qb
            u = c4 * pl / (256.0 * nc)
            if u > bu + 1e-9:
                bu, best = u, (qb, pl, nc)
    _, PL, nchunk = best
    units = N * OH * _cdiv(OW, 4)
    gx = min(512 // nchunk, _cdiv(units, PL * 3), max(64, pixels // 32))
    return max(1, min(gx, rows)), PL


def _wgrad_restated(cls, d, N, H, W, C, k, s, geo, accumulate):
    """The fp32 yardstick of the weight gradient: torch's fp32 CPU result is NOT used, because the kernels' documented summation structure is
    less accurate than it by design and a correct kernel then misses _check's bound on some data (module docstring, "Finding").  This restates
    that structure, not the kernel's code: a block takes a contiguous range of units (quad class: runs of 4 output columns) or pixels (scalar
    class); pixel lane pl of its PL lanes takes every PL-th of them and accumulates each tap in fp32, one fused multiply-add per pixel (quad)
    or a rounded product and an addition (scalar); the lanes are added in fp32 in lane order; the blocks' rows are added in float64 and the
    total is rounded to fp32 (and added to the previous dw in fp32 when accumulating).  -> (C, 1, k, k) fp32"""
    (p, OH, _), (_, OW, _) = geo
    nb, PL = _wgrad_geometry(cls, N, OH, OW, C)
    m = np.arange(N * OH * OW)
    ow, oh, n = m % OW, (m // OW) % OH, m // (OW * OH)
    if cls == "quad":
        runs = _cdiv(OW, 4)
        per = _cdiv(N * OH * runs, nb)
        u = (n * OH + oh) * runs + ow // 4
        blk, j = u // per, u % per
        lane, pos, steps = j % PL, (j // PL) * 4 + ow % 4, _cdiv(per, PL) * 4
    else:
        per = _cdiv(N * OH * OW, nb)
        blk, j = m // per, m % per
        lane, pos, steps = j % PL, j // PL, _cdiv(per, PL)
    x, dy = d["x"].numpy(), d["dy"].numpy().reshape(-1, C)
    G = np.zeros((nb, PL, steps, C), np.float32)
    G[blk, lane, pos] = dy
    out = np.zeros((k * k, C), np.float64)
    for kh in range(k):
        for kw in range(k):
            ih, iw = oh * s - p + kh, ow * s - p + kw
            ok = (ih >= 0) & (ih < H) & (iw >= 0) & (iw < W)
            V = np.zeros_like(G)
            V[blk, lane, pos] = np.where(ok[:, None], x[n, np.clip(ih, 0, H - 1), np.clip(iw, 0, W - 1)], np.float32(0))
            acc = np.zeros((nb, PL, C), np.float32)
            for i in range(steps):
                if cls == "quad":      # fmaf: the exact product (48 bits, held by float64) plus the accumulator, rounded to fp32
                    acc = (G[:, :, i].astype(np.float64) * V[:, :, i] + acc).astype(np.float32)
                else:
                    acc = acc + G[:, :, i] * V[:, :, i]
            tot = np.zeros((nb, C), np.float32)
            for q in range(PL):
                tot = tot + acc[:, q]
            out[kh * k + kw] = tot.astype(np.float64).sum(0)
    dw = torch.from_numpy(out.astype(np.float32)).t().reshape(C, 1, k, k)
    return d["dw0"] + dw if accumulate else dw


def _dw_one(dev, dtype, C, N, H, W, k, s, cls, w_off=0, accumulate=0, expect_rows=None, pad=None):
    """rd_dwconv_fwd, rd_dwconv_dgrad and rd_dwconv_wgrad on the same tensors.  expect_rows: the weight gradient goes through
    rd_dwconv_wgrad_partial + rd_dw_wgrad_finalize_batch instead, and item.rows must be that literal.  pad: see _geometry."""
    lib = _E().L()
    (p, OH, _), (_, OW, _) = _geometry(H, W, k, s, pad)
    assert _class_of(N, OH, OW, C, k, s) == cls, "C=%d k=%d s=%d is listed as %s" % (C, k, s, cls)
    d = _dw_data(dtype, C, N, H, W, k, s, pad)
    r64, r32 = _dw_ref(torch.float64, d, k, s, H, W, pad), _dw_ref(F32, d, k, s, H, W, pad)
    what = "dwconv %s %s N=%d %dx%d -> %dx%d C=%d k=%d s=%d p=%d w_off=%d accumulate=%d" % (cls, dtype, N, H, W, OH, OW, C, k, s, p, w_off, accumulate)
    grp = "dw %s " % cls
    X, Wt, DY = Buf(dev, d["x"].numel(), dtype, d["x"]), Buf(dev, d["w"].numel(), F32, d["w"], off=w_off), Buf(dev, d["dy"].numel(), dtype, d["dy"])
    Y, DX = _nanbuf(dev, N * OH * OW * C, dtype), _nanbuf(dev, N * H * W * C, dtype)
    geo, tail = (N, H, W, C, OH, OW, k, s, p), (DT[dtype], _S(X.v))
    _call("rd_dwconv_fwd", _P(X.v), _P(Wt.v), _P(Y.v), *geo, *tail)
    _check(what + " y", Y.v.view(N, OH, OW, C), r64[0], r32[0], grp + "fwd")
    _call("rd_dwconv_dgrad", _P(DY.v), _P(Wt.v), _P(DX.v), *geo, *tail)
    _check(what + " dx", DX.v.view(N, H, W, C), r64[1], r32[1], grp + "dgrad")
    rows = lib.rd_dw_rows(N * OH * OW, C)
    PT = _nanbuf(dev, rows * C * k * k, F32)
    DW = Buf(dev, C * k * k, F32, d["dw0"]) if accumulate else _nanbuf(dev, C * k * k, F32)
    if expect_rows is None:
        _call("rd_dwconv_wgrad", _P(X.v), _P(DY.v), _P(PT.v), _P(DW.v), accumulate, *geo, *tail)
    else:
        it = _item()
        _call("rd_dwconv_wgrad_partial", _P(X.v), _P(DY.v), _P(PT.v), _P(DW.v), accumulate, *geo, DT[dtype], ctypes.byref(it), _S(X.v))
        assert it.rows == expect_rows, "%s: %d partial rows, the launcher's arithmetic gives %d" % (what, it.rows, expect_rows)
        assert cls == "scalar" or it.rows == _wgrad_geometry(cls, N, OH, OW, C)[0], what
        if it.rows:
            _call("rd_dw_wgrad_finalize_batch", ctypes.byref(it), 1, _S(X.v))
    r64dw = r64[2] + d["dw0"].double() if accumulate else r64[2]
    _check(what + " dw", DW.v.view(C, 1, k, k), r64dw, _wgrad_restated(cls, d, N, H, W, C, k, s, _geometry(H, W, k, s, pad), accumulate), grp + "wgrad")
    TORCH_WGRAD[0] = max(TORCH_WGRAD[0], float((r32[2].double() - r64[2]).abs().max() / r64[2].abs().max()))
    for b_ in (Y, DX, PT, DW):
        b_.check(what)
    for b_ in (X, Wt, DY):
        b_.check(what, unchanged=True)


def _dw_cfgs(dtypes, classes):
    """(dtype, class, C, (N, H, W), k, s) of the cross products whose two leading pads agree"""
    out = []
    for dt in dtypes:
        if "quad" in classes:
            out += [(dt, "quad", C, g, k, s) for C in QUAD_C for g in (WIDE_GEOMS if C >= WIDE_C else GEOMS) for k in (3, 5) for s in (1, 2)]
        if "scalar" in classes:
            out += [(dt, "scalar", C, g, k, s) for C in SCALAR_C for g in GEOMS for k in (3, 5) for s in (1, 2)]
            out += [(dt, "scalar", C, g, k, s) for (C, k, s) in SCALAR_ODD_K for g in ((2, 5, 9), (2, 40, 52))]
            out += [(dt, "scalar", C, g, k, s) for (C, g, k, s) in SCALAR_WIDE]
    return [c for c in out if _geometry(c[3][1], c[3][2], c[4], c[5]) is not None]


def _dw_feats(c):
    dt, cls, C, g, k, s = c
    p = _geometry(g[1], g[2], k, s)[0][0]
    return [("route", cls, k, s, p & 1, dt), ("C", C, k), ("geom", g, s), ("wide", C >= WIDE_C, dt, s)]


# shapes whose weight gradient must report this many partial rows: (dtype, C, (N, H, W), k, s, rows, full mode only) with
# gx = min(512 / nchunk, ceil(units / (3 PL)), max(64, pixels / 32), rd_dw_rows); units = N OH ceil(OW / 4), (QB, PL, nchunk) = qgeom(C, 256)
WGRAD_CLAMPS = (
    (F32, 36, (2, 40, 52), 3, 1, 2, False),       # qgeom (1, 256, 9): min(56, ceil(1040 / 768) = 2, 130, ceil(4160 / 256) = 17)
    (F32, 260, (1, 148, 148), 3, 1, 7, True),     # qgeom (1, 256, 65): min(512 / 65 = 7, ceil(5476 / 768) = 8, 684, ceil(21904 / 64) = 343)
    (BF16, 512, (1, 64, 64), 5, 1, 64, True),     # qgeom (128, 2, 1): min(512, ceil(1024 / 6) = 171, 128, ceil(4096 / 64) = 64)
)


def dw_case(dev, quick=False, dtypes=DTYPES, classes=CLASSES):
    """forward, data gradient and weight gradient of every (class, channel count, geometry, k, s); full mode adds the sizes past ew_grid's
    4096 blocks (scalar class) and past each reachable clamp of the weight gradient's block count (quad class)."""
    assert _E().L().rd_dw_rows(2 * 40 * 52, 130) == 65
    ran = set()
    for dt, cls, C, (N, H, W), k, s in _cover(_dw_cfgs(dtypes, classes), _dw_feats, quick, "dw"):
        _dw_one(dev, dt, C, N, H, W, k, s, cls)
        ran.add((cls, k, s, _geometry(H, W, k, s)[0][0] & 1, dt))
    for dt in dtypes:      # every (class, k, s, pad parity) ran, quick or not; stride 1 has the one parity of (k - 1) / 2
        for cls in classes:
            for k in (3, 5):
                assert (cls, k, 1, ((k - 1) // 2) & 1, dt) in ran and (cls, k, 2, 0, dt) in ran and (cls, k, 2, 1, dt) in ran, (cls, k, dt, sorted(map(str, ran)))
    if "quad" in classes:
        for dt, C, (N, H, W), k, s, rows, full in WGRAD_CLAMPS:
            if dt in dtypes and not (full and quick):
                assert N * H * W * C * 4 < 64 * 2 ** 20
                _dw_one(dev, dt, C, N, H, W, k, s, "quad", expect_rows=rows)
    if "scalar" in classes and not quick and F32 in dtypes:
        assert 2 * 300 * 300 * 6 > 4096 * 256
        _dw_one(dev, F32, 6, 2, 300, 300, 3, 1, "scalar", expect_rows=0)


def dw_fp16_case(dev, quick=False):
    """the fp16 build of the same kernels on three shapes: quad stride 1, quad stride 2, scalar"""
    with bf16_mode("fp16"):
        _dw_one(dev, F16, 12, 2, 5, 9, 3, 1, "quad")
        _dw_one(dev, F16, 36, 1, 8, 10, 5, 2, "quad")
        _dw_one(dev, F16, 3, 2, 5, 9, 3, 2, "scalar")


def dw_variants_case(dev, quick=False):
    """weights off the 16-byte boundary (the scalar branch of dw_stage_weights; one case per k and one on many chunks), accumulate = 1
    onto random values in both classes, and leading pads that are not TF-SAME's: torch's symmetric padding 0 ... k - 1 with the output size
    that goes with it (both pad parities of the stride-2 data gradient at both sizes' parities; windows that stop short of the last rows)"""
    for cls, C in (("quad", 12), ("quad", 64), ("scalar", 6)):
        for k in (3, 5):
            for s in (1, 2):
                for pad in range(k):
                    for i, (N, H, W) in enumerate(((2, 5, 9), (1, 8, 10))):
                        _dw_one(dev, BF16 if (pad + i) % 3 == 2 else F32, C, N, H, W, k, s, cls, pad=pad)
    for dt, C, (N, H, W), k, s in ((F32, 12, (2, 5, 9), 3, 1), (BF16, 36, (1, 8, 10), 5, 2), (F32, 36, (2, 5, 9), 5, 1), (BF16, 4, (1, 8, 10), 3, 2),
                                   (F32, 260, (1, 8, 10), 3, 1), (BF16, 1028, (2, 5, 9), 5, 2)):
        _dw_one(dev, dt, C, N, H, W, k, s, "quad", w_off=1)
    for dt, cls, C, (N, H, W), k, s in ((F32, "quad", 12, (2, 40, 52), 3, 2), (BF16, "quad", 260, (2, 5, 9), 5, 1), (F32, "scalar", 6, (2, 40, 52), 5, 1),
                                        (BF16, "scalar", 8, (2, 5, 9), 4, 1), (F32, "scalar", 3, (1, 8, 10), 3, 2)):
        _dw_one(dev, dt, C, N, H, W, k, s, cls, accumulate=1)


BATCH_SHAPES = ((F32, 12, (2, 5, 9), 3, 1), (F32, 16, (1, 8, 10), 5, 2), (BF16, 4, (2, 5, 9), 5, 1), (F32, 8, (1, 8, 10), 3, 2),
                (F32, 6, (2, 5, 9), 3, 1))                  # the last one is of the scalar class
BATCH_ROWS33 = (F32, 256, (1, 40, 52), 3, 1)                # qgeom (64, 4, 1): min(512, ceil(520 / 12) = 44, 65, ceil(2080 / 64) = 33) = 33 rows
BATCH_CYCLES = 17                                           # 85 calls, 68 of them pending: the second launch takes 4 items + the 33-row one


class _BatchShape(object):
    """inputs of one shape on the device, its float64 / fp32 gradients, and rd_dwconv_wgrad's own dw for accumulate 0 and 1"""

    def __init__(self, dev, dtype, C, geom, k, s):
        lib = _E().L()
        N, H, W = geom
        (p, OH, _), (_, OW, _) = _geometry(H, W, k, s)
        self.cls = _class_of(N, OH, OW, C, k, s)
        self.what = "wgrad batch %s %s N=%d %dx%d C=%d k=%d s=%d" % (self.cls, dtype, N, H, W, C, k, s)
        self.d = d = _dw_data(dtype, C, N, H, W, k, s)
        self.n, self.rows, self.dtype = C * k * k, lib.rd_dw_rows(N * OH * OW, C), dtype
        self.X, self.DY = Buf(dev, d["x"].numel(), dtype, d["x"]), Buf(dev, d["dy"].numel(), dtype, d["dy"])
        self.args = (N, H, W, C, OH, OW, k, s, p, DT[dtype])
        self.r64 = _dw_ref(torch.float64, d, k, s, H, W)[2].reshape(-1)
        self.r32 = [_wgrad_restated(self.cls, d, N, H, W, C, k, s, _geometry(H, W, k, s), acc).reshape(-1) for acc in (0, 1)]
        self.gx = _wgrad_geometry(self.cls, N, OH, OW, C)[0]
        self.direct = []
        for acc in (0, 1):
            PT, DW = self.bufs(dev, acc)
            _call("rd_dwconv_wgrad", _P(self.X.v), _P(self.DY.v), _P(PT.v), _P(DW.v), acc, *self.args, _S(self.X.v))
            PT.check(self.what); DW.check(self.what)
            self.direct.append(DW.cpu().clone())

    def bufs(self, dev, acc):
        return _nanbuf(dev, self.rows * self.n, F32), (Buf(dev, self.n, F32, self.d["dw0"]) if acc else _nanbuf(dev, self.n, F32))


def wgrad_batch_case(dev, quick=False):
    """rd_dwconv_wgrad_partial for 86 items (accumulate on every other one), then ONE rd_dw_wgrad_finalize_batch over the pending ones: every
    dw bit-identical to rd_dwconv_wgrad's on the same inputs (the header promises its summation order) and within _check of float64; the
    scalar-class items come back with rows == 0 and dw already final; partial rows and dw keep their sentinels.  Full mode adds the item
    whose C k k / 64 = 1025 passes the batch kernel's 1024-block grid cap."""
    from riders_amd import _lib
    shapes = [_BatchShape(dev, *sh) for sh in BATCH_SHAPES]
    order = [shapes[i % len(shapes)] for i in range(BATCH_CYCLES * len(shapes))] + [_BatchShape(dev, *BATCH_ROWS33)]
    if not quick:
        order.append(_BatchShape(dev, F32, 2624, (1, 3, 4), 5, 1))
        assert order[-1].n // 64 == 1025
    assert [sh.cls for sh in shapes] == ["quad"] * 4 + ["scalar"]
    calls, pending = [], []
    for i, sh in enumerate(order):
        acc = i % 2
        PT, DW = sh.bufs(dev, acc)
        it = _lib.DwWgradItem()
        _call("rd_dwconv_wgrad_partial", _P(sh.X.v), _P(sh.DY.v), _P(PT.v), _P(DW.v), acc, *sh.args, ctypes.byref(it), _S(sh.X.v))
        calls.append((sh, acc, PT, DW, it.rows))
        if sh.cls == "scalar":
            assert it.rows == 0, sh.what + ": a scalar-class item must be finished at once (rows = %d)" % it.rows
            _exact(sh.what + " (finished by the partial call)", DW.v, sh.direct[acc])
        else:
            assert it.rows == sh.gx and 0 < it.rows <= sh.rows and it.partial == PT.v.data_ptr() and it.dw == DW.v.data_ptr() and (it.C, it.KK, it.accumulate) == (sh.args[3], sh.args[6] ** 2, acc), sh.what
            pending.append(it)
    assert calls[BATCH_CYCLES * len(shapes)][4] == 33, "the 33-row item has %d rows" % calls[BATCH_CYCLES * len(shapes)][4]
    assert len(pending) > 64, "one launch would take all %d pending items" % len(pending)
    arr = (_lib.DwWgradItem * len(pending))(*pending)
    _call("rd_dw_wgrad_finalize_batch", arr, len(pending), _S(shapes[0].X.v))
    for i, (sh, acc, PT, DW, rows) in enumerate(calls):
        what = "%s item %d accumulate=%d (%d rows)" % (sh.what, i, acc, rows)
        _exact(what + " against rd_dwconv_wgrad", DW.v, sh.direct[acc])
        _check(what, DW.v, sh.r64 + sh.d["dw0"].reshape(-1).double() if acc else sh.r64, sh.r32[acc], "dw %s wgrad (batch)" % sh.cls)
        PT.check(what); DW.check(what)
    for sh in set(order):
        sh.X.check(sh.what, unchanged=True); sh.DY.check(sh.what, unchanged=True)


# ---------------------------------------------------------------------------------------------------------------- 2. bilinear
# exact 2x (twice), non-integer up-sampling, 3x .. 4x and 3.5x / 1.67x (more than four readers per source pixel: the loop fall-back of
# bilinear_bwd_vec_kernel), down-sampling (twice), one source pixel, the identity
BIL_SIZES = (((5, 7), (10, 14)), ((1, 4), (2, 8)), ((5, 7), (7, 9)), ((3, 5), (9, 20)), ((2, 3), (7, 5)), ((4, 6), (2, 3)), ((9, 9), (3, 4)),
             ((1, 1), (3, 3)), ((6, 6), (6, 6)))
BIL_C = (8, 4, 3)      # vector form for both dtypes; vector fp32, scalar bf16; scalar
BIL_FORMS = ("vec", "scalar")


def _bil_form(C, dtype):
    return "vec" if C % (4 if dtype == F32 else 8) == 0 else "scalar"


def _bil_one(dev, dtype, N, C, H, W, OH, OW, align):
    rs = _rs("bilinear", str(dtype), N, C, H, W, OH, OW, align)
    x, dy = _r(_randn(rs, N, H, W, C), dtype), _r(_randn(rs, N, OH, OW, C), dtype)
    refs = []
    for dt in (torch.float64, F32):
        xr = x.to(dt).permute(0, 3, 1, 2).contiguous().requires_grad_()
        y = F.interpolate(xr, size=(OH, OW), mode="bilinear", align_corners=bool(align))
        y.backward(dy.to(dt).permute(0, 3, 1, 2).contiguous())
        refs.append((y.detach().permute(0, 2, 3, 1), xr.grad.permute(0, 2, 3, 1)))
    what = "bilinear %s %s N=%d C=%d %dx%d -> %dx%d align_corners=%d" % (_bil_form(C, dtype), dtype, N, C, H, W, OH, OW, align)
    grp = "bilinear %s " % _bil_form(C, dtype)
    X, DY = Buf(dev, x.numel(), dtype, x), Buf(dev, dy.numel(), dtype, dy)
    Y, DX = _nanbuf(dev, dy.numel(), dtype), _nanbuf(dev, x.numel(), dtype)
    _call("rd_bilinear_fwd", _P(X.v), _P(Y.v), N, H, W, C, OH, OW, align, DT[dtype], _S(X.v))
    _check(what + " y", Y.v.view(N, OH, OW, C), refs[0][0], refs[1][0], grp + "fwd")
    _call("rd_bilinear_bwd", _P(DY.v), _P(DX.v), N, H, W, C, OH, OW, align, DT[dtype], _S(X.v))
    _check(what + " dx", DX.v.view(N, H, W, C), refs[0][1], refs[1][1], grp + "bwd")
    Y.check(what); DX.check(what); X.check(what, unchanged=True); DY.check(what, unchanged=True)


def bilinear_case(dev, quick=False, dtypes=DTYPES, forms=BIL_FORMS):
    """rd_bilinear_fwd / _bwd against F.interpolate(size=...) and its autograd: BIL_SIZES x both align_corners x C = 8, 4, 3 at N = 2; full mode
    adds one size past ew_grid's 4096 blocks per form, forward and backward."""
    cfgs = [(dt, C, hw, ohw, al) for dt in dtypes for C in BIL_C if _bil_form(C, dt) in forms for (hw, ohw) in BIL_SIZES for al in (1, 0)]
    ran = set()
    for dt, C, (H, W), (OH, OW), al in _cover(cfgs, lambda c: [("size", _bil_form(c[1], c[0]), c[2], c[3], c[4]), ("C", c[0], c[1])], quick, "bilinear"):
        _bil_one(dev, dt, 2, C, H, W, OH, OW, al)
        ran.add((dt, _bil_form(C, dt)))
    assert ran == set((dt, f) for dt in dtypes for f in forms), ran
    if not quick and F32 in dtypes:
        # the forward's grid runs over the destination, the backward's over the source: the up-sampling passes the cap forward, its mirror backward
        if "vec" in forms:
            assert 2 * 128 * 128 * (260 // 4) > 4096 * 256 > 2 * 64 * 64 * (260 // 4)
            _bil_one(dev, F32, 2, 260, 64, 64, 128, 128, 1)
            _bil_one(dev, F32, 2, 260, 128, 128, 64, 64, 0)
        if "scalar" in forms:
            assert 2 * 600 * 600 * 3 > 4096 * 256 > 2 * 300 * 300 * 3
            _bil_one(dev, F32, 2, 3, 300, 300, 600, 600, 0)
            _bil_one(dev, F32, 2, 3, 600, 600, 300, 300, 1)


def bilinear_fp16_case(dev, quick=False):
    with bf16_mode("fp16"):
        _bil_one(dev, F16, 2, 8, 3, 5, 9, 20, 0)


# ---------------------------------------------------------------------------------------------------------------- 3. SML head, reciprocal
HEAD_N = (1, 255, 1000)
HEAD_BIG = 4096 * 256 + 777                                        # past ew_grid's 4096 blocks
HEAD_BOUNDS = ((10.0, 1.0 / 255), (-1.0, -1.0), (0.8, 0.3))        # (hi, lo); a bound <= 0 disables its clamp
HEAD_DTYPES = (F32, BF16, F16)
TIE = 1e-3      # planted and drawn values keep this relative distance from p == hi, p == lo and 1 + out == 0 (other than the planted zeros)


def _head_ref(dt, out, d, dpred, hi, lo):
    """pred = d * relu(1 + out), then the two clamps; dout = dpred * d where 1 + out > 0 and the prediction was not clamped, else 0"""
    sc = 1.0 + out.to(dt)
    p = d.to(dt) * sc.clamp(min=0)
    clamped = torch.zeros_like(p, dtype=torch.bool)
    pred = p.clone()
    if hi > 0:
        clamped |= p > hi
        pred = torch.where(p > hi, torch.full_like(p, hi), pred)
    if lo > 0:
        low = ~clamped & (p < lo)
        clamped |= low
        pred = torch.where(low, torch.full_like(p, lo), pred)
    keep = (sc > 0) & ~clamped
    return pred, torch.where(keep, dpred.to(dt) * d.to(dt), torch.zeros_like(p)), keep, p


def _head_one(dev, dtype, n, hi, lo):
    hi, lo = float(np.float32(hi)), float(np.float32(lo))
    rs = _rs("head", str(dtype), n, hi, lo)
    draw = lambda: (_r(0.6 * _randn(rs, n), dtype), torch.exp(torch.from_numpy(rs.uniform(np.log(0.002), np.log(30.0), n).astype(np.float32))))      # noqa: E731
    out, d = draw()
    planted = torch.zeros(n, dtype=torch.bool)
    for i, v in enumerate((-1.0, -1.5, -3.0, -1.0)[:n]):      # scale exactly 0, and below it
        out[(i * 7) % n] = v; planted[(i * 7) % n] = True
    while True:
        sc = 1.0 + out.double()
        p = d.double() * sc.clamp(min=0)
        bad = ~planted & (sc.abs() < TIE)
        for b in (hi, lo):
            if b > 0:
                bad |= (p - b).abs() <= TIE * b
        if not bool(bad.any()):
            break
        o2, d2 = draw()
        out, d = torch.where(bad, o2, out), torch.where(bad, d2, d)
    dpred = _randn(rs, n)
    (p64, g64, k64, raw64), (p32, g32, k32, raw32) = _head_ref(torch.float64, out, d, dpred, hi, lo), _head_ref(F32, out, d, dpred, hi, lo)
    what = "sml_head %s n=%d hi=%g lo=%g" % (dtype, n, hi, lo)
    assert torch.equal(k64, k32) and torch.equal(raw64 > hi, raw32 > hi) and torch.equal(raw64 < lo, raw32 < lo), what + ": the reference sees a tie"
    if n >= 255:
        assert bool(k64.any()) and bool((~k64).any()) and (hi <= 0 or (bool((raw64 > hi).any()) and bool((raw64 < lo).any()))), what + ": a branch is not exercised"
    O, D, DP = Buf(dev, n, dtype, out), Buf(dev, n, F32, d), Buf(dev, n, F32, dpred)
    PR, DO = _nanbuf(dev, n, F32), _nanbuf(dev, n, dtype)
    _call("rd_sml_head_fwd", _P(O.v), _P(D.v), _P(PR.v), n, hi, lo, DT[dtype], _S(O.v))
    _check(what + " pred", PR.v, p64, p32, "sml_head fwd")
    _call("rd_sml_head_bwd", _P(O.v), _P(D.v), _P(DP.v), _P(DO.v), n, hi, lo, DT[dtype], _S(O.v))
    _check(what + " dout", DO.v, g64, g32, "sml_head bwd")
    assert not bool((DO.cpu().float() != 0)[~k64].any()), what + ": the backward passes a gradient where the forward had scale 0 or clamped"
    PR.check(what); DO.check(what)
    for b_ in (O, D, DP):
        b_.check(what, unchanged=True)


def head_case(dev, quick=False, dtypes=HEAD_DTYPES):
    """rd_sml_head_fwd / _bwd: sizes x clamp bounds x the type of `out`, with out = -1 exactly and out < -1 planted"""
    for dt in dtypes:
        for n in HEAD_N + (() if quick else (HEAD_BIG,)):
            for hi, lo in (HEAD_BOUNDS if n < HEAD_BIG else HEAD_BOUNDS[:1]):
                if dt == F16:
                    with bf16_mode("fp16"):
                        _head_one(dev, dt, n, hi, lo)
                else:
                    _head_one(dev, dt, n, hi, lo)


def reciprocal_case(dev, quick=False):
    """rd_reciprocal: out = 1 / x (dy NULL) and dx = -dy / x^2, |x| >= 0.05"""
    for n in HEAD_N + (() if quick else (HEAD_BIG,)):
        rs = _rs("reciprocal", n)
        x = _randn(rs, n)
        x = torch.where(x < 0, x - 0.05, x + 0.05)
        dy = _randn(rs, n)
        assert float(x.abs().min()) >= 0.05
        X, DYb, Y, DX = Buf(dev, n, F32, x), Buf(dev, n, F32, dy), _nanbuf(dev, n, F32), _nanbuf(dev, n, F32)
        what = "reciprocal n=%d" % n
        _call("rd_reciprocal", _P(X.v), None, _P(Y.v), n, _S(X.v))
        _check(what + " fwd", Y.v, 1.0 / x.double(), 1.0 / x, "reciprocal fwd")
        _call("rd_reciprocal", _P(X.v), _P(DYb.v), _P(DX.v), n, _S(X.v))
        _check(what + " bwd", DX.v, -dy.double() / (x.double() * x.double()), -dy / (x * x), "reciprocal bwd")
        Y.check(what); DX.check(what); X.check(what, unchanged=True); DYb.check(what, unchanged=True)


# ---------------------------------------------------------------------------------------------------------------- 4. argument checks
def refusals_case(dev, quick=False):
    """the depthwise and bilinear entry points refuse s < 1, a size < 1 and p outside [0, k) with "bad args" before any launch: nothing is
    written.  (Valid arguments otherwise; every call here must fail on the host.)"""
    N, H, W, C, k, s, p = 1, 4, 4, 4, 3, 1, 1
    good = dict(N=N, H=H, W=W, C=C, OH=H, OW=W, k=k, s=s, p=p)
    bad = [dict(s=0), dict(s=-1), dict(p=-1), dict(p=k), dict(p=k + 2)] + [{nm: v} for nm in ("N", "H", "W", "C", "OH", "OW") for v in (0, -3)]
    n = N * H * W * C
    X, Wt, DYb = Buf(dev, n, F32, torch.ones(n)), Buf(dev, C * k * k, F32, torch.ones(C * k * k)), Buf(dev, n, F32, torch.ones(n))
    Y, DX, ST = _nanbuf(dev, n, F32), _nanbuf(dev, n, F32), _nanbuf(dev, 64 * C * 2, F32)
    PT, DW = _nanbuf(dev, 64 * C * k * k, F32), _nanbuf(dev, C * k * k, F32)
    outs = (Y, DX, ST, PT, DW)
    it = _item()
    for b in bad:
        a = dict(good, **b)
        geo = tuple(a[nm] for nm in ("N", "H", "W", "C", "OH", "OW", "k", "s", "p"))
        _refused("rd_dwconv_fwd", "dwconv_fwd: bad args", _P(X.v), _P(Wt.v), _P(Y.v), *geo, 0, _S(X.v))
        _refused("rd_dwconv_fwd_stats", "dwconv_fwd_stats: bad args", _P(X.v), _P(Wt.v), _P(Y.v), _P(ST.v), *geo, 0, _S(X.v))
        _refused("rd_dwconv_dgrad", "dwconv_dgrad: bad args", _P(DYb.v), _P(Wt.v), _P(DX.v), *geo, 0, _S(X.v))
        _refused("rd_dwconv_wgrad", "dwconv_wgrad: bad args", _P(X.v), _P(DYb.v), _P(PT.v), _P(DW.v), 0, *geo, 0, _S(X.v))
        _refused("rd_dwconv_wgrad_partial", "dwconv_wgrad_partial: bad args", _P(X.v), _P(DYb.v), _P(PT.v), _P(DW.v), 0, *geo, 0, ctypes.byref(it), _S(X.v))
        if not set(b) & set("ksp"):
            _refused("rd_bilinear_fwd", "bilinear_fwd: bad args", _P(X.v), _P(Y.v), *geo[:6], 1, 0, _S(X.v))
            _refused("rd_bilinear_bwd", "bilinear_bwd: bad args", _P(DYb.v), _P(DX.v), *geo[:6], 0, 0, _S(X.v))
        for o in outs:
            o.check("refused %s" % b, unchanged=True)
    for i_ in (X, Wt, DYb):
        i_.check("refusals", unchanged=True)
