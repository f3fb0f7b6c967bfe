"""Direct parity cases for the BatchNorm kernel family: the statistics producers (rd_bn_stats, rd_dwconv_fwd_stats), rd_bn_finalize and
rd_bn_finalize_apply, rd_affine_act / rd_affine_act_add, and the backward family (rd_bn_act_bwd, _recompute, _recompute_phases, _from_partial,
_slab).  Harness and bound as tests/parity_cases_glue.py: every kernel through the C ABI, every buffer a kernel writes a `Buf` with sentinels on
both sides, outputs prefilled with NaN, references plain float64 restatements on the values the kernel receives (rounded 16-bit inputs, the fp32
mean / rstd / scale / shift that are passed in), bound from torch's own fp32 error -- nothing in a bound comes from a kernel's output.

The streaming kernels have three forms chosen by channel count (rd_norm.hip vec_ok / gen_ok): `vec` (the number of 16-byte channel vectors divides
256), `gen` (whole vectors, at most 256 of them) and the scalar fall-back.  CH lists the channel counts per form and dtype; `_assert_form` checks
each against rd_bn_kernel_name at every use, so a routing change cannot silently empty a class.

quick=True (the emulator twin) runs a covering selection of each cross product (`_cover`: every (form, dtype) pair with every activation, pixel
count and switch value at least once); the GPU twin runs the cross products and, per form, one size past the launcher's grid cap:
  ew_grid / ew_grid_per / the gen grids: 2048 blocks (a second grid-stride iteration), reached for every apply kernel;
  dw_rows: 512 rows (rd_bn_stats at 32 769 pixels x 256 channels); dw_stats_ppb: 1024 rows (rd_dwconv_fwd_stats at 2 x 96 x 96 x 256);
  red_rows (the backward reduce): 4096 rows is NOT reachable under 64 MB -- its smallest tensor is 32 769 pixels x 1025 channels of a 16-bit
  type, 67.2 MB -- and is not tested.

Measured (relative to max|ref|, fp32 outputs; in brackets torch's own fp32 CPU error against float64; 16-bit outputs sit within their half ulp,
at most 3.8e-3):
  emulator (the covering selection): bn_stats totals 2.2e-7 (1.6e-7), dwconv_fwd_stats totals 2.3e-7 (1.1e-7); finalize mean / rstd / scale / shift /
            running statistics 4.5e-8 ... 1.1e-7 (1.1e-7 ... 2.8e-3: the fp32 E2 - m^2 of the count = 1 case); affine_act 8.0e-8 (8.0e-8),
            affine_act_add 1.2e-7 (1.2e-7); backward dy 1.1e-7 (1.1e-7), dgamma 4.1e-7 (3.0e-7), dbeta 3.2e-7 (4.0e-7)
  MI355X (the cross products): bn_stats totals 3.7e-7 (2.4e-7), dwconv_fwd_stats totals 3.2e-7 (1.7e-7); finalize 5.4e-8 ... 1.2e-7; affine_act 1.2e-7 (1.2e-7),
            affine_act_add 1.3e-7 (1.3e-7); backward dy 1.8e-7 (1.8e-7), dgamma 4.1e-7 (3.4e-7), dbeta 6.1e-7 (4.4e-7); 16-bit outputs <= 3.8e-3
  rstd on inputs of std 0.1, emulator and MI355X alike (the sums are taken in a fixed order) (kernel / sequential-fp32-row restatement / torch fp32 batch_norm):
            mean 3:  700x24 8.5e-5 / 3.8e-4 / 1.0e-7    5000x16 7.8e-5 / 4.9e-4 / 1.6e-7
            mean 30: 700x24 1.0e-2 / 4.0e-2 / 1.2e-7    5000x16 6.5e-3 / 3.5e-2 / 1.7e-7
"""
import numpy as np
import torch
import torch.nn.functional as F

from tests.parity_cases import TOL
from tests.parity_cases_glue import (BF16, EPS32, F16, F32, FLOOR_ULPS, MEASURED, TINY32, Buf, _call, _check, _E, _exact, _half_ulp, _ints, _P, _r,
                                     _randn, _refused, _rs, _S, report)

NAN = float("nan")
SLOPE = float(np.float32(0.2))
BN_EPS, BN_MOM = float(np.float32(1e-5)), float(np.float32(0.1))
ACTS = (0, 1, 2, 3)      # none, ReLU, LeakyReLU, ReLU6 (engine.ACT_*)
DT = {F32: 0, BF16: 1, F16: 2}
DTYPES = (F32, BF16, F16)
_C16 = dict(vec=(16, 64), gen=(24, 40, 136, 1392), scalar=(6, 12, 2056))
CH = {F32: dict(vec=(16, 64), gen=(24, 40, 288), scalar=(3, 6, 1028)), BF16: _C16, F16: _C16}
FORMS = ("vec", "gen", "scalar")
PIXELS = (1, 63, 64, 65, 257, 1000)
CENSUS = {}              # network -> (max over layers of max_c |mean| * rstd, layer, calls seen, BatchNorm layers): filled by the emulator twin


def _pixels(C, quick=False):
    """around the 64-pixel partial row; wider than 256 channels red_rows switches to short per-block ranges (8 pixels at C >= 1025): 57, 113.
    quick (the emulator, whose cost is the number of elements): the wide channel counts leave 257 and 1000 pixels to the narrow ones"""
    if C > 256:
        return (1, 57, 65, 113) if quick else PIXELS + (57, 113)
    return PIXELS


def _ve(dtype):
    return 4 if dtype == F32 else 8


def _nanbuf(dev, n, dtype):
    return Buf(dev, n, dtype, torch.full((n,), NAN))


def _form_of(name):
    return "vec" if "_vec_kernel<" in name else "gen" if "_gen_kernel<" in name else "scalar"


def _recomputes(C, dtype):
    """the backward kernels of this channel count recompute the activation's argument from y (vec / gen forms); the scalar fall-back reads z"""
    return _form_of(_E().L().rd_bn_kernel_name(1, C, DT[dtype], 0, 1).decode()) != "scalar"


def _wide(dt, C):
    return (dt, C) if C > 300 else None


def _assert_form(C, dtype, form):
    """the channel count runs the form it is listed under, for the forward apply, the backward reduce and the backward apply, with and without
    the residual / recompute flag"""
    lib = _E().L()
    assert C in CH[dtype][form]
    for which in (0, 1, 2):
        for flag in (0, 1):
            for act in (0, 3):
                name = lib.rd_bn_kernel_name(which, C, DT[dtype], act, flag).decode()
                assert name and _form_of(name) == form, "C=%d %s is listed as %s but routed to %s" % (C, dtype, form, name)


QUICK_WIDE = ((F32, 1028), (BF16, 1392), (F16, 2056))      # the wide channel counts the emulator twin runs (one per dtype)


def _cover(configs, feats, quick, key, wide=None):
    """full mode: every config.  quick: a covering selection -- the configs are shuffled (fixed seed) and one is kept whenever it shows a
    feature (feats(config)) no kept config has shown.  wide(config) -> (dtype, C) of a config on a wide channel count, else None: under the
    emulator a launch costs ~30 ms per 256-fibre block that shuffles, and the finalize and one-launch kernels are one block per channel or
    channel vector, so of the wide counts only QUICK_WIDE run there, and only for what the narrow counts cannot show"""
    configs = list(configs)
    if not quick:
        return configs
    order = [int(i) for i in _rs("cover", key).permutation(len(configs))]
    if wide is not None:
        order = [i for i in order if wide(configs[i]) is None] + [i for i in order if wide(configs[i]) in QUICK_WIDE]
    seen, out = set(), []
    for i in order:
        f = set(feats(configs[i]))
        if not f <= seen:
            out.append(configs[i]); seen |= f
    return out


def _act(u, act, slope):
    if act == 1:
        return u.clamp(min=0)
    if act == 2:
        return torch.where(u > 0, u, u * slope)
    if act == 3:
        return u.clamp(0, 6)
    return u


def _dact(u, act, slope):
    """act_grad_from_out's convention on the activation's argument (same sign pattern as on its output): strictly > 0, strictly < 6"""
    one = torch.ones_like(u)
    if act == 1:
        return torch.where(u > 0, one, torch.zeros_like(u))
    if act == 2:
        return torch.where(u > 0, one, torch.full_like(u, slope))
    if act == 3:
        return torch.where((u > 0) & (u < 6), one, torch.zeros_like(u))
    return one


def _fp32_bound(ref64, ref32):
    """_check's fp32 part: min(max(4 * torch's fp32 error, FLOOR_ULPS fp32 ulp of max|ref|, TINY32), TOL * max|ref|)"""
    m = float(ref64.abs().max()) if ref64.numel() else 0.0
    ref_err = float((ref32.double() - ref64).abs().max()) if ref64.numel() else 0.0
    return min(max(4.0 * ref_err, FLOOR_ULPS * EPS32 * m, TINY32), max(TOL * m, TINY32)), ref_err, m


def _check_rounded_z(what, got, ref64, ref32, z64, z32, group):
    """_check for out = act2(round(z) + residual), whose intermediate z the kernel rounds to the activation type (riders_hip.h, rd_affine_act_add).
    The reference rounds its float64 z; the kernel rounds its fp32 z, which differs from it by fp32 rounding, so where z lies within the fp32
    bound (of z) of a rounding tie of the 16-bit type the two may round to different neighbours: there, and only there, the result may differ
    by one whole ulp of that type at |z|, on top of _check's bound and the half ulp of the result.  fp32 outputs: plain _check."""
    out_dt = got.dtype
    if out_dt == F32:
        return _check(what, got, ref64, ref32, group)
    g = got.detach().cpu().double().reshape(-1)
    r, z = ref64.double().reshape(-1), z64.double().reshape(-1)
    assert g.shape == r.shape and bool(torch.isfinite(g).all()), what + ": shape / non-finite values"
    bound, ref_err, m = _fp32_bound(r, ref32.reshape(-1))
    zbound = _fp32_bound(z, z32.reshape(-1))[0]
    hz = _half_ulp(out_dt, z)
    near_tie = (hz - (z - z.to(out_dt).double()).abs()) <= zbound
    extra = torch.where(near_tie, 2.0 * hz, torch.zeros_like(hz))
    diff = (g - r).abs()
    err = float(diff.max()) if diff.numel() else 0.0
    if m > 0:
        cur = MEASURED.setdefault(group + " 16-bit", [0.0, 0.0])
        cur[0] = max(cur[0], ref_err / m); cur[1] = max(cur[1], err / m)
    ok = bool((diff <= bound + _half_ulp(out_dt, r) + extra).all())
    assert ok, "%s: kernel error %.3e, torch fp32's own error %.3e, fp32 bound %.3e (+ half an ulp of %s, + one ulp at |z| on %d ties)" % (
        what, err, ref_err, bound, out_dt, int(near_tie.sum()))


# ---------------------------------------------------------------------------------------------------------------- 1. statistics producers
def _stats_totals(what, PT, rows, C, y, group):
    """column totals of the rows against float64 sums of the stored y; every row element written (finite from a NaN prefill)"""
    st = PT.cpu().view(rows, C, 2)
    assert bool(torch.isfinite(st).all()), what + ": a statistics row element was not written"
    tot = st.double().sum(0)
    y2 = y.reshape(-1, C)
    _check(what + " sum", tot[:, 0], y2.double().sum(0), y2.sum(0), group)
    _check(what + " sum of squares", tot[:, 1], (y2.double() * y2.double()).sum(0), (y2 * y2).sum(0), group)
    PT.check(what)


def _bn_stats_one(dev, dtype, C, pixels):
    lib = _E().L()
    y = _r(0.3 + 1.5 * _randn(_rs("bn_stats", str(dtype), C, pixels), pixels, C), dtype)
    rows = lib.rd_dw_rows(pixels, C)
    Y, PT = Buf(dev, pixels * C, dtype, y), _nanbuf(dev, rows * C * 2, F32)
    what = "bn_stats %s pixels=%d C=%d (%d rows)" % (dtype, pixels, C, rows)
    _call("rd_bn_stats", _P(Y.v), _P(PT.v), pixels, C, DT[dtype], _S(Y.v))
    _stats_totals(what, PT, rows, C, y, "bn_stats totals")
    Y.check(what, unchanged=True)


def _same_pad(i, k, s):
    o = -(-i // s)
    return max((o - 1) * s + k - i, 0) // 2, o, max((o - 1) * s + k - i, 0)


def _dw_stats_one(dev, dtype, C, N, H, W, k, s):
    lib = _E().L()
    rs = _rs("dw_stats", str(dtype), C, N, H, W, k, s)
    x = _r(0.3 + _randn(rs, N, H, W, C), dtype)
    w = _randn(rs, C, 1, k, k) / k
    (ph, OH, th), (pw, OW, tw) = _same_pad(H, k, s), _same_pad(W, k, s)
    assert ph == pw
    rows = lib.rd_dwconv_stats_rows(N, OH, OW, C, k, s)
    assert rows > 0
    X, Wt = Buf(dev, x.numel(), dtype, x), Buf(dev, w.numel(), F32, w)
    Y, PT = _nanbuf(dev, N * OH * OW * C, dtype), _nanbuf(dev, rows * C * 2, F32)
    what = "dwconv_fwd_stats %s N=%d %dx%d C=%d k=%d s=%d (%d rows)" % (dtype, N, H, W, C, k, s, rows)
    _call("rd_dwconv_fwd_stats", _P(X.v), _P(Wt.v), _P(Y.v), _P(PT.v), N, H, W, C, OH, OW, k, s, ph, DT[dtype], _S(X.v))
    refs = [F.conv2d(F.pad(x.to(dt).permute(0, 3, 1, 2), (pw, tw - pw, ph, th - ph)), w.to(dt), None, stride=s, groups=C).permute(0, 2, 3, 1)
            for dt in (torch.float64, F32)]
    _check(what + " y", Y.v, refs[0], refs[1], "dwconv_fwd_stats y")
    _stats_totals(what, PT, rows, C, Y.cpu().float(), "dwconv_fwd_stats totals")      # the statistics are those of the STORED output
    Y.check(what); X.check(what, unchanged=True); Wt.check(what, unchanged=True)


def stats_case(dev, quick=False):
    """rd_bn_stats with rows from rd_dw_rows (one kernel, its block geometry by channel count: 4 ... 256 channel lanes, two channel chunks at
    C = 300 and above) and rd_dwconv_fwd_stats with rows from rd_dwconv_stats_rows (k 3 / 5, stride 1 / 2, a ragged last run of output columns):
    the column totals of the (sum, sum^2) rows against float64 sums of the stored y.  Full mode adds the sizes past the 512-row and 1024-row caps."""
    cfgs = [(dt, C, p) for dt in DTYPES for C in sorted(set(sum(CH[dt].values(), ()) + (300,))) for p in _pixels(C, quick)]
    for dt, C, p in _cover(cfgs, lambda c: [("dt", c[0]), ("C", c[1]), ("pix", c[2]), ("wide-pix", c[1] > 256, c[2])], quick, "stats", lambda c: _wide(c[0], c[1])):
        _bn_stats_one(dev, dt, C, p)
    cfgs = [(dt, C, N, H, W, k, s) for dt in DTYPES for C in (8, 24, 300) for (N, H, W) in ((1, 7, 9), (2, 6, 10), (3, 5, 13))
            for k in (3, 5) for s in (1, 2)]
    for c in _cover(cfgs, lambda c: [("dt", c[0], c[5], c[6]), ("C", c[1], c[5]), ("geom", c[2:5], c[6])], quick, "dwstats"):
        _dw_stats_one(dev, *c)
    if not quick:
        _bn_stats_one(dev, F32, 256, 512 * 64 + 1)       # dw_rows caps at 512 rows: 65 pixels per row, the last rows empty
        _dw_stats_one(dev, F32, 256, 2, 96, 96, 3, 1)    # dw_stats_ppb caps at 1024 rows: 4608 units on 4 pixel lanes


# ---------------------------------------------------------------------------------------------------------------- 2. finalize
FIN_GEOMS = ((1, 37), (3, 3 * 64 - 3), (257, 257 * 8 - 3), (1000, 1000 * 5 - 3))      # (rows, pixels): the last row is short


def _rows_of(y, rows):
    """(sum, sum^2) rows as a producer's epilogue leaves them: float64 sums over consecutive pixels, rounded to fp32 (as bn_slab_cases builds them)"""
    pixels, C = y.shape
    per = -(-pixels // rows)
    yd = y.double()
    st = torch.zeros(rows, C, 2, dtype=torch.float64)
    for r in range(rows):
        blk = yd[r * per:(r + 1) * per]
        st[r, :, 0] = blk.sum(0); st[r, :, 1] = (blk * blk).sum(0)
    return st.float()


def _finalize_ref(dt, st, count, gamma, beta, rm, rv, training):
    """mean, rstd, scale, shift, running_mean, running_var in dtype dt from the fp32 rows the kernel receives"""
    if training:
        tot = st.to(dt).sum(0)
        m = tot[:, 0] / count
        v = (tot[:, 1] / count - m * m).clamp(min=0)
        unb = v * count / (count - 1.0) if count > 1 else v
        nrm, nrv = (None, None) if rm is None else ((1.0 - BN_MOM) * rm.to(dt) + BN_MOM * m, (1.0 - BN_MOM) * rv.to(dt) + BN_MOM * unb)
    else:
        m, v, nrm, nrv = rm.to(dt), rv.to(dt), rm.to(dt), rv.to(dt)
    rstd = (v + BN_EPS).rsqrt()
    g = torch.ones_like(m) if gamma is None else gamma.to(dt)
    b = torch.zeros_like(m) if beta is None else beta.to(dt)
    return dict(mean=m, rstd=rstd, scale=g * rstd, shift=b - m * g * rstd, rm=nrm, rv=nrv)


def _finalize_one(dev, rows, pixels, C, family="normal", affine=True, running=True, training=1, apply=None):
    """apply = (dtype, act): rd_bn_finalize_apply (bn_slab = 2 is set by the caller) instead of rd_bn_finalize"""
    lib = _E().L()
    rs = _rs("finalize", rows, pixels, C, family, affine, running, training, str(apply))
    dtype = apply[0] if apply else F32
    y = _r(0.3 + 1.5 * _randn(rs, pixels, C), dtype)
    if family == "constant":      # every channel constant: exact values (computed variance exactly 0) and inexact ones (rounding noise of either sign)
        vals = torch.tensor([1.75, 1.1, 3.3, 0.7, 100.1, -2.6, 0.3, 17.9])
        y = _r(vals[torch.arange(C) % len(vals)].repeat(pixels, 1), dtype)
    st = _rows_of(y, rows)
    gamma, beta = (0.5 + torch.rand(C, generator=torch.Generator().manual_seed(C)), 0.5 * _randn(rs, C)) if affine else (None, None)
    rm0, rv0 = (0.25 + 0.1 * _randn(rs, C), 1.5 + 0.2 * torch.from_numpy(rs.rand(C).astype(np.float32))) if running else (None, None)
    r64, r32 = (_finalize_ref(dt, st, float(pixels), gamma, beta, rm0, rv0, training) for dt in (torch.float64, F32))
    what = "%s rows=%d pixels=%d C=%d %s affine=%s running=%s training=%d %s" % (
        "bn_finalize_apply" if apply else "bn_finalize", rows, pixels, C, family, affine, running, training, apply or "")
    grp = "bn_finalize" + (" (constant)" if family == "constant" else "")
    std = st.to(dev)
    gd, bd = (None, None) if gamma is None else (gamma.to(dev), beta.to(dev))
    RM, RV = (None, None) if rm0 is None else (Buf(dev, C, F32, rm0), Buf(dev, C, F32, rv0))
    M, R, SC, SH = (_nanbuf(dev, C, F32) for _ in range(4))
    rmp, rvp = (None, None) if RM is None else (_P(RM.v), _P(RV.v))
    if apply:
        act = apply[1]
        assert lib.rd_bn_slab_ok(pixels, C, DT[dtype]) == 1, what
        Y, Z = Buf(dev, pixels * C, dtype, y), _nanbuf(dev, pixels * C, dtype)
        _call("rd_bn_finalize_apply", _P(std), rows, _P(Y.v), _P(gd), _P(bd), BN_EPS, BN_MOM, rmp, rvp, _P(M.v), _P(R.v), _P(SC.v), _P(SH.v), _P(Z.v),
              pixels, C, act, SLOPE, DT[dtype], _S(std))
        z64, z32 = (_act(y.to(dt) * r["scale"] + r["shift"], act, SLOPE) for dt, r in ((torch.float64, r64), (F32, r32)))
        _check(what + " z", Z.v.view(pixels, C), z64, z32, "bn_finalize_apply z")
        Z.check(what); Y.check(what, unchanged=True)
    else:
        _call("rd_bn_finalize", _P(std), rows, C, float(pixels), _P(gd), _P(bd), BN_EPS, BN_MOM, training, rmp, rvp, _P(M.v), _P(R.v), _P(SC.v), _P(SH.v),
              _S(std))
    for nm, B_ in (("mean", M), ("rstd", R), ("scale", SC), ("shift", SH)):
        _check(what + " " + nm, B_.v, r64[nm], r32[nm], grp + " " + nm)
        B_.check(what)
    if RM is not None:
        if training:
            _check(what + " running_mean", RM.v, r64["rm"], r32["rm"], grp + " running_mean")
            _check(what + " running_var", RV.v, r64["rv"], r32["rv"], grp + " running_var")
            RM.check(what); RV.check(what)
        else:
            RM.check(what, unchanged=True); RV.check(what, unchanged=True)
    if family == "constant":
        tot = st.double().sum(0)
        v = tot[:, 1] / pixels - (tot[:, 0] / pixels) ** 2
        assert bool((v < 0).any()) and bool((v == 0).any()), what + ": the case must hold computed variances below and at zero"
        top = BN_EPS ** -0.5
        got = R.cpu().double()[v <= 0]
        assert bool(((got - top).abs() <= FLOOR_ULPS * EPS32 * top).all()), what + ": var must clamp to 0, rstd = 1/sqrt(eps)"


def finalize_case(dev, quick=False):
    """rd_bn_finalize from rows built in float64 (1, 3, 257, 1000 rows; the four-loads-in-flight loop needs > 768): mean, rstd, scale, shift and
    the running statistics (unbiased variance, momentum 0.1, from non-trivial values); count = 1; gamma / beta NULL; running_* NULL; training = 0
    (running statistics used and left unchanged); constant channels (computed variance zero or just below it: var clamps to 0).  Then
    rd_bn_finalize_apply on the same rows, against float64 directly: both register-set sizes, every activation, the three dtypes."""
    E = _E()
    for rows, pixels in FIN_GEOMS:
        for C in (3, 40):
            _finalize_one(dev, rows, pixels, C)
    _finalize_one(dev, 1, 1, 5)                              # count = 1: the unbiased variance equals the biased one
    _finalize_one(dev, 3, 189, 24, affine=False)
    _finalize_one(dev, 3, 189, 24, running=False)
    _finalize_one(dev, 3, 189, 24, training=0)
    _finalize_one(dev, 3, 189, 16, family="constant")
    _finalize_one(dev, 257, 2053, 16, family="constant")
    try:
        E.set_option("bn_slab", 2)
        cfgs = [(g, dt, C, act) for g in FIN_GEOMS for dt in DTYPES for C in ((8, 24) if dt == F32 else (8, 40)) for act in ACTS]
        for (rows, pixels), dt, C, act in _cover(cfgs, lambda c: [("geom", c[0], c[1]), ("act", c[3], c[1]), ("C", c[2], c[1])], quick, "fin_apply"):
            _finalize_one(dev, rows, pixels, C, apply=(dt, act))
        _finalize_one(dev, 1, 1, 8, apply=(F32, 0))
        _finalize_one(dev, 3, 189, 8, affine=False, running=False, apply=(BF16, 3))
        _finalize_one(dev, 3, 189, 16, family="constant", apply=(F32, 0))
    finally:
        E.set_option("bn_slab", None)


# ---------------------------------------------------------------------------------------------------------------- 3. affine_act / affine_act_add
NULLS = ((False, False), (True, True), (True, False), (False, True))      # (scale NULL, shift NULL)


def _affine_data(dtype, C, pixels):
    rs = _rs("affine", str(dtype), C, pixels)
    return dict(y=_r(0.3 + 1.5 * _randn(rs, pixels, C), dtype), res=_r(_randn(rs, pixels, C), dtype),
                scale=0.4 + torch.from_numpy(rs.rand(C).astype(np.float32)), shift=1.5 * _randn(rs, C))


def _affine_one(dev, dtype, C, pixels, act, with_res, nulls, d=None):
    d = d or _affine_data(dtype, C, pixels)
    sc, sh = (None if nulls[0] else d["scale"]), (None if nulls[1] else d["shift"])
    refs = []
    for dt in (torch.float64, F32):
        u = d["y"].to(dt)
        if sc is not None:
            u = u * sc.to(dt)
        if sh is not None:
            u = u + sh.to(dt)
        refs.append(_act(u + d["res"].to(dt) if with_res else u, act, SLOPE))
    Y, O = Buf(dev, pixels * C, dtype, d["y"]), _nanbuf(dev, pixels * C, dtype)
    Rb = Buf(dev, pixels * C, dtype, d["res"]) if with_res else None
    what = "affine_act %s pixels=%d C=%d act=%d residual=%s scale/shift NULL=%s" % (dtype, pixels, C, act, with_res, nulls)
    scd, shd = (None if sc is None else sc.to(dev)), (None if sh is None else sh.to(dev))      # (held: a temporary's memory is reused at once)
    _call("rd_affine_act", _P(Y.v), _P(scd), _P(shd), _P(Rb.v if Rb else None), _P(O.v),
          pixels, C, act, SLOPE, DT[dtype], _S(Y.v))
    _check(what, O.v.view(pixels, C), refs[0], refs[1], "affine_act")
    O.check(what); Y.check(what, unchanged=True)
    if Rb:
        Rb.check(what, unchanged=True)


def _affine_add_one(dev, dtype, C, pixels, act1, act2, d=None):
    lib = _E().L()
    d = d or _affine_data(dtype, C, pixels)
    slope2 = float(np.float32(0.1))
    Y, Rb, O = Buf(dev, pixels * C, dtype, d["y"]), Buf(dev, pixels * C, dtype, d["res"]), _nanbuf(dev, pixels * C, dtype)
    scd, shd = d["scale"].to(dev), d["shift"].to(dev)
    args = (_P(Y.v), _P(scd), _P(shd), act1, SLOPE, _P(Rb.v), _P(O.v), pixels, C, act2, slope2, DT[dtype], _S(Y.v))
    what = "affine_act_add %s pixels=%d C=%d act1=%d act2=%d" % (dtype, pixels, C, act1, act2)
    if lib.rd_affine_act_add_ok(C, DT[dtype]) == 0:
        assert C not in CH[dtype]["vec"], what
        _refused("rd_affine_act_add", "has no vector form", *args)
        O.check(what, unchanged=True)
        return
    assert C in CH[dtype]["vec"], what
    _call("rd_affine_act_add", *args)
    z64 = _act(d["y"].double() * d["scale"].double() + d["shift"].double(), act1, SLOPE)
    z32 = _act(d["y"] * d["scale"] + d["shift"], act1, SLOPE)
    r64 = _act(z64.to(dtype).double() + d["res"].double(), act2, slope2)      # z rounded to the activation type, as rd_affine_act stores it
    r32 = _act(z32.to(dtype).float() + d["res"], act2, slope2)
    _check_rounded_z(what, O.v.view(pixels, C), r64, r32, z64, z32, "affine_act_add")
    O.check(what); Y.check(what, unchanged=True); Rb.check(what, unchanged=True)


def _form_cfgs(dtypes, forms, quick=False):
    return [(dt, f, C, p) for dt in dtypes for f in forms for C in CH[dt][f] for p in _pixels(C, quick)]


def affine_case(dev, quick=False, dtypes=DTYPES, forms=FORMS):
    """rd_affine_act: forms x dtypes x activations x residual absent / present x the four scale / shift NULL patterns (NULLS; the pattern is part
    of the config, and the covering selection shows each one in every (form, dtype) class), and rd_affine_act_add for every channel count: refused where rd_affine_act_add_ok says 0, otherwise against a
    reference that rounds the intermediate z to the activation type.  Full mode adds, per form, a size past the 2048-block grid cap."""
    for dt in dtypes:
        for f in forms:
            for C in CH[dt][f]:
                _assert_form(C, dt, f)
    base = _form_cfgs(dtypes, forms, quick)
    cfgs = [c + (act, res, ni) for c in base for act in ACTS for res in (False, True) for ni in range(len(NULLS))]
    fd = lambda c: (c[0], c[1])      # noqa: E731
    sel = _cover(cfgs, lambda c: [("C", c[0], c[2]), ("act", fd(c), c[4]), ("pix", fd(c), c[3]), ("res", fd(c), c[5]), ("null", fd(c), c[6]), ("act-res", c[4], c[5]), ("res-null", c[5], c[6])],
                 quick, "affine", lambda c: _wide(c[0], c[2]))
    cache = {}
    for dt, f, C, p, act, res, ni in sel:
        if (dt, C, p) not in cache:
            cache.clear(); cache[(dt, C, p)] = _affine_data(dt, C, p)
        _affine_one(dev, dt, C, p, act, res, NULLS[ni], cache[(dt, C, p)])
    pairs = tuple((a, a) for a in ACTS) + ((3, 1), (2, 0))
    cfgs = [c + pr for c in base for pr in pairs]
    for dt, f, C, p, a1, a2 in _cover(cfgs, lambda c: [("C", c[0], c[2]), ("acts", fd(c), c[4:]), ("pix", fd(c), c[3])], quick, "affine_add",
                                         lambda c: _wide(c[0], c[2])):
        _affine_add_one(dev, dt, C, p, a1, a2)
    if not quick:
        for dt in dtypes:
            ve = _ve(dt)
            big = dict(vec=[(16, (2048 * 1024 + 300) * ve // 16)],                                        # ew_grid_per(nvec, 4): four vectors per thread
                       gen=[(288, 2048 * 8 * 3 + 8)] if dt == F32 else [(1392, 2048 * 8 + 8)],            # gen_ppt() = 8 pixels per thread
                       scalar=[(6, 2048 * 256 // 6 + 3000), (1028 if dt == F32 else 2056, 2048 * 1024 // 1028 + 60)])      # ew_grid, one element / four
            for f in forms:
                for C, p in big[f]:
                    assert p * C * (4 if dt == F32 else 2) < 64 * 2 ** 20
                    _affine_one(dev, dt, C, p, 3, f != "gen", NULLS[0])
            if "vec" in forms:
                _affine_add_one(dev, dt, 64, (2048 * 256 + 300) * ve // 64, 2, 2)                          # ew_grid(nvec)


# ---------------------------------------------------------------------------------------------------------------- 4. backward
def _bwd_data(dtype, C, pixels, exact=False):
    """y, dz and the fp32 mean / rstd / scale / shift that are passed in.  y is drawn so that no activation argument scale * y + shift lies within
    0.01 of 0 or within 1 % of 6 (elements that do are drawn again): the derivative is then the same whether it is taken from z or recomputed
    from y, in any arithmetic, and no 16-bit rounding of z onto 6.0 can decide it.  exact: the integer threshold data of thresholds_case."""
    rs = _rs("bwd", str(dtype), C, pixels, exact)
    if exact:
        y, dz = _ints(rs, -2, 8, pixels, C), _ints(rs, -4, 4, pixels, C)
        y.reshape(-1)[:4] = torch.tensor([0.0, 6.0, -0.0, 5.0])[:min(4, y.numel())]
        one, zero = torch.ones(C), torch.zeros(C)
        return dict(y=y, dz=dz, mean=zero, rstd=one, scale=one.clone(), shift=zero.clone())
    mean = 0.3 + 0.1 * _randn(rs, C)
    rstd = (1.0 / 1.5) * (1.0 + 0.1 * torch.from_numpy(rs.rand(C).astype(np.float32)))
    gamma, beta = 0.5 + torch.from_numpy(rs.rand(C).astype(np.float32)), 0.5 * _randn(rs, C)
    scale = (gamma.double() * rstd.double()).float()
    shift = (beta.double() - mean.double() * scale.double()).float()
    y = _r(0.3 + 1.5 * _randn(rs, pixels, C), dtype)
    while True:
        u = y.double() * scale.double() + shift.double()
        bad = (u.abs() < 0.01) | ((u - 6.0).abs() < 0.06)
        if not bool(bad.any()):
            break
        y = torch.where(bad, _r(0.3 + 1.5 * _randn(rs, pixels, C), dtype), y)
    return dict(y=y, dz=_r(_randn(rs, pixels, C), dtype), mean=mean, rstd=rstd, scale=scale, shift=shift)


def _bwd_ref(dt, d, act, slope, prev=None, rows=None):
    """g = dz act'; dbeta = sum g; dgamma = sum g xhat; dy = scale (g - mean(g) - xhat mean(g xhat)); xhat = (y - mean) rstd; dres = g.
    rows: the (sum g, sum g xhat) partial rows handed to rd_bn_act_bwd_from_partial stand in for the sums."""
    y, dz, mean, rstd, scale, shift = (d[k].to(dt) for k in ("y", "dz", "mean", "rstd", "scale", "shift"))
    count = float(y.shape[0])
    g = dz * _dact(y * scale + shift, act, slope)
    xh = (y - mean) * rstd
    db, dg = (g.sum(0), (g * xh).sum(0)) if rows is None else (rows.to(dt).sum(0)[:y.shape[1], 0], rows.to(dt).sum(0)[:y.shape[1], 1])
    dy = scale * (g - db / count - xh * (dg / count))
    if prev is not None:
        dg, db = dg + prev[0].to(dt), db + prev[1].to(dt)
    return dict(dy=dy, dres=g, dgamma=dg, dbeta=db)


class _BwdBufs(object):
    def __init__(self, dev, dtype, C, pixels, rows, prev, dres):
        n = pixels * C
        self.DY, self.DR = _nanbuf(dev, n, dtype), (_nanbuf(dev, n, dtype) if dres else None)
        self.DG, self.DB = Buf(dev, C, F32, prev[0]), Buf(dev, C, F32, prev[1])
        self.PT, self.CF = (_nanbuf(dev, rows * C * 2, F32) if rows else None), (_nanbuf(dev, 2 * C, F32) if rows is not None else None)
        self.all = [b for b in (self.DY, self.DR, self.DG, self.DB, self.PT, self.CF) if b is not None]

    def check(self, what, scratch_written=True):
        for b in self.all:
            b.check(what)
        for b in (self.PT, self.CF):
            if b is not None and scratch_written:
                assert bool(torch.isfinite(b.cpu()).all()), what + ": a partial-row / coefficient element was not written"


def _bwd_call(dev, fn, d, dtype, act, slope, acc, dres, phases=None, rows_in=None, use_z=True):
    """one backward call on fresh guarded buffers -> (_BwdBufs, prev)"""
    lib = _E().L()
    pixels, C = d["y"].shape
    prev = (torch.full((C,), 2.0) + torch.arange(C) * 0.125, torch.full((C,), -3.0) + torch.arange(C) * 0.25)
    dv = {k: v.to(dev).to(dtype if k in ("y", "dz") else F32) for k, v in d.items()}
    z = _r(_act(d["y"].double() * d["scale"].double() + d["shift"].double(), act, slope).float(), dtype).to(dev).to(dtype) if use_z else None
    rows = {"rd_bn_act_bwd_slab": None, "rd_bn_act_bwd_from_partial": 0}.get(fn, lib.rd_bn_bwd_rows(pixels, C))
    B = _BwdBufs(dev, dtype, C, pixels, rows, prev, dres)
    st, tail = _S(dv["y"]), (pixels, C, act, slope, DT[dtype])
    stat = (_P(dv["mean"]), _P(dv["rstd"]), _P(dv["scale"]))
    grads = (_P(B.DG.v), _P(B.DB.v), acc, _P(B.DY.v))
    if fn == "rd_bn_act_bwd":
        _call(fn, _P(dv["dz"]), _P(z), _P(dv["y"]), *stat, _P(B.PT.v), _P(B.CF.v), *grads, _P(B.DR.v if dres else None), *tail, st)
    elif fn == "rd_bn_act_bwd_recompute":
        _call(fn, _P(dv["dz"]), _P(z), _P(dv["y"]), *stat, _P(dv["shift"]), _P(B.PT.v), _P(B.CF.v), *grads, _P(B.DR.v if dres else None), *tail, st)
    elif fn == "rd_bn_act_bwd_recompute_phases":
        for ph in phases:
            _call(fn, _P(dv["dz"]), _P(z), _P(dv["y"]), *stat, _P(dv["shift"]), _P(B.PT.v), _P(B.CF.v), *grads, _P(B.DR.v if dres else None), *tail, ph, st)
    elif fn == "rd_bn_act_bwd_from_partial":
        rd = rows_in.to(dev)
        B.keep = rd
        _call(fn, _P(dv["dz"]), _P(dv["y"]), *stat, _P(dv["shift"]), _P(rd), rows_in.shape[0], rows_in.shape[1], _P(B.CF.v), *grads, *tail, st)
    else:
        _call(fn, _P(dv["dz"]), _P(dv["y"]), *stat, _P(dv["shift"]), *grads, *tail, st)
    return B, prev


def _partial_rows(d, act, slope, nrows, extra):
    """(sum g, sum g xhat) rows of `nrows` pixel ranges with `extra` unused trailing channels (NaN: they must not be read), float64 -> fp32"""
    pixels, C = d["y"].shape
    y, dz, mean, rstd, scale, shift = (d[k].double() for k in ("y", "dz", "mean", "rstd", "scale", "shift"))
    g = dz * _dact(y * scale + shift, act, slope)
    gx = g * ((y - mean) * rstd)
    per = -(-pixels // nrows)
    rows = torch.full((nrows, C + extra, 2), NAN, dtype=torch.float64)
    for r in range(nrows):
        rows[r, :C, 0] = g[r * per:(r + 1) * per].sum(0); rows[r, :C, 1] = gx[r * per:(r + 1) * per].sum(0)
    return rows.float()


def _bwd_one(dev, dtype, C, pixels, act, fn, acc, dres):
    lib = _E().L()
    d = _bwd_data(dtype, C, pixels)
    whole = C % _ve(dtype) == 0
    what = "%s %s pixels=%d C=%d act=%d accumulate=%d dres=%s" % (fn, dtype, pixels, C, act, acc, dres)
    rows_in = None
    if fn == "rd_bn_act_bwd_from_partial":
        assert _bwd_runs(dtype, C, act, fn)      # (refused otherwise: thresholds_case checks the refusal)
        rows_in = _partial_rows(d, act, SLOPE, 1 if pixels < 3 else 3, 8)
        dres = False
    if fn == "rd_bn_act_bwd_slab":
        assert whole
        assert lib.rd_bn_slab_ok(pixels, C, DT[dtype]) == 1, what
        dres = False
    # recompute: z is only consulted by the scalar fall-back; NULL otherwise
    use_z = fn == "rd_bn_act_bwd" or (fn == "rd_bn_act_bwd_recompute" and not _recomputes(C, dtype))
    B, prev = _bwd_call(dev, fn, d, dtype, act, SLOPE, acc, dres, rows_in=rows_in, use_z=use_z)
    rows_ref = None if rows_in is None else torch.nan_to_num(rows_in, nan=0.0)
    r64, r32 = (_bwd_ref(dt, d, act, SLOPE, prev if acc else None, rows_ref) for dt in (torch.float64, F32))
    grp = "bn bwd"
    _check(what + " dy", B.DY.v.view(pixels, C), r64["dy"], r32["dy"], grp + " dy")
    if dres:
        _check(what + " dres", B.DR.v.view(pixels, C), r64["dres"], r32["dres"], grp + " dres")
    _check(what + " dgamma", B.DG.v, r64["dgamma"], r32["dgamma"], grp + " dgamma")
    _check(what + " dbeta", B.DB.v, r64["dbeta"], r32["dbeta"], grp + " dbeta")
    B.check(what)
    return True


BWD_FNS = ("rd_bn_act_bwd", "rd_bn_act_bwd_recompute", "rd_bn_act_bwd_from_partial", "rd_bn_act_bwd_slab")


def _bwd_runs(dtype, C, act, fn):
    """from_partial has no z: with an activation it needs a kernel that recomputes it; the one-launch form needs whole vectors"""
    if fn == BWD_FNS[2]:
        return act == 0 or _recomputes(C, dtype)
    return fn != BWD_FNS[3] or C % _ve(dtype) == 0


def backward_case(dev, quick=False, dtypes=DTYPES, forms=FORMS, acts=ACTS):
    """rd_bn_act_bwd (reads z), rd_bn_act_bwd_recompute (z NULL where the channel count allows, shift given), rd_bn_act_bwd_from_partial (rows
    computed here in float64, row_channels = C + 8) and rd_bn_act_bwd_slab (bn_slab = 2): dy, the optional dres, dgamma / dbeta with accumulate
    0 and 1 from prefilled values, against the float64 restatement.  Full mode adds, per form, a size past the apply kernels' 2048-block cap."""
    E = _E()
    for dt in dtypes:
        for f in forms:
            for C in CH[dt][f]:
                _assert_form(C, dt, f)
    cfgs = [c + (act, fn, acc, dres) for c in _form_cfgs(dtypes, forms, quick) for act in acts for fn in BWD_FNS for acc in (0, 1) for dres in (False, True)
            if not (dres and fn in BWD_FNS[2:]) and _bwd_runs(c[0], c[2], act, fn)]
    fd = lambda c: (c[0], c[1])      # noqa: E731
    sel = _cover(cfgs, lambda c: [("C", c[0], c[2]), ("pix", c[3])] if _wide(c[0], c[2]) else
                 [("C", c[0], c[2]), ("act", fd(c), c[4]), ("pix", fd(c), c[3]), ("fn", fd(c), c[5]), ("acc", c[0], c[5], c[6]), ("dres", c[0], c[5], c[7])],
                 quick, "bwd", lambda c: _wide(c[0], c[2]))
    ran = set()
    try:
        E.set_option("bn_slab", 2)
        for dt, f, C, p, act, fn, acc, dres in sel:
            if _bwd_one(dev, dt, C, p, act, fn, acc, dres):
                ran.add((dt, f, fn))
        if not quick and 3 in acts:
            for dt in dtypes:
                ve = _ve(dt)
                big = dict(vec=[(16, (2048 * 512 + 300) * ve // 16)],                                      # ew_grid_per(nvec, 2)
                           gen=[(288, 2048 * 2 * 3 + 8)] if dt == F32 else [(1392, 2048 * 2 + 8)],         # two pixels per thread
                           scalar=[(6, 2048 * 256 // 6 + 3000), (1028 if dt == F32 else 2056, 2048 * 1024 // 1028 + 60)])
                for f in forms:
                    for C, p in big[f]:
                        assert p * C * (4 if dt == F32 else 2) < 64 * 2 ** 20
                        _bwd_one(dev, dt, C, p, 3, BWD_FNS[1 if f != "scalar" or C > 256 else 0], 1, True)
    finally:
        E.set_option("bn_slab", None)
    for dt in dtypes:      # every function ran in every (form, dtype) class it supports (quick: on the narrow channel counts)
        for f in forms:
            for fn in BWD_FNS:
                if any(_bwd_runs(dt, C, a, fn) for a in acts for C in CH[dt][f] if not (quick and _wide(dt, C))):
                    assert (dt, f, fn) in ran, "no %s case ran for %s %s" % (fn, f, dt)


# ---------------------------------------------------------------------------------------------------------------- 5. thresholds
def thresholds_case(dev, quick=False, dtypes=DTYPES, forms=FORMS):
    """Integer y, scale = 1, shift = 0, integer dz, slope 0.25: activation arguments land exactly on 0 and on 6 and every product is exact.  All
    backward forms and dtypes return exactly act_grad_from_out's convention (strictly z > 0, strictly z < 6): dres of rd_bn_act_bwd and
    rd_bn_act_bwd_recompute, dy of rd_bn_act_bwd_from_partial on zero rows (dy = g), dbeta of rd_bn_act_bwd_slab.  The last is weaker than the
    others: the one-launch form has no dres and its dy is not exact on these inputs, so what is exact is the column sum of g -- errors of single
    elements that cancel within a channel would pass it (backward_case compares its dy element by element, away from the thresholds)."""
    E = _E()
    slope = 0.25
    cfgs = [(dt, f, C, p, act) for dt in dtypes for f in forms for C in CH[dt][f] for p in ((65,) if quick and C > 256 else (65, 257)) for act in ACTS]
    try:
        E.set_option("bn_slab", 2)
        for dt, f, C, p, act in _cover(cfgs, lambda c: [("C", c[0], c[2]), ("act", c[0], c[1], c[4]), ("pix", c[0], c[1], c[3])], quick, "thresholds",
                                         lambda c: None if c[2] <= 300 else ((c[0], c[2]) if c[0] == F32 else "left to the GPU twin")):
            _assert_form(C, dt, f)
            d = _bwd_data(dt, C, p, exact=True)
            whole, rec = C % _ve(dt) == 0, _recomputes(C, dt)
            g = d["dz"] * _dact(d["y"], act, slope)
            what = "thresholds %s pixels=%d C=%d act=%d" % (dt, p, C, act)
            assert bool((d["y"] == 0).any()) and bool((d["y"] == 6).any())
            for fn, use_z in (("rd_bn_act_bwd", True), ("rd_bn_act_bwd_recompute", not rec)):
                B, _ = _bwd_call(dev, fn, d, dt, act, slope, 0, True, use_z=use_z)
                _exact(what + " " + fn + " dres", B.DR.v.view(p, C), g)
                B.check(what)
            if rec or not act:
                B, _ = _bwd_call(dev, "rd_bn_act_bwd_from_partial", d, dt, act, slope, 0, False, rows_in=torch.zeros(2, C + 4, 2))
                _exact(what + " from_partial dy", B.DY.v.view(p, C), g)
                B.check(what)
            if whole:
                B, _ = _bwd_call(dev, "rd_bn_act_bwd_slab", d, dt, act, slope, 0, False)
                _exact(what + " slab dbeta", B.DB.v, g.sum(0))
                B.check(what)
            if act and not rec:      # no z to read and no kernel that recomputes it from y: refused, nothing written
                dv = {k: v.to(dev).to(dt if k in ("y", "dz") else F32) for k, v in d.items()}
                O, CF = _nanbuf(dev, p * C, dt), _nanbuf(dev, 2 * C, F32)
                rows = torch.zeros(2, C, 2, device=dev)
                _refused("rd_bn_act_bwd_recompute", "this channel count needs z", _P(dv["dz"]), None, _P(dv["y"]), _P(dv["mean"]), _P(dv["rstd"]), _P(dv["scale"]),
                         _P(dv["shift"]), _P(rows), _P(CF.v), None, None, 0, _P(O.v), None, p, C, act, slope, DT[dt], _S(rows))
                _refused("rd_bn_act_bwd_from_partial", "this channel count needs z", _P(dv["dz"]), _P(dv["y"]), _P(dv["mean"]), _P(dv["rstd"]), _P(dv["scale"]),
                         _P(dv["shift"]), _P(rows), 2, C, _P(CF.v), None, None, 0, _P(O.v), p, C, act, slope, DT[dt], _S(rows))
                O.check(what, unchanged=True); CF.check(what, unchanged=True)
    finally:
        E.set_option("bn_slab", None)


# ---------------------------------------------------------------------------------------------------------------- 6. phases
def phases_case(dev, quick=False):
    """rd_bn_act_bwd_recompute_phases with phases 1, then 2, then 4 is bit-identical to phases = 7 and to rd_bn_act_bwd_recompute: dy, dres, dgamma,
    dbeta (accumulating), the partial rows and the coefficients."""
    cfgs = [(dt, f, CH[dt][f][1 if f != "scalar" else 0], p, act) for dt in DTYPES for f in FORMS for p in (65, 1000) for act in (0, 2, 3)]
    for dt, f, C, p, act in _cover(cfgs, lambda c: [("fd", c[0], c[1]), ("act", c[4], c[1]), ("pix", c[3], c[1])], quick, "phases"):
        d = _bwd_data(dt, C, p)
        use_z = not _recomputes(C, dt)
        runs = [_bwd_call(dev, "rd_bn_act_bwd_recompute_phases", d, dt, act, SLOPE, 1, True, phases=ph, use_z=use_z)[0] for ph in ((1, 2, 4), (7,))]
        runs.append(_bwd_call(dev, "rd_bn_act_bwd_recompute", d, dt, act, SLOPE, 1, True, use_z=use_z)[0])
        what = "phases %s pixels=%d C=%d act=%d" % (dt, p, C, act)
        for other, nm in ((runs[1], "phases = 7"), (runs[2], "rd_bn_act_bwd_recompute")):
            for a, b in zip(runs[0].all, other.all):
                _exact(what + ": phases 1, 2, 4 against " + nm, a.v, b.v)
        for B in runs:
            B.check(what)


# ---------------------------------------------------------------------------------------------------------------- 7. conditioning
def conditioning_case(dev, quick=False):
    """rd_bn_stats -> rd_bn_finalize end to end in fp32 on inputs of std 0.1 and mean 3 / 30 (|mean| / std = 30 / 300).  The variance is taken as
    E[y^2] - E[y]^2 from fp32 (sum, sum^2) rows, which loses digits with the square of that ratio, so torch's accuracy is out of reach by design.
    The yardstick is a restatement of the documented FORMAT, not of the kernel: per partial row the sum and the sum of squares in SEQUENTIAL
    fp32 (np.cumsum, not the pairwise np.sum), rows combined in float64, var = E2 - m^2 clamped at 0.  The kernel's rstd error against float64
    must not exceed the restatement's own, with no extra margin; rstd is finite and at most 1/sqrt(eps) (var >= 0); the mean meets _check.
    (mean 100 is left out: there the restatement itself collapses, var clamped to 0.)"""
    lib = _E().L()
    for pixels, C in ((700, 24), (5000, 16)):
        for mu in (3.0, 30.0):
            y = (mu + 0.1 * _randn(_rs("conditioning", pixels, C, mu), pixels, C)).float()
            rows = lib.rd_dw_rows(pixels, C)
            Y, PT = Buf(dev, pixels * C, F32, y), _nanbuf(dev, rows * C * 2, F32)
            M, R, SC, SH = (_nanbuf(dev, C, F32) for _ in range(4))
            what = "conditioning mean=%g %dx%d" % (mu, pixels, C)
            _call("rd_bn_stats", _P(Y.v), _P(PT.v), pixels, C, 0, _S(Y.v))
            _call("rd_bn_finalize", _P(PT.v), rows, C, float(pixels), None, None, BN_EPS, BN_MOM, 1, None, None, _P(M.v), _P(R.v), _P(SC.v), _P(SH.v), _S(Y.v))
            for b_ in (PT, M, R, SC, SH):
                b_.check(what)
            yd = y.double()
            m64 = yd.mean(0)
            rstd64 = ((yd - m64).pow(2).mean(0) + BN_EPS).rsqrt()
            per = -(-pixels // rows)
            yn = y.numpy()
            s = np.zeros((rows, C), np.float32); q = np.zeros((rows, C), np.float32)
            for r in range(rows):
                blk = yn[r * per:(r + 1) * per]
                if len(blk):
                    s[r] = np.cumsum(blk, axis=0, dtype=np.float32)[-1]; q[r] = np.cumsum(blk * blk, axis=0, dtype=np.float32)[-1]
            mr = s.astype(np.float64).sum(0) / pixels
            vr = np.maximum(q.astype(np.float64).sum(0) / pixels - mr * mr, 0.0)
            rstd_r = torch.from_numpy(1.0 / np.sqrt(vr + BN_EPS))
            _, _, rstd_t = torch.native_batch_norm(y, None, None, None, None, True, BN_MOM, BN_EPS)
            rel = lambda a: float(((a.double() - rstd64).abs() / rstd64).max())      # noqa: E731
            got = R.cpu()
            ek, er, et = rel(got), rel(rstd_r), rel(rstd_t)
            MEASURED["rstd %s (kernel)" % what[13:]] = [et, ek]
            MEASURED["rstd %s (fp32 rows)" % what[13:]] = [et, er]
            print("bn %s: rstd error kernel %.3e, fp32-row restatement %.3e, torch fp32 %.3e" % (what, ek, er, et))
            assert bool(torch.isfinite(got).all()) and float(got.max()) <= BN_EPS ** -0.5 * (1.0 + FLOOR_ULPS * EPS32), what + ": rstd not finite or var < 0"
            _check(what + " mean", M.v, m64, y.mean(0), "bn conditioning mean")
            assert ek <= er, "%s: rstd error %.3e exceeds the fp32-row format's own %.3e (torch fp32: %.3e)" % (what, ek, er, et)


def report_bn():
    report()
    for k in sorted(CENSUS):
        v = CENSUS[k]
        print("bn census %-8s max |mean| * rstd %.3f at %s (%d finalize calls, %d BatchNorm layers)" % (k, v[0], v[1], v[2], v[3]))
