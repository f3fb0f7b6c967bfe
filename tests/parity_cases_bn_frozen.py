"""Direct parity cases for rd_bn_act_bwd_frozen, the backward through a BatchNorm that normalised with its running statistics: one pass over
(dz, y) writes dy = scale * g (and dres = g for a layer with a residual) and, when gamma / beta want gradients, the (sum g, sum g * xhat) rows
the family's finalize launch sums.  Harness, data, channel counts, pixel counts and bound are those of tests/parity_cases_bn.py, imported and
unchanged: guarded NaN-prefilled buffers, `_bwd_data` (every activation argument away from the kinks), `_check` (4 x torch's fp32 error,
floored, plus half an ulp of a 16-bit output).  What is new is the reference: torch autograd in float64 through
F.batch_norm(training=False) + activation (+ residual), built from the rounded inputs the kernel receives -- running_var, gamma and beta are
recovered in float64 from the fp32 (mean, rstd, scale, shift) that are passed in; the fp32 reference runs the same graph in fp32.

A layer with a residual hands the kernel z and gets dres back; as in parity_cases_bn the residual is zero, so z = act(scale * y + shift) stays
away from the kinks however it is rounded.  Without dres z is NULL for EVERY channel count, the scalar form included.
"""
import torch
import torch.nn.functional as F

from tests import parity_cases_bn as B
from tests.parity_cases_glue import F32, Buf, _call, _check, _E, _exact, _P, _refused, _S

FN = "rd_bn_act_bwd_frozen"


def _assert_form(C, dtype, form):
    """the channel count runs the form it is listed under, whatever the flags (bit 0: sums wanted, bit 1: dres given)"""
    lib = _E().L()
    assert C in B.CH[dtype][form]
    for flag in (0, 1, 2, 3):
        for act in (0, 3):
            name = lib.rd_bn_kernel_name(3, C, B.DT[dtype], act, flag).decode()
            assert name.startswith("bn_frozen_bwd_") and B._form_of(name) == form, "C=%d %s is listed as %s but routed to %s" % (C, dtype, form, name)


def _ref(dt, d, act, slope, with_res):
    """torch autograd in `dt` through F.batch_norm(training=False) + activation (+ a zero residual) -> dy, dres, dgamma, dbeta"""
    pixels, C = d["y"].shape
    mean, rstd, scale, shift = (d[k].double() for k in ("mean", "rstd", "scale", "shift"))
    var = 1.0 / (rstd * rstd) - B.BN_EPS                 # rstd = 1 / sqrt(var + eps)
    gamma = (scale / rstd).to(dt).requires_grad_()       # scale = gamma * rstd
    beta = (shift + mean * scale).to(dt).requires_grad_()      # shift = beta - mean * scale
    y = d["y"].to(dt).requires_grad_()
    res = torch.zeros(pixels, C, dtype=dt, requires_grad=True)
    nchw = lambda a: a.t().reshape(1, C, pixels, 1)      # noqa: E731
    u = F.batch_norm(nchw(y), mean.to(dt), var.to(dt), gamma, beta, False, B.BN_MOM, B.BN_EPS)
    z = B._act(u + nchw(res) if with_res else u, act, slope)
    z.backward(nchw(d["dz"].to(dt)))
    return dict(dy=y.grad, dres=res.grad if with_res else None, dgamma=gamma.grad, dbeta=beta.grad)


class _Bufs(object):
    """guarded, NaN-prefilled outputs; without sums the row / gradient buffers are decoys that are NOT passed and must stay untouched"""

    def __init__(self, dev, dtype, C, pixels, prev, with_res):
        n = pixels * C
        self.rows = _E().L().rd_bn_bwd_rows(pixels, C)
        self.DY, self.DR = B._nanbuf(dev, n, dtype), (B._nanbuf(dev, n, dtype) if with_res else None)
        self.DG, self.DB = Buf(dev, C, F32, prev[0]), Buf(dev, C, F32, prev[1])
        self.PT = B._nanbuf(dev, self.rows * C * 2, F32)

    def check(self, what, sums):
        self.DY.check(what)
        if self.DR is not None:
            self.DR.check(what)
        for b in (self.DG, self.DB, self.PT):
            b.check(what, unchanged=not sums)
        if sums:
            assert bool(torch.isfinite(self.PT.cpu()).all()), what + ": a partial-row element was not written"


def _prev(C):
    return torch.full((C,), 2.0) + torch.arange(C) * 0.125, torch.full((C,), -3.0) + torch.arange(C) * 0.25


def _run(dev, d, dtype, act, slope, with_res, sums, acc):
    """one call on fresh buffers.  with_res: z given, dres written; otherwise z NULL.  sums False: partial, dgamma, dbeta NULL."""
    pixels, C = d["y"].shape
    prev = _prev(C)
    dv = {k: v.to(dev).to(dtype if k in ("y", "dz") else F32) for k, v in d.items()}
    z = None
    if with_res:
        z = B._r(B._act(d["y"].double() * d["scale"].double() + d["shift"].double(), act, slope).float(), dtype).to(dev).to(dtype)
    bufs = _Bufs(dev, dtype, C, pixels, prev, with_res)
    _call(FN, _P(dv["dz"]), _P(z), _P(dv["y"]), _P(dv["mean"]), _P(dv["rstd"]), _P(dv["scale"]), _P(dv["shift"]),
          _P(bufs.PT.v if sums else None), _P(bufs.DG.v if sums else None), _P(bufs.DB.v if sums else None), acc, _P(bufs.DY.v),
          _P(bufs.DR.v if with_res else None), pixels, C, act, slope, B.DT[dtype], _S(dv["y"]))
    return bufs, prev


def _one(dev, dtype, C, pixels, act, with_res, sums, acc, refs):
    key = (dtype, C, pixels, act, with_res)
    if key not in refs:      # one reference per tensor set, shared by the sums / accumulate variants and left unchanged
        refs.clear()
        d = B._bwd_data(dtype, C, pixels)
        refs[key] = (d, _ref(torch.float64, d, act, B.SLOPE, with_res), _ref(F32, d, act, B.SLOPE, with_res))
    d, r64, r32 = refs[key]
    what = "%s %s pixels=%d C=%d act=%d residual=%s sums=%s accumulate=%d" % (FN, dtype, pixels, C, act, with_res, sums, acc)
    bufs, prev = _run(dev, d, dtype, act, B.SLOPE, with_res, sums, acc)
    grp = "bn frozen bwd"
    _check(what + " dy", bufs.DY.v.view(pixels, C), r64["dy"], r32["dy"], grp + " dy")
    if with_res:
        _check(what + " dres", bufs.DR.v.view(pixels, C), r64["dres"], r32["dres"], grp + " dres")
    if sums:
        add = (lambda g, p: g + p.to(g.dtype)) if acc else (lambda g, p: g)
        _check(what + " dgamma", bufs.DG.v, add(r64["dgamma"], prev[0]), add(r32["dgamma"], prev[0]), grp + " dgamma")
        _check(what + " dbeta", bufs.DB.v, add(r64["dbeta"], prev[1]), add(r32["dbeta"], prev[1]), grp + " dbeta")
    bufs.check(what, sums)


def _big(dt):
    """per form a size whose no-sums launch reaches a second grid-stride iteration (2048 blocks x two vectors / two pixels per thread);
    the scalar form and every sums launch walk a pixel range per block, many iterations at any of the sizes"""
    ve = B._ve(dt)
    return dict(vec=[(16, (2048 * 512 + 300) * ve // 16)],
                gen=[(288, 2048 * 2 * 3 + 8)] if dt == F32 else [(1392, 2048 * 2 + 8)],
                scalar=[(6, 2048 * 256 // 6 + 3000)])


def backward_case(dev, quick=False, dtypes=B.DTYPES, forms=B.FORMS, acts=B.ACTS):
    """dtypes x forms (channel counts of B.CH, each asserted to run its form) x activations x {no residual, z NULL | residual, dres} x
    {sums, no sums} x accumulate 0 / 1 at B._pixels, against float64 autograd.  quick: the covering selection of the emulator twin."""
    for dt in dtypes:
        for f in forms:
            for C in B.CH[dt][f]:
                _assert_form(C, dt, f)
    cfgs = [c + (act, res, sums, acc) for c in B._form_cfgs(dtypes, forms, quick) for act in acts for res in (False, True) for sums in (True, False)
            for acc in (0, 1)]
    fd = lambda c: (c[0], c[1])      # noqa: E731
    sel = B._cover(cfgs, lambda c: [("C", c[0], c[2]), ("pix", c[3])] if B._wide(c[0], c[2]) else
                   [("C", c[0], c[2]), ("act", fd(c), c[4], c[5]), ("pix", fd(c), c[3]), ("res-sums", fd(c), c[5], c[6]), ("acc", c[0], c[6], c[7])],
                   quick, "frozen_bwd", lambda c: B._wide(c[0], c[2]))
    refs, ran = {}, set()
    for dt, f, C, p, act, res, sums, acc in sel:
        _one(dev, dt, C, p, act, res, sums, acc, refs)
        ran.add((dt, f, res, sums))
    if not quick and 3 in acts:
        for dt in dtypes:
            for f in forms:
                for C, p in _big(dt)[f]:
                    assert p * C * (4 if dt == F32 else 2) < 64 * 2 ** 20
                    _one(dev, dt, C, p, 3, False, False, 0, refs)
                    _one(dev, dt, C, p, 3, True, True, 1, refs)
    for dt in dtypes:
        for f in forms:
            for res in (False, True):
                for sums in (False, True):
                    assert (dt, f, res, sums) in ran, "no case ran for %s %s residual=%s sums=%s" % (f, dt, res, sums)


def thresholds_case(dev, quick=False, dtypes=B.DTYPES, forms=B.FORMS):
    """B._bwd_data(exact=True): integer y holding 0, 6 and -0, unit scale, integer dz, slope 0.25 -- every product is exact and activation
    arguments sit on the kinks.  dy and dres equal g = dz * act'(.) bit for bit, with act' in act_grad_from_out's convention (strictly > 0,
    strictly < 6) whether it is recomputed from y or read from z; dres is also bit-equal to rd_bn_act_bwd_recompute's, whose dy differs from
    scale * g only by the two batch-mean terms the frozen form does not have.  Then the refusal: dres given with z NULL writes nothing."""
    slope = 0.25
    cfgs = [(dt, f, C, p, act) for dt in dtypes for f in forms for C in B.CH[dt][f] for p in ((65,) if quick and C > 256 else (65, 257)) for act in B.ACTS]
    for dt, f, C, p, act in B._cover(cfgs, lambda c: [("C", c[0], c[2]), ("act", c[0], c[1], c[4]), ("pix", c[0], c[1], c[3])], quick, "frozen_thresholds",
                                     lambda c: None if c[2] <= 300 else ((c[0], c[2]) if c[0] == F32 else "left to the GPU twin")):
        _assert_form(C, dt, f)
        d = B._bwd_data(dt, C, p, exact=True)
        g = d["dz"] * B._dact(d["y"], act, slope)
        what = "frozen thresholds %s pixels=%d C=%d act=%d" % (dt, p, C, act)
        assert bool((d["y"] == 0).any()) and bool((d["y"] == 6).any())
        for with_res, sums in ((False, False), (False, True), (True, False), (True, True)):
            bufs, _ = _run(dev, d, dt, act, slope, with_res, sums, 0)
            _exact(what + " dy (residual=%s sums=%s)" % (with_res, sums), bufs.DY.v.view(p, C), g)
            if with_res:
                _exact(what + " dres", bufs.DR.v.view(p, C), g)
                rc, _ = B._bwd_call(dev, "rd_bn_act_bwd_recompute", d, dt, act, slope, 0, True, use_z=not B._recomputes(C, dt))
                _exact(what + " dres against rd_bn_act_bwd_recompute", bufs.DR.v, rc.DR.v)
            if sums:
                _exact(what + " dbeta", bufs.DB.v, g.sum(0))      # (integer sums: exact in any order)
            bufs.check(what, sums)
        # dres without z: refused with a message, nothing launched
        dv = {k: v.to(dev).to(dt if k in ("y", "dz") else F32) for k, v in d.items()}
        bufs = _Bufs(dev, dt, C, p, _prev(C), True)
        _refused(FN, "derivative from z", _P(dv["dz"]), None, _P(dv["y"]), _P(dv["mean"]), _P(dv["rstd"]), _P(dv["scale"]), _P(dv["shift"]), _P(bufs.PT.v),
                 _P(bufs.DG.v), _P(bufs.DB.v), 0, _P(bufs.DY.v), _P(bufs.DR.v), p, C, act, slope, B.DT[dt], _S(dv["y"]))
        for b_ in (bufs.DY, bufs.DR, bufs.DG, bufs.DB, bufs.PT):
            b_.check(what + " refusal", unchanged=True)
