"""Direct parity cases for the small kernels around the convolutions: element-wise add / cast, layout changes, nearest up-sampling,
LayerNorm, column sums, activation backward, masked BCE / sigmoid and Adam (see tests/parity_cases.py for how case functions are used
by the emulator and GPU twins).

Every kernel is compared with a plain float64 torch restatement on the values the kernel sees (16-bit inputs: the rounded values).
Every buffer a kernel writes through the C ABI is an interior view of a larger allocation with PAD sentinel elements on both sides,
which must come back bit-identical.  Data movement and integer-data cases are `torch.equal`; arithmetic cases use `_check`, whose bound
is derived from torch's own fp32 CPU error against float64, never from the kernel's output.

`quick=True` (the emulator twin) drops only the sizes above 100 K elements, i.e. the grid-stride second iterations.
"""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from tests.parity_cases import TOL, bf16_mode

PAD = 64
EPS32 = 2.0 ** -23
TINY32 = 2.0 ** -126      # smallest normal fp32: differences below it are below the number format's resolution
FLOOR_ULPS = 4            # floor under the fp32 bound, for quantities torch's fp32 computes (almost) exactly
# half an ulp of a 16-bit output at |ref| is 2^(floor(log2 |ref|) - HALF_ULP_EXP): between 2^-9 |ref| and 2^-8 |ref| for bf16 (8 significant bits),
# between 2^-12 |ref| and 2^-11 |ref| for fp16 (11); a correctly rounded tie sits exactly on it.  (significant bits, smallest normal exponent)
HALF_ULP_EXP = {torch.bfloat16: (8, -126), torch.float16: (11, -14)}


def _half_ulp(dtype, r):
    if dtype not in HALF_ULP_EXP:
        return torch.zeros_like(r)
    bits, emin = HALF_ULP_EXP[dtype]
    e = torch.frexp(r.abs())[1].double() - 1.0      # |r| in [2^e, 2^(e+1))
    return torch.where(r == 0, torch.zeros_like(r), torch.pow(2.0, torch.clamp(e, min=emin) - bits))

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
MEASURED = {}             # group -> [reference error / max|ref|, kernel error / max|ref|] maxima, printed by the twins


def _E():
    from riders_amd import engine
    return engine


def report():
    for k in sorted(MEASURED):
        print("glue parity %-28s torch fp32 error %.3e   kernel error %.3e   (relative to max|ref|)" % (k, MEASURED[k][0], MEASURED[k][1]))


def _bits(x):
    return x.contiguous().view(torch.int32 if x.element_size() == 4 else torch.int16)


def _r(x, dtype):
    """fp32 CPU values rounded to `dtype` (what a kernel fed that dtype sees)"""
    return x.to(dtype).to(torch.float32)


class Buf(object):
    """n elements inside a larger allocation: PAD sentinel elements on each side (+ `off` elements in front to misalign the view)."""

    def __init__(self, dev, n, dtype, init=None, off=0):
        total = PAD + off + n + PAD
        pat = ((torch.arange(total) % 251) - 125).to(torch.float32) + (0.0 if dtype == torch.int32 else 0.5)
        self.full = pat.to(dtype).to(dev)
        self.lo, self.hi = PAD + off, PAD + off + n
        self.v = self.full[self.lo:self.hi]
        if init is not None:
            self.v.copy_(init.reshape(-1).to(dtype))
        self.snap = self.full.clone()
        assert self.v.data_ptr() % 16 == (off * self.v.element_size()) % 16

    def cpu(self):
        return self.v.detach().cpu()

    def check(self, what, unchanged=False):
        """sentinels bit-identical; unchanged=True: the interior too (an input, or an output of a call that must write nothing)"""
        a, b = _bits(self.full).cpu(), _bits(self.snap).cpu()
        assert torch.equal(a[:self.lo], b[:self.lo]), what + ": elements in front of the buffer were overwritten"
        assert torch.equal(a[self.hi:], b[self.hi:]), what + ": elements behind the buffer were overwritten"
        if unchanged:
            assert torch.equal(a[self.lo:self.hi], b[self.lo:self.hi]), what + ": buffer changed"


def _call(fn_name, *args):
    E = _E()
    E._chk(getattr(E.L(), fn_name)(*args), fn_name)


def _refused(fn_name, text, *args):
    E = _E()
    rc = getattr(E.L(), fn_name)(*args)
    msg = E.L().rd_last_error_string()
    assert rc != 0 and text in (msg.decode() if msg else ""), "%s: expected refusal %r, got rc=%d %r" % (fn_name, text, rc, msg)


def _check(what, got, ref64, ref32=None, group=None):
    """|got - ref64| <= min(max(4 * max|ref32 - ref64|, FLOOR_ULPS fp32 ulp of max|ref|, TINY32), TOL * max|ref|) + half an ulp of got's
    16-bit type at |ref| (_half_ulp).  ref32 is torch's own fp32 CPU result (None: torch's fp32 is exact for this quantity, the floor alone)."""
    g = got.detach().cpu()
    out_dt = g.dtype
    g = g.double().reshape(-1)
    r = ref64.detach().double().reshape(-1)
    assert g.shape == r.shape, (what, g.shape, r.shape)
    assert bool(torch.isfinite(g).all()), what + ": non-finite values"
    m = float(r.abs().max()) if r.numel() else 0.0
    ref_err = float((ref32.detach().double().reshape(-1) - r).abs().max()) if ref32 is not None else 0.0
    bound = min(max(4.0 * ref_err, FLOOR_ULPS * EPS32 * m, TINY32), max(TOL * m, TINY32))
    diff = (g - r).abs()
    err = float(diff.max()) if diff.numel() else 0.0
    if group is not None and m > 0:
        cur = MEASURED.setdefault(group + (" 16-bit" if out_dt in HALF_ULP_EXP else ""), [0.0, 0.0])
        cur[0] = max(cur[0], ref_err / m); cur[1] = max(cur[1], err / m)
    ok = bool((diff <= bound + _half_ulp(out_dt, r)).all())
    assert ok, "%s: kernel error %.3e, torch fp32's own error %.3e, fp32 bound %.3e (+ half an ulp of %s), max|ref| %.3e" % (
        what, err, ref_err, bound, out_dt, m)


def _exact(what, got, ref):
    g, r = got.detach().cpu(), ref.detach().cpu().to(got.dtype)
    assert g.shape == r.shape, (what, g.shape, r.shape)
    assert torch.equal(_bits(g), _bits(r)) or torch.equal(g, r), what + ": not bit-exact (%d of %d elements differ)" % (int((g != r).sum()), g.numel())


def _moved(what, got, ref64, src_dt, group):
    """Result of a copy with an optional fp32 scale: exact into fp32 (an fp32 product is the correctly rounded exact product, which float64
    holds) and into the same 16-bit type at scale 1; a narrowing store rounds once more, judged by the half-ulp rule."""
    if got.dtype == F32 or (got.dtype == src_dt and ref64.dtype != torch.float64):
        _exact(what, got, ref64.float())
    else:
        _check(what, got, ref64.double(), None, group)


def _rs(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) % (2 ** 31))


def _randn(rs, *shape):
    return torch.from_numpy(rs.standard_normal(shape).astype(np.float32))


def _ints(rs, lo, hi, *shape):
    return torch.from_numpy(rs.randint(lo, hi + 1, shape).astype(np.float32))


def _dt(t):
    return _E().rd_of(t)


def _P(t):
    return _E()._p(t)


def _S(t):
    return _E()._stream(t)


# ---------------------------------------------------------------------------------------------------------------- 1. add
def _add_one(dev, dtype, n, mis=None, alias=False):
    rs = _rs("add", str(dtype), n, mis, alias)
    a, b = _r(_randn(rs, n), dtype), _r(_randn(rs, n), dtype)
    A = Buf(dev, n, dtype, a, off=1 if mis == "a" else 0)
    B = Buf(dev, n, dtype, b, off=1 if mis == "b" else 0)
    O = A if alias else Buf(dev, n, dtype, off=1 if mis == "out" else 0)
    _call("rd_add", _P(A.v), _P(B.v), _P(O.v), n, _dt(A.v), _S(A.v))
    what = "add %s n=%d misaligned=%s alias=%s" % (dtype, n, mis, alias)
    ref = a.double() + b.double()
    if dtype == F32:
        _exact(what, O.v, ref.float())      # IEEE addition is correctly rounded
    else:
        _check(what, O.v, ref, None, "add")
    O.check(what); B.check(what, unchanged=True)
    if not alias:
        A.check(what, unchanged=True)


def add_case(dev, quick=False):
    """rd_add: the 16-byte vector kernel with its scalar tail (all operands aligned), the scalar kernel (any operand off by one element),
    out aliasing a (Tape accumulation), and in full mode a size whose vector body AND tail run a second grid-stride iteration."""
    for dtype, ve in ((F32, 4), (BF16, 8)):
        for n in (1, ve - 1, ve, ve + 1, 1023, 4099):
            for mis in (None, "a", "b", "out"):
                _add_one(dev, dtype, n, mis)
            _add_one(dev, dtype, n, alias=True)
        if not quick:
            _add_one(dev, dtype, 4096 * 256 * ve + ve * 300 + (3 if ve == 4 else 5))
    with bf16_mode("fp16"):
        _add_one(dev, F16, 1023)
        _add_one(dev, F16, 9, "b")


# ---------------------------------------------------------------------------------------------------------------- 2. cast
def _cast_one(dev, sd, dd, scale, n):
    rs = _rs("cast", str(sd), str(dd), scale, n)
    x = _r(_randn(rs, n), sd)
    X, Y = Buf(dev, n, sd, x), Buf(dev, n, dd)
    sc = float(np.float32(scale))
    _call("rd_cast", _P(X.v), _P(Y.v), n, _dt(X.v), _dt(Y.v), sc, _S(X.v))
    what = "cast %s -> %s scale=%g n=%d" % (sd, dd, scale, n)
    if scale == 1:
        _moved(what, Y.v, x, sd, "cast")
    else:
        _moved(what, Y.v, x.double() * sc, sd, "cast")
    Y.check(what); X.check(what, unchanged=True)


def cast_case(dev, quick=False):
    """rd_cast over every dtype pair of both builds, three scales, sizes around one block and (full mode) a second grid-stride iteration;
    the unsupported bf16 -> fp16 pair is refused."""
    for sd, dd in ((F32, F32), (F32, BF16), (BF16, F32), (BF16, BF16), (F32, F16), (F16, F32)):
        for scale in (1, 1.0 / 255, 4096):
            for n in (1, 255, 257) + (() if quick else (4096 * 256 + 777,)):
                _cast_one(dev, sd, dd, scale, n)
    X, Y = Buf(dev, 8, BF16, torch.ones(8)), Buf(dev, 8, F16)
    _refused("rd_cast", "bf16 <-> fp16 is not supported", _P(X.v), _P(Y.v), 8, 1, 2, 1.0, _S(X.v))
    Y.check("refused cast", unchanged=True)


# ---------------------------------------------------------------------------------------------------------------- 3. layouts
def layout_case(dev, quick=False):
    """rd_nchw_to_nhwc / rd_nhwc_to_nchw against permute (mixed dtype pairs, forward scale, round trip), rd_transpose_last2 (twice = identity),
    rd_concat2 / rd_split2 (split(concat(a, b)) = a, b), rd_pad_channels (pad lanes exactly +0) and rd_unpad_weight_grad."""
    for (N, C, H, W) in ((1, 1, 1, 1), (2, 3, 5, 7), (1, 5, 9, 4), (3, 16, 3, 3)):
        n = N * C * H * W
        for sd, dd in ((F32, F32), (F32, BF16), (BF16, F32), (BF16, BF16)):
            x = _r(_randn(_rs("nchw", N, C, H, W, str(sd)), N, C, H, W), sd)
            X = Buf(dev, n, sd, x)
            what = "nchw<->nhwc %s -> %s %s" % (sd, dd, (N, C, H, W))
            for scale in (1, 1.0 / 255):
                sc = float(np.float32(scale))
                Y = Buf(dev, n, dd)
                _call("rd_nchw_to_nhwc", _P(X.v), _P(Y.v), N, C, H, W, _dt(X.v), _dt(Y.v), sc, _S(X.v))
                ref = x.permute(0, 2, 3, 1).contiguous()
                _moved(what + " fwd scale=%g" % scale, Y.v.view(N, H, W, C), ref if scale == 1 else ref.double() * sc, sd, "layout")
                Y.check(what)
            X.check(what, unchanged=True)
            # inverse: x read as NHWC
            Z = Buf(dev, n, dd)
            _call("rd_nhwc_to_nchw", _P(X.v), _P(Z.v), N, C, H, W, _dt(X.v), _dt(Z.v), _S(X.v))
            _moved(what + " inverse", Z.v.view(N, C, H, W), x.reshape(N, H, W, C).permute(0, 3, 1, 2).contiguous(), sd, "layout")
            Z.check(what)
            if sd == dd:      # round trip
                Y = Buf(dev, n, dd); Z = Buf(dev, n, dd)
                _call("rd_nchw_to_nhwc", _P(X.v), _P(Y.v), N, C, H, W, _dt(X.v), _dt(Y.v), 1.0, _S(X.v))
                _call("rd_nhwc_to_nchw", _P(Y.v), _P(Z.v), N, C, H, W, _dt(Y.v), _dt(Z.v), _S(X.v))
                _exact(what + " round trip", Z.v, x.reshape(-1))
                Y.check(what); Z.check(what)
    for (B, R, Cc) in ((1, 1, 1), (1, 7, 13), (3, 21, 8), (2, 64, 5)):
        for dtype in (F32, BF16):
            n = B * R * Cc
            x = _r(_randn(_rs("tr", B, R, Cc), B, R, Cc), dtype)
            X, Y, Z = Buf(dev, n, dtype, x), Buf(dev, n, dtype), Buf(dev, n, dtype)
            what = "transpose_last2 %s %s" % (dtype, (B, R, Cc))
            _call("rd_transpose_last2", _P(X.v), _P(Y.v), B, R, Cc, _dt(X.v), _S(X.v))
            _exact(what, Y.v.view(B, Cc, R), x.transpose(1, 2).contiguous())
            _call("rd_transpose_last2", _P(Y.v), _P(Z.v), B, Cc, R, _dt(X.v), _S(X.v))
            _exact(what + " twice", Z.v, x.reshape(-1))
            for b_ in (X, Y, Z):
                b_.check(what, unchanged=b_ is X)
    for rows in (1, 5, 257):
        for (Ca, Cb) in ((1, 1), (3, 5), (8, 24), (128, 128)):
            for dtype in (F32, BF16):
                rs = _rs("cat", rows, Ca, Cb)
                a, b = _r(_randn(rs, rows, Ca), dtype), _r(_randn(rs, rows, Cb), dtype)
                A, B_ = Buf(dev, rows * Ca, dtype, a), Buf(dev, rows * Cb, dtype, b)
                O = Buf(dev, rows * (Ca + Cb), dtype)
                A2, B2 = Buf(dev, rows * Ca, dtype), Buf(dev, rows * Cb, dtype)
                what = "concat2/split2 %s rows=%d %s" % (dtype, rows, (Ca, Cb))
                _call("rd_concat2", _P(A.v), _P(B_.v), _P(O.v), rows, Ca, Cb, _dt(A.v), _S(A.v))
                _exact(what + " concat", O.v.view(rows, Ca + Cb), torch.cat([a, b], 1))
                _call("rd_split2", _P(O.v), _P(A2.v), _P(B2.v), rows, Ca, Cb, _dt(A.v), _S(A.v))
                _exact(what + " split a", A2.v, a.reshape(-1)); _exact(what + " split b", B2.v, b.reshape(-1))
                for b_ in (A, B_, O, A2, B2):
                    b_.check(what, unchanged=b_ in (A, B_))
    for (C, Cp) in ((3, 4), (3, 8), (5, 8)):
        for rows in (1, 33):
            for dtype in (F32, BF16):
                x = _r(_randn(_rs("pad", C, Cp, rows), rows, C), dtype)
                X, Y = Buf(dev, rows * C, dtype, x), Buf(dev, rows * Cp, dtype)
                what = "pad_channels %s %d->%d rows=%d" % (dtype, C, Cp, rows)
                _call("rd_pad_channels", _P(X.v), _P(Y.v), rows, C, Cp, _dt(X.v), _S(X.v))
                y = Y.v.view(rows, Cp)
                _exact(what, y[:, :C], x)
                assert int(_bits(y[:, C:]).cpu().abs().max()) == 0, what + ": pad lanes are not +0"
                Y.check(what); X.check(what, unchanged=True)
    for (Co, Ci, Cp, taps) in ((4, 3, 4, 9), (32, 3, 8, 49)):
        rs = _rs("unpad", Co, Ci)
        dwp, dw0 = _randn(rs, Co, Cp, taps), _randn(rs, Co, Ci, taps)
        for acc in (0, 1):
            X, Y = Buf(dev, dwp.numel(), F32, dwp), Buf(dev, dw0.numel(), F32, dw0)
            what = "unpad_weight_grad %s accumulate=%d" % ((Co, Ci, Cp, taps), acc)
            _call("rd_unpad_weight_grad", _P(X.v), _P(Y.v), Co, Ci, Cp, taps, acc, _S(X.v))
            ref = dwp[:, :Ci].double() + (dw0.double() if acc else 0.0)
            _exact(what, Y.v.view(Co, Ci, taps), ref.float())
            Y.check(what); X.check(what, unchanged=True)


# ---------------------------------------------------------------------------------------------------------------- 4. nearest
UPSAMPLE_GEOMS = (((7, 3), (14, 6)), ((7, 3), (15, 6)), ((30, 12), (60, 25)), ((3, 2), (13, 9)), ((5, 4), (5, 4)), ((9, 8), (4, 3)),
                  ((1, 1), (4, 5)),
                  # more than three readers along ONE axis only: the fast path's `nh <= 3 && nw <= 3` must fail on either count alone
                  ((3, 3), (13, 8)), ((3, 3), (8, 13)))


def _upsample_one(dev, dtype, N, src, dst, C):
    (Hs, Ws), (Hv, Wv) = src, dst
    rs = _rs("up", N, Hs, Ws, Hv, Wv, C)
    x, dy = _ints(rs, -3, 3, N, Hs, Ws, C), _ints(rs, -3, 3, N, Hv, Wv, C)
    x64 = x.double().permute(0, 3, 1, 2).contiguous().requires_grad_()
    y64 = F.interpolate(x64, size=(Hv, Wv), mode="nearest")
    (y64 * dy.double().permute(0, 3, 1, 2)).sum().backward()
    y32 = F.interpolate(x.permute(0, 3, 1, 2).contiguous(), size=(Hv, Wv), mode="nearest")
    what = "nearest %s N=%d %s->%s C=%d" % (dtype, N, src, dst, C)
    assert torch.equal(y32.double(), y64.detach()), what + ": torch's fp32 and float64 forwards pick different source pixels"
    X, Y = Buf(dev, x.numel(), dtype, x), Buf(dev, dy.numel(), dtype)
    _call("rd_upsample_nearest_fwd", _P(X.v), _P(Y.v), N, Hs, Ws, Hv, Wv, C, _dt(X.v), _S(X.v))
    _exact(what + " forward", Y.v.view(N, Hv, Wv, C), y64.detach().permute(0, 2, 3, 1).contiguous().float())
    Y.check(what); X.check(what, unchanged=True)
    DY, DX = Buf(dev, dy.numel(), dtype, dy), Buf(dev, x.numel(), dtype)
    _call("rd_upsample_nearest_bwd", _P(DY.v), _P(DX.v), N, Hs, Ws, Hv, Wv, C, _dt(DY.v), _S(DY.v))
    _exact(what + " backward", DX.v.view(N, Hs, Ws, C), x64.grad.permute(0, 2, 3, 1).contiguous().float())
    DX.check(what); DY.check(what, unchanged=True)


def upsample_case(dev, quick=False):
    """rd_upsample_nearest_fwd / _bwd standalone on integer data, bit for bit against F.interpolate(mode='nearest') and its autograd:
    the scalar backward kernel (C not a multiple of the vector width), the vector kernel's nine-load fast path (<= 3 x 3 readers) and
    its general loop (3x2 -> 13x9: up to 5 x 5 readers), identity, a single source pixel, and down-sampling, where source pixels nobody
    reads get exactly 0.  torch's fp32 and float64 CPU forwards agree on every geometry here and so does the kernel: no geometry needed
    a decision."""
    for N in (1, 2):
        for src, dst in UPSAMPLE_GEOMS:
            for C in (3, 6, 4, 8, 20):
                _upsample_one(dev, F32, N, src, dst, C)
            for C in (4, 12, 8, 24):
                _upsample_one(dev, BF16, N, src, dst, C)
    with bf16_mode("fp16"):
        _upsample_one(dev, F16, 2, (7, 3), (15, 6), 8)
        _upsample_one(dev, F16, 1, (3, 2), (13, 9), 12)


# ---------------------------------------------------------------------------------------------------------------- 5. LayerNorm
LN_EPS = 1e-5


def _ln_inputs(rs, family, rows, C):
    if family == "normal":
        return _randn(rs, rows, C)
    if family == "offset":      # a large mean beside a small spread
        return 100.0 + 0.1 * _randn(rs, rows, C)
    x = _randn(rs, rows, C)
    r = rs.randint(0, rows)
    if family == "constant":    # one constant row: var = 0
        x[r] = 1.75
    else:                       # "spike": one row with a single non-zero element
        x[r] = 0.0
        x[r, rs.randint(0, C)] = 3.0
    return x


def _ln_ref(dt, x, res, gam, bet, douts):
    """float64: the plain two-pass restatement (mean, centred values, biased variance), which is exact where the kernel must be -- a constant
    row has xhat = 0 and contributes exactly nothing; fp32: torch's own F.layer_norm, whose error against it sets the bound."""
    x_, g_, b_ = (v.detach().clone().to(dt).requires_grad_() for v in (x, gam, bet))
    if dt == torch.float64:
        xc = x_ - x_.mean(1, keepdim=True)
        y = xc * (xc * xc).mean(1, keepdim=True).add(LN_EPS).rsqrt() * g_ + b_
    else:
        y = F.layer_norm(x_, (x.shape[1],), g_, b_, LN_EPS)
    out = y if res is None else y + res.to(dt)
    dxs = []
    for d in douts:      # the parameter gradients of both backward runs add up
        (gx,) = torch.autograd.grad((out * d.to(dt)).sum(), x_, retain_graph=True)
        dxs.append(gx)
    sum(((out * d.to(dt)).sum() for d in douts)).backward()
    xd = x.detach().to(dt)
    mean = xd.mean(1)
    rstd = (xd.var(1, unbiased=False) + LN_EPS).rsqrt()
    return dict(out=out.detach(), mean=mean, rstd=rstd, dx=dxs, dg=g_.grad, db=b_.grad)


def _ln_one(dev, dtype, C, rows, with_res, family):
    E = _E()
    rs = _rs("ln", str(dtype), C, rows, with_res, family)
    x = _r(_ln_inputs(rs, family, rows, C), dtype)
    res = _r(_randn(rs, rows, C), dtype) if with_res else None
    gam, bet = 1.0 + 0.5 * _randn(rs, C), 0.3 * _randn(rs, C)
    douts = [_r(_randn(rs, rows, C), dtype), _r(_randn(rs, rows, C), dtype)]
    r64, r32 = _ln_ref(torch.float64, x, res, gam, bet, douts), _ln_ref(F32, x, res, gam, bet, douts)
    what = "layernorm %s C=%d rows=%d residual=%s %s" % (dtype, C, rows, with_res, family)
    grp = "layernorm"
    ln = torch.nn.LayerNorm(C, eps=LN_EPS).to(dev)
    with torch.no_grad():
        ln.weight.copy_(gam); ln.bias.copy_(bet)
    xd = x.to(dev).to(dtype)
    rd = None if res is None else res.to(dev).to(dtype)
    # (a) engine.layernorm under a Tape, twice into the same parameter-gradient slots: the second run must add
    DG, DB = Buf(dev, C, F32), Buf(dev, C, F32)
    for k, d in enumerate(douts):
        tape = E.Tape(); tape.mark(xd)
        if rd is not None:
            tape.mark(rd)
        tape.grad_alloc = lambda p: DG.v if p is ln.weight else DB.v
        with E._active(tape):
            out = E.layernorm(xd, ln, rd)
            dd = d.to(dev).to(dtype)
            tape.grads[id(out)] = dd
            tape.backward()
        _check(what + " out", out, r64["out"], r32["out"], grp + " out")
        _check(what + " dx (run %d)" % k, tape.grads[id(xd)], r64["dx"][k], r32["dx"][k], grp + " dx")
        if rd is not None:
            _exact(what + " dresidual", tape.grads[id(rd)], d)
        ln.weight.grad, ln.bias.grad = DG.v, DB.v      # the slots now hold this step's gradient: the next tape accumulates (Tape.param_grad)
    _check(what + " dgamma (two runs)", DG.v, r64["dg"], r32["dg"], grp + " dgamma")
    _check(what + " dbeta (two runs)", DB.v, r64["db"], r32["db"], grp + " dbeta")
    DG.check(what); DB.check(what)
    ln.weight.grad = ln.bias.grad = None
    # (b) the C ABI with guarded outputs: statistics, and the per-block partial rows finished by the deferred rd_ln_grad_batch flush
    lib, st = E.L(), _S(xd)
    O, M, R = Buf(dev, rows * C, dtype), Buf(dev, rows, F32), Buf(dev, rows, F32)
    _call("rd_layernorm_fwd", _P(xd), _P(ln.weight.detach()), _P(ln.bias.detach()), _P(rd), _P(O.v), _P(M.v), _P(R.v), rows, C, LN_EPS, _dt(xd), st)
    _check(what + " out (C ABI)", O.v.view(rows, C), r64["out"], r32["out"], grp + " out")
    _check(what + " mean", M.v, r64["mean"], r32["mean"], grp + " mean")
    _check(what + " rstd", R.v, r64["rstd"], r32["rstd"], grp + " rstd")
    if family == "constant":
        assert abs(float(R.cpu().max()) - LN_EPS ** -0.5) <= 4 * EPS32 * LN_EPS ** -0.5, what + ": rstd of a constant row"
    nb = lib.rd_layernorm_bwd_rows(rows)
    DG2, DB2 = Buf(dev, C, F32, torch.zeros(C)), Buf(dev, C, F32, torch.zeros(C))
    tape = E.Tape()
    keep = []
    for k, d in enumerate(douts):
        DX, PT = Buf(dev, rows * C, dtype), Buf(dev, nb * C * 2, F32)
        dd = d.to(dev).to(dtype)
        _call("rd_layernorm_bwd", _P(dd), _P(xd), _P(ln.weight.detach()), _P(M.v), _P(R.v), _P(DX.v), _P(PT.v), None, None, 0, rows, C, _dt(xd), st)
        _check(what + " dx (C ABI, run %d)" % k, DX.v.view(rows, C), r64["dx"][k], r32["dx"][k], grp + " dx")
        DX.check(what); PT.check(what)
        tape.defer_ln_grad(ln.weight, DG2.v, DB2.v, 1, PT.v, nb)      # accumulate = 1 onto zeros
        keep.append(PT)
    tape.flush_ln_grads()
    _check(what + " dgamma (batched finalize)", DG2.v, r64["dg"], r32["dg"], grp + " dgamma")
    _check(what + " dbeta (batched finalize)", DB2.v, r64["db"], r32["db"], grp + " dbeta")
    for b_ in (O, M, R, DG2, DB2):
        b_.check(what)


def layernorm_case(dev, quick=False, Cs=(64, 128, 256, 512), extras=True):
    """engine.layernorm under a Tape (forward, backward twice into the same parameter-gradient slots) and rd_layernorm_fwd / _bwd through the
    C ABI with the partial rows finished by Tape.flush_ln_grads (rd_ln_grad_batch): every supported width class (1, 2, 4, 8 values per lane),
    row counts around the four-rows-per-block grouping, and in full mode 2048 + 7 rows (the stride loop of the 512-block backward); a constant
    row, a single non-zero element, a large mean beside a small spread.  C = 96 and C = 576 are refused."""
    E = _E()
    if quick:
        # a finalize launch is one 256-thread block per channel and the emulator runs every thread as a fiber: the full cross product took
        # 20 minutes there.  The emulator runs a covering selection (every width, row count, family, dtype, with and without residual at least
        # once, every family at every width); the GPU twin runs the cross product
        N_, O_, K_, S_ = "normal", "offset", "constant", "spike"
        sel = {64: [(r, d, i % 2 == 1, N_) for i, (r, d) in enumerate((r, d) for r in (1, 3, 4, 5, 67) for d in (F32, BF16))]
                   + [(5, F32, True, O_), (5, BF16, False, K_), (4, F32, False, S_)],
               128: [(3, F32, True, O_), (5, BF16, False, K_), (67, F32, False, S_), (4, BF16, True, N_)],
               256: [(1, F32, False, O_), (5, BF16, True, S_), (4, F32, True, K_), (3, BF16, False, N_)],
               512: [(1, F32, False, O_), (5, BF16, True, N_), (3, F32, True, K_), (67, BF16, False, S_)]}
        for C in Cs:
            for rows, dtype, with_res, fam in sel[C]:
                _ln_one(dev, dtype, C, rows, with_res, fam)
    else:
        for C in Cs:
            for rows in (1, 3, 4, 5, 67, 2048 + 7):
                for with_res in (False, True):
                    for dtype in (F32, BF16):
                        for fam in ("normal", "offset", "constant", "spike"):
                            _ln_one(dev, dtype, C, rows, with_res, fam)
    if not extras:
        return
    with bf16_mode("fp16"):
        _ln_one(dev, F16, 128, 5, True, "normal")
    for C in (96, 576):
        x = torch.zeros(4 * C, device=dev); g = torch.ones(C, device=dev); s = torch.zeros(4, device=dev)
        O = Buf(dev, 4 * C, F32)
        msg = "layernorm: C must be a multiple of 64 and <= 512 (got %d)" % C
        _refused("rd_layernorm_fwd", msg, _P(x), _P(g), _P(g), None, _P(O.v), _P(s), _P(s), 4, C, LN_EPS, 0, _S(x))
        _refused("rd_layernorm_bwd", msg, _P(x), _P(x), _P(g), _P(s), _P(s), _P(O.v), _P(x), None, None, 0, 4, C, 0, _S(x))
        O.check("refused layernorm", unchanged=True)


# ---------------------------------------------------------------------------------------------------------------- 6. colsum / act_bwd
def _colsum_data(rows, C, dtype):
    rs = _rs("colsum", rows, C)
    return _r(10.0 + _randn(rs, rows, C), dtype), 100.0 * _randn(rs, C)


def colsum_case(dev, quick=False):
    """rd_colsum (scalar, 16-byte-vector and any-channel-count reduce kernels + its own finalize) and rd_colsum_partial +
    rd_colsum_finalize_batch with two items of different C in one launch; data with mean 10 so that cancellation would show."""
    E = _E()
    lib = E.L()
    Cs = (1, 3, 8, 40, 144, 1392)
    for dtype in (F32, BF16):
        for rows in (1, 63, 1000):
            for acc in (0, 1):
                for C in Cs:
                    x, prev = _colsum_data(rows, C, dtype)
                    X, O = Buf(dev, rows * C, dtype, x), Buf(dev, C, F32, prev)
                    PT = Buf(dev, lib.rd_colsum_rows(rows, C) * C * 2, F32)
                    what = "colsum %s rows=%d C=%d accumulate=%d" % (dtype, rows, C, acc)
                    _call("rd_colsum", _P(X.v), _P(PT.v), _P(O.v), acc, rows, C, _dt(X.v), _S(X.v))
                    r64 = x.double().sum(0) + (prev.double() if acc else 0.0)
                    r32 = x.sum(0) + (prev if acc else 0.0)
                    _check(what, O.v, r64, r32, "colsum")
                    O.check(what); PT.check(what); X.check(what, unchanged=True)
                for Ca, Cb in ((1, 1392), (144, 3), (8, 40)):
                    items, bufs = [], []
                    for C in (Ca, Cb):
                        x, prev = _colsum_data(rows, C, dtype)
                        X, O = Buf(dev, rows * C, dtype, x), Buf(dev, C, F32, prev)
                        nr = lib.rd_colsum_rows(rows, C)
                        PT = Buf(dev, nr * C * 2, F32)
                        _call("rd_colsum_partial", _P(X.v), _P(PT.v), rows, C, _dt(X.v), _S(X.v))
                        it = E._lib.ColsumItem()
                        it.partial, it.out, it.rows, it.C, it.accumulate = PT.v.data_ptr(), O.v.data_ptr(), nr, C, acc
                        items.append(it); bufs.append((x, prev, X, O, PT))
                    arr = (E._lib.ColsumItem * 2)(*items)
                    _call("rd_colsum_finalize_batch", arr, 2, _S(bufs[0][2].v))
                    for C, (x, prev, X, O, PT) in zip((Ca, Cb), bufs):
                        what = "colsum batch %s rows=%d C=%d (of %d,%d) accumulate=%d" % (dtype, rows, C, Ca, Cb, acc)
                        _check(what, O.v, x.double().sum(0) + (prev.double() if acc else 0.0), x.sum(0) + (prev if acc else 0.0), "colsum")
                        O.check(what); PT.check(what); X.check(what, unchanged=True)


def act_bwd_case(dev, quick=False):
    """rd_act_bwd for every activation code the engine defines: dx = dz * f'(z) with f' taken from the activation OUTPUT z (exact zeros of
    both signs, negative and positive values, 6 and above for ReLU6)."""
    E = _E()
    slope = float(np.float32(0.2))
    zvals = torch.tensor([0.0, -0.0, -2.0, 0.5, -0.5, 3.0, 6.0, 7.0, 5.5, -1e-3, 1e-3])
    for act in (E.ACT_NONE, E.ACT_RELU, E.ACT_LRELU, E.ACT_RELU6):
        for dtype in (F32, BF16):
            for n in (1, 255, 1025):
                rs = _rs("act", act, n)
                z = _r(zvals[torch.from_numpy(rs.randint(0, len(zvals), n))] if n > 1 else zvals[:1].clone(), dtype)
                dz = _r(_randn(rs, n), dtype)
                if act == E.ACT_RELU:
                    fac = (z > 0).double()
                elif act == E.ACT_LRELU:
                    fac = torch.where(z > 0, 1.0, slope).double()
                elif act == E.ACT_RELU6:
                    fac = ((z > 0) & (z < 6)).double()
                else:
                    fac = torch.ones(n, dtype=torch.float64)
                DZ, Z, DX = Buf(dev, n, dtype, dz), Buf(dev, n, dtype, z), Buf(dev, n, dtype)
                what = "act_bwd act=%d %s n=%d" % (act, dtype, n)
                _call("rd_act_bwd", _P(DZ.v), _P(Z.v), _P(DX.v), n, act, slope, _dt(DZ.v), _S(DZ.v))
                ref = dz.double() * fac
                if dtype == F32:
                    _exact(what, DX.v, ref.float())
                else:
                    _check(what, DX.v, ref, None, "act_bwd")
                DX.check(what); DZ.check(what, unchanged=True); Z.check(what, unchanged=True)


# ---------------------------------------------------------------------------------------------------------------- 7. BCE / sigmoid
def _logits(rs, n, dtype):
    special = np.array([0, 1e-4, -1e-4, 3, -3, 20, -20, 88, -88, 200, -200], np.float32)
    x = rs.uniform(-5, 5, n).astype(np.float32)
    pick = rs.rand(n) < 0.5
    x[pick] = special[rs.randint(0, len(special), int(pick.sum()))]
    if n >= len(special):
        x[:len(special)] = special      # every special value at least once
    return _r(torch.from_numpy(x), dtype)


def bce_case(dev, quick=False):
    """rd_bce_masked_fwd / _bwd as engine.bce_masked calls them, and rd_sigmoid, on saturating logits (+-20, +-88, +-200), pos_weight up to 50,
    ~60 % validity: loss, sums and dlogits against float64 binary_cross_entropy_with_logits and its autograd; nothing NaN or inf."""
    E = _E()
    lib = E.L()
    for dtype in (F32, BF16):
        for n in (1, 255, 1025, 5 * 12 * 9):
            rs = _rs("bce", n)
            x = _logits(rs, n, dtype)
            y = torch.from_numpy((rs.rand(n) < 0.4).astype(np.float32))
            valid = torch.from_numpy((rs.rand(n) < 0.6).astype(np.float32))
            valid[0] = 1.0
            dloss = torch.tensor([1.7])
            X = Buf(dev, n, dtype, x)
            yd, vd, gd = y.to(dev), valid.to(dev), dloss.to(dev)
            for pw in (1.0, 2.5, 50.0):
                refs = {}
                for dt in (torch.float64, F32):
                    x_ = x.detach().clone().to(dt).requires_grad_()
                    l = F.binary_cross_entropy_with_logits(x_, y.to(dt), pos_weight=torch.tensor([pw], dtype=dt), reduction="none")
                    s0, s1 = (valid.to(dt) * l).sum(), valid.to(dt).sum()
                    loss = s0 / s1
                    (loss * dloss.to(dt)[0]).backward()
                    refs[dt] = (loss.detach().reshape(1), torch.stack([s0.detach(), s1]), x_.grad)
                rows = lib.rd_bce_rows(n)
                PT, LS, SM, DL = Buf(dev, rows * 2, F32), Buf(dev, 1, F32), Buf(dev, 2, F32), Buf(dev, n, dtype)
                what = "bce %s n=%d pos_weight=%g" % (dtype, n, pw)
                _call("rd_bce_masked_fwd", _P(X.v), _P(yd), _P(vd), pw, _P(PT.v), _P(LS.v), _P(SM.v), n, _dt(X.v), _S(X.v))
                _call("rd_bce_masked_bwd", _P(X.v), _P(yd), _P(vd), pw, _P(SM.v), _P(gd), _P(DL.v), n, _dt(X.v), _S(X.v))
                _check(what + " loss", LS.v, refs[torch.float64][0], refs[F32][0], "bce loss")
                _check(what + " sums", SM.v, refs[torch.float64][1], refs[F32][1], "bce sums")
                _check(what + " dlogits", DL.v, refs[torch.float64][2], refs[F32][2], "bce dlogits")
                for b_ in (PT, LS, SM, DL):
                    b_.check(what)
                X.check(what, unchanged=True)
            Y = Buf(dev, n, dtype)
            what = "sigmoid %s n=%d" % (dtype, n)
            _call("rd_sigmoid", _P(X.v), _P(Y.v), n, _dt(X.v), _S(X.v))
            r64 = torch.sigmoid(x.double())
            _check(what, Y.v, r64, torch.sigmoid(x), "sigmoid")
            got = Y.cpu().float()
            one = got == 1.0
            assert bool((r64.float().to(dtype).float()[one] == 1.0).all()), what + ": exactly 1 where the output type does not saturate"
            assert bool((r64[got == 0.0] < TINY32).all()), what + ": exactly 0 where fp32 does not underflow"
            Y.check(what); X.check(what, unchanged=True)


# ---------------------------------------------------------------------------------------------------------------- 8. Adam
LR, B1, B2, AEPS = (float(np.float32(v)) for v in (2e-3, 0.9, 0.999, 1e-8))


def _adam_ref64(p, g, m, v, step, wd, gscale):
    """torch's single-tensor Adam (L2-coupled weight decay) in float64, with the gradient scale the kernel folds in"""
    g = g * gscale + wd * p
    m = B1 * m + (1.0 - B1) * g
    v = B2 * v + (1.0 - B2) * g * g
    bc1, bc2 = 1.0 - B1 ** step, 1.0 - B2 ** step
    p = p - (LR / bc1) * m / (v.sqrt() / (bc2 ** 0.5) + AEPS)
    return p, m, v


def _adam_grads(rs, family, n):
    if family == "normal":
        return _randn(rs, n)
    if family == "zero":
        return torch.zeros(n)
    return 1e-20 * _randn(rs, n)


def _adam_args(bufs, G, n, step, wd, gscale):
    P_, M, V = bufs
    return (_P(P_.v), _P(G), _P(M.v), _P(V.v), n, LR, B1, B2, AEPS, wd, step, gscale)


def _adam_direct(dev, n, wd, gscale, family):
    wd, gscale = float(np.float32(wd)), float(np.float32(gscale))
    rs = _rs("adam", n, wd, gscale, family)
    p0 = _randn(rs, n)
    P_, M, V = Buf(dev, n, F32, p0), Buf(dev, n, F32, torch.zeros(n)), Buf(dev, n, F32, torch.zeros(n))
    p64, m64, v64 = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    p32 = torch.nn.Parameter(p0.clone())
    opt32 = torch.optim.Adam([p32], lr=LR, betas=(B1, B2), eps=AEPS, weight_decay=wd, foreach=False)
    what = "adam n=%d weight_decay=%g gscale=%g %s" % (n, wd, gscale, family)
    for step in (1, 2, 3):
        g = _adam_grads(rs, family, n)
        G = Buf(dev, n, F32, g)
        _call("rd_adam_step", *(_adam_args((P_, M, V), G.v, n, step, wd, gscale) + (_S(G.v),)))
        p64, m64, v64 = _adam_ref64(p64, g.double(), m64, v64, step, wd, gscale)
        p32.grad = g * gscale
        opt32.step()
        G.check(what, unchanged=True)
    s32 = opt32.state[p32]
    _check(what + " p", P_.v, p64, p32.detach(), "adam p")
    _check(what + " exp_avg", M.v, m64, s32["exp_avg"], "adam exp_avg")
    _check(what + " exp_avg_sq", V.v, v64, s32["exp_avg_sq"], "adam exp_avg_sq")
    if family == "zero":
        moved = bool((P_.cpu() != p0).any())
        assert moved == (wd > 0), what + ": with zero gradients p moves through weight decay only"
    for b_ in (P_, M, V):
        b_.check(what)


def _flat_adam(dev):
    from riders_amd.optim import FlatAdam
    wd = 1e-2
    rs = _rs("flatadam")
    init = [_randn(rs, 7, 5), _randn(rs, 33), _randn(rs, 4, 3, 3, 3)]
    ps = [torch.nn.Parameter(x.clone().to(dev)) for x in init]
    opt = FlatAdam(ps, lr=LR, betas=(B1, B2), eps=AEPS, weight_decay=wd)
    refs = {}
    for dt in (torch.float64, F32):
        rp = [torch.nn.Parameter(x.clone().to(dt)) for x in init]
        refs[dt] = (rp, torch.optim.Adam(rp, lr=LR, betas=(B1, B2), eps=AEPS, weight_decay=wd, foreach=False))
    o1 = opt.offsets[1]
    for step in (1, 2, 3):
        opt.zero_grad()
        before = [t_[o1:o1 + 33].clone() for t_ in (opt.flat_param, opt.exp_avg, opt.exp_avg_sq)]
        for i, p in enumerate(ps):
            skip = step == 2 and i == 1
            g = None if skip else _randn(rs, *p.shape)
            p.grad = None if skip else g.to(dev)
            for dt in refs:
                refs[dt][0][i].grad = None if skip else g.to(dt)
        opt.step()
        for dt in refs:
            refs[dt][1].step()
        if step == 2:
            after = [t_[o1:o1 + 33] for t_ in (opt.flat_param, opt.exp_avg, opt.exp_avg_sq)]
            for a, b, nm in zip(after, before, ("p", "exp_avg", "exp_avg_sq")):
                assert torch.equal(_bits(a).cpu(), _bits(b).cpu()), "FlatAdam: %s of the slot without a gradient changed" % nm
            assert opt.steps == [2, 1, 2], opt.steps
    assert opt.steps == [3, 2, 3], opt.steps
    sd = opt.state_dict()["state"]
    for i, p in enumerate(ps):
        r64, r32 = refs[torch.float64], refs[F32]
        _check("FlatAdam p%d" % i, p, r64[0][i].detach(), r32[0][i].detach(), "adam p")
        for k in ("exp_avg", "exp_avg_sq"):
            _check("FlatAdam %s %d" % (k, i), sd[i][k], r64[1].state[r64[0][i]][k], r32[1].state[r32[0][i]][k], "adam " + k)
        assert int(sd[i]["step"]) == int(r64[1].state[r64[0][i]]["step"])


def _adam_guarded(dev, n):
    rs = _rs("guard", n)
    p0 = _randn(rs, n)
    P_, M, V = Buf(dev, n, F32, p0), Buf(dev, n, F32, torch.zeros(n)), Buf(dev, n, F32, torch.zeros(n))
    FL = Buf(dev, 2, torch.int32, torch.zeros(2))
    p64, m64, v64 = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    bufs, skips, step = (P_, M, V), 0, 0
    st = _S(P_.v)

    def flag():
        return [int(a) for a in FL.cpu()]

    def finite_step():
        nonlocal p64, m64, v64, step
        step += 1
        g = _randn(rs, n)
        G = Buf(dev, n, F32, g)
        _call("rd_grad_finite_check", _P(G.v), n, _P(FL.v), st)
        assert flag() == [0, skips], ("finite gradients raised the flag", n, flag())
        _call("rd_adam_step_guarded", *(_adam_args(bufs, G.v, n, step, 0.0, 1.0) + (_P(FL.v), st)))
        _call("rd_adam_skip_count", _P(FL.v), st)
        assert flag() == [0, skips], flag()
        p64, m64, v64 = _adam_ref64(p64, g.double(), m64, v64, step, 0.0, 1.0)
        for b_, r in zip(bufs, (p64, m64, v64)):
            _check("guarded adam n=%d finite step %d" % (n, step), b_.v, r, None, None)      # floor only: a few fp32 ulp of max|ref|

    finite_step()      # moments are non-trivial from here on
    last_vec = (n // 4 - 1) * 4 + 2
    for bad in (float("inf"), float("nan")):
        for idx in (0, last_vec, n - 1):
            g = _randn(rs, n)
            g[idx] = bad
            G = Buf(dev, n, F32, g)
            what = "guarded adam n=%d %s at %d" % (n, bad, idx)
            for b_ in bufs:
                b_.snap = b_.full.clone()
            _call("rd_grad_finite_check", _P(G.v), n, _P(FL.v), st)
            assert flag()[0] != 0 and flag()[1] == skips, what + ": flag not raised %s" % flag()
            _call("rd_adam_step_guarded", *(_adam_args(bufs, G.v, n, step + 1, 0.0, 1.0) + (_P(FL.v), st)))
            for b_ in bufs:
                b_.check(what, unchanged=True)
            _call("rd_adam_skip_count", _P(FL.v), st)
            skips += 1
            assert flag() == [0, skips], what + ": skip counter / flag %s" % flag()
            finite_step()
    for big in (3.4028234e38, -3.4028234e38):
        for idx in (0, last_vec, n - 1):
            g = _randn(rs, n)
            g[idx] = big
            G = Buf(dev, n, F32, g)
            _call("rd_grad_finite_check", _P(G.v), n, _P(FL.v), st)
            assert flag() == [0, skips], "the largest finite fp32 tripped the flag (n=%d, index %d)" % (n, idx)
    FL.check("guarded adam flag")
    for b_ in bufs:
        b_.check("guarded adam n=%d" % n)


def adam_case(dev, quick=False):
    """rd_adam_step directly (vector body, scalar tail, in full mode a second grid-stride iteration of both) with weight decay and a
    gradient scale, three steps, against torch's single-tensor Adam arithmetic in float64; FlatAdam with weight_decay > 0 (the per-slot
    launch path) and a parameter without a gradient on step 2 against torch.optim.Adam in float64; the guarded step: one inf / NaN at the
    first element, in the last full vector or in the last tail element raises the flag, leaves p / m / v bit-identical, counts one skip and
    clears the flag, and the next finite step applies; +-FLT_MAX does not trip it."""
    for n in (1, 3, 4, 5, 1023, 1025) + (() if quick else (2048 * 256 * 4 + 4 * 300 + 3,)):
        for wd, gscale in ((0.0, 1.0), (1e-2, 1.0), (0.0, 1.0 / 1024), (1e-2, 0.5)):
            for family in ("normal", "zero", "tiny"):
                _adam_direct(dev, n, wd, gscale, family)
    _flat_adam(dev)
    for n in (5, 1025):
        _adam_guarded(dev, n)
