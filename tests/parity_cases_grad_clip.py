"""Global-norm gradient clipping on the device: rd_grad_clip_init / rd_grad_norm_partial / rd_grad_clip_finalize / rd_adam_step_groups_clipped
through the C ABI, FlatAdam.set_grad_clip and riders_amd.clip_grad_norm_ against torch.nn.utils.clip_grad_norm_ + torch.optim.Adam on the CPU, and
RC-Net / SML training steps, eager against graphed (see tests/parity_cases.py for how case functions are used by the emulator and GPU twins).

The references are torch's own functions on the CPU: torch.nn.utils.clip_grad_norm_ (the coefficient through torch.nn.utils.clip_grads_with_norm_
on a one-element gradient of 1.0) with torch.optim.Adam(foreach=False), and GradScaler("cpu") with unscale_ where a dynamic scale is involved.
Arithmetic comparisons are tests.parity_cases_glue._check (at most 4 x the error of torch's own fp32 result against the float64 restatement, floor
4 fp32 ulp of max|ref|); buffers handed to the C ABI carry sentinels on both sides.  Gradient scales and loss scales are powers of two, so the
float64 twin's multiplication is exact.  Every max_norm is at least 1 % away from the norm it is compared with (0.37 x or 1.9 x the float64 norm
in the ABI cases), so the fp32 results on both sides clamp alike.
"""
import numpy as np
import torch

from tests import parity_cases_adam_groups as A
from tests.parity_cases_glue import F32, Buf, _bits, _call, _check, _P, _randn, _refused, _rs, _S

NEW_ENTRIES = ("rd_grad_clip_init", "rd_grad_norm_partial", "rd_grad_clip_finalize", "rd_adam_step_groups_clipped")
OLD_ENTRIES = ("rd_grad_finite_check", "rd_adam_step", "rd_adam_step_guarded", "rd_adam_step_groups", "rd_adam_step_groups_scaled", "rd_adam_skip_count",
               "rd_loss_scale_update")
ROWS, L2, INF = 2048, 2, 0
KIND = {L2: 2.0, INF: float("inf")}
LARGE = 2048 * 256 * 4 + 1203      # a second grid-stride sweep (GPU twin only)
SIZES = (3, 1027, 1031)
TOTAL, COEF, PASSES, CLIPPED, NONFINITE = range(5)      # word index of the fields of rd_grad_clip_state


def _E():
    from riders_amd import engine
    return engine


def _sizes(quick):
    return SIZES if quick else SIZES + (LARGE,)


# ---------------------------------------------------------------------------------------------------------------- buffers
class Clip(object):
    """rd_grad_clip_state inside a sentinel-guarded int32 buffer"""

    def __init__(self, dev):
        self.buf = Buf(dev, 8, torch.int32, torch.full((8,), 0x5a5a5a5a, dtype=torch.int32))
        _call("rd_grad_clip_init", _P(self.buf.v), _S(self.buf.v))
        self.snapshot()
        assert self.get() == dict(total_norm=0.0, coef=1.0, passes=0, clipped=0, nonfinite=0, reserved=[0, 0, 0]), self.get()

    def snapshot(self):
        self.buf.snap = self.buf.full.clone()

    def words(self):
        return self.buf.cpu()

    def floats(self):
        return self.words()[0:2].view(F32).clone()

    def get(self):
        w = self.words()
        f = w[0:2].view(F32)
        return dict(total_norm=float(f[0]), coef=float(f[1]), passes=int(w[PASSES]), clipped=int(w[CLIPPED]), nonfinite=int(w[NONFINITE]),
                    reserved=[int(x) for x in w[5:8]])

    def poke_coef(self, coef):
        self.buf.v[COEF] = int(np.float32(coef).view(np.int32))
        self.snapshot()


class Buf64(Buf):
    """Buf for doubles: the sentinels are compared as 64-bit words (Buf's _bits views 8-byte elements as 16-bit ones, so its indices would be off)"""

    def check(self, what, unchanged=False):
        a, b = self.full.view(torch.int64).cpu(), self.snap.view(torch.int64).cpu()
        assert torch.equal(a[:self.lo], b[:self.lo]), what + ": elements in front of the buffer were overwritten"
        assert torch.equal(a[self.hi:], b[self.hi:]), what + ": elements behind the buffer were overwritten"
        if unchanged:
            assert torch.equal(a[self.lo:self.hi], b[self.lo:self.hi]), what + ": buffer changed"


def _partial(dev):
    """the partial rows, every one a NaN before the first launch: accumulate = 0 has to define them all"""
    return Buf64(dev, ROWS, torch.float64, torch.full((ROWS,), float("nan"), dtype=torch.float64))


class LossState(object):
    """rd_loss_scale_state inside a sentinel-guarded int32 buffer"""

    def __init__(self, dev, scale):
        self.buf = Buf(dev, 8, torch.int32, torch.full((8,), 0x5a5a5a5a, dtype=torch.int32))
        _call("rd_loss_scale_init", _P(self.buf.v), float(scale), 0, _S(self.buf.v))
        self.buf.snap = self.buf.full.clone()

    def poke(self, word, value):
        self.buf.v[word] = int(value)
        self.buf.snap = self.buf.full.clone()

    def inv(self):
        return float(self.buf.cpu()[0:2].view(F32)[1])


def _norm_launch(G, n, pre, state, kind, PB, accumulate=0, flag=None, off=0):
    _call("rd_grad_norm_partial", _P(G.v[off:off + n]), n, float(pre), _P(state.buf.v) if state is not None else None, kind, _P(PB.v), ROWS, accumulate,
          _P(flag.v) if flag is not None else None, _S(G.v))


def _finalize(PB, max_norm, kind, C):
    _call("rd_grad_clip_finalize", _P(PB.v), ROWS, float(max_norm), kind, _P(C.buf.v), _S(PB.v))


def _torch_norm(pieces, max_norm, kind, dt):
    """torch.nn.utils.clip_grad_norm_ on CPU parameters whose gradients are `pieces` -> (total norm, coefficient), both 0-dim tensors of dt; the
    coefficient is what torch.nn.utils.clip_grads_with_norm_ multiplies a gradient of 1.0 by"""
    ps = [torch.nn.Parameter(torch.zeros_like(g, dtype=dt)) for g in pieces]
    for p, g in zip(ps, pieces):
        p.grad = g.to(dt).clone()
    total = torch.nn.utils.clip_grad_norm_(ps, max_norm, norm_type=KIND[kind], foreach=False)
    one = torch.nn.Parameter(torch.zeros(1, dtype=dt))
    one.grad = torch.ones(1, dtype=dt)
    torch.nn.utils.clip_grads_with_norm_([one], max_norm, total, foreach=False)
    return total.detach(), one.grad[0].detach()


def _max_norms(pieces64, kind):
    """one max_norm that clips and one that does not, both far from the float64 norm, as the fp32 values the C ABI receives"""
    ref = float(_torch_norm(pieces64, 1.0, kind, torch.float64)[0])
    return [float(np.float32(f * ref)) for f in (0.37, 1.9)]


def _check_state(what, C, pieces, max_norm, kind, exact_norm=False):
    """total_norm and coef of the device state against torch's on `pieces` (the gradients the norm was taken of, already multiplied by pre)"""
    t64, c64 = _torch_norm([g.double() for g in pieces], max_norm, kind, torch.float64)
    t32, c32 = _torch_norm(pieces, max_norm, kind, F32)
    f = C.floats()
    _check(what + " total_norm", f[0:1], t64.reshape(1), t32.reshape(1), "grad_clip total_norm")
    _check(what + " coef", f[1:2], c64.reshape(1), c32.reshape(1), "grad_clip coef")
    if exact_norm:
        assert torch.equal(f[0:1], t32.reshape(1)), "%s: inf norm %r, torch %r" % (what, float(f[0]), float(t32))
    assert (float(f[1]) < 1.0) == (float(c64) < 1.0), (what, float(f[1]), float(c64))
    return float(c64) < 1.0


# ---------------------------------------------------------------------------------------------------------------- 1. norm pass + finalize
def _norm_one(dev, n, kind, gscale, scale=None):
    rs = _rs("grad_norm", n, kind, gscale, scale)
    g = _randn(rs, n) * (1.0 if scale is None else scale)
    G, PB, C = Buf(dev, n, F32, g), _partial(dev), Clip(dev)
    S = LossState(dev, scale) if scale is not None else None
    pre = float(np.float32(gscale) * np.float32(S.inv())) if S is not None else gscale      # the kernel's fp32 product (a power of two)
    seen = g * pre
    what = "grad_norm n=%d kind=%s gscale=%g scale=%s" % (n, KIND[kind], gscale, scale)
    clipped = 0
    for k, mn in enumerate(_max_norms([seen.double()], kind)):
        _norm_launch(G, n, gscale, S, kind, PB)
        _finalize(PB, mn, kind, C)
        clips = _check_state("%s max_norm=%g" % (what, mn), C, [seen], mn, kind, exact_norm=kind == INF and pre == 1.0)
        assert clips == (k == 0), (what, mn)
        clipped += clips
        st = C.get()
        assert (st["passes"], st["clipped"], st["nonfinite"]) == (2 * k + 1, 2 * clipped - clips, 0), (what, st)
        rows = PB.cpu()
        assert bool(torch.isfinite(rows).all()), what + ": accumulate = 0 left undefined rows"
        blocks = min((n + 1023) // 1024, ROWS)
        assert bool((rows[blocks:] == 0).all()), what + ": rows without data are not 0"
        before = (_bits(C.floats()).clone(), _bits(rows).clone())
        _norm_launch(G, n, gscale, S, kind, PB)
        _finalize(PB, mn, kind, C)
        assert torch.equal(_bits(C.floats()), before[0]) and torch.equal(_bits(PB.cpu()), before[1]), what + ": a second identical call differs"
        assert C.get()["passes"] == 2 * k + 2 and C.get()["clipped"] == 2 * clipped, (what, C.get())
    assert clipped == 1, (what, clipped)
    for b_ in (G,) + ((S.buf,) if S is not None else ()):
        b_.check(what, unchanged=True)
    PB.check(what)
    C.buf.check(what)


def norm_case(dev, quick=False):
    """rd_grad_norm_partial + rd_grad_clip_finalize for both norm kinds at 3 (tail only), 1027 (one vector sweep and the tail), 1031 and, on the GPU
    twin, a second grid-stride sweep; grad_scale 1 and 0.5, once with a live loss-scale state at 2^16.  total_norm and coef pass _check with a
    max_norm that clips and one that does not; the inf norm with pre = 1 equals torch's; a second identical call returns the same bits; rows
    without data hold 0; the counters count."""
    for kind in (L2, INF):
        for n in _sizes(quick):
            for gscale in (1.0, 0.5):
                _norm_one(dev, n, kind, gscale)
        _norm_one(dev, 1031, kind, 0.5, scale=2.0 ** 16)
    _norm_one(dev, 1027, L2, 1.0, scale=2.0 ** 16)


def accumulate_case(dev, quick=False):
    """accumulate: two disjoint ranges with a gap of poison between them give the norm of the two ranges alone (and leave a flag down); a smaller
    range with accumulate = 0 after a larger one is not polluted by stale rows; an all-zero arena gives norm 0 and coef 1"""
    for kind in (L2, INF):
        rs = _rs("grad_norm accumulate", kind)
        a, gap, b = 516, 8, 1027 if quick else LARGE
        g = _randn(rs, a + gap + b)
        g[a:a + gap] = torch.tensor([float("nan"), float("inf"), 1e30, -1e30] * 2)
        G, PB, C = Buf(dev, a + gap + b, F32, g), _partial(dev), Clip(dev)
        FL = Buf(dev, 2, torch.int32, torch.zeros(2, dtype=torch.int32))
        pieces = [g[:a].clone(), g[a + gap:].clone()]
        what = "grad_norm two ranges kind=%s" % KIND[kind]
        for mn in _max_norms([p_.double() for p_ in pieces], kind):
            _norm_launch(G, a, 1.0, None, kind, PB, 0, FL, 0)
            _norm_launch(G, b, 1.0, None, kind, PB, 1, FL, a + gap)
            _finalize(PB, mn, kind, C)
            _check_state(what, C, pieces, mn, kind, exact_norm=kind == INF)
        FL.check(what + ": the poison in the gap raised the flag", unchanged=True)
        G.check(what, unchanged=True)
        # a larger range first (several blocks' rows), then three elements alone
        n_big = 5000 if quick else LARGE
        big = Buf(dev, n_big, F32, 100.0 * _randn(rs, n_big))
        _norm_launch(big, n_big, 1.0, None, kind, PB)
        small = _randn(rs, 3)
        SM = Buf(dev, 3, F32, small)
        for mn in _max_norms([small.double()], kind):
            _norm_launch(SM, 3, 1.0, None, kind, PB)
            _finalize(PB, mn, kind, C)
            _check_state("grad_norm 3 elements after %d kind=%s" % (n_big, KIND[kind]), C, [small], mn, kind, exact_norm=kind == INF)
        Z = Buf(dev, 1031, F32, torch.zeros(1031))
        _norm_launch(Z, 1031, 0.5, None, kind, PB)
        _finalize(PB, 1.0, kind, C)
        f = C.floats()
        assert float(f[0]) == 0.0 and float(f[1]) == 1.0, (KIND[kind], f)
        for b_ in (PB, C.buf):
            b_.check("grad_norm accumulate")


# ---------------------------------------------------------------------------------------------------------------- 2. the finite flag
def finite_flag_case(dev, quick=False):
    """one inf or NaN at the first, the last or a tail element raises the flag pair exactly as rd_grad_finite_check does on the same buffer; a
    finite buffer leaves it down; the non-finite norm is counted and gives torch's coefficient (NaN for NaN, 0 for inf)"""
    for kind in (L2, INF):
        for n in (3, 1027, 1031) + (() if quick else (LARGE,)):
            tail0 = n & ~3
            for pos in sorted(set((0, n - 1, tail0 if tail0 < n else n - 1, n // 2))) + [None]:
                for bad in (float("inf"), float("nan"), -float("inf")) if pos is not None else (0.0,):
                    rs = _rs("grad_norm flag", n, pos)
                    g = _randn(rs, n)
                    if pos is not None:
                        g[pos] = bad
                    G, PB, C = Buf(dev, n, F32, g), _partial(dev), Clip(dev)
                    ours = Buf(dev, 2, torch.int32, torch.tensor([0, 7], dtype=torch.int32))
                    theirs = Buf(dev, 2, torch.int32, torch.tensor([0, 7], dtype=torch.int32))
                    _norm_launch(G, n, 0.5, None, kind, PB, 0, ours)
                    _call("rd_grad_finite_check", _P(G.v), n, _P(theirs.v), _S(G.v))
                    what = "grad_norm flag n=%d pos=%s value=%s kind=%s" % (n, pos, bad, KIND[kind])
                    assert torch.equal(ours.cpu(), theirs.cpu()), "%s: flag pair %s, rd_grad_finite_check %s" % (what, ours.cpu().tolist(), theirs.cpu().tolist())
                    assert (int(ours.cpu()[0]) != 0) == (pos is not None) and int(ours.cpu()[1]) == 7, (what, ours.cpu().tolist())
                    _finalize(PB, 1.0, kind, C)
                    st = C.get()
                    assert st["nonfinite"] == (pos is not None) and st["passes"] == 1, (what, st)
                    if pos is not None:
                        t32, c32 = _torch_norm([g * 0.5], 1.0, kind, F32)
                        assert np.isnan(st["total_norm"]) == bool(torch.isnan(t32)) and (np.isnan(st["total_norm"]) or st["total_norm"] == float(t32)), (what, st, t32)
                        assert np.isnan(st["coef"]) == bool(torch.isnan(c32)) and (np.isnan(st["coef"]) or st["coef"] == float(c32) == 0.0), (what, st, c32)
                        assert st["clipped"] == (0 if np.isnan(st["coef"]) else 1), (what, st)
                    for b_ in (ours, theirs, PB, C.buf):
                        b_.check(what)
                    G.check(what, unchanged=True)


# ---------------------------------------------------------------------------------------------------------------- 3. the clipped Adam launch
TABLES = ((3, (3,)), (1027, (1027,)), (1031, (512, 516, 1031)))


def _tables(quick):
    return TABLES if quick else TABLES + ((LARGE, (2048 * 256 * 4 + 400, LARGE)),)


def clipped_adam_identity_case(dev, quick=False):
    """coef = 1.0 (a freshly initialised state): parameters and moments bit-identical to rd_adam_step_groups in the static form (with and without
    a lowered skip flag) and to rd_adam_step_groups_scaled in the live-state form (host steps 0 and 2 ahead)"""
    for n, ends in _tables(quick):
        for shift in (0, 1):
            groups = A._groups(ends, shift)
            for live in (False, True):
                rs = _rs("adam_groups_clipped identity", n, shift, live)
                p0 = _randn(rs, n)
                X = [Buf(dev, n, F32, x) for x in (p0, torch.zeros(n), torch.zeros(n))]
                Y = [Buf(dev, n, F32, x) for x in (p0, torch.zeros(n), torch.zeros(n))]
                C = Clip(dev)
                S = LossState(dev, 1024.0) if live else None
                late, base = (2, 3) if live else (0, 0)
                if live:
                    S.poke(3, base + late)
                FL = Buf(dev, 2, torch.int32, torch.zeros(2, dtype=torch.int32))
                for step in (1, 2):
                    G = Buf(dev, n, F32, _randn(rs, n) * (1024.0 if live else 1.0))
                    t = A._table(groups, step + late)
                    if live:
                        _call("rd_adam_step_groups_scaled", _P(X[0].v), _P(G.v), _P(X[1].v), _P(X[2].v), n, t, 0.5, _P(S.buf.v), base, _S(G.v))
                        _call("rd_adam_step_groups_clipped", _P(Y[0].v), _P(G.v), _P(Y[1].v), _P(Y[2].v), n, t, 0.5, None, _P(S.buf.v), base, _P(C.buf.v), _S(G.v))
                    else:
                        skip = _P(FL.v) if step == 2 else None
                        _call("rd_adam_step_groups", _P(X[0].v), _P(G.v), _P(X[1].v), _P(X[2].v), n, t, 0.5, skip, _S(G.v))
                        _call("rd_adam_step_groups_clipped", _P(Y[0].v), _P(G.v), _P(Y[1].v), _P(Y[2].v), n, t, 0.5, skip, None, 0, _P(C.buf.v), _S(G.v))
                    G.check("adam_groups_clipped identity", unchanged=True)
                what = "rd_adam_step_groups_clipped with coef 1 (n=%d, ends=%s, %s)" % (n, ends, "live state" if live else "static")
                for x, y, nm in zip(X, Y, ("p", "exp_avg", "exp_avg_sq")):
                    assert torch.equal(_bits(x.full).cpu(), _bits(y.full).cpu()), "%s differs from the unclipped launch in %s" % (what, nm)
                assert not torch.equal(_bits(Y[1].v).cpu(), _bits(Y[1].snap[Y[1].lo:Y[1].hi]).cpu()), what + " wrote nothing"
                C.buf.check(what, unchanged=True)
                FL.check(what, unchanged=True)
                if live:
                    S.buf.check(what, unchanged=True)


def _clipped(dev, n, groups, coef, scale=None, late=0, base=0, gscale=0.5, nsteps=3, tag=""):
    """nsteps launches of rd_adam_step_groups_clipped with `coef` in the state against the float64 restatement of Adam on g * (pre * coef) and
    torch's fp32 Adam on the same gradient, group by group (static form, or the live-state form with the host steps `late` ahead)"""
    gscale = float(np.float32(gscale))
    rs = _rs("adam_groups_clipped", n, tuple(g.end for g in groups), coef, scale, late, tag)
    C = Clip(dev)
    C.poke_coef(coef)
    S = LossState(dev, scale) if scale is not None else None
    if S is not None:
        S.poke(3, base + late)
    pre = float(np.float32(gscale) * np.float32(S.inv())) if S is not None else gscale
    mult = float(np.float32(pre) * np.float32(coef))      # the kernel's fp32 product
    p0 = _randn(rs, n)
    P_, M, V = Buf(dev, n, F32, p0), Buf(dev, n, F32, torch.zeros(n)), Buf(dev, n, F32, torch.zeros(n))
    spans = list(zip([0] + [g.end for g in groups[:-1]], [g.end for g in groups]))
    r64 = [(p0[a:b].double(), torch.zeros(b - a, dtype=torch.float64), torch.zeros(b - a, dtype=torch.float64)) for a, b in spans]
    q32 = [torch.nn.Parameter(p0[a:b].clone()) for a, b in spans]
    opt32 = torch.optim.Adam(A._torch_groups(q32, groups), foreach=False)
    what = "adam_groups_clipped n=%d ends=%s coef=%g scale=%s late=%d %s" % (n, [g.end for g in groups], coef, scale, late, tag)
    for step in range(1, nsteps + 1):
        g = _randn(rs, n) * (1.0 if scale is None else float(scale))
        G = Buf(dev, n, F32, g)
        t = A._table(groups, step + late)
        _call("rd_adam_step_groups_clipped", _P(P_.v), _P(G.v), _P(M.v), _P(V.v), n, t, gscale, None, _P(S.buf.v) if S is not None else None, base,
              _P(C.buf.v), _S(G.v))
        for k, ((a, b), grp) in enumerate(zip(spans, groups)):
            q32[k].grad = None if grp.inactive else g[a:b] * mult
            if not grp.inactive:
                r64[k] = A._ref64_step(r64[k][0], g[a:b].double(), r64[k][1], r64[k][2], grp, step, mult)
        opt32.step()
        G.check(what, unchanged=True)
        C.buf.check(what, unchanged=True)
    got = [b_.cpu() for b_ in (P_, M, V)]
    for k, ((a, b), grp) in enumerate(zip(spans, groups)):
        if grp.inactive:
            for b_, nm in zip((P_, M, V), ("p", "exp_avg", "exp_avg_sq")):
                assert torch.equal(_bits(b_.v[a:b]).cpu(), _bits(b_.snap[b_.lo + a:b_.lo + b]).cpu()), "%s: %s of inactive group %d changed" % (what, nm, k)
            continue
        s32 = opt32.state[q32[k]]
        for x, r, r32, nm in zip(got, r64[k], (q32[k].detach(), s32["exp_avg"], s32["exp_avg_sq"]), ("p", "exp_avg", "exp_avg_sq")):
            _check("%s group %d %s" % (what, k, nm), x[a:b], r, r32, "adam_groups_clipped " + nm)
    for b_ in (P_, M, V):
        b_.check(what)


def clipped_adam_case(dev, quick=False):
    """coef 0.25 and 0.3 against float64 Adam on g * coef: coupled and decoupled decay (A._groups alternates them; the shift swaps the kinds), an
    inactive group, the group table (512, 516, 1031), both forms"""
    for coef in (0.25, 0.3):
        for n, ends in _tables(quick):
            for shift in (0, 1):
                _clipped(dev, n, A._groups(ends, shift), coef, nsteps=2 if n == LARGE else 3)
        _clipped(dev, 1031, A._groups((512, 516, 1031), 1), coef, gscale=1.0, tag="grad_scale 1")
        _clipped(dev, 1031, A._groups((512, 516, 1031), 0), coef, scale=1024.0, late=0, tag="live state")
        _clipped(dev, 1031, A._groups((512, 516, 1031), 1), coef, scale=2.0 ** 16, late=2, base=1, tag="live state, host 2 ahead")
        _clipped(dev, 1027, A._groups((1027,), 0), coef, scale=1024.0, late=1, tag="live state, one group")
        gs = A._groups((512, 516, 1031), 1, inactive=(1,))
        gs[1].hp, gs[1].wd = A.HP[2], A.WDS[2]
        _clipped(dev, 1031, gs, coef, tag="inactive middle group")
        _clipped(dev, 1031, A._groups((512, 516, 1031), 0, inactive=(2,)), coef, scale=1024.0, tag="live state, inactive last group")


def clipped_adam_skip_case(dev, quick=False):
    """skip_flag up, or found_inf up: nothing is written, bit for bit; lowered: the step applies"""
    n, groups = 1031, A._groups((512, 516, 1031), 0)
    for live in (False, True):
        rs = _rs("adam_groups_clipped skip", live)
        p0, g = _randn(rs, n), _randn(rs, n)
        P_, M, V, G = Buf(dev, n, F32, p0), Buf(dev, n, F32, torch.zeros(n)), Buf(dev, n, F32, torch.zeros(n)), Buf(dev, n, F32, g)
        C = Clip(dev)
        C.poke_coef(0.25)
        FL = Buf(dev, 2, torch.int32, torch.tensor([1, 0]))
        S = LossState(dev, 1.0)
        S.poke(2, 1)      # found_inf
        args = lambda: (_P(P_.v), _P(G.v), _P(M.v), _P(V.v), n, A._table(groups, 1), 1.0, None if live else _P(FL.v), _P(S.buf.v) if live else None, 0,      # noqa: E731
                        _P(C.buf.v), _S(G.v))
        _call("rd_adam_step_groups_clipped", *args())
        for b_ in (P_, M, V, G, FL, S.buf, C.buf):
            b_.check("adam_groups_clipped with the flag raised (%s)" % ("found_inf" if live else "skip_flag"), unchanged=True)
        FL.v.zero_()
        FL.snap = FL.full.clone()
        S.poke(2, 0)
        _call("rd_adam_step_groups_clipped", *args())
        assert not torch.equal(_bits(P_.v).cpu(), _bits(P_.snap[P_.lo:P_.hi]).cpu()), "adam_groups_clipped with the flag lowered wrote nothing"
        for b_ in (FL, S.buf, C.buf, G):
            b_.check("adam_groups_clipped flag lowered", unchanged=True)
        for b_ in (P_, M, V):
            b_.check("adam_groups_clipped flag lowered")


def refusal_case(dev, quick=False):
    """what the four entries refuse, with a message and without writing anything"""
    n = 1028
    rs = _rs("grad_clip refusals")
    bufs = [Buf(dev, n, F32, _randn(rs, n)) for _ in range(4)]
    P_, G, M, V = bufs
    PB, C, S = _partial(dev), Clip(dev), LossState(dev, 1024.0)
    FL = Buf(dev, 2, torch.int32, torch.zeros(2, dtype=torch.int32))
    everything = bufs + [PB, C.buf, S.buf, FL]
    st = _S(G.v)

    def refused(fn, text, *args):
        _refused(fn, text, *args)
        for b_ in everything:
            b_.check("refused %s (%s)" % (fn, text), unchanged=True)

    refused("rd_grad_clip_init", "null pointer", None, st)
    norm = lambda **k: (k.get("g", _P(G.v)), k.get("n", n), 1.0, None, k.get("kind", L2), k.get("pb", _P(PB.v)), k.get("rows", ROWS), k.get("acc", 0),      # noqa: E731
                        _P(FL.v), st)
    refused("rd_grad_norm_partial", "null pointer", *norm(g=None))
    refused("rd_grad_norm_partial", "null pointer", *norm(pb=None))
    for bad_n in (0, -4):
        refused("rd_grad_norm_partial", "n must be > 0", *norm(n=bad_n))
    for kind in (1, 3, -1):
        refused("rd_grad_norm_partial", "unknown norm kind", *norm(kind=kind))
    for rows in (0, 256, ROWS + 1):
        refused("rd_grad_norm_partial", "rows must be %d" % ROWS, *norm(rows=rows))
    refused("rd_grad_norm_partial", "accumulate must be 0 or 1", *norm(acc=2))
    fin = lambda **k: (k.get("pb", _P(PB.v)), k.get("rows", ROWS), k.get("mn", 1.0), k.get("kind", L2), k.get("c", _P(C.buf.v)), st)      # noqa: E731
    refused("rd_grad_clip_finalize", "null pointer", *fin(pb=None))
    refused("rd_grad_clip_finalize", "null pointer", *fin(c=None))
    refused("rd_grad_clip_finalize", "unknown norm kind", *fin(kind=1))
    refused("rd_grad_clip_finalize", "rows must be %d" % ROWS, *fin(rows=ROWS - 1))
    for mn in (0.0, -1.0, float("inf"), float("nan")):
        refused("rd_grad_clip_finalize", "max_norm must be finite and > 0", *fin(mn=mn))
    good = A._groups((512, 516, 1028))

    def adam(text, t, p=True, n_=n, skip=False, state=False, clip=True):
        refused("rd_adam_step_groups_clipped", text, _P(P_.v) if p else None, _P(G.v), _P(M.v), _P(V.v), n_, t, 1.0, _P(FL.v) if skip else None,
                _P(S.buf.v) if state else None, 0, _P(C.buf.v) if clip else None, st)

    adam("null pointer", A._table(good, 1), p=False)
    adam("null pointer", A._table(good, 1), clip=False)
    adam("null pointer", None)
    adam("n must be > 0", A._table(good, 1), n_=0)
    adam("exclusive", A._table(good, 1), skip=True, state=True)
    for state in (False, True):
        t = A._table(good, 1)
        t.count = 9
        adam("count must be 1..8", t, state=state)
        adam("strictly ascending", A._table(A._groups((516, 512, 1028)), 1), state=state)
        adam("not a multiple of 4", A._table(A._groups((510, 1028)), 1), state=state)
        adam("must equal n", A._table(good, 1), n_=1027, state=state)
        adam("must be >= 1", A._table(good, 0), state=state)


# ---------------------------------------------------------------------------------------------------------------- 5. FlatAdam against torch
INF_STEPS = (1, 3, 7)
NSTEPS = 10
SUBSET_STEP = 2      # parameters 1 and 3 get no gradient: their slots keep the gradient of step 1, which must not count
MAX_NORM = 1.0       # the toy gradients' norm is about 0.35 at amplitude 0.02 and about 17 at amplitude 1


def _amp(step):
    return 0.02 if step % 3 == 0 else 1.0


def _record(names):
    return [A._Count(nm) for nm in names]


class _Counts(object):
    def __init__(self, names=NEW_ENTRIES + OLD_ENTRIES):
        self.cs = _record(names)

    def __enter__(self):
        for c in self.cs:
            c.__enter__()
        return self

    def __exit__(self, *exc):
        for c in reversed(self.cs):
            c.__exit__(None, None, None)

    def __getitem__(self, name):
        return [c.n for c in self.cs if c.name == name][0]

    def dict(self):
        return dict((c.name, c.n) for c in self.cs if c.n)


def _give(dev, opt, ps, refs, grads, in_arena):
    """hand the step's gradients over: as user-assigned tensors outside the arena, or written into the arena views as a backward kernel writes them"""
    A._set_grads(dev, ps, refs, grads)
    if in_arena:
        for p, g in zip(ps, grads):
            p.grad = None
            if g is not None:
                opt._grad_view(p).copy_(g.to(dev))


def _flat_run(dev, what, init, split, hyper, cls=None, flat_kwargs=None, mode="plain", norm_type=2.0):
    rs = _rs("flatadam clip", what, mode, norm_type)
    ps, opt, refs = A._trio(dev, init, split, hyper, cls=cls, flat_kwargs=flat_kwargs)
    order = A._order(split) if split is not None else list(range(len(ps)))
    opt.set_grad_clip(MAX_NORM, norm_type)
    gss = None
    if mode == "dynamic":
        from tests.parity_cases_loss_scale import _scaler_pair
        scaler, gss = _scaler_pair(dev, 2.0 ** 12)
        opt.loss_scale = scaler
    elif mode == "static":
        opt.loss_scale = 1024.0
    clipped = skipped = zeroed = 0
    for step in range(1, NSTEPS + 1):
        scale = gss[F32].get_scale() if gss else 1024.0 if mode == "static" else 1.0
        grads = [_randn(rs, *s) * (_amp(step) * scale) for s in A.SHAPES]
        if step == SUBSET_STEP:
            grads[1] = grads[3] = None
        bad = mode != "plain" and step in INF_STEPS
        if bad:
            grads[2].view(-1)[step % 3] = float("nan") if step == 3 else float("inf")      # a NaN norm gives a NaN coefficient, an infinite one 0
        opt.zero_grad()
        for dt in refs:
            refs[dt][1].zero_grad()
        _give(dev, opt, ps, refs, grads, in_arena=step % 2 == 0)
        snap = [_bits(t_).clone() for t_ in (opt.flat_param, opt.exp_avg, opt.exp_avg_sq)]
        with _Counts() as c:
            opt.step()
        launches = c.dict()
        assert c["rd_grad_finite_check"] == 0, "%s step %d: rd_grad_finite_check ran while clipping is on (%s)" % (what, step, launches)
        assert c["rd_grad_norm_partial"] >= 1 and c["rd_grad_clip_finalize"] == 1 and c["rd_adam_step_groups_clipped"] >= 1, (what, step, launches)
        assert c["rd_adam_step"] == c["rd_adam_step_guarded"] == c["rd_adam_step_groups"] == c["rd_adam_step_groups_scaled"] == 0, (what, step, launches)
        assert c["rd_loss_scale_update"] == (mode == "dynamic") and c["rd_adam_skip_count"] == (mode == "static"), (what, step, launches)
        if step == SUBSET_STEP:
            assert c["rd_grad_norm_partial"] >= 2, (what, launches)      # the written slots form several runs
        norms = {}
        for dt, (rp, topt) in refs.items():
            if gss:
                gss[dt].unscale_(topt)
            elif mode == "static":
                for q in rp:
                    if q.grad is not None:
                        q.grad.mul_(1.0 / 1024.0)
            norms[dt] = torch.nn.utils.clip_grad_norm_(rp, MAX_NORM, norm_type=norm_type, foreach=False).detach()
            if gss:
                gss[dt].step(topt)
                gss[dt].update()
            elif not bad:
                topt.step()
        if bad:
            skipped += 1
            zeroed += step != 3
            for t_, s_, nm in zip((opt.flat_param, opt.exp_avg, opt.exp_avg_sq), snap, ("p", "exp_avg", "exp_avg_sq")):
                assert torch.equal(_bits(t_), s_), "%s step %d: %s changed in a skipped step" % (what, step, nm)
        else:
            clipped += float(norms[torch.float64]) > MAX_NORM
            assert abs(float(norms[torch.float64]) / MAX_NORM - 1.0) > 0.01
            _check("%s step %d grad_norm" % (what, step), opt.grad_norm.reshape(1), norms[torch.float64].reshape(1), norms[F32].reshape(1), "flatadam clip norm")
        st = opt.clip_stats()
        assert st["passes"] == step and st["clipped"] == clipped + zeroed and st["nonfinite"] == skipped, (what, step, st, clipped, zeroed, skipped)
        if gss:
            ss = scaler.stats()
            assert ss["scale"] == gss[F32].get_scale() and ss["growth_tracker"] == gss[F32]._get_growth_tracker(), (what, step, ss, gss[F32].state_dict())
            assert ss["skipped"] == skipped and ss["found_inf"] == 0, (what, step, ss)
        if mode == "static":
            assert opt.skipped_steps() == skipped
        sd = opt.state_dict()["state"]
        tsteps = [int(refs[F32][1].state[q]["step"]) if refs[F32][1].state.get(q) else 0 for q in refs[F32][0]]
        assert [int(sd[pos]["step"]) if pos in sd else 0 for pos in range(len(order))] == [tsteps[i] for i in order], (what, step, tsteps)
        for pos, i in enumerate(order):
            _check("%s step %d p%d" % (what, step, i), ps[i], refs[torch.float64][0][i].detach(), refs[F32][0][i].detach(), "flatadam clip p")
    assert 0 < clipped < NSTEPS - skipped, (what, clipped)      # some steps clipped, some did not
    r64, r32 = refs[torch.float64], refs[F32]
    sd = opt.state_dict()["state"]
    for pos, i in enumerate(order):
        for k in ("exp_avg", "exp_avg_sq"):
            _check("%s %s %d" % (what, k, i), sd[pos][k], r64[1].state[r64[0][i]][k], r32[1].state[r32[0][i]][k], "flatadam clip " + k)


def flat_adam_case(dev, quick=False):
    """FlatAdam.set_grad_clip against torch.nn.utils.clip_grad_norm_ + torch.optim.Adam on toy parameters: one group, two groups and FlatAdamW, ten
    steps whose gradients alternate between amplitudes that clip and that do not; step 2 gives gradients to a subset only; odd steps hand the
    gradients over as user-assigned tensors, even steps write them into the arena.  After each step the parameters and grad_norm pass _check.
    The same under a DynamicLossScale against GradScaler("cpu") with unscale_ (inf / NaN at steps 1, 3 and 7: scale, tracker and step counts
    equal, skipped steps leave everything bit-unchanged, no rd_grad_finite_check is launched) and under a static scale of 1024."""
    from riders_amd.optim import FlatAdamW
    E = _E()
    try:
        kw = dict(lr=A.HP[0][0], betas=A.HP[0][1:3], eps=A.HP[0][3])
        for mode in ("plain", "dynamic", "static"):
            _flat_run(dev, "one group", A._toy(), None, None, flat_kwargs=dict(kw, weight_decay=A.WDS[1]), mode=mode)
            _flat_run(dev, "two groups", A._toy(), A.SPLITS[2], A._hyper(2), mode=mode)
            _flat_run(dev, "FlatAdamW", A._toy(), None, None, cls=FlatAdamW, flat_kwargs=kw, mode=mode)
        _flat_run(dev, "two groups, inf norm", A._toy(), A.SPLITS[2], A._hyper(2), mode="plain", norm_type=float("inf"))
        _flat_run(dev, "one group, inf norm", A._toy(), None, None, flat_kwargs=dict(kw, weight_decay=0.0), mode="dynamic", norm_type=float("inf"))
        ps, opt, _ = A._trio(dev, A._toy(), None, None, flat_kwargs=kw)
        for bad in (1, 3.0, 0, "fro"):
            try:
                opt.set_grad_clip(1.0, bad)
            except ValueError:
                continue
            raise AssertionError("set_grad_clip accepted norm_type %r" % (bad,))
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            try:
                opt.set_grad_clip(bad)
            except ValueError:
                continue
            raise AssertionError("set_grad_clip accepted max_norm %r" % (bad,))
    finally:
        E.set_param_grad_allocator(None)


# ---------------------------------------------------------------------------------------------------------------- 6. off means untouched
class _Sequence(object):
    """the ordered names of the optimizer entries called, by wrapping the library attributes"""

    def __init__(self, names=NEW_ENTRIES + OLD_ENTRIES):
        self.names, self.log, self.saved = names, [], {}

    def __enter__(self):
        self.lib = _E().L()
        for nm in self.names:
            fn = getattr(self.lib, nm)
            self.saved[nm] = fn
            setattr(self.lib, nm, (lambda nm_, fn_: lambda *a: (self.log.append(nm_), fn_(*a))[1])(nm, fn))
        return self

    def __exit__(self, *exc):
        for nm, fn in self.saved.items():
            setattr(self.lib, nm, fn)


def _off_run(dev, split, mode, clip):
    """three steps; clip: None = never set, "reset" = set and reset to None, a number = set_grad_clip(that) -> (bits of p / m / v, call sequence,
    largest norm if clipping)"""
    from riders_amd.optim import DynamicLossScale, FlatAdam
    rs = _rs("clip off", split, mode)
    ps = [torch.nn.Parameter(x.clone().to(dev)) for x in A._toy(rs)]
    opt = FlatAdam(ps, lr=2e-3) if split is None else FlatAdam(A._dicts(ps, split, A._hyper(2)))
    scale = 1.0
    if mode == "dynamic":
        opt.loss_scale = DynamicLossScale(init_scale=1024.0, growth_interval=2, device=dev)
        scale = 1024.0
    elif mode == "static":
        opt.loss_scale = scale = 1024.0
    if clip == "reset":
        opt.set_grad_clip(0.5)
        opt.set_grad_clip(None)
    elif clip is not None:
        opt.set_grad_clip(clip)
    largest = 0.0
    with _Sequence() as seq:
        for step in (1, 2, 3):
            opt.zero_grad()
            for i, p in enumerate(ps):
                p.grad = None if (step == 2 and i == 1) else (_randn(rs, *p.shape) * scale).to(dev)
            opt.step()
            if clip not in (None, "reset"):
                largest = max(largest, float(opt.grad_norm))
    return [_bits(t_).cpu().clone() for t_ in (opt.flat_param, opt.exp_avg, opt.exp_avg_sq)], seq.log, largest


def _parent_sequence(split, mode):
    """What the three steps of _off_run called before clipping existed, written out.  Step 1 is uniform: one Adam launch.  Step 2 leaves parameter 1
    without a gradient: the written slots form two runs ([0] and [2, 3, 4]; with two groups one run per group), two launches.  Step 3 has every
    slot written but parameter 1 one step behind: three runs ([0], [1], [2, 3, 4]), three launches.  The static mode brackets the launches of a
    step with rd_grad_finite_check and rd_adam_skip_count, the dynamic mode with rd_grad_finite_check and rd_loss_scale_update."""
    if mode == "default":
        adam = "rd_adam_step" if split is None else "rd_adam_step_groups"
        return [adam] * 6
    if mode == "static":
        adam = "rd_adam_step_guarded" if split is None else "rd_adam_step_groups"
        return (["rd_grad_finite_check", adam, "rd_adam_skip_count"] + ["rd_grad_finite_check", adam, adam, "rd_adam_skip_count"]
                + ["rd_grad_finite_check", adam, adam, adam, "rd_adam_skip_count"])
    adam = "rd_adam_step_groups_scaled"
    return (["rd_grad_finite_check", adam, "rd_loss_scale_update"] + ["rd_grad_finite_check", adam, adam, "rd_loss_scale_update"]
            + ["rd_grad_finite_check", adam, adam, adam, "rd_loss_scale_update"])


def off_case(dev, quick=False):
    """clipping never set, or set and reset to None: a recorded step calls none of the new entries and exactly the sequence of old ones, in the
    default, static and dynamic modes, one group and two; with max_norm at >= 2 x the largest norm of the run a clipped run ends bit-identical
    to the unclipped one in parameters and moments"""
    E = _E()
    try:
        for split in (None, A.SPLITS[2]):
            for mode in ("default", "static", "dynamic"):
                base, seq0, _ = _off_run(dev, split, mode, None)
                reset, seq1, _ = _off_run(dev, split, mode, "reset")
                what = "clipping off (%s, %s)" % ("one group" if split is None else "two groups", mode)
                assert not set(seq0) & set(NEW_ENTRIES) and seq0 == seq1, (what, seq0, seq1)
                assert seq0 == _parent_sequence(split, mode), (what, seq0, _parent_sequence(split, mode))
                assert all(torch.equal(a, b) for a, b in zip(base, reset)), what + ": set and reset differs from never set"
                wide, seq2, largest = _off_run(dev, split, mode, 1e4)
                assert 0.0 < largest <= 0.5e4 and "rd_adam_step_groups_clipped" in seq2 and "rd_grad_finite_check" not in seq2, (what, largest, seq2)
                for a, b, nm in zip(base, wide, ("p", "exp_avg", "exp_avg_sq")):
                    assert torch.equal(a, b), "%s: a run clipped at 1e4 (largest norm %g) differs from the unclipped run in %s" % (what, largest, nm)
    finally:
        E.set_param_grad_allocator(None)


# ---------------------------------------------------------------------------------------------------------------- 7. the drop-in function
def _drop_run(dev, split, mode, norm_type, drop_in, extra_step=False):
    """three steps clipped at 0.5 (the third one's gradients are small: no clipping), persistently or through riders_amd.clip_grad_norm_ before
    every step() -> (bits of p / m / v, bits of (total_norm, coef) after each step)"""
    import riders_amd
    from riders_amd.optim import DynamicLossScale, FlatAdam
    rs = _rs("drop in", split, mode)
    ps = [torch.nn.Parameter(x.clone().to(dev)) for x in A._toy(rs)]
    opt = FlatAdam(ps, lr=2e-3) if split is None else FlatAdam(A._dicts(ps, split, A._hyper(2)))
    scale = 1.0
    if mode == "dynamic":
        opt.loss_scale = DynamicLossScale(init_scale=1024.0, growth_interval=2, device=dev)
        scale = 1024.0
    if not drop_in:
        opt.set_grad_clip(0.5, norm_type)
    norms = []
    for step in (1, 2, 3):
        opt.zero_grad()
        for i, p in enumerate(ps):
            p.grad = None if (step == 2 and i == 1) else (_randn(rs, *p.shape) * (scale * (0.001 if step == 3 else 1.0))).to(dev)
        if drop_in:
            with _Counts() as c:
                out = riders_amd.clip_grad_norm_((p_ for p_ in ps), 0.5, norm_type)      # a generator, as model.parameters() is
            assert c["rd_grad_norm_partial"] >= 1 and c["rd_grad_clip_finalize"] == 1 and c["rd_adam_step_groups_clipped"] == 0, c.dict()
            assert out.data_ptr() == opt.grad_norm.data_ptr() and out.dim() == 0 and out.dtype == F32 and out.device == opt.flat_param.device
        with _Counts() as c:
            opt.step()
        assert c["rd_adam_step_groups_clipped"] >= 1 and c["rd_grad_clip_finalize"] == (0 if drop_in else 1), c.dict()
        assert c["rd_grad_finite_check"] == (1 if drop_in and mode == "dynamic" else 0), c.dict()
        norms.append(_bits(opt._clip_state[0:2]).cpu().clone())
    st = opt.clip_stats()
    assert st["clipped"] == 2 and st["passes"] == 3 and st["nonfinite"] == 0, st
    bits = [_bits(t_).cpu().clone() for t_ in (opt.flat_param, opt.exp_avg, opt.exp_avg_sq)]
    if extra_step:      # armed for one step only: the next one is the plain launch
        opt.zero_grad()
        for p in ps:
            p.grad = (_randn(rs, *p.shape) * scale).to(dev)
        with _Counts() as c:
            opt.step()
        assert not set(c.dict()) & set(NEW_ENTRIES), c.dict()
        assert opt.clip_stats()["passes"] == 3
    return bits, norms


def _alias_case(dev):
    """INTEGRATION.md's aliasing line, torch.nn.utils.clip_grad_norm_ = riders_amd.clip_grad_norm_: the fast path through the alias, and every
    fallback (a plain parameter of no FlatAdam, a subset, norm_type 3, error_if_nonfinite) reaches torch's OWN function, not the alias again"""
    import riders_amd
    from riders_amd.optim import FlatAdam
    original = torch.nn.utils.clip_grad_norm_
    torch.nn.utils.clip_grad_norm_ = riders_amd.clip_grad_norm_
    try:
        rs = _rs("drop in alias")
        plain = torch.nn.Parameter(_randn(rs, 7).to(dev))
        plain.grad = (10.0 * _randn(rs, 7)).to(dev)
        twin = torch.nn.Parameter(plain.detach().cpu().clone())
        twin.grad = plain.grad.detach().cpu().clone()
        got, want = torch.nn.utils.clip_grad_norm_([plain], 1.0), original([twin], 1.0)
        _check("aliased clip_grad_norm_ on a plain parameter: norm", got.reshape(1), want.double().reshape(1), None)
        _check("aliased clip_grad_norm_ on a plain parameter: gradient", plain.grad, twin.grad.double(), None)
        ps = [torch.nn.Parameter(x.clone().to(dev)) for x in A._toy(rs)]
        opt = FlatAdam(ps, lr=2e-3)
        for kwargs, subset in ((dict(), None), (dict(), (0, 2)), (dict(norm_type=3), None), (dict(error_if_nonfinite=True), None)):
            opt.zero_grad()
            for p in ps:
                p.grad = _randn(rs, *p.shape).to(dev)
            with _Counts() as c:
                out = torch.nn.utils.clip_grad_norm_([ps[i] for i in subset] if subset else ps, 0.5, **kwargs)
            fast = not kwargs and subset is None
            assert (c["rd_grad_clip_finalize"] == 1) == fast and (out.data_ptr() == opt.grad_norm.data_ptr()) == fast, (kwargs, subset, c.dict())
            with _Counts() as c:
                opt.step()
            assert (c["rd_adam_step_groups_clipped"] >= 1) == fast and (c["rd_adam_step"] >= 1) == (not fast), (kwargs, subset, c.dict())
        # the armed coefficient belongs to the gradients it was formed from: zero_grad() drops it
        opt.zero_grad()
        for p in ps:
            p.grad = _randn(rs, *p.shape).to(dev)
        torch.nn.utils.clip_grad_norm_(ps, 0.5)
        opt.zero_grad()
        for p in ps:
            p.grad = _randn(rs, *p.shape).to(dev)
        with _Counts() as c:
            opt.step()
        assert not set(c.dict()) & set(NEW_ENTRIES), c.dict()
    finally:
        torch.nn.utils.clip_grad_norm_ = original
        _E().set_param_grad_allocator(None)


def drop_in_case(dev, quick=False):
    """riders_amd.clip_grad_norm_: the fast path equals the persistent form bit for bit, returns the optimizer's device norm tensor and arms
    exactly one step; a subset of the parameters, error_if_nonfinite=True and norm_type=3 return what torch returns and leave the plain launch"""
    import riders_amd
    from riders_amd.optim import FlatAdam
    E = _E()
    try:
        for split in (None, A.SPLITS[2]):
            for mode in ("default", "dynamic"):
                for norm_type in (2.0, float("inf")):
                    what = "clip_grad_norm_ + step() against set_grad_clip (%s, %s, %s)" % (split, mode, norm_type)
                    bits0, norms0 = _drop_run(dev, split, mode, norm_type, False)
                    bits1, norms1 = _drop_run(dev, split, mode, norm_type, True, extra_step=True)
                    assert all(torch.equal(a, b) for a, b in zip(norms0, norms1)), what + ": norm / coefficient bits differ"
                    for a, b, nm in zip(bits0, bits1, ("p", "exp_avg", "exp_avg_sq")):
                        assert torch.equal(a, b), "%s differs in %s" % (what, nm)
        _alias_case(dev)
        # fallbacks: torch's own function on the same tensors
        rs = _rs("drop in fallback")
        ps = [torch.nn.Parameter(x.clone().to(dev)) for x in A._toy(rs)]
        opt = FlatAdam(ps, lr=2e-3)
        for kwargs, subset in ((dict(), (0, 2)), (dict(error_if_nonfinite=True), None), (dict(norm_type=3), None), (dict(norm_type=3.0, foreach=False), None)):
            opt.zero_grad()
            grads = [_randn(rs, *p.shape) for p in ps]
            for p, g in zip(ps, grads):
                p.grad = g.clone().to(dev)
            sel = [ps[i] for i in subset] if subset else ps
            twins = [torch.nn.Parameter(torch.zeros_like(g)) for g in grads]
            for q, g in zip(twins, grads):
                q.grad = g.clone()
            want = torch.nn.utils.clip_grad_norm_([twins[i] for i in subset] if subset else twins, 0.5, **kwargs)
            with _Counts() as c:
                got = riders_amd.clip_grad_norm_(sel, 0.5, **kwargs)
                assert not c.dict(), c.dict()
                assert torch.equal(got.detach().cpu(), want) or float((got.detach().cpu() - want).abs()) <= 4 * 2.0 ** -23 * float(want), (kwargs, got, want)
                for p, q in zip(ps, twins):
                    _check("fallback %s clipped gradient" % (kwargs,), p.grad, q.grad.double(), None, None)
                opt.step()
                assert not set(c.dict()) & set(NEW_ENTRIES) and c["rd_adam_step"] >= 1, c.dict()
    finally:
        E.set_param_grad_allocator(None)


# ---------------------------------------------------------------------------------------------------------------- 8. models (GPU twin)
def _arena_norm_check(what, opt, grads, touched, inv_scale):
    """torch's clip_grad_norm_ on the CPU copy of the arena gradient (unscaled, the written slots only) against grad_norm"""
    pieces = [grads[o:o + p.numel()] * inv_scale for i, (p, o) in enumerate(zip(opt.params, opt.offsets)) if i in touched]
    t64 = _torch_norm([x.double() for x in pieces], 1.0, L2, torch.float64)[0]
    t32 = _torch_norm(pieces, 1.0, L2, F32)[0]
    _check(what, opt.grad_norm.reshape(1), t64.reshape(1), t32.reshape(1), "model clip norm")
    return float(t64)


def _model_case(dev, name, precision, build, eager_step, graphed_step):
    """three steps with set_grad_clip at a max_norm below the first step's norm: eager against graphed, parameters and the 32 bytes of clip
    state bit-identical; after each eager step the arena gradient, copied to the CPU, gives grad_norm through torch"""
    from riders_amd import engine
    from riders_amd.optim import DynamicLossScale
    engine.set_compute_dtype(precision)
    engine.clear_caches()
    try:
        # the first step's norm, from a probe run without clipping
        model, opt, ctx = build()
        scaler = DynamicLossScale(init_scale=2.0 ** 10, growth_interval=2, device=dev) if precision == "fp16" else None
        opt.set_grad_clip(1e30)
        eager_step(model, opt, ctx, scaler)
        first = float(opt.grad_norm)
        assert np.isfinite(first) and first > 0, (name, precision, first)
        max_norm = float(np.float32(first * 0.25))
        engine.set_param_grad_allocator(None)
        engine.clear_caches()
        runs = []
        for graphed in (False, True):
            model, opt, ctx = build()
            scaler = DynamicLossScale(init_scale=2.0 ** 10, growth_interval=2, device=dev) if precision == "fp16" else None
            opt.set_grad_clip(max_norm)
            if graphed:
                step = graphed_step(model, opt, ctx, scaler)
                for _ in range(3):
                    step()
                del step
            else:
                for k in range(3):
                    inv = 1.0 / scaler.get_scale() if scaler is not None else 1.0
                    eager_step(model, opt, ctx, scaler, before_step=lambda o: (o.flat_grad.detach().cpu(), set(o.touched_indices())), holder=runs)
                    grads, touched = runs.pop()
                    norm = _arena_norm_check("%s %s step %d grad_norm" % (name, precision, k + 1), opt, grads, touched, inv)
                    print("%s %s step %d: gradient norm %.5g, max_norm %.5g, coef %.4f" % (name, precision, k + 1, norm, max_norm, opt.clip_stats()["coef"]))
                assert opt.clip_stats()["clipped"] >= 1
            runs.append((_bits(opt.flat_param).clone(), _bits(opt._clip_state).cpu().clone(), scaler.stats() if scaler is not None else None))
            assert bool(torch.isfinite(opt.flat_param).all())
            engine.set_param_grad_allocator(None)
            engine.clear_caches()
        assert runs[0][2] == runs[1][2], (runs[0][2], runs[1][2])
        assert torch.equal(runs[0][1], runs[1][1]), "%s %s: clip state of the graphed steps differs from the eager ones" % (name, precision)
        assert torch.equal(runs[0][0], runs[1][0]), "%s %s: graphed clipped steps differ from the eager ones" % (name, precision)
    finally:
        engine.set_compute_dtype("fp32")
        engine.set_param_grad_allocator(None)
        engine.clear_caches()


def rcnet_case(dev, precision):
    """RC-Net at 2 images of 64 x 96, K = 3 (the geometry of the fp16 loss-scale case), bf16 without a scale or fp16 with a DynamicLossScale"""
    from riders_amd import engine, rcnet_main
    from riders_amd.optim import FlatAdam
    from tests.parity_cases_frozen import _g6_model
    lr, betas, eps = float(np.float32(1e-3)), A.HP[0][1:3], A.HP[0][3]

    def build():
        model, cfg = _g6_model(dev)
        model.train()
        return model, FlatAdam(model.parameters(), lr=lr, betas=betas, eps=eps), (cfg, rcnet_main.synthetic_batch(2, 64, 96, cfg, seed=77, device=dev))

    def eager(model, opt, ctx, scaler, before_step=None, holder=None):
        cfg, batch = ctx
        rcnet_main.compute_gradients(model, opt, batch, cfg, **(dict(loss_scale=scaler) if scaler is not None else {}))
        if before_step is not None:
            holder.append(before_step(opt))
        opt.step()

    def graphed(model, opt, ctx, scaler):
        cfg, batch = ctx
        return rcnet_main.GraphedTrainStep(model, opt, batch, cfg, warmup=1, **(dict(loss_scale=scaler) if scaler is not None else {}))

    engine.set_deterministic_roi_pool(True)
    try:
        _model_case(dev, "rcnet", precision, build, eager, graphed)
    finally:
        engine.set_deterministic_roi_pool(False)


def sml_case(dev, precision):
    """Scale Map Learner at 2 frames of 64 x 96, bf16 without a scale or fp16 with a DynamicLossScale"""
    from riders_amd import sml_main
    from riders_amd.optim import FlatAdam
    cfg = sml_main.ZJU_SML_CONFIG

    def build():
        torch.manual_seed(0)
        m = sml_main.build_model(dev, cfg)
        m.train()
        return m, FlatAdam(m.parameters(), lr=cfg['learning_rate']), (sml_main.synthetic_batch(2, 64, 96, seed=33, device=dev), sml_main.make_outlier_removal(cfg))

    def eager(model, opt, ctx, scaler, before_step=None, holder=None):
        batch, outlier = ctx
        if before_step is None:
            sml_main.train_step(model, opt, batch, cfg, outlier=outlier, **(dict(loss_scale=scaler) if scaler is not None else {}))
            return
        real = opt.step      # train_step runs opt.step() itself: look at the arena just before it

        def spy():
            holder.append(before_step(opt))
            real()
        opt.step = spy
        try:
            sml_main.train_step(model, opt, batch, cfg, outlier=outlier, **(dict(loss_scale=scaler) if scaler is not None else {}))
        finally:
            del opt.step

    def graphed(model, opt, ctx, scaler):
        batch, outlier = ctx
        return sml_main.GraphedTrainStep(model, opt, batch, cfg, outlier=outlier, warmup=1, **(dict(loss_scale=scaler) if scaler is not None else {}))

    _model_case(dev, "sml", precision, build, eager, graphed)
