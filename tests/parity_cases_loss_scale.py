"""Dynamic fp16 loss scale on the device: rd_loss_scale_init / rd_loss_scale_update / rd_adam_step_groups_scaled through the C ABI, FlatAdam with an
optim.DynamicLossScale against torch.amp.GradScaler("cpu") + torch.optim.Adam, the static path's launches, and RC-Net / SML fp16 training steps,
eager and graphed (see tests/parity_cases.py for how case functions are used by the emulator and GPU twins).

The references are torch's own: torch._amp_update_scale_ on CPU tensors for the update rule (scale and growth tracker must be EQUAL after every
step) and GradScaler("cpu") + torch.optim.Adam(foreach=False) for everything that steps.  Arithmetic comparisons are tests.parity_cases_glue._check
(at most 4 x the error of torch's own fp32 result against the float64 restatement, floor 4 fp32 ulp of max|ref|); buffers handed to the C ABI
carry sentinels on both sides.  Scales are powers of two or 3 * 2^10, so the float64 twin's unscale is exact.
"""
import ctypes

import numpy as np
import torch

from tests import parity_cases_adam_groups as A
from tests.parity_cases_glue import F32, Buf, _bits, _call, _check, _P, _randn, _refused, _rs, _S

FLT_MIN = 2.0 ** -126
NEW_ENTRIES = ("rd_loss_scale_init", "rd_loss_scale_update", "rd_adam_step_groups_scaled")
SCALE, INV, FOUND, SKIPPED, TRACKER, BACKOFFS, GROWTHS = range(7)      # word index of every field of rd_loss_scale_state


def _E():
    from riders_amd import engine
    return engine


# ---------------------------------------------------------------------------------------------------------------- the state buffer
class State(object):
    """rd_loss_scale_state inside a sentinel-guarded int32 buffer"""

    def __init__(self, dev, scale, tracker=0):
        self.buf = Buf(dev, 8, torch.int32, torch.full((8,), 0x5a5a5a5a, dtype=torch.int32))
        _call("rd_loss_scale_init", _P(self.buf.v), float(scale), tracker, _S(self.buf.v))
        self.snapshot()

    def snapshot(self):
        self.buf.snap = self.buf.full.clone()

    def poke(self, word, value):
        self.buf.v[word] = int(value)
        self.snapshot()

    def words(self):
        return self.buf.cpu()

    def get(self):
        w = self.words()
        f = w[0:2].view(torch.float32)
        return dict(scale=float(f[0]), inv_scale=float(f[1]), found_inf=int(w[FOUND]), skipped=int(w[SKIPPED]), growth_tracker=int(w[TRACKER]),
                    backoffs=int(w[BACKOFFS]), growths=int(w[GROWTHS]), reserved=int(w[7]))

    def raise_flag(self, dev):
        """as FlatAdam does: rd_grad_finite_check on &state->found_inf, here over a gradient with one inf"""
        g = torch.ones(5)
        g[3] = float("inf")
        G = Buf(dev, 5, F32, g)
        _call("rd_grad_finite_check", _P(G.v), 5, _P(self.buf.v[FOUND:FOUND + 2]), _S(G.v))
        assert self.get()["found_inf"] != 0


def _inv32(scale):
    """(float)(1.0 / (double)scale)"""
    return float(np.float32(1.0 / float(np.float32(scale))))


# ---------------------------------------------------------------------------------------------------------------- 2. the update kernel
PATTERNS = ("0000000000", "1111100000", "0100100010", "0011001100", "1010101010", "0000011111")


def _update_run(dev, init, growth, backoff, interval, pattern):
    growth, backoff = float(np.float32(growth)), float(np.float32(backoff))
    S = State(dev, init)
    st = S.get()
    assert st == dict(scale=float(np.float32(init)), inv_scale=_inv32(init), found_inf=0, skipped=0, growth_tracker=0, backoffs=0, growths=0, reserved=0), st
    sc, tr = torch.tensor([init], dtype=F32), torch.zeros(1, dtype=torch.int32)
    skipped = backoffs = growths = 0
    what = "loss_scale_update init=%g growth=%g backoff=%g interval=%d pattern=%s" % (init, growth, backoff, interval, pattern)
    for i, c in enumerate(pattern):
        bad = c == "1"
        if bad:
            S.raise_flag(dev)
        before = float(sc)
        _call("rd_loss_scale_update", _P(S.buf.v), growth, backoff, interval, _S(S.buf.v))
        torch._amp_update_scale_(sc, tr, torch.tensor([1.0 if bad else 0.0]), growth, backoff, interval)
        skipped += bad
        backoffs += float(sc) < before
        growths += float(sc) > before
        got = S.get()
        want = dict(scale=float(sc), inv_scale=_inv32(float(sc)), found_inf=0, skipped=skipped, growth_tracker=int(tr), backoffs=backoffs, growths=growths,
                    reserved=0)
        assert got == want, "%s, step %d: state %s, torch %s" % (what, i, got, want)
    S.buf.check(what)
    return S


def update_case(dev, quick=False):
    """rd_loss_scale_update against torch._amp_update_scale_ on the CPU: scale, tracker, reciprocal and counters equal after every step of every
    scripted overflow pattern, for factors 2 / 0.5 at intervals 1, 2, 3 and for 1.5 / 0.75 at interval 2; at 2^127 a growth by 2 is not finite:
    the scale stays and the tracker resets, as torch does."""
    for interval in (1, 2, 3):
        for pattern in PATTERNS:
            _update_run(dev, 65536.0, 2.0, 0.5, interval, pattern)
    for pattern in PATTERNS:
        _update_run(dev, 1024.0, 1.5, 0.75, 2, pattern)
    S = _update_run(dev, 2.0 ** 127, 2.0, 0.5, 1, "000")
    assert S.get()["scale"] == 2.0 ** 127 and S.get()["growth_tracker"] == 0 and S.get()["growths"] == 0
    S = _update_run(dev, 2.0 ** 127, 2.0, 0.5, 2, "0001000")
    assert S.get()["scale"] == 2.0 ** 127 and S.get()["backoffs"] == 1 and S.get()["growths"] == 1


def update_floor_case(dev, quick=False):
    """the one departure from torch: repeated backoff from 2^-125 stops at a normal fp32 whose reciprocal is finite (torch goes denormal, then 0)"""
    S = State(dev, 2.0 ** -125)
    for i in range(5):
        S.raise_flag(dev)
        _call("rd_loss_scale_update", _P(S.buf.v), 2.0, 0.5, 2, _S(S.buf.v))
        st = S.get()
        assert st["scale"] >= FLT_MIN and np.isfinite(st["inv_scale"]) and st["inv_scale"] == _inv32(st["scale"]), (i, st)
        assert st["found_inf"] == 0 and st["skipped"] == i + 1 and st["growth_tracker"] == 0, (i, st)
    assert st["scale"] == FLT_MIN and st["backoffs"] == 1, st
    for factor in (0.75, 0.999):      # a factor that would land between the denormals and FLT_MIN
        S = State(dev, FLT_MIN * 1.25)
        S.raise_flag(dev)
        _call("rd_loss_scale_update", _P(S.buf.v), 2.0, float(np.float32(factor)), 2, _S(S.buf.v))
        st = S.get()
        assert st["scale"] >= FLT_MIN and np.isfinite(st["inv_scale"]), st
    S.buf.check("loss_scale_update floor")


def update_refusal_case(dev, quick=False):
    """what the two state entries refuse, with a message and without touching the state"""
    S = State(dev, 1024.0, tracker=3)
    assert S.get()["growth_tracker"] == 3
    st = _S(S.buf.v)
    for scale in (0.0, -1.0, float("inf"), float("nan"), 1e-39):
        _refused("rd_loss_scale_init", "scale must be finite and >= FLT_MIN", _P(S.buf.v), scale, 0, st)
    _refused("rd_loss_scale_init", "growth_tracker must be >= 0", _P(S.buf.v), 2.0, -1, st)
    _refused("rd_loss_scale_init", "null pointer", None, 2.0, 0, st)
    for growth in (1.0, 0.5, float("nan"), float("inf")):
        _refused("rd_loss_scale_update", "growth_factor must be > 1", _P(S.buf.v), growth, 0.5, 2, st)
    for backoff in (0.0, 1.0, 1.5, -0.5, float("nan")):
        _refused("rd_loss_scale_update", "backoff_factor must be in (0, 1)", _P(S.buf.v), 2.0, backoff, 2, st)
    for interval in (0, -1):
        _refused("rd_loss_scale_update", "growth_interval must be >= 1", _P(S.buf.v), 2.0, 0.5, interval, st)
    _refused("rd_loss_scale_update", "null pointer", None, 2.0, 0.5, 2, st)
    S.buf.check("refused loss-scale entries", unchanged=True)


# ---------------------------------------------------------------------------------------------------------------- 3. the scaled Adam launch
def _table_late(groups, step, late):
    t = A._table(groups, step)
    for k, g in enumerate(groups):
        t.step[k] = g.step0 + step + late      # the host counted the skipped steps too
    return t


def _scaled(dev, n, groups, scale, late=0, base=0, gscale=0.5, nsteps=3, tag=""):
    """nsteps launches of rd_adam_step_groups_scaled with the host steps `late` ahead (state->skipped = base + late) against the float64 restatement
    and torch's fp32 Adam at the EFFECTIVE step, group by group; the launch leaves the state bit-unchanged"""
    gscale = float(np.float32(gscale))
    rs = _rs("adam_groups_scaled", n, tuple(g.end for g in groups), scale, late, base, tag)
    S = State(dev, scale)
    S.poke(SKIPPED, base + late)
    unscale = float(np.float32(gscale) * np.float32(S.get()["inv_scale"]))      # the kernel's fp32 product
    p0 = _randn(rs, n)
    P_, M, V = Buf(dev, n, F32, p0), Buf(dev, n, F32, torch.zeros(n)), Buf(dev, n, F32, torch.zeros(n))
    spans = list(zip([0] + [g.end for g in groups[:-1]], [g.end for g in groups]))
    r64 = [(p0[a:b].double(), torch.zeros(b - a, dtype=torch.float64), torch.zeros(b - a, dtype=torch.float64)) for a, b in spans]
    q32 = [torch.nn.Parameter(p0[a:b].clone()) for a, b in spans]
    opt32 = torch.optim.Adam(A._torch_groups(q32, groups), foreach=False)
    for q, g in zip(q32, groups):
        if g.step0 > 0:
            opt32.state[q] = dict(step=torch.tensor(float(g.step0)), exp_avg=torch.zeros_like(q), exp_avg_sq=torch.zeros_like(q))
    what = "adam_groups_scaled n=%d ends=%s scale=%g late=%d base=%d %s" % (n, [g.end for g in groups], scale, late, base, tag)
    for step in range(1, nsteps + 1):
        g = _randn(rs, n) * float(scale)      # a scaled gradient
        G = Buf(dev, n, F32, g)
        _call("rd_adam_step_groups_scaled", _P(P_.v), _P(G.v), _P(M.v), _P(V.v), n, _table_late(groups, step, late), gscale, _P(S.buf.v), base, _S(G.v))
        for k, ((a, b), grp) in enumerate(zip(spans, groups)):
            q32[k].grad = g[a:b] * unscale
            r64[k] = A._ref64_step(r64[k][0], g[a:b].double(), r64[k][1], r64[k][2], grp, grp.step0 + step, unscale)
        opt32.step()
        G.check(what, unchanged=True)
        S.buf.check(what, unchanged=True)
    got = [b_.cpu() for b_ in (P_, M, V)]
    for k, ((a, b), grp) in enumerate(zip(spans, groups)):
        s32 = opt32.state[q32[k]]
        assert int(s32["step"]) == grp.step0 + nsteps
        for x, r, r32, nm in zip(got, r64[k], (q32[k].detach(), s32["exp_avg"], s32["exp_avg_sq"]), ("p", "exp_avg", "exp_avg_sq")):
            _check("%s group %d %s" % (what, k, nm), x[a:b], r, r32, "adam_groups_scaled " + nm)
    for b_ in (P_, M, V):
        b_.check(what)


SCALES = (2.0 ** 10, 3.0 * 2.0 ** 10)
ARENAS = ((8, (8,)), (8, (4, 8)), (12, (4, 8, 12)), (1028, (1028,)), (1028, (512, 516, 1028)), (2052, (1024, 2052)), (2052, (1024, 1028, 2052)),
          (1031, (512, 516, 1031)), (1023, (1023,)))


def scaled_adam_case(dev, quick=False):
    """rd_adam_step_groups_scaled on arenas of 8, 12, 1028 and 2052 elements (and 1031 / 1023: a scalar tail) in 1 to 3 groups, coupled and decoupled
    decay (A._groups alternates them; the shift swaps the kinds), scales 2^10 and 3 * 2^10 with grad_scale 0.5, and the host steps 0, 1 and 5
    ahead of the device's skip count (with and without a non-zero skipped_base)."""
    for i, (n, ends) in enumerate(ARENAS):
        for shift in (0, 1):
            for j, late in enumerate((0, 1, 5)):
                _scaled(dev, n, A._groups(ends, shift), SCALES[(i + shift + j) % 2], late=late, base=(0, 3)[(i + j) % 2])
    _scaled(dev, 1028, A._groups((512, 1028), 1, step0s=(0, 6)), SCALES[1], late=2, base=1, tag="steps 1 and 7")


def first_applied_step_case(dev, quick=False):
    """5 skips, then the first applied step: the host hands in step 6, the update must be the one of a twin whose step is 1 (with the host's
    count the bias correction 1 - 0.9^6 would make it 4.7 x too small)"""
    for n, ends in ((12, (4, 8, 12)), (1031, (512, 516, 1031)), (1028, (1028,))):
        for shift in (0, 2):
            _scaled(dev, n, A._groups(ends, shift), SCALES[0], late=5, base=0, nsteps=1, tag="first applied step")
            _scaled(dev, n, A._groups(ends, shift), SCALES[1], late=5, base=7, nsteps=1, tag="first applied step, base 7")


def scaled_adam_found_inf_case(dev, quick=False):
    """found_inf raised: parameters, moments and the state are bit-unchanged by the launch; cleared: the step applies"""
    n, groups = 1031, A._groups((512, 516, 1031), 0)
    rs = _rs("adam_groups_scaled found_inf")
    p0, g = _randn(rs, n), _randn(rs, n) * 1024.0
    P_, M, V, G = Buf(dev, n, F32, p0), Buf(dev, n, F32, torch.zeros(n)), Buf(dev, n, F32, torch.zeros(n)), Buf(dev, n, F32, g)
    S = State(dev, 1024.0)
    S.raise_flag(dev)
    S.snapshot()
    args = lambda: (_P(P_.v), _P(G.v), _P(M.v), _P(V.v), n, A._table(groups, 1), 1.0, _P(S.buf.v), 0, _S(G.v))      # noqa: E731
    _call("rd_adam_step_groups_scaled", *args())
    for b_ in (P_, M, V, G, S.buf):
        b_.check("adam_groups_scaled with found_inf raised", unchanged=True)
    S.poke(FOUND, 0)
    _call("rd_adam_step_groups_scaled", *args())
    S.buf.check("adam_groups_scaled state", unchanged=True)
    got = P_.cpu()
    unscale = float(np.float32(1.0 / 1024.0))
    for k, (a, b) in enumerate(((0, 512), (512, 516), (516, n))):
        r = A._ref64_step(p0[a:b].double(), g[a:b].double(), torch.zeros(b - a, dtype=torch.float64), torch.zeros(b - a, dtype=torch.float64),
                          groups[k], 1, unscale)
        q = torch.nn.Parameter(p0[a:b].clone())
        q.grad = g[a:b] * unscale
        torch.optim.Adam(A._torch_groups([q], [groups[k]]), foreach=False).step()
        _check("adam_groups_scaled with found_inf cleared, group %d" % k, got[a:b], r[0], q.detach(), "adam_groups_scaled p")
    for b_ in (P_, M, V):
        b_.check("adam_groups_scaled found_inf")


def scaled_adam_refusal_case(dev, quick=False):
    """a NULL state and the malformed tables rd_adam_step_groups refuses are refused, and nothing is written"""
    n = 1028
    rs = _rs("adam_groups_scaled refusals")
    bufs = [Buf(dev, n, F32, _randn(rs, n)) for _ in range(4)]
    P_, G, M, V = bufs
    S = State(dev, 1024.0)
    good = A._groups((512, 516, 1028))

    def refused(text, t, state=True, n_=n):
        _refused("rd_adam_step_groups_scaled", text, _P(P_.v), _P(G.v), _P(M.v), _P(V.v), n_, t, 1.0, _P(S.buf.v) if state else None, 0, _S(G.v))
        for b_ in bufs + [S.buf]:
            b_.check("refused adam_groups_scaled (%s)" % text, unchanged=True)

    refused("null pointer", A._table(good, 1), state=False)
    refused("null pointer", None)
    t = A._table(good, 1)
    t.count = 9
    refused("count must be 1..8", t)
    refused("strictly ascending", A._table(A._groups((516, 512, 1028)), 1))
    refused("not a multiple of 4", A._table(A._groups((510, 1028)), 1))
    refused("must equal n", A._table(good, 1), n_=1027)
    refused("must be >= 1", A._table(good, 0))


def scaled_adam_large_case(dev, quick=False):
    """a 2 M-element arena with a group boundary in the second grid-stride sweep (GPU twin only), the host one step ahead"""
    if quick:
        return
    n = 2048 * 256 * 4 + 1203
    _scaled(dev, n, A._groups((2048 * 256 * 4 + 400, n), 1), SCALES[1], late=1, base=2, nsteps=2, tag="second sweep")


# ---------------------------------------------------------------------------------------------------------------- 4. FlatAdam + DynamicLossScale
INF_STEPS = (1, 2, 3, 7)      # three skips before the first applied step, one more later


def _scaler_pair(dev, init_scale, interval=2):
    from riders_amd.optim import DynamicLossScale
    ours = DynamicLossScale(init_scale=init_scale, growth_interval=interval, device=dev)
    refs = {}
    for dt in (torch.float64, F32):
        gs = torch.amp.GradScaler("cpu", init_scale=init_scale, growth_interval=interval)
        gs.scale(torch.zeros(1))      # GradScaler creates its tensors on the first scale()
        refs[dt] = gs
    return ours, refs


def _torch_step(gs, params, topt):
    gs.step(topt)
    gs.update()
    return [int(topt.state[q]["step"]) if topt.state.get(q) else 0 for q in params]


def _flat_run(dev, what, init, split, hyper, cls=None, flat_kwargs=None, reconcile_every_step=True, nsteps=10):
    rs = _rs("flatadam dynamic", what)
    ps, opt, refs = A._trio(dev, init, split, hyper, cls=cls, flat_kwargs=flat_kwargs)
    order = A._order(split) if split is not None else list(range(len(ps)))
    scaler, gss = _scaler_pair(dev, 2.0 ** 12)
    opt.loss_scale = scaler
    before_attach = scaler.stats()
    for step in range(1, nsteps + 1):
        scale = gss[F32].get_scale()
        assert scale == gss[torch.float64].get_scale()
        grads = [_randn(rs, *s) * scale for s in A.SHAPES]      # what a backward seeded with the scale leaves in the arena
        if step in INF_STEPS:
            grads[step % len(grads)].view(-1)[step % 3] = float("inf") if step % 2 else float("nan")
        opt.zero_grad()
        A._set_grads(dev, ps, refs, grads)
        snap = [_bits(t_).clone() for t_ in (opt.flat_param, opt.exp_avg, opt.exp_avg_sq)]
        with A._Count("rd_adam_step_groups_scaled") as cs, A._Count("rd_adam_step_groups") as cg, A._Count("rd_adam_step") as c1, \
                A._Count("rd_adam_step_guarded") as c2, A._Count("rd_loss_scale_update") as cu, A._Count("rd_adam_skip_count") as ck:
            opt.step()
        assert cs.n >= 1 and cu.n == 1 and cg.n == c1.n == c2.n == ck.n == 0, (cs.n, cu.n, cg.n, c1.n, c2.n, ck.n)
        tsteps = {dt: _torch_step(gss[dt], refs[dt][0], refs[dt][1]) for dt in refs}
        if step in INF_STEPS:
            for t_, s_, nm in zip((opt.flat_param, opt.exp_avg, opt.exp_avg_sq), snap, ("p", "exp_avg", "exp_avg_sq")):
                assert torch.equal(_bits(t_), s_), "%s step %d: %s changed in a skipped step" % (what, step, nm)
        st = scaler.stats()
        assert st["scale"] == gss[F32].get_scale() and st["growth_tracker"] == gss[F32]._get_growth_tracker(), (what, step, st, gss[F32].state_dict())
        assert st["skipped"] == sum(1 for s_ in INF_STEPS if s_ <= step) and st["found_inf"] == 0, (what, step, st)
        if reconcile_every_step or step == nsteps:
            sd = opt.state_dict()["state"]
            assert [int(sd[pos]["step"]) for pos in range(len(order))] == [tsteps[F32][i] for i in order] == [tsteps[torch.float64][i] for i in order], \
                (what, step, [int(sd[pos]["step"]) for pos in range(len(order))], tsteps)
        else:      # the host counters run ahead by the skips not reconciled; the kernel subtracts them
            late = st["skipped"] - opt._dyn_reconciled
            assert [opt.steps[pos] - late for pos in range(len(order))] == [tsteps[F32][i] for i in order], (what, step, opt.steps, late, tsteps)
        for pos, i in enumerate(order):
            _check("%s step %d p%d" % (what, step, i), ps[i], refs[torch.float64][0][i].detach(), refs[F32][0][i].detach(), "flatadam dynamic p")
    assert opt.skipped_steps() == len(INF_STEPS) and before_attach["skipped"] == 0
    sd = opt.state_dict()["state"]
    r64, r32 = refs[torch.float64], refs[F32]
    for pos, i in enumerate(order):
        for k in ("exp_avg", "exp_avg_sq"):
            _check("%s %s %d" % (what, k, i), sd[pos][k], r64[1].state[r64[0][i]][k], r32[1].state[r32[0][i]][k], "flatadam dynamic " + k)
        assert int(sd[pos]["step"]) == int(r32[1].state[r32[0][i]]["step"]) == nsteps - len(INF_STEPS)
    return scaler, gss[F32]


def flat_adam_dynamic_case(dev, quick=False):
    """FlatAdam + DynamicLossScale against GradScaler("cpu") + torch.optim.Adam on toy parameters: one group, two groups and FlatAdamW, ten steps at
    growth_interval 2 with an inf or NaN written into one gradient at steps 1, 2, 3 and 7.  After each step the scale, the tracker and every
    parameter's `step` equal torch's and the parameters pass _check; once with the host counters reconciled every step (state_dict()), once left
    running ahead until the end.  The scaler's state_dict() equals GradScaler's and loads into one and back."""
    from riders_amd.optim import DynamicLossScale, FlatAdamW
    E = _E()
    try:
        kw = dict(lr=A.HP[0][0], betas=A.HP[0][1:3], eps=A.HP[0][3])
        for every in (True, False):
            tag = "reconciled every step" if every else "reconciled at the end"
            scaler, gs = _flat_run(dev, "one group, " + tag, A._toy(), None, None, flat_kwargs=dict(kw, weight_decay=A.WDS[1]), reconcile_every_step=every)
            _flat_run(dev, "two groups, " + tag, A._toy(), A.SPLITS[2], A._hyper(2), reconcile_every_step=every)
            _flat_run(dev, "FlatAdamW, " + tag, A._toy(), None, None, cls=FlatAdamW, flat_kwargs=kw, reconcile_every_step=every)
        mine, theirs = scaler.state_dict(), gs.state_dict()
        assert mine == theirs and [type(mine[k]) for k in sorted(mine)] == [type(theirs[k]) for k in sorted(theirs)], (mine, theirs)
        fresh = torch.amp.GradScaler("cpu", init_scale=3.0, growth_factor=4.0, backoff_factor=0.25, growth_interval=7)
        fresh.load_state_dict(mine)
        assert fresh.state_dict() == theirs and fresh.get_scale() == theirs["scale"]
        other = dict(scale=3.0 * 2.0 ** 10, growth_factor=1.5, backoff_factor=0.75, growth_interval=5, _growth_tracker=4)
        fresh.load_state_dict(other)
        back = DynamicLossScale(device=dev)
        back.load_state_dict(fresh.state_dict())
        assert back.state_dict() == other and back.get_scale() == other["scale"] and back.stats()["inv_scale"] == _inv32(other["scale"])
        assert back.skipped_steps() == 0 and scaler.skipped_steps() == len(INF_STEPS)
        scaler.load_state_dict(other)      # the device counters restart; the skips counted so far are carried on the host
        assert scaler.skipped_steps() == len(INF_STEPS) and scaler.stats()["skipped"] == 0
        for bad in (dict(init_scale=0.0), dict(growth_factor=1.0), dict(backoff_factor=1.0), dict(growth_interval=0)):
            try:
                DynamicLossScale(device=dev, **bad)
            except (ValueError, RuntimeError):
                continue
            raise AssertionError("DynamicLossScale accepted %s" % bad)
    finally:
        E.set_param_grad_allocator(None)


# ---------------------------------------------------------------------------------------------------------------- 5. the static path
def static_path_case(dev, quick=False):
    """with a float loss_scale (and with the default 1.0) none of the three new entries is called, and the guarded step counts its skips with
    rd_adam_skip_count as before"""
    from riders_amd.optim import FlatAdam
    E = _E()
    try:
        for split, scale in ((None, 1024.0), (A.SPLITS[2], 1024.0), (None, 1.0), (A.SPLITS[2], 1.0)):
            rs = _rs("static path", split, scale)
            ps = [torch.nn.Parameter(x.clone().to(dev)) for x in A._toy(rs)]
            opt = FlatAdam(ps, lr=2e-3) if split is None else FlatAdam(A._dicts(ps, split, A._hyper(2)))
            opt.loss_scale = scale
            assert opt.loss_scale == scale and isinstance(opt.loss_scale, float)
            for step in (1, 2, 3):
                opt.zero_grad()
                for i, p in enumerate(ps):
                    p.grad = (_randn(rs, *p.shape) * scale).to(dev)
                if step == 2:
                    ps[1].grad.view(-1)[2] = float("inf")
                counts = [A._Count(nm) for nm in NEW_ENTRIES + ("rd_adam_skip_count", "rd_grad_finite_check")]
                for c in counts:
                    c.__enter__()
                try:
                    opt.step()
                finally:
                    for c in reversed(counts):
                        c.__exit__(None, None, None)
                guarded = 1 if scale != 1.0 else 0
                assert [c.n for c in counts] == [0, 0, 0, guarded, guarded], (split, scale, step, [(c.name, c.n) for c in counts])
            assert opt.skipped_steps() == (1 if scale != 1.0 else 0)
            if scale != 1.0:
                assert int(opt.state_dict()["state"][0]["step"]) == 2
    finally:
        E.set_param_grad_allocator(None)


# ---------------------------------------------------------------------------------------------------------------- 6. RC-Net, fp16 (GPU twin)
# The smallest power of two at which the emulated fp16 backward of this model on this batch overflows is 2^RCNET_OVERFLOW_LOG2 (bisected on the
# emulator: finite at 2^8, 2^17, 2^21, 2^23, 2^24, not finite at 2^25, 2^26, 2^44; the GPU agrees at every power from 2^8 to 2^35); the initial
# scale is 16 times that, so the run starts with skipped steps, settles, and probes upward every growth_interval = 2 applied steps.  On the
# emulator the run from 2^29 skips 2^29 ... 2^25 (five steps, the parameters do not move) and then applies four steps in a row at 2^24, 2^24,
# 2^25, 2^25 (the first update shrinks the gradient; run there from 2^26, i.e. without the first three identical skipped steps), which meets `skipped >= 2 and applied >= 3` with room; on the GPU the twelve steps are
# 5 skipped, 6 applied (the scale climbing to 2^27), 1 skipped.
RCNET_OVERFLOW_LOG2 = 25     # (the gradient of a mean over 2 x 3 x 64 x 32 logits is small: nothing overflows fp16 below 2^25)
RCNET_STEPS = 12


def seed_case(dev, quick=False):
    """engine.StepTape.seed given the scaler's tensor uses THAT tensor (same address: a replay reads the value of the moment), the staged backward
    seeded with it leaves the gradients of the static seed of the same value bit for bit, follows the word when it changes, and reads the state only"""
    from riders_amd import engine, rcnet_main
    from riders_amd.optim import DynamicLossScale, FlatAdam
    from tests.test_host_logic import _toy_batch, _toy_loss, _TwoStage
    try:
        torch.manual_seed(3)
        model = _TwoStage().to(dev)
        model.train()
        opt = FlatAdam(list(model.parameters()), lr=1e-3)
        x, label, valid = (t_.to(dev) for t_ in _toy_batch(1))
        fwd = lambda: _toy_loss(model, x, label, valid)      # noqa: E731
        scaler = DynamicLossScale(init_scale=1024.0, growth_interval=2, device=dev)
        st = engine.StepTape()
        loss = st.forward(fwd)
        st.seed(loss, scaler.scale_tensor)
        assert st.tape.grads[id(loss)].data_ptr() == scaler.scale_tensor.data_ptr() == scaler._state.data_ptr()
        before = _bits(scaler._state).clone()
        for value in (1024.0, 256.0):
            scaler.load_state_dict(dict(scaler.state_dict(), scale=value))
            before = _bits(scaler._state).clone()
            rcnet_main.staged_gradients(fwd, opt, None, value)
            static = _bits(opt.flat_grad).clone()
            assert opt.loss_scale == value
            opt.flat_grad.zero_()
            rcnet_main.staged_gradients(fwd, opt, None, scaler)
            assert opt.loss_scale is scaler
            assert torch.equal(_bits(opt.flat_grad), static), "the backward seeded with the scaler's word differs from the static seed %g" % value
            assert torch.equal(_bits(scaler._state), before), "a backward changed the scaler's state"
            opt.flat_grad.zero_()
            loss = fwd()
            opt.zero_grad()
            rcnet_main.scaled_backward(loss, opt, scaler)      # through torch.autograd, as an unchanged training script runs it
            assert torch.equal(_bits(opt.flat_grad), static), "scaled_backward with a scaler differs from the static seed %g" % value
        assert float(opt.flat_grad.abs().max()) > 0
    finally:
        engine.set_param_grad_allocator(None)


def _state_bytes(scaler):
    return _bits(scaler._state).cpu().clone()


def rcnet_fp16_case(dev):
    """RC-Net in fp16 at the g6 fixture's geometry (2 images of 64 x 96, K = 3), growth_interval 2, from an initial scale 16 x the smallest
    overflowing power of two, so the run begins with skipped steps, settles, and probes upward again.  Eager: after each backward the arena
    gradient is copied to the CPU and drives GradScaler("cpu") + torch.optim.Adam twins in float64 and fp32; the scale, the tracker and every
    step count equal torch's after each step, the parameters pass _check and stay finite, and at least 2 steps are skipped and 3 applied.  The
    same steps on a fresh model through GraphedTrainStep(loss_scale=scaler): constructing the step leaves the 32 state bytes unchanged, and
    flat_param and the state bytes end bit-identical to the eager run."""
    from riders_amd import engine, rcnet_main
    from riders_amd.optim import DynamicLossScale, FlatAdam
    from tests.parity_cases_frozen import _g6_model
    lr, betas, eps = float(np.float32(1e-3)), A.HP[0][1:3], A.HP[0][3]
    init = 2.0 ** (RCNET_OVERFLOW_LOG2 + 4)

    def build():
        model, cfg = _g6_model(dev)
        model.train()
        return model, cfg, FlatAdam(model.parameters(), lr=lr, betas=betas, eps=eps)

    engine.set_deterministic_roi_pool(True)
    engine.set_compute_dtype("fp16")
    engine.clear_caches()
    try:
        model, cfg, opt = build()
        batch = rcnet_main.synthetic_batch(2, 64, 96, cfg, seed=77, device=dev)
        scaler, gss = _scaler_pair(dev, init)
        twins = {}
        for dt in (torch.float64, F32):
            tp = [torch.nn.Parameter(p.detach().cpu().to(dt).clone()) for p in opt.params]
            twins[dt] = (tp, torch.optim.Adam(tp, lr=lr, betas=betas, eps=eps, foreach=False))
        applied = 0
        for step in range(1, RCNET_STEPS + 1):
            loss = rcnet_main.compute_gradients(model, opt, batch, cfg, loss_scale=scaler)
            grads, touched = opt.flat_grad.detach().cpu(), set(opt.touched_indices())
            finite = bool(torch.isfinite(grads).all())
            opt.step()
            for dt, (tp, topt) in twins.items():
                for i, (q, o) in enumerate(zip(tp, opt.offsets)):
                    q.grad = grads[o:o + q.numel()].view(q.shape).to(dt).clone() if i in touched else None
                tsteps = _torch_step(gss[dt], tp, topt)
            applied += finite
            st = scaler.stats()
            print("rcnet fp16 step %2d: loss %.5f  gradient finite %s  scale 2^%g  tracker %d  skipped %d" % (
                step, float(loss.detach()), finite, np.log2(st["scale"]), st["growth_tracker"], st["skipped"]))
            assert st["scale"] == gss[F32].get_scale() == gss[torch.float64].get_scale(), (step, st, gss[F32].state_dict())
            assert st["growth_tracker"] == gss[F32]._get_growth_tracker() and st["skipped"] == step - applied, (step, st)
            sd = opt.state_dict()["state"]
            assert [int(sd[i]["step"]) if i in sd else 0 for i in range(len(opt.params))] == [s_ if i in touched else 0 for i, s_ in enumerate(tsteps)], step
            cat = lambda xs: torch.cat([x.detach().reshape(-1).cpu() for x in xs])      # noqa: E731
            _check("rcnet fp16 dynamic scale, step %d" % step, cat(opt.params), cat(twins[torch.float64][0]), cat(twins[F32][0]), "rcnet fp16 dynamic p")
        skipped = opt.skipped_steps()
        assert skipped >= 2 and applied >= 3 and skipped + applied == RCNET_STEPS, (skipped, applied)
        assert bool(torch.isfinite(opt.flat_param).all())
        eager, eager_state = opt.flat_param.clone(), _state_bytes(scaler)
        engine.set_param_grad_allocator(None)
        engine.clear_caches()
        model, cfg, opt = build()
        scaler2, _ = _scaler_pair(dev, init)
        fresh = _state_bytes(scaler2)
        step_fn = rcnet_main.GraphedTrainStep(model, opt, batch, cfg, warmup=1, loss_scale=scaler2)
        assert torch.equal(_state_bytes(scaler2), fresh), "constructing a GraphedTrainStep changed the scaler's state"
        for _ in range(RCNET_STEPS):
            step_fn()
        assert torch.equal(_state_bytes(scaler2), eager_state), (scaler2.stats(), scaler.stats())
        assert opt.step_count == RCNET_STEPS      # nothing synchronised so far: the host counters still include the skipped steps
        assert opt.skipped_steps() == skipped and opt.reconcile_skipped() == skipped and opt.step_count == applied
        assert torch.equal(_bits(opt.flat_param), _bits(eager)), "graphed fp16 steps under the dynamic scale differ from the eager run in %d elements" % int(
            (opt.flat_param != eager).sum())
    finally:
        engine.set_compute_dtype("fp32")
        engine.set_deterministic_roi_pool(False)
        engine.set_param_grad_allocator(None)
        engine.clear_caches()


# ---------------------------------------------------------------------------------------------------------------- 7. SML, fp16 (GPU twin)
def sml_fp16_case(dev):
    """Scale Map Learner in fp16 at 2 frames of 64 x 96: three steps with a scaler at 2^16, eager train_step against GraphedTrainStep: parameters
    and the 32 state bytes bit-identical"""
    from riders_amd import engine, sml_main
    from riders_amd.optim import DynamicLossScale, FlatAdam
    cfg = sml_main.ZJU_SML_CONFIG
    engine.set_compute_dtype("fp16")
    engine.clear_caches()
    try:
        batch = sml_main.synthetic_batch(2, 64, 96, seed=33, device=dev)
        runs = []
        for graphed in (False, True):
            torch.manual_seed(0)
            m = sml_main.build_model(dev, cfg)
            m.train()
            opt = FlatAdam(m.parameters(), lr=cfg['learning_rate'])
            scaler = DynamicLossScale(init_scale=2.0 ** 16, growth_interval=2, device=dev)
            outlier = sml_main.make_outlier_removal(cfg)
            if graphed:
                fresh = _state_bytes(scaler)
                step = sml_main.GraphedTrainStep(m, opt, batch, cfg, outlier=outlier, warmup=1, loss_scale=scaler)
                assert torch.equal(_state_bytes(scaler), fresh), "constructing a GraphedTrainStep changed the scaler's state"
                for _ in range(3):
                    step()
                del step
            else:
                for _ in range(3):
                    sml_main.train_step(m, opt, batch, cfg, outlier=outlier, loss_scale=scaler)
            print("sml fp16 %s: %s" % ("graphed" if graphed else "eager", scaler.stats()))
            runs.append((_bits(opt.flat_param).clone(), _state_bytes(scaler), opt.skipped_steps()))
            assert bool(torch.isfinite(opt.flat_param).all())
            engine.set_param_grad_allocator(None)
            engine.clear_caches()
        assert torch.equal(runs[0][1], runs[1][1]), "scaler state of the graphed SML steps differs from the eager ones"
        assert torch.equal(runs[0][0], runs[1][0]), "graphed SML fp16 steps under the dynamic scale differ from the eager ones"
        assert runs[0][2] == runs[1][2]
    finally:
        engine.set_compute_dtype("fp32")
        engine.set_param_grad_allocator(None)
        engine.clear_caches()
