"""Parameter groups of the fused Adam: rd_adam_step_groups through the C ABI, FlatAdam built from torch's list of group dictionaries, the
optimizer-state exchange with torch.optim.Adam for several groups, the gradient bucketing, and one RC-Net fine-tuning step pair (see
tests/parity_cases.py for how case functions are used by the emulator and GPU twins).

Every comparison is tests.parity_cases_glue._check: the error against a float64 restatement may be at most 4 x the error of torch's own fp32
CPU result (torch.optim.Adam(..., foreach=False) with the same groups), with its floor of 4 fp32 ulp of max|ref|.  No compared range has fewer
than 3 elements: with a single element the floor is 4 ulp of that one value and three roundings of exp_avg can exceed it, so a smaller
parameter is compared concatenated with its neighbours.  Buffers handed to the C ABI carry sentinels on both sides.
"""
import numpy as np
import torch

from tests.parity_cases_glue import F32, Buf, _bits, _call, _check, _P, _randn, _refused, _rs, _S

# (lr, beta1, beta2, eps) as the fp32 values the C ABI receives
HP = [tuple(float(np.float32(v)) for v in hp) for hp in ((2e-3, .9, .999, 1e-8), (1e-4, .9, .999, 1e-8), (5e-2, .5, .9, 1e-3), (0.0, .9, .999, 1e-8))]
WDS = [float(np.float32(v)) for v in (0.0, 1e-2, 0.1)]


def _E():
    from riders_amd import engine
    return engine


def _lib():
    from riders_amd import _lib
    return _lib


class Group(object):
    def __init__(self, end, hp, wd, decoupled, step0=0, inactive=False):
        self.end, self.hp, self.wd, self.decoupled, self.step0, self.inactive = end, hp, wd, decoupled, step0, inactive


def _groups(ends, shift=0, step0s=None, inactive=()):
    """one different hyperparameter set, decay and decay kind per group"""
    return [Group(e, HP[(k + shift) % len(HP)], WDS[(k + shift + 1) % len(WDS)], (k + shift) % 2 == 1, 0 if step0s is None else step0s[k], k in inactive)
            for k, e in enumerate(ends)]


def _table(groups, step):
    L = _lib()
    t = L.AdamGroups()
    t.count = len(groups)
    for k, g in enumerate(groups):
        t.end[k] = g.end
        t.flags[k] = (L.ADAM_DECOUPLED if g.decoupled else 0) | (L.ADAM_INACTIVE if g.inactive else 0)
        t.step[k] = g.step0 + step
        t.lr[k], t.beta1[k], t.beta2[k], t.eps[k] = g.hp
        t.weight_decay[k] = g.wd
    return t


def _ref64_step(p, g, m, v, grp, step, gscale):
    """torch's single-tensor Adam in float64 with the gradient scale the kernel folds in; decoupled decay scales p first"""
    lr, b1, b2, eps = grp.hp
    g = g * gscale
    if grp.decoupled:
        p = p * (1.0 - lr * grp.wd)
    else:
        g = g + grp.wd * p
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    return p - (lr / bc1) * m / (v.sqrt() / (bc2 ** 0.5) + eps), m, v


def _grads(rs, family, n):
    if family == "normal":
        return _randn(rs, n)
    if family == "zero":
        return torch.zeros(n)
    return 1e-20 * _randn(rs, n)


def _torch_groups(params, groups):
    return [dict(params=[q], lr=g.hp[0], betas=(g.hp[1], g.hp[2]), eps=g.hp[3], weight_decay=g.wd, decoupled_weight_decay=g.decoupled)
            for q, g in zip(params, groups)]


def _direct(dev, n, groups, gscale=1.0, family="normal", nsteps=3, tag=""):
    """nsteps launches of rd_adam_step_groups on sentinel-guarded buffers against the float64 restatement and torch's fp32 Adam, group by group"""
    gscale = float(np.float32(gscale))
    rs = _rs("adam_groups", n, tuple(g.end for g in groups), gscale, family, tag)
    p0 = _randn(rs, n)
    P_, M, V = Buf(dev, n, F32, p0), Buf(dev, n, F32, torch.zeros(n)), Buf(dev, n, F32, torch.zeros(n))
    spans = list(zip([0] + [g.end for g in groups[:-1]], [g.end for g in groups]))
    r64 = [(p0[a:b].double(), torch.zeros(b - a, dtype=torch.float64), torch.zeros(b - a, dtype=torch.float64)) for a, b in spans]
    q32 = [torch.nn.Parameter(p0[a:b].clone()) for a, b in spans]
    opt32 = torch.optim.Adam(_torch_groups(q32, groups), foreach=False)
    for q, g in zip(q32, groups):
        if g.step0 > 0:
            opt32.state[q] = dict(step=torch.tensor(float(g.step0)), exp_avg=torch.zeros_like(q), exp_avg_sq=torch.zeros_like(q))
    what = "adam_groups n=%d ends=%s gscale=%g %s %s" % (n, [g.end for g in groups], gscale, family, tag)
    for step in range(1, nsteps + 1):
        g = _grads(rs, family, n)
        G = Buf(dev, n, F32, g)
        _call("rd_adam_step_groups", _P(P_.v), _P(G.v), _P(M.v), _P(V.v), n, _table(groups, step), gscale, None, _S(G.v))
        for k, ((a, b), grp) in enumerate(zip(spans, groups)):
            q32[k].grad = None if grp.inactive else g[a:b] * gscale
            if not grp.inactive:
                r64[k] = _ref64_step(r64[k][0], g[a:b].double(), r64[k][1], r64[k][2], grp, grp.step0 + step, gscale)
        opt32.step()
        G.check(what, unchanged=True)
    got = [b_.cpu() for b_ in (P_, M, V)]
    for k, ((a, b), grp) in enumerate(zip(spans, groups)):
        if grp.inactive:
            for b_, nm in zip((P_, M, V), ("p", "exp_avg", "exp_avg_sq")):
                assert torch.equal(_bits(b_.v[a:b]).cpu(), _bits(b_.snap[b_.lo + a:b_.lo + b]).cpu()), "%s: %s of inactive group %d changed" % (what, nm, k)
            continue
        s32 = opt32.state[q32[k]]
        for x, r, r32, nm in zip(got, r64[k], (q32[k].detach(), s32["exp_avg"], s32["exp_avg_sq"]), ("p", "exp_avg", "exp_avg_sq")):
            _check("%s group %d %s" % (what, k, nm), x[a:b], r, r32, "adam_groups " + nm)
    for b_ in (P_, M, V):
        b_.check(what)


def kernel_multi_case(dev, quick=False):
    """(a) two and three groups on arenas of 8, 12, 1028 and 2052 elements: boundaries inside a 1024-element chunk (at 4, and at 512 / 516) and
    exactly on a chunk edge and one vector later (1024 / 1028); (b) a last group that ends in a scalar tail; (e) a different step count per
    group (1 and 7); both gradient scales and the zero / tiny gradient families once each."""
    for n, ends in ((8, (4, 8)), (12, (4, 8, 12)), (1028, (4, 1028)), (1028, (512, 516, 1028)), (2052, (1024, 2052)), (2052, (1024, 1028, 2052)),
                    (1023, (512, 1023)), (1025, (1024, 1025))):
        for shift in (0, 1, 2, 3):
            _direct(dev, n, _groups(ends, shift))
    _direct(dev, 1028, _groups((512, 516, 1028), 1), gscale=1.0 / 1024)
    _direct(dev, 1023, _groups((512, 1023), 2), gscale=1.0 / 1024, family="tiny")
    _direct(dev, 2052, _groups((1024, 1028, 2052), 0), family="zero")
    _direct(dev, 1028, _groups((512, 1028), 0, step0s=(0, 6)), tag="steps 1 and 7")
    _direct(dev, 1028, _groups((512, 1028), 1, step0s=(6, 0)), tag="steps 7 and 1")


def kernel_eight_case(dev, quick=False):
    """(c) eight groups of 4 ... 132 elements"""
    sizes = (4, 132, 8, 64, 12, 100, 36, 20)
    ends = tuple(int(e) for e in np.cumsum(sizes))
    for shift in (0, 1):
        _direct(dev, ends[-1], _groups(ends, shift))
    _direct(dev, ends[-1] + 3, _groups(ends[:-1] + (ends[-1] + 3,), 2), tag="scalar tail")


def kernel_refusal_case(dev, quick=False):
    """(c) nine groups and every malformed table are refused with a message and write nothing"""
    n = 1028
    rs = _rs("adam_groups refusals")
    bufs = [Buf(dev, n, F32, _randn(rs, n)) for _ in range(4)]
    P_, G, M, V = bufs

    def refused(text, t, p=True, n_=n):
        _refused("rd_adam_step_groups", text, _P(P_.v) if p else None, _P(G.v), _P(M.v), _P(V.v), n_, t, 1.0, None, _S(G.v))
        for b_ in bufs:
            b_.check("refused adam_groups (%s)" % text, unchanged=True)

    good = _groups((512, 516, 1028))
    refused("null pointer", _table(good, 1), p=False)
    _refused("rd_adam_step_groups", "null pointer", _P(P_.v), _P(G.v), _P(M.v), _P(V.v), n, None, 1.0, None, _S(G.v))
    for count in (9, 0, -1):
        t = _table(good, 1)
        t.count = count
        refused("count must be 1..8", t)
    refused("strictly ascending", _table(_groups((516, 512, 1028)), 1))
    refused("strictly ascending", _table(_groups((512, 512, 1028)), 1))
    refused("strictly ascending", _table(_groups((0, 1028)), 1))
    refused("not a multiple of 4", _table(_groups((510, 1028)), 1))
    refused("must equal n", _table(_groups((512, 1024)), 1))
    refused("must equal n", _table(good, 1), n_=1027)
    refused("must be >= 1", _table(good, 0))
    t = _table(_groups((512, 516, 1028), inactive=(1,)), 1)
    t.step[1] = 0      # an inactive group's step is not looked at ...
    t.step[2] = 0      # ... an active one's is
    refused("step[2] must be >= 1", t)


def kernel_inactive_case(dev, quick=False):
    """(d) an inactive middle group (and an inactive first / last one): its param / exp_avg / exp_avg_sq ranges and every sentinel are bit-identical,
    its neighbours match the reference; the inactive group carries constants that would show (lr 5e-2, step 0)"""
    for n, ends, off in ((1028, (512, 516, 1028), (1,)), (2052, (1024, 1028, 2052), (1,)), (2052 + 1024, (4, 2052, 2052 + 1024), (1,)),
                         (1028, (512, 516, 1028), (0,)), (1031, (512, 516, 1031), (2,)), (1028, (512, 516, 1028), (0, 2))):
        gs = _groups(ends, 1, inactive=off)
        for k in off:
            gs[k].hp, gs[k].wd, gs[k].step0 = HP[2], WDS[2], -1
        _direct(dev, n, gs, tag="inactive %s" % (off,))


def kernel_skip_flag_case(dev, quick=False):
    """(f) skip_flag raised: nothing is written; cleared: the step applies"""
    n, groups = 1031, _groups((512, 516, 1031), 0)
    rs = _rs("adam_groups skip")
    p0, g = _randn(rs, n), _randn(rs, n)
    P_, M, V, G = Buf(dev, n, F32, p0), Buf(dev, n, F32, torch.zeros(n)), Buf(dev, n, F32, torch.zeros(n)), Buf(dev, n, F32, g)
    FL = Buf(dev, 2, torch.int32, torch.tensor([1, 0]))
    args = lambda: (_P(P_.v), _P(G.v), _P(M.v), _P(V.v), n, _table(groups, 1), 1.0, _P(FL.v), _S(G.v))      # noqa: E731
    _call("rd_adam_step_groups", *args())
    for b_ in (P_, M, V, G, FL):
        b_.check("adam_groups with the skip flag raised", unchanged=True)
    FL.v.zero_()
    FL.snap = FL.full.clone()
    _call("rd_adam_step_groups", *args())
    FL.check("adam_groups skip flag", unchanged=True)
    got = P_.cpu()
    for k, (a, b) in enumerate(((0, 512), (512, 516), (516, n))):
        r = _ref64_step(p0[a:b].double(), g[a:b].double(), torch.zeros(b - a, dtype=torch.float64), torch.zeros(b - a, dtype=torch.float64),
                        groups[k], 1, 1.0)
        q = torch.nn.Parameter(p0[a:b].clone())
        q.grad = g[a:b].clone()
        torch.optim.Adam(_torch_groups([q], [groups[k]]), foreach=False).step()
        _check("adam_groups with the skip flag cleared, group %d" % k, got[a:b], r[0], q.detach(), "adam_groups p")
    for b_ in (P_, M, V):
        b_.check("adam_groups skip flag")


def kernel_ties_to_adam_step_case(dev, quick=False):
    """(g) one group with the constants of an rd_adam_step call on a copy of the buffers: bit-identical parameters and moments"""
    for n in (3, 4, 7, 1023, 1025, 4099):
        for hp, wd, gscale in ((HP[0], WDS[1], 0.5), (HP[2], WDS[0], 1.0), (HP[3], WDS[2], 1.0 / 1024)):
            rs = _rs("adam_groups tie", n, hp, wd)
            p0 = _randn(rs, n)
            A = [Buf(dev, n, F32, x) for x in (p0, torch.zeros(n), torch.zeros(n))]
            B = [Buf(dev, n, F32, x) for x in (p0, torch.zeros(n), torch.zeros(n))]
            grp = [Group(n, hp, wd, False)]
            for step in (1, 2, 3):
                G = Buf(dev, n, F32, _randn(rs, n))
                _call("rd_adam_step", _P(A[0].v), _P(G.v), _P(A[1].v), _P(A[2].v), n, hp[0], hp[1], hp[2], hp[3], wd, step, gscale, _S(G.v))
                _call("rd_adam_step_groups", _P(B[0].v), _P(G.v), _P(B[1].v), _P(B[2].v), n, _table(grp, step), gscale, None, _S(G.v))
            for a, b, nm in zip(A, B, ("p", "exp_avg", "exp_avg_sq")):
                assert torch.equal(_bits(a.full).cpu(), _bits(b.full).cpu()), "rd_adam_step_groups (one group) differs from rd_adam_step in %s, n=%d" % (nm, n)
            assert not torch.equal(_bits(A[1].v).cpu(), _bits(A[1].snap[A[1].lo:A[1].hi]).cpu()), "rd_adam_step wrote nothing"


def kernel_large_case(dev, quick=False):
    """(h) a second grid-stride sweep with a group boundary in it (GPU twin and the emulator's full mode only)"""
    if quick:
        return
    n = 2048 * 256 * 4 + 1203
    _direct(dev, n, _groups((2048 * 256 * 4 + 400, n), 1), tag="second sweep")
    _direct(dev, n, _groups((1024, 2048 * 256 * 4 + 400, n), 0, inactive=(1,)), nsteps=1, tag="second sweep, inactive middle")


# ---------------------------------------------------------------------------------------------------------------- 2. FlatAdam with groups
SHAPES = ((7, 5), (33,), (4, 3, 3, 3), (3,), (130,))
SPLITS = {2: ((0, 1), (2, 3, 4)), 3: ((0, 1), (2, 3), (4,))}


def _toy(rs=None):
    rs = rs or _rs("flatadam groups")
    return [_randn(rs, *s) for s in SHAPES]


def _hyper(ngroups):
    """group dictionaries without 'params': a different set per group, the second group with decoupled decay"""
    out = []
    for k in range(ngroups):
        lr, b1, b2, eps = HP[k % 3]
        out.append(dict(lr=lr, betas=(b1, b2), eps=eps, weight_decay=WDS[(k + 1) % 3], decoupled_weight_decay=k == 1))
    return out


def _dicts(params, split, hyper):
    return [dict(h, params=[params[i] for i in idx]) for idx, h in zip(split, hyper)]


class _Count(object):
    """counts the calls of one entry point by wrapping the library attribute"""

    def __init__(self, name):
        self.name, self.n = name, 0

    def __enter__(self):
        lib = _E().L()
        self.lib, self.fn = lib, getattr(lib, self.name)

        def wrapped(*a):
            self.n += 1
            return self.fn(*a)
        setattr(lib, self.name, wrapped)
        return self

    def __exit__(self, *exc):
        setattr(self.lib, self.name, self.fn)


def _order(split):
    return [i for idx in split for i in idx]


def _trio(dev, init, split, hyper, cls=None, flat_kwargs=None):
    """(FlatAdam on dev, {dtype: (params, torch optimizer)}) on the same groups.  split None: the flat form with flat_kwargs."""
    from riders_amd.optim import FlatAdam
    ps = [torch.nn.Parameter(x.clone().to(dev)) for x in init]
    refs = {}
    if split is None:
        opt = (cls or FlatAdam)(ps, **flat_kwargs)
    else:
        opt = FlatAdam(_dicts(ps, split, hyper))
    for dt in (torch.float64, F32):
        rp = [torch.nn.Parameter(x.clone().to(dt)) for x in init]
        if split is None:
            refs[dt] = (rp, (torch.optim.AdamW if cls is not None else torch.optim.Adam)(rp, foreach=False, **flat_kwargs))
        else:
            refs[dt] = (rp, torch.optim.Adam(_dicts(rp, split, hyper), foreach=False))
    return ps, opt, refs


def _set_grads(dev, ps, refs, grads):
    for i, p in enumerate(ps):
        g = grads[i]
        p.grad = None if g is None else g.to(dev)
        for dt in refs:
            refs[dt][0][i].grad = None if g is None else g.to(dt)


def _compare(what, opt, ps, refs, order):
    """parameters, moments and step counts of every parameter (FlatAdam's index pos = torch's) under _check"""
    r64, r32 = refs[torch.float64], refs[F32]
    sd = opt.state_dict()["state"]
    for pos, i in enumerate(order):
        _check("%s p%d" % (what, i), ps[i], r64[0][i].detach(), r32[0][i].detach(), "flatadam groups p")
        st64 = r64[1].state.get(r64[0][i])
        assert (pos in sd) == bool(st64), "%s: parameter %d has optimizer state here %s, in torch %s" % (what, i, pos in sd, bool(st64))
        if not st64:
            continue
        for k in ("exp_avg", "exp_avg_sq"):
            _check("%s %s %d" % (what, k, i), sd[pos][k], st64[k], r32[1].state[r32[0][i]][k], "flatadam groups " + k)
        assert int(sd[pos]["step"]) == int(st64["step"]), (what, i, int(sd[pos]["step"]), int(st64["step"]))


def flat_adam_groups_case(dev, quick=False):
    """Toy parameters split into 2 and 3 groups against torch.optim.Adam built from the same list of dictionaries, in float64 and fp32: three
    steps, every group's lr changed after step 1 (the reference's schedule idiom), parameter 3 -- in the group with decoupled decay -- without a
    gradient on step 2 (slot bit-unchanged, step counts as torch's); the uniform first step is ONE rd_adam_step_groups launch."""
    E = _E()
    try:
        for ng, split in sorted(SPLITS.items()):
            rs = _rs("flatadam groups", ng)
            ps, opt, refs = _trio(dev, _toy(rs), split, _hyper(ng))
            order = _order(split)
            assert [id(p) for p in opt.params] == [id(ps[i]) for i in order] and len(opt.param_groups) == ng
            hole = order.index(3)
            assert opt.param_groups[1]['decoupled_weight_decay'] and any(q is ps[3] for q in opt.param_groups[1]['params'])
            o3 = opt.offsets[hole]
            for step in (1, 2, 3):
                opt.zero_grad()
                before = [t_[o3:o3 + 4].clone() for t_ in (opt.flat_param, opt.exp_avg, opt.exp_avg_sq)]
                _set_grads(dev, ps, refs, [None if (step == 2 and i == 3) else _randn(rs, *s) for i, s in enumerate(SHAPES)])
                with _Count("rd_adam_step_groups") as cg, _Count("rd_adam_step") as c1:
                    opt.step()
                assert c1.n == 0 and cg.n >= 1, (c1.n, cg.n)
                if step == 1:
                    assert cg.n == 1, "a uniform step over %d groups took %d launches" % (ng, cg.n)
                for dt in refs:
                    refs[dt][1].step()
                if step == 2:
                    for a, b, nm in zip((opt.flat_param, opt.exp_avg, opt.exp_avg_sq), before, ("p", "exp_avg", "exp_avg_sq")):
                        assert torch.equal(_bits(a[o3:o3 + 4]).cpu(), _bits(b).cpu()), "FlatAdam groups: %s of the slot without a gradient changed" % nm
                    assert [opt.steps[order.index(i)] for i in range(5)] == [2, 2, 2, 1, 2], opt.steps
                if step == 1:      # the schedule idiom, per group
                    for k in range(ng):
                        for o in [opt] + [refs[dt][1] for dt in refs]:
                            o.param_groups[k]['lr'] = o.param_groups[k]['lr'] * (0.5 + 0.25 * k)
            assert [opt.steps[order.index(i)] for i in range(5)] == [3, 3, 3, 2, 3], opt.steps
            _compare("FlatAdam %d groups" % ng, opt, ps, refs, order)
    finally:
        E.set_param_grad_allocator(None)


def flat_adam_idle_group_case(dev, quick=False):
    """A whole group without gradients (the middle one, with a decay that would show) stays bit-untouched and has no optimizer state, in one
    launch per step; its neighbours follow torch."""
    E = _E()
    try:
        split = SPLITS[3]
        hyper = _hyper(3)
        hyper[0]['weight_decay'] = hyper[2]['weight_decay'] = 0.0
        rs = _rs("flatadam idle group")
        ps, opt, refs = _trio(dev, _toy(rs), split, hyper)
        a, b = opt.offsets[2], opt.offsets[4]
        before = [t_[a:b].clone() for t_ in (opt.flat_param, opt.exp_avg, opt.exp_avg_sq)]
        for step in (1, 2, 3):
            opt.zero_grad()
            _set_grads(dev, ps, refs, [None if i in split[1] else _randn(rs, *s) for i, s in enumerate(SHAPES)])
            with _Count("rd_adam_step_groups") as cg:
                opt.step()
            assert cg.n == 1, cg.n
            for dt in refs:
                refs[dt][1].step()
        for x, y, nm in zip((opt.flat_param, opt.exp_avg, opt.exp_avg_sq), before, ("p", "exp_avg", "exp_avg_sq")):
            assert torch.equal(_bits(x[a:b]).cpu(), _bits(y).cpu()), "FlatAdam: %s of a group without gradients changed" % nm
        assert opt.steps == [3, 3, 0, 0, 3], opt.steps
        _compare("FlatAdam idle group", opt, ps, refs, _order(split))
    finally:
        E.set_param_grad_allocator(None)


def flat_adamw_case(dev, quick=False):
    """FlatAdamW (flat parameter list, AdamW's default decay 1e-2, then 0.1) against torch.optim.AdamW: one launch per step"""
    from riders_amd.optim import FlatAdamW
    E = _E()
    try:
        # (betas as the fp32 values the C ABI receives: the kernel forms 1 - beta in fp32, torch in double from the Python float)
        for kw in (dict(lr=HP[0][0], betas=HP[0][1:3], eps=HP[0][3]), dict(lr=HP[2][0], betas=HP[2][1:3], eps=HP[2][3], weight_decay=WDS[2])):
            rs = _rs("flatadamw", kw["lr"])
            ps, opt, refs = _trio(dev, _toy(rs), None, None, cls=FlatAdamW, flat_kwargs=kw)
            assert opt.param_groups[0]['decoupled_weight_decay'] and opt.param_groups[0]['weight_decay'] == kw.get("weight_decay", 1e-2)
            for step in (1, 2, 3):
                opt.zero_grad()
                _set_grads(dev, ps, refs, [_randn(rs, *s) for s in SHAPES])
                with _Count("rd_adam_step_groups") as cg:
                    opt.step()
                assert cg.n == 1, cg.n
                for dt in refs:
                    refs[dt][1].step()
            _compare("FlatAdamW lr=%g" % kw["lr"], opt, ps, refs, list(range(5)))
    finally:
        E.set_param_grad_allocator(None)


def reference_literal_case(dev, quick=False):
    """The reference's constructor argument, `[{'params': parameters, 'weight_decay': w}]` with lr as a keyword (RCNet/rcnet_main.py:233-238),
    constructs and steps like the flat form bit for bit, through the same rd_adam_step launches."""
    from riders_amd.optim import FlatAdam
    E = _E()
    try:
        for w in (0.0, 1e-2):
            res = []
            for literal in (False, True):
                rs = _rs("literal", w)
                ps = [torch.nn.Parameter(x.clone().to(dev)) for x in _toy(rs)]
                opt = FlatAdam([{'params': ps, 'weight_decay': w}], lr=2e-3) if literal else FlatAdam(ps, lr=2e-3, weight_decay=w)
                with _Count("rd_adam_step_groups") as cg, _Count("rd_adam_step") as c1:
                    for step in (1, 2, 3):
                        opt.zero_grad()
                        for i, p in enumerate(ps):
                            p.grad = None if (step == 2 and i == 1) else _randn(rs, *p.shape).to(dev)
                        opt.step()
                assert cg.n == 0 and c1.n >= 3
                res.append(([_bits(t_).cpu().clone() for t_ in (opt.flat_param, opt.exp_avg, opt.exp_avg_sq)], opt.steps, c1.n, opt.state_dict()["param_groups"]))
            assert all(torch.equal(a, b) for a, b in zip(res[0][0], res[1][0])), "the reference's literal form differs from the flat form (weight_decay %g)" % w
            assert res[0][1:] == res[1][1:]
    finally:
        E.set_param_grad_allocator(None)


def constructor_refusals_case(dev, quick=False):
    from riders_amd.optim import FlatAdam
    E = _E()

    def raises(exc, text, fn):
        try:
            fn()
        except exc as e:
            assert text in str(e), (text, str(e))
            return
        raise AssertionError("expected %s(%r)" % (exc.__name__, text))

    try:
        mk = lambda: [torch.nn.Parameter(x.clone().to(dev)) for x in _toy()]      # noqa: E731
        ps = mk()
        raises(ValueError, "optimizer got an empty parameter list", lambda: FlatAdam([]))
        raises(ValueError, "optimizer got an empty parameter list", lambda: FlatAdam([dict(params=ps[:2]), dict(params=[])]))
        raises(ValueError, "some parameters appear in more than one parameter group", lambda: FlatAdam([dict(params=ps[:3]), dict(params=ps[2:])]))
        nine = [torch.nn.Parameter(torch.zeros(4, device=dev)) for _ in range(9)]
        raises(ValueError, "at most 8 parameter groups", lambda: FlatAdam([dict(params=[p]) for p in nine]))
        raises(ValueError, "fp32 parameters on one device", lambda: FlatAdam([dict(params=ps[:2]), dict(params=[torch.nn.Parameter(torch.zeros(4, dtype=torch.float64, device=dev))])]))
        raises(ValueError, "amsgrad / maximize", lambda: FlatAdam([dict(params=mk(), amsgrad=True)]))
        for p, x in zip(ps, _toy()):      # a refused construction has not touched the parameters
            assert torch.equal(p.detach().cpu(), x)
        opt = FlatAdam([dict(params=[p]) for p in nine[:8]], lr=1e-3)
        assert len(opt.param_groups) == 8
        raises(NotImplementedError, "sized at construction", lambda: opt.add_param_group(dict(params=[nine[8]])))
        g = FlatAdam([dict(params=mk(), lr=0.5, foo=3)], lr=1e-3, betas=(0.8, 0.9), decoupled_weight_decay=True).param_groups[0]
        assert (g['lr'], g['betas'], g['eps'], g['weight_decay'], g['decoupled_weight_decay'], g['foo']) == (0.5, (0.8, 0.9), 1e-8, 0.0, True, 3)
    finally:
        E.set_param_grad_allocator(None)


# ---------------------------------------------------------------------------------------------------------------- 3. state exchange
def state_exchange_case(dev, quick=False):
    """FlatAdam (2 groups) -> state_dict() -> a fresh torch.optim.Adam with matching groups, and the reverse; both continue for one more step and
    agree with the float64 run under _check.  Group count or group size mismatch raises ValueError; a single-group state round-trips."""
    from riders_amd.optim import FlatAdam
    E = _E()
    try:
        split, hyper = SPLITS[2], _hyper(2)
        order = _order(split)
        rs = _rs("flatadam exchange")
        ps, fa, refs = _trio(dev, _toy(rs), split, hyper)
        for step in (1, 2):
            fa.zero_grad()
            _set_grads(dev, ps, refs, [None if (step == 2 and i == 1) else _randn(rs, *s) for i, s in enumerate(SHAPES)])
            fa.step()
            for dt in refs:
                refs[dt][1].step()
            for o in [fa] + [refs[dt][1] for dt in refs]:
                o.param_groups[1]['lr'] = 3e-3
        sd = fa.state_dict()
        assert [g['params'] for g in sd['param_groups']] == [[0, 1], [2, 3, 4]] and sorted(sd['state']) == [0, 1, 2, 3, 4]
        t32 = refs[F32][1]
        tsd = t32.state_dict()
        for mine, theirs in zip(sd['param_groups'], tsd['param_groups']):
            assert set(mine) == set(theirs), (sorted(mine), sorted(theirs))
            for k in ('lr', 'eps', 'weight_decay', 'decoupled_weight_decay'):
                assert mine[k] == theirs[k], (k, mine[k], theirs[k])
            assert tuple(mine['betas']) == tuple(theirs['betas'])
        # ours -> torch: a fresh torch optimizer (other hyperparameters) on FlatAdam's parameter values
        tp = [torch.nn.Parameter(p.detach().cpu().clone()) for p in ps]
        tb = torch.optim.Adam([dict(params=[tp[i] for i in idx]) for idx in split], lr=1.0, foreach=False)
        tb.load_state_dict(sd)
        assert [g['lr'] for g in tb.param_groups] == [hyper[0]['lr'], 3e-3] and tb.param_groups[1]['decoupled_weight_decay']
        # torch -> ours: a fresh FlatAdam on torch's fp32 parameter values
        fp = [torch.nn.Parameter(q.detach().clone().to(dev)) for q in refs[F32][0]]
        fb = FlatAdam([dict(params=[fp[i] for i in idx]) for idx in split], lr=1.0)
        fb.load_state_dict(tsd)
        assert [g['lr'] for g in fb.param_groups] == [hyper[0]['lr'], 3e-3]
        assert [g['decoupled_weight_decay'] for g in fb.param_groups] == [False, True] and fb.param_groups[1]['betas'] == hyper[1]['betas']
        assert [fb.steps[order.index(i)] for i in range(5)] == [2, 1, 2, 2, 2], fb.steps
        grads = [_randn(rs, *s) for s in SHAPES]
        fb.zero_grad()
        _set_grads(dev, fp, refs, grads)
        for q, g in zip(tp, grads):
            q.grad = g.clone()
        fb.step(); tb.step()
        for dt in refs:
            refs[dt][1].step()
        _compare("torch state loaded into FlatAdam", fb, fp, refs, order)
        for i in range(5):
            _check("FlatAdam state loaded into torch p%d" % i, tp[i], refs[torch.float64][0][i].detach(), refs[F32][0][i].detach(), "flatadam groups p")
        # mismatches
        for bad, text in ((SPLITS[3], "different number of parameter groups"), (((0,), (1, 2, 3, 4)), "doesn't match the size")):
            other = FlatAdam([dict(params=[torch.nn.Parameter(x.clone().to(dev)) for x in [_toy()[i] for i in idx]]) for idx in bad], lr=1e-3)
            for s in (sd, tsd):
                try:
                    other.load_state_dict(s)
                except ValueError as e:
                    assert text in str(e), str(e)
                else:
                    raise AssertionError("load_state_dict accepted a state with other groups (%s)" % text)
        # single group: as before
        one = FlatAdam([torch.nn.Parameter(x.clone().to(dev)) for x in _toy()], lr=2e-3)
        one.zero_grad()
        for p, g in zip(one.params, grads):
            p.grad = g.to(dev)
        one.step()
        sd1 = one.state_dict()
        assert len(sd1['param_groups']) == 1 and sd1['param_groups'][0]['params'] == [0, 1, 2, 3, 4] and sd1['param_groups'][0]['lr'] == 2e-3
        two = FlatAdam([torch.nn.Parameter(x.clone().to(dev)) for x in _toy()], lr=1.0)
        two.load_state_dict(sd1)
        assert torch.equal(two.exp_avg, one.exp_avg) and torch.equal(two.exp_avg_sq, one.exp_avg_sq) and two.steps == one.steps == [1] * 5
        assert two.param_groups[0]['lr'] == 2e-3
        t1 = torch.optim.Adam([torch.nn.Parameter(x.clone()) for x in _toy()], lr=1.0)
        t1.load_state_dict(sd1)
        two.load_state_dict(t1.state_dict())
        assert torch.equal(two.exp_avg, one.exp_avg) and two.steps == [1] * 5
    finally:
        E.set_param_grad_allocator(None)


# ---------------------------------------------------------------------------------------------------------------- 4. bucketing
def bucketing_case(dev, quick=False):
    """slot_range of the same parameter sets under one group and under three groups: identical merged ranges, and every parameter's slot covered"""
    from riders_amd.optim import FlatAdam
    E = _E()
    try:
        opts = []
        for split in (None, SPLITS[3]):
            ps = [torch.nn.Parameter(x.clone().to(dev)) for x in _toy()]
            opts.append((ps, FlatAdam(ps, lr=1e-3) if split is None else FlatAdam(_dicts(ps, split, _hyper(3)))))
        for sel in ((0, 1, 2, 3, 4), (0, 1), (2, 3), (4,), (1, 3), (0, 2, 4), (3,)):
            ranges = []
            for ps, opt in opts:
                r = opt.slot_range([ps[i] for i in sel])
                for i in sel:
                    o = opt.offsets[opt._index[id(ps[i])]]
                    assert any(s <= o and o + ps[i].numel() <= e for s, e in r), (sel, i, r)
                assert all(s % 4 == 0 and e % 4 == 0 and s < e <= opt.numel for s, e in r) and all(a[1] < b[0] for a, b in zip(r, r[1:])), r
                ranges.append(r)
            assert ranges[0] == ranges[1], (sel, ranges)
            assert sum(e - s for s, e in ranges[0]) == sum((ps[i].numel() + 3) // 4 * 4 for i in sel)
    finally:
        E.set_param_grad_allocator(None)


# ---------------------------------------------------------------------------------------------------------------- 5. end to end (GPU only)
def finetune_case(dev):
    """RC-Net at the g6 fixture's geometry, fine-tuning style: freeze_batch_norm(model.encoder), encoder group at lr x 0.1 without decay, decoder
    group at lr with decoupled decay 1e-2.  Two eager training steps; after each backward the arena gradients are copied to the CPU and step a
    float64 and an fp32 torch.optim.Adam twin, and the parameters of each group are compared under _check.  The same two steps through
    GraphedTrainStep leave the parameters bit-identical to the eager pair."""
    import riders_amd
    from riders_amd import engine, rcnet_main
    from riders_amd.optim import FlatAdam
    from tests.parity_cases_frozen import _g6_model
    lr, betas, eps = float(np.float32(1e-3)), HP[0][1:3], HP[0][3]      # fp32-representable, as the C ABI receives them

    def build():
        model, cfg = _g6_model(dev)
        riders_amd.freeze_batch_norm(model.encoder)
        model.train()
        enc, dec = list(model.encoder.parameters()), list(model.decoder.parameters())
        opt = FlatAdam([dict(params=enc, lr=lr * 0.1), dict(params=dec, weight_decay=1e-2, decoupled_weight_decay=True)], lr=lr, betas=betas, eps=eps)
        return model, cfg, opt, (len(enc), len(dec))

    engine.set_deterministic_roi_pool(True)
    try:
        model, cfg, opt, (ne, nd) = build()
        batch = rcnet_main.synthetic_batch(2, 64, 96, cfg, seed=77, device=dev)
        twins = {}
        for dt in (torch.float64, F32):
            tp = [torch.nn.Parameter(p.detach().cpu().to(dt).clone()) for p in opt.params]
            twins[dt] = (tp, torch.optim.Adam([dict(params=tp[:ne], lr=lr * 0.1), dict(params=tp[ne:], weight_decay=1e-2, decoupled_weight_decay=True)],
                                              lr=lr, betas=betas, eps=eps, foreach=False))
        for step in (1, 2):
            loss = rcnet_main.forward_loss(model, batch, cfg)
            opt.zero_grad()
            loss.backward()
            grads, touched = opt.flat_grad.detach().cpu(), set(opt.touched_indices())
            assert any(i < ne for i in touched) and any(i >= ne for i in touched)
            with _Count("rd_adam_step_groups") as cg, _Count("rd_adam_step") as c1:
                opt.step()
            assert c1.n == 0 and cg.n >= 1
            print("fine-tuning step %d: %d of %d parameters have gradients, %d rd_adam_step_groups launches" % (step, len(touched), ne + nd, cg.n))
            for dt, (tp, topt) in twins.items():
                for i, (q, o) in enumerate(zip(tp, opt.offsets)):
                    q.grad = grads[o:o + q.numel()].view(q.shape).to(dt).clone() if i in touched else None
                topt.step()
            for name, a, b in (("encoder", 0, ne), ("decoder", ne, ne + nd)):
                cat = lambda xs: torch.cat([x.detach().reshape(-1).cpu() for x in xs[a:b]])      # noqa: E731
                _check("fine-tuning step %d, %s group" % (step, name), cat(opt.params), cat(twins[torch.float64][0]), cat(twins[F32][0]), "finetune " + name)
        eager = opt.flat_param.clone()
        engine.set_param_grad_allocator(None)
        engine.clear_caches()
        model, cfg, opt, _ = build()
        step_fn = rcnet_main.GraphedTrainStep(model, opt, batch, cfg, warmup=1)
        for _ in range(2):
            step_fn()
        assert opt.step_count == 2
        assert torch.equal(_bits(opt.flat_param), _bits(eager)), "graphed fine-tuning steps differ from the eager pair in %d elements" % int((opt.flat_param != eager).sum())
    finally:
        engine.set_deterministic_roi_pool(False)
        engine.set_param_grad_allocator(None)
