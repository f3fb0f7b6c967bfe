"""Direct parity cases for softmax ('full') attention and for the token masks: rd_full_attention_fwd / _bwd (rd_attention_full.hip) and
rd_linear_attention_masked_fwd / _bwd (attn_head's MASK flag, rd_attention_head.h) through the C ABI, and the modules that route to them
(FullAttention, masked LinearAttention, LoFTREncoderLayer / LocalFeatureTransformer with attention='full' or masks).

Harness and bound are those of tests/parity_cases_glue.py and tests/parity_cases_attn.py, imported, not copied: token matrices are `Mat`s inside
guarded, NaN-prefilled `Buf`s (pad columns NaN, required bit-identical afterwards), inputs are checked unchanged, references are float64 torch
(tests/ref_full_attn.py, pinned against the reference's own float64 results by tests/test_golden_full_attn.py) on the values the kernel
receives, and `_check` takes torch's fp32 CPU result of the same expression as the yardstick.  No tolerance constant is added here.

Cases (`attention_case`, both ops, forward and backward):
  lengths  every pair of LENS with (N, H) cycling through NH (all residues of N * H mod 4, more than one block); masks alternate between none,
           both scattered and a prefix, so that every tile shape meets a mask
  staging  parity_cases_attn.CAUSES at (21, 21), (16, 17), (1, 32): both load paths for every tensor
  masks    at (21, 17) and (32, 32): none; kv_mask only; q_mask only; both scattered (seeded Bernoulli 0.5, a valid key forced in all but the
           last sequence); prefix-valid keys with 1 (a softmax of exactly 1), 15, 16, 17 (across the 16-row tile edge) and S valid keys; "dead":
           sequence 0 without a valid key and the last sequence without a valid query
  data     unit normal; times 6 (scores beyond 88: exp() overflows unless the row maximum is subtracted); q = 0 (A uniform over the admissible
           keys); linear entries only: eps = 1e-30 with masked query rows (Z^2 of a masked row overflows: the dKsum guard), every sequence
           keeping a valid key there ("bothk"): a sequence without one has den = eps on its VALID query rows too, which is NaN in fp32 for the
           reference and the kernel alike
  Exact properties, asserted on every masked case for both ops: query rows without an admissible key (full) / masked query rows (linear) are
  exactly 0 in out and dq; masked key rows are exactly 0 in dk and dv; everything is finite.
  S = 1, linear entries: dq and dk are two terms that cancel to O(eps), which torch's own fp32 cannot compute; parity_cases_attn's rule for it
  (`_check_s1`, its docstring, 3) is imported and used as it stands; a sequence whose mask leaves one valid key is the same situation.
  Edges: N = 0 (returns 0, writes nothing), the refusals, two fp16 cases; the masked linear entries with both masks NULL are bit-equal to
  rd_linear_attention_fwd / _bwd.

The fp32 yardstick of the linear entries at eps = 1e-30 with masked query rows is the restatement's (tests/ref_full_attn.py), which divides a
masked row by 1 and sets its Z to 0 as the kernel documents; the reference's own expression is 0 * (1 / eps)^2 = NaN in fp32 there, which is
what the kernel's guard exists to avoid.  That is the yardstick of a documented chain in the sense of "Finding 2" of parity_cases_attn.py, not a
wider bound.

Modules (`layer_case`, `transformer_case`, fp32): LoFTREncoderLayer(128, 8, 'full') with a source mask, LocalFeatureTransformer(['self', 'cross'], 1, 128, 8) with
attention 'full' and 'linear' and masks, on the inputs of g20 (e), (f), (g): against the float64 restatement by `_check`, and against the
fixture's stored elements wherever the reference is finite.  `state_dict_case`: the keys of an attention='full' transformer are those of the
linear one.  `default_route_case`: LocalFeatureTransformer(..., 'linear') without masks still takes the fused route: bit-identical to the same
layers run through engine.loftr_layer directly.

Measured (relative to max|ref|, fp32 outputs; in brackets torch's fp32 error against float64; 16-bit outputs sit within their half ulp, at most
3.9e-3 of max|ref|).  The largest figures of the full op come from the times-6 data, where a row of A is one-hot to fp32 and kernel and torch
return v's row itself: both are off float64 by the same 1 - A.
  emulator (the covering selection):
    full           vector staging fwd 3.4e-7 (3.4e-7), bwd 3.4e-7 (3.4e-7); element-wise staging fwd 2.5e-6 (2.5e-6), bwd 2.6e-6 (2.6e-6)
    masked linear  vector staging fwd 3.7e-7 (3.5e-7), bwd 9.5e-7 (5.5e-7); element-wise staging fwd 3.2e-7 (2.9e-7), bwd 5.3e-7 (5.4e-7);
                   one valid key (the S = 1 rule) 5.5e-7 (4.5e-7)
  MI355X (the cross products):
    full           fwd 3.4e-6 (3.4e-6), bwd 3.6e-6 (3.6e-6) in both stagings (the times-6 data; unit normal data: fwd 3.5e-7 (3.4e-7), bwd 4.1e-7 (3.4e-7))
    masked linear  fwd 3.7e-7 (4.4e-7), bwd 8.2e-7 (6.9e-7) in both stagings; one valid key (the S = 1 rule) 5.5e-7 (4.5e-7)
    modules        3.0e-6 (2.1e-6)
No case needed another yardstick than torch's fp32 of the restatement.
"""
import itertools

import numpy as np
import torch

from tests import ref_full_attn as R
from tests.parity_cases import bf16_mode
from tests.parity_cases_attn import CAUSES, LENS, NH, Mat, _cancel_scales, _check_s1, _is_vec, _lds, _ve
from tests.parity_cases_bn import _cover
from tests.parity_cases_glue import BF16, F16, F32, MEASURED, Buf, _call, _check, _dt, _E, _exact, _P, _r, _randn, _refused, _rs, _S  # noqa: F401

OPS = ("full", "linear")
DTYPES = (F32, BF16)
SWEEPS = ("lengths", "staging", "masks", "data")
MASKS = (None, "kv", "q", "both", "prefix1", "prefix15", "prefix16", "prefix17", "prefixS", "dead")
DATA = ("normal", "x6", "q0", "tiny_eps")
EPS_A, SCALE = 1e-6, 0.25


def report():
    for k in sorted(MEASURED):
        if k.startswith("fattn "):
            print("full-attn parity %-34s torch fp32 error %.3e   kernel error %.3e   (relative to max|ref|)" % (k, MEASURED[k][0], MEASURED[k][1]))


def _masks(kind, N, L, S, key):
    """(q_mask, kv_mask) as torch.bool CPU tensors or None; drawn once per case from a seed of the case"""
    if kind is None:
        return None, None
    rs = _rs("fattn mask", kind, N, L, S, key)
    qm, km = torch.from_numpy(rs.rand(N, L) < 0.5), torch.from_numpy(rs.rand(N, S) < 0.5)
    if kind == "kv":
        return None, km
    if kind == "q":
        return qm, None
    if kind in ("both", "bothk"):
        km[:N if kind == "bothk" else max(N - 1, 1), int(rs.randint(S))] = True      # a valid key in all but the last sequence (N = 1: in the only one)
        return qm, km                                                                # ("bothk": in every sequence)
    if kind.startswith("prefix"):
        cnt = S if kind == "prefixS" else min(int(kind[6:]), S)
        return torch.ones(N, L, dtype=torch.bool), (torch.arange(S)[None, :] < cnt).expand(N, S).clone()
    assert kind == "dead" and N >= 2
    qm[:, 0], km[:, 0] = True, True
    km[0], qm[N - 1] = False, False
    return qm, km


def _data(dtype, N, L, S, H, data, key):
    rs = _rs("fattn", str(dtype), N, L, S, H, data, key)
    q, k, v, do = _randn(rs, N * L, H * 16), _randn(rs, N * S, H * 16), _randn(rs, N * S, H * 16), _randn(rs, N * L, H * 16)
    if data == "x6":
        q, k = q * 6, k * 6
    elif data == "q0":
        q = torch.zeros_like(q)
    return [_r(a, dtype) for a in (q, k, v, do)]


def _ref(op, dt, q, k, v, do, qm, km, N, L, S, H, eps):
    q_, k_, v_ = [a.to(dt).view(N, -1, H, 16).clone().requires_grad_() for a in (q, k, v)]
    out = R.full_attention_abi(q_, k_, v_, qm, km, SCALE) if op == "full" else R.linear_attention(q_, k_, v_, qm, km, eps)
    out.backward(do.to(dt).view(N, L, H, 16))
    return [a.detach().reshape(a.shape[0] * a.shape[1], H * 16) for a in (out, q_.grad, k_.grad, v_.grad)]


def _entries(op, masked=True):
    if op == "full":
        return "rd_full_attention_fwd", "rd_full_attention_bwd"
    return ("rd_linear_attention_masked_fwd", "rd_linear_attention_masked_bwd") if masked else ("rd_linear_attention_fwd", "rd_linear_attention_bwd")


def _run(dev, op, dtype, N, L, S, H, cause, q, k, v, do, qm, km, eps, what, masked=True):
    """both entries on guarded buffers -> (out, dq, dk, dv) as CPU tensors; every guard checked"""
    Cc, ve = H * 16, _ve(dtype)
    ldq, ldk, ldv, ldo = _lds(cause, Cc, ve)
    Q = Mat(dev, N * L, Cc, ldq, dtype, q, off=1 if cause == "q" else 0)
    K = Mat(dev, N * S, Cc, ldk, dtype, k, off=1 if cause == "k" else 0)
    V = Mat(dev, N * S, Cc, ldv, dtype, v, off=1 if cause == "v" else 0)
    DO = Mat(dev, N * L, Cc, ldo, dtype, do, off=1 if cause == "dout" else 0)
    OUT, DQ, DK, DV = Mat(dev, N * L, Cc, ldo, dtype), Mat(dev, N * L, Cc, ldq, dtype), Mat(dev, N * S, Cc, ldk, dtype), Mat(dev, N * S, Cc, ldv, dtype)
    for bwd in (False, True):
        aligned = all(m_.B.v.data_ptr() % 16 == 0 for m_ in ((Q, K, V, DO) if bwd else (Q, K, V)))
        lds_ok = all(l_ % ve == 0 for l_ in ((ldq, ldk, ldv, ldo) if bwd else (ldq, ldk, ldv)))
        assert (aligned and lds_ok) == _is_vec(cause, dtype, bwd), what + ": the case is not in the staging class it is listed under"
    qd, kd = [None if m_ is None else m_.to(dev).contiguous() for m_ in (qm, km)]
    mp = [None if m_ is None else _P(m_) for m_ in (qd, kd)] if masked else []
    sc = SCALE if op == "full" else eps
    fwd, bwd = _entries(op, masked)
    _call(fwd, Q.p, K.p, V.p, OUT.p, *mp, N, L, S, H, ldq, ldk, ldv, ldo, sc, _dt(Q.B.v), _S(Q.B.v))
    _call(bwd, Q.p, K.p, V.p, DO.p, DQ.p, DK.p, DV.p, *mp, N, L, S, H, ldq, ldk, ldv, ldo, sc, _dt(Q.B.v), _S(Q.B.v))
    for m_ in (Q, K, V, DO):
        m_.check(what, unchanged=True)
    for m_, ref_ in ((qd, qm), (kd, km)):
        assert m_ is None or torch.equal(m_.cpu(), ref_), what + ": a mask was overwritten"
    for m_ in (OUT, DQ, DK, DV):
        m_.check(what, unchanged=(N == 0))
    return [m_.data() for m_ in (OUT, DQ, DK, DV)]


def _one(dev, op, dtype, N, L, S, H, cause=None, data="normal", mask=None, key=0):
    eps = 1e-30 if data == "tiny_eps" else EPS_A
    q, k, v, do = _data(dtype, N, L, S, H, data, key)
    qm, km = _masks(mask, max(N, 1), L, S, key) if N else (None, None)
    what = "%s attention %s N=%d L=%d S=%d H=%d staging=%s data=%s mask=%s" % (op, dtype, N, L, S, H, cause, data, mask)
    got = _run(dev, op, dtype, N, L, S, H, cause, q, k, v, do, qm, km, eps, what)
    if N == 0:
        return
    r64, r32 = _ref(op, torch.float64, q, k, v, do, qm, km, N, L, S, H, eps), _ref(op, torch.float32, q, k, v, do, qm, km, N, L, S, H, eps)
    gf = "fattn %s %s fwd" % (op, "vec" if _is_vec(cause, dtype, False) else "scalar")
    gb = "fattn %s %s bwd" % (op, "vec" if _is_vec(cause, dtype, True) else "scalar")
    if op == "linear" and (S == 1 or (km is not None and int(km.sum(1).min()) <= 1)):
        # one valid key in a sequence: dq and dk are pure cancellation there, parity_cases_attn's rule (its docstring, 3).  Its float64 scales take
        # no masks; a masked token enters them as q or k = -inf (elu(-inf) + 1 = 0 = the masked feature) and v = 0, which is the same arithmetic
        ninf = lambda x, m_, n_: x if m_ is None else torch.where(m_.reshape(-1, 1), x, torch.full_like(x, n_))      # noqa: E731
        cq, ck, _, _ = _cancel_scales(ninf(q, qm, float("-inf")), ninf(k, km, float("-inf")), ninf(v, km, 0.0), do, N, L, S, H, eps)
        _check(what + " out", got[0], r64[0], r32[0], gf)
        _check(what + " dv", got[3], r64[3], r32[3], gb)
        _check_s1(what + " dq", got[1], r64[1], r32[1], cq.max(), gb + " S=1")
        _check_s1(what + " dk", got[2], r64[2], r32[2], ck.max(), gb + " S=1")
        return
    for name, g_, a64, a32, grp in zip(("out", "dq", "dk", "dv"), got, r64, r32, (gf, gb, gb, gb)):
        _check(what + " " + name, g_, a64, a32, grp)
    # exact properties
    Cc = H * 16
    out, dq, dk, dv = [a.float().view(N, -1, Cc) for a in got]
    qv = torch.ones(N, L, dtype=torch.bool) if qm is None else qm
    kvv = torch.ones(N, S, dtype=torch.bool) if km is None else km
    zero_q = ~qv if op == "linear" else ~(qv & kvv.any(1, keepdim=True))      # rows of out / dq that must be exactly 0
    if bool(zero_q.any()):
        assert float(out[zero_q].abs().max()) == 0.0 and float(dq[zero_q].abs().max()) == 0.0, what + ": rows that must be exactly zero are not"
    if bool((~kvv).any()):
        assert float(dk[~kvv].abs().max()) == 0.0 and float(dv[~kvv].abs().max()) == 0.0, what + ": dk / dv of masked keys are not exactly zero"
    if mask == "prefix1" and op == "full":      # one admissible key: A = 1 exactly, so out is v's first row of the sequence, bit for bit
        vv = v.view(N, S, Cc)[:, :1].expand(N, L, Cc)
        assert torch.equal(out, vv.to(got[0].dtype).float()), what + ": a softmax over one key is not exactly 1"
    if mask == "dead":
        assert bool(zero_q[N - 1].all()) and float(out[0].abs().max()) == 0.0      # (linear: K = V = 0 makes KV = 0, so out is 0 without a rule)
        if op == "full":
            assert bool(zero_q[0].all())      # a sequence without a valid key adds nothing to dk / dv; one without a valid query neither
            assert float(dk[0].abs().max()) == 0.0 and float(dv[0].abs().max()) == 0.0 and float(dk[N - 1].abs().max()) == 0.0 and float(dv[N - 1].abs().max()) == 0.0, what


def _configs(op, sweeps, dtypes):
    out = []
    for dtype in dtypes:
        if "lengths" in sweeps:
            for i, L in enumerate(LENS):
                for j, S in enumerate(LENS):
                    N, H = NH[(i * len(LENS) + j) % len(NH)]
                    mask = (None, "both", "prefix16")[(i + 2 * j) % 3]
                    out.append((dtype, N, L, S, H, (None, "ldv", "k")[(i + j) % 3], "normal", mask))
        if "staging" in sweeps:
            for cause in CAUSES:
                for (N, H) in NH[:4]:
                    for (L, S) in ((21, 21), (16, 17), (1, 32)):
                        out.append((dtype, N, L, S, H, cause, "normal", "both" if (N + L) % 2 else None))
        if "masks" in sweeps:
            for mask in MASKS:
                for (L, S), (N, H) in (((21, 17), (2, 3)), ((32, 32), (3, 5))):
                    for cause in (None, "ldq"):
                        out.append((dtype, N, L, S, H, cause, "normal", mask))
        if "data" in sweeps:
            for data in DATA[1:]:
                if data == "tiny_eps" and op == "full":
                    continue
                for cause in (None, "q"):
                    for (L, S) in ((21, 17), (17, 16), (32, 32)):
                        for mask in ((("q", "bothk", "prefix17") if data == "tiny_eps" else (None, "both", "prefix17"))):
                            out.append((dtype, 2, L, S, 3, cause, data, mask))
    return out


def _feats(c):
    dtype, N, L, S, H, cause, data, mask = c
    lt, stl = (L + 15) >> 4, (S + 15) >> 4
    return [("L", L), ("S", S), ("tiles", (lt > stl) - (lt < stl)), ("res", (N * H) % 4), ("H", H), ("cause", dtype, cause), ("data", dtype, data),
            ("mask", mask, _is_vec(cause, dtype, True)), ("mask at", mask, (L, S) if (L, S) in ((21, 17), (32, 32)) else None), ("blocks", N * H > 4)]


def attention_case(dev, op, quick=False, dtypes=DTYPES, sweeps=SWEEPS):
    """one op over its sweeps (module docstring).  quick: a covering selection, whose coverage is asserted."""
    cfgs = _cover(_configs(op, sweeps, dtypes), _feats, quick, "fattn " + op)
    if set(sweeps) == set(SWEEPS):
        seen = set(itertools.chain.from_iterable(_feats(c) for c in cfgs))
        for n in LENS:
            assert ("L", n) in seen and ("S", n) in seen, n
        assert {("tiles", -1), ("tiles", 0), ("tiles", 1)} <= seen and {("res", r) for r in range(4)} <= seen
        for dtype in dtypes:
            assert {("cause", dtype, c) for c in CAUSES} <= seen and {("data", dtype, d) for d in DATA if not (d == "tiny_eps" and op == "full")} <= seen
        for m_ in MASKS:
            assert ("mask at", m_, (21, 17)) in seen and ("mask at", m_, (32, 32)) in seen, m_
    for c in cfgs:
        _one(dev, op, *c)
    return len(cfgs)


def edges_case(dev, quick=False):
    """N = 0 (returns 0, writes nothing), two fp16 cases per op, and the masked linear entries with both masks NULL against the unmasked ones."""
    for op in OPS:
        _one(dev, op, F32, 0, 21, 17, 3)
        _one(dev, op, BF16, 0, 1, 32, 8, "ldq")
        with bf16_mode("fp16"):
            _one(dev, op, F16, 2, 21, 17, 3, None, "normal", "both")
            _one(dev, op, F16, 2, 16, 32, 5, "v", "x6" if op == "full" else "normal", "dead")
    for dtype, N, L, S, H, cause in ((F32, 3, 21, 17, 3, None), (F32, 2, 32, 32, 5, "k"), (BF16, 3, 17, 31, 3, None), (BF16, 1, 16, 1, 8, "ldo")):
        q, k, v, do = _data(dtype, N, L, S, H, "normal", "null masks")
        what = "masked linear entries with NULL masks %s N=%d L=%d S=%d H=%d staging=%s" % (dtype, N, L, S, H, cause)
        a = _run(dev, "linear", dtype, N, L, S, H, cause, q, k, v, do, None, None, EPS_A, what, masked=True)
        b = _run(dev, "linear", dtype, N, L, S, H, cause, q, k, v, do, None, None, EPS_A, what, masked=False)
        for name, x, y in zip(("out", "dq", "dk", "dv"), a, b):
            _exact(what + " " + name, x, y)


def refusals_case(dev, quick=False):
    """by return code and message only; nothing is launched, and the outputs come back unchanged"""
    N, L, S, H = 1, 4, 4, 1
    q, k, v, do = _data(F32, N, L, S, H, "normal", "refuse")
    Q, K, V, DO = (Mat(dev, 4, 16, 16, F32, a) for a in (q, k, v, do))
    outs = [Mat(dev, 4, 16, 16, F32) for _ in range(4)]
    OUT, DQ, DK, DV = outs
    st, dt = _S(Q.B.v), _dt(Q.B.v)
    for op, sc in (("full", SCALE), ("linear", EPS_A)):
        fwd, bwd = _entries(op)
        tail = [None, None, N, L, S, H, 16, 16, 16, 16, sc]
        for (l_, s_) in ((0, 4), (4, 0), (33, 4), (4, 33), (-1, 4)):
            _refused(fwd, "L,S must be in 1..32", Q.p, K.p, V.p, OUT.p, None, None, N, l_, s_, H, 16, 16, 16, 16, sc, dt, st)
            _refused(bwd, "L,S must be in 1..32", Q.p, K.p, V.p, DO.p, DQ.p, DK.p, DV.p, None, None, N, l_, s_, H, 16, 16, 16, 16, sc, dt, st)
        fa, ba = [Q.p, K.p, V.p, OUT.p], [Q.p, K.p, V.p, DO.p, DQ.p, DK.p, DV.p]
        for i in range(4):
            a = list(fa); a[i] = None
            _refused(fwd, fwd[3:] + ": bad args", *(a + tail + [dt, st]))
        for i in range(7):
            a = list(ba); a[i] = None
            _refused(bwd, bwd[3:] + ": bad args", *(a + tail + [dt, st]))
        for bad in (3, -1, 99):
            _refused(fwd, fwd[3:] + ": bad args", *(fa + tail + [bad, st]))
            _refused(bwd, bwd[3:] + ": bad args", *(ba + tail + [bad, st]))
    for m_ in (Q, K, V, DO) + tuple(outs):
        m_.check("refused attention", unchanged=True)


# ---------------------------------------------------------------------------------------------------------------- modules
_GOLD = {}


def _gold():
    """fixture, recipe and the float64 / fp32 restatement results of the module cases: computed once, left unchanged"""
    if not _GOLD:
        import os
        from tests.golden.make_golden_full_attn import STRIDE, recipe
        _GOLD.update(g=dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "g20_full_attention.npz"))), r=recipe(), stride=STRIDE, refs={})
    return _GOLD


def _against_fixture(what, got, key, ref32, finite_rows=None):
    """the stored elements of the fixture (every STRIDE-th) wherever the reference is finite, by _check with the restatement's fp32 as yardstick"""
    G = _gold()
    g_, r32 = got.detach().cpu().float(), ref32.detach().float()
    if finite_rows is not None:
        g_, r32 = [torch.where(finite_rows[..., None], a, torch.zeros_like(a)) for a in (g_, r32)]
    _check(what + " against the fixture", g_.reshape(-1)[::G["stride"]], torch.from_numpy(G["g"][key]), r32.reshape(-1)[::G["stride"]], "fattn modules")


def _module_refs(name, build, sd_of):
    G = _gold()
    if name not in G["refs"]:
        G["refs"][name] = [build(dt, {k_: v_.detach().to(dt).clone().requires_grad_() for k_, v_ in sd_of.items()}) for dt in (torch.float64, torch.float32)]
    return G["refs"][name]


def layer_case(dev, quick=False):
    """LoFTREncoderLayer(128, 8, 'full') with a source mask, fp32: g20 (e)"""
    from riders_amd.linear_attention import FullAttention, LoFTREncoderLayer
    from tests.golden.fill import fill_state_dict
    c = _gold()["r"]["e"]
    m = LoFTREncoderLayer(128, 8, "full").to(dev)
    assert isinstance(m.attention, FullAttention)
    sd = fill_state_dict(m, "g20.layer")

    def build(dt, sd_):
        x, s = c["x"].to(dt).clone().requires_grad_(), c["s"].to(dt).clone().requires_grad_()
        o = R.loftr_layer(x, s, sd_, "", "full", c["x_mask"], c["source_mask"])
        (o * c["w"].to(dt)).sum().backward()
        res = {"out": o.detach(), "dx": x.grad, "ds": s.grad}
        res.update({"grad " + k_: v_.grad for k_, v_ in sd_.items()})
        return res
    r64, r32 = _module_refs("layer", build, sd)
    x, s = c["x"].float().to(dev).requires_grad_(), c["s"].float().to(dev).requires_grad_()
    o = m(x, s, c["x_mask"].to(dev), c["source_mask"].to(dev))
    (o * c["w"].float().to(dev)).sum().backward()
    res = {"out": o.detach().cpu(), "dx": x.grad.cpu(), "ds": s.grad.cpu()}
    res.update({"grad " + k_: p.grad.detach().cpu() for k_, p in m.named_parameters()})
    assert set(res) == set(r64)
    for k_ in sorted(res):
        _check("layer 'full' with a source mask: " + k_, res[k_], r64[k_], r32[k_], "fattn modules")
    for k_ in ("out", "dx", "ds"):
        _against_fixture("layer 'full' " + k_, res[k_], "e." + k_, r32[k_])


def transformer_case(dev, attention, quick=False):
    """LocalFeatureTransformer(['self', 'cross'], 1, 128, 8, attention) with mask0 all true and mask1 partial, fp32: g20 (f) / (g)"""
    from riders_amd.linear_attention import LocalFeatureTransformer
    from tests.golden.fill import fill_state_dict
    G = _gold()
    c = G["r"]["f"]
    m = LocalFeatureTransformer(["self", "cross"], 1, 128, 8, attention).to(dev)
    sd = fill_state_dict(m, "g20.tf")

    def build(dt, sd_):
        a, b = c["a"].to(dt).clone().requires_grad_(), c["b"].to(dt).clone().requires_grad_()
        o0, o1 = R.local_feature_transformer(a, b, sd_, "", ("self", "cross"), attention, c["mask0"], c["mask1"])
        ((o0 * c["w0"].to(dt)).sum() + (o1 * c["w1"].to(dt)).sum()).backward()
        res = {"out0": o0.detach(), "out1": o1.detach(), "da": a.grad, "db": b.grad}
        res.update({"grad " + k_: v_.grad for k_, v_ in sd_.items()})
        return res
    r64, r32 = _module_refs("tf " + attention, build, sd)
    a, b = c["a"].float().to(dev).requires_grad_(), c["b"].float().to(dev).requires_grad_()
    o0, o1 = m(a, b, c["mask0"].to(dev), c["mask1"].to(dev))
    ((o0 * c["w0"].float().to(dev)).sum() + (o1 * c["w1"].float().to(dev)).sum()).backward()
    res = {"out0": o0.detach().cpu(), "out1": o1.detach().cpu(), "da": a.grad.cpu(), "db": b.grad.cpu()}
    res.update({"grad " + k_: p.grad.detach().cpu() for k_, p in m.named_parameters()})
    assert set(res) == set(r64)
    for k_ in sorted(res):
        _check("transformer '%s' with masks: %s" % (attention, k_), res[k_], r64[k_], r32[k_], "fattn modules")
    if attention == "full":      # the reference is NaN on the rows of f.nan0 / f.nan1 (every row of a sequence with a masked token); finite here
        for k_, nan in (("out0", "f.nan0"), ("out1", "f.nan1")):
            _against_fixture("transformer 'full' " + k_, res[k_], "f." + k_, r32[k_], ~torch.from_numpy(G["g"][nan]))
    else:
        for k_ in ("out0", "out1", "da", "db"):
            _against_fixture("transformer 'linear' " + k_, res[k_], "g." + k_, r32[k_])


def state_dict_case():
    from riders_amd.linear_attention import FullAttention, LocalFeatureTransformer
    full, lin = LocalFeatureTransformer(["self", "cross"], 2, 128, 8, "full"), LocalFeatureTransformer(["self", "cross"], 2, 128, 8, "linear")
    assert list(full.state_dict().keys()) == list(lin.state_dict().keys())
    assert all(isinstance(l.attention, FullAttention) for l in full.layers)
    full.load_state_dict(lin.state_dict())      # an attention='full' checkpoint loads: same keys, same shapes


def default_route_case(dev, quick=False):
    """LocalFeatureTransformer(..., 'linear') without masks: the route it took before masks existed -- every layer one fused engine.loftr_layer
    launch -- bit for bit.  ('unmerged' and the default route are bit-equal in outputs: parity_cases_attn, 4.)"""
    from riders_amd.linear_attention import LocalFeatureTransformer
    from tests.golden.fill import fill_state_dict
    E = _E()
    N, L, C = 2, 21, 128
    rs = _rs("fattn default route")
    a, b = _randn(rs, N, L, C).to(dev), _randn(rs, N, L, C).to(dev)
    m = LocalFeatureTransformer(["self", "cross"], 1, C, 8, "linear").to(dev)
    fill_state_dict(m, "fattn.route")
    assert E.fused_loftr()
    with torch.no_grad():
        o0, o1 = m(a, b)

        def direct(x, y):
            f0, f1 = E.tokens_in(x, C), E.tokens_in(y, C)
            f0 = E.loftr_layer(f0, f0, m.layers[0], N, L, L)
            f1 = E.loftr_layer(f1, f1, m.layers[0], N, L, L)
            f0 = E.loftr_layer(f0, f1, m.layers[1], N, L, L)
            f1 = E.loftr_layer(f1, f0, m.layers[1], N, L, L)
            return E.alias_cast_view(f0, x.dtype, (N, L, C)), E.alias_cast_view(f1, y.dtype, (N, L, C))
        d0, d1 = E.run_region(direct, (a, b), [])
    _exact("default route, out0", o0, d0)
    _exact("default route, out1", o1, d1)
