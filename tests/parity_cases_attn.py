"""Direct parity cases for the attention code: rd_linear_attention_fwd / _bwd (rd_attention.hip, rd_attention_head.h) and the fused LoFTR
encoder layer rd_loftr_layer_fwd / _bwd (rd_loftr.hip), both through the C ABI, and the routes of LocalFeatureTransformer that nothing compared.
Harness and bound as tests/parity_cases_glue.py and tests/parity_cases_bn.py (imported, not copied): every buffer a kernel writes is a `Buf`
with sentinels on both sides and a NaN prefill, inputs are checked unchanged, references are plain float64 torch on the values the kernel
receives (16-bit inputs: the rounded values), `_check` takes torch's own fp32 CPU result of the same expression as the yardstick.  No tolerance
constant is added here.

1. Attention (`attention_case`).  A token matrix is (N * L, ld) with the H * 16 head columns in front; `Mat` fills the pad columns of inputs and
   outputs with NaN and requires those of outputs to come back bit-identical.  Staging classes (restated from the documented condition in
   attn_head: the 16-byte path needs q, k, v -- and dout in the backward -- 16-byte aligned and ldq, ldk, ldv -- ldo in the backward -- multiples
   of VE = 4 / 8): `None` all aligned, ld = 16 H; "pad" the vector path with four different ld > 16 H; "q" / "k" / "v" / "dout" that pointer off by
   one element; "ldq" / "ldk" / "ldv" / "ldo" that ld = 16 H + 1; "ld4" every ld = 16 H + 4 (vector for fp32, element-wise for 16-bit); "mixed" four
   different odd ld's.  Data kinds: unit normal; times 6 (both branches of the feature map and of phi'); shifted by -9 and -14 (den comparable to
   eps); exact zeros in q and k (phi' at its joint); eps = 1e-30, where the padded rows' Z^2 overflows and their dden is NaN, which the
   `l < L` guard of the dKsum sum exists for.  N * H mod 4 takes every residue (inactive waves), N = 0 returns 0 and writes nothing.

2. Fused layer (`fused_case`), stage by stage: the kernel rounds at each stored tensor and consumes what it stored, so each stored tensor is
   compared with a float64 reference computed from the kernel's OWN stored inputs of that stage, with the weights the packed copy holds.  That
   makes 16-bit checkable to half an ulp and places a failure in one phase.  fp32 additionally gets one end-to-end comparison per case against
   oracle.rcnet.loftr_layer in float64 with autograd (a stage-wise suite alone would pass if two stages agreed on a wrong convention).
   Every saved / gradient buffer is allocated EXTRA rows longer than N * L (N * S) and those rows must stay bit-identical; `out` is always a row
   range of a larger matrix.

   Unstored rounded intermediates.  dmpre / lnp1 come through rnd(dhid . W0)[:, 128:], dx and dsrc through rnd(dhid . W0)[:, :128], rnd(dq . Wq),
   rnd(dk . Wk) and rnd(dv . Wv), none of which is stored.  The kernel rounds its fp32 value, the reference its float64 value; where that value
   lies within the fp32 bound of a rounding tie of the 16-bit type the two may pick different neighbours (about one element in a few thousand,
   i.e. some case of every run, and on different elements for any two correct fp32 evaluations -- so an fp32 restatement as the yardstick would
   not agree with a correct kernel either).  Handled as tests/parity_cases_bn.py handles rd_affine_act_add (`_check_rounded_z`): on those
   elements, and only there, the result may additionally differ by the image of one ulp of the intermediate under the documented linear map
   that follows (dx, dsrc: the ulp itself; dmpre: rs * (w + mean(w) + |xhat| mean(w |xhat|)) with w = |gamma| ulp; lnp1: the column sums).  No
   constant is involved and fp32 has no such term.

3. S = 1 (`_check_s1`): out = v (Q.K) / (Q.K + eps), so dq and dk are two terms that cancel to O(eps); torch's own fp32 is several times max|ref|
   off there.  Where -- and only where -- torch's fp32 error on the quantity exceeds TOL * max|ref| (asserted inside), the scale m of _check's
   bound is the float64 maximum of |dP KV^T| + |dden Ksum| times phi' (dq) or |V dKV^T| + |dKsum| times phi' (dk) instead of max|ref|.  The pinned
   case (1, 32, 1, H = 1) asserts that the rule was needed.  out, dv and the stage-wise dx / dsrc (computed from the kernel's stored dq, dk) stay
   on the normal rule; so do dx and dsrc of the end-to-end comparison, whose well-conditioned terms dominate (torch's fp32 stays inside
   TOL there, so the exemption cannot attach).

4. Routes (`routes_case`): LocalFeatureTransformer(['self', 'cross'], 2 layers, 128) at N = 2 in fp32 against oracle.rcnet.local_feature_transformer in
   float64, bound from the fp32 oracle's own error (the emulator twin: one layer pair, and marked slow).  Routes: default, merge_self_layers off,
   loftr_cross_inplace off, defer_wgrad off at L = S = 21; (L, S) = (7, 30), which takes the per-layer loop with fused layers, and the same with
   set_fused_loftr(False).  L = 33 raises the library's 1..32 error.  Bit-equality with the default route, decided from the code:
     merge_self_layers off  -- a workgroup's arithmetic does not depend on how many sequences the launch has, and in fp32 the in-kernel
                               dsrc_accumulate (v + old) and the tape's rd_add (old + v) are the same two-operand sum: outputs and input gradients
                               bit-equal; parameter gradients sum over N and 2 N sequences in different groupings: by the bound.
     loftr_cross_inplace off -- the same launches on the same data, only the gradient add moves out of the kernel: everything bit-equal.
     defer_wgrad off         -- outputs and input gradients bit-equal; the LayerNorm parameter sums are finished per call instead of per stage and
                               the weight gradients ungrouped: by the bound.

Finding: rd_loftr_layer_bwd checked the members of its gradient struct for NULL but not those of the weight and saved structs, which the kernel
reads just the same; it now refuses them like the forward does (refusals_case).

Finding 2: torch's blocked fp32 matmul is more accurate than one sequential fp32 chain over K = 256, and a correct token GEMM then misses
_check's bound on some data: under the emulator, fp32 cross N = 1, L = 7, S = 30 (defer_ln 0, accumulate 1), hid is 1.955e-6 from float64 at
max|ref| 3.364 where torch's fp32 is 4.12e-7 off, so the bound is 1.649e-6.  Nothing is wrong with the kernel and no constant is widened: as for
the depthwise weight gradient (tests/parity_cases_dw.py), the fp32 yardstick of the token GEMMs is a restatement of the documented chain (`_mm`),
written from tok_mma's comments, not from what the kernel returns.  Against it the full cross products pass on the emulator and on the MI355X.

Measured (relative to max|ref|, fp32 outputs; in brackets the fp32 yardstick's own error against float64: torch's fp32 CPU result, for the token
GEMMs the restatement; 16-bit outputs sit within their half ulp, at most 3.8e-3 of max|ref|):
  emulator (the covering selection):
    attention  vector staging fwd 2.6e-7 (2.7e-7), bwd 5.2e-7 (3.3e-7); element-wise staging fwd 2.9e-7 (2.9e-7), bwd 5.9e-7 (8.3e-7);
               shifted by -9 / -14 (exp() of the host): fwd 3.9e-7, bwd 3.8e-7 (torch's fp32 elu(x) + 1 itself: 7.6e-3, 1.0e-2, so the bound there is
               its cap, TOL)
    fused fwd  q 5.2e-7 (4.4e-7), k 4.9e-7 (5.5e-7), v 4.9e-7 (4.7e-7), att 2.9e-7 (2.6e-7), mpre 6.1e-7 (6.8e-7), stats 3.1e-6 (1.9e-6), msg 1.8e-7 (1.8e-7),
               hid 1.1e-6 (1.1e-6), m2pre 4.4e-7 (5.2e-7), out 1.6e-7 (1.2e-7)
    fused bwd  dm2pre 1.1e-7 (1.1e-7), dhid 4.6e-7 (5.6e-7), dmpre 5.7e-7 (5.7e-7), datt 4.7e-7 (5.4e-7), dq 5.1e-7 (3.8e-7), dk 2.1e-7 (2.3e-7),
               dv 2.2e-7 (2.3e-7), dx 2.8e-7 (2.7e-7), dsrc 4.5e-7 (3.8e-7), lnp 2.2e-6 (4.1e-7; the kernel's figure is a 16-bit case's flipped tie,
               inside its allowance), dg / db 7.5e-8 (8.3e-8)
    end to end out 2.3e-6 (1.9e-6), dx 2.0e-6 (2.5e-6), dsrc 5.4e-7 (5.1e-7), LayerNorm parameters 2.6e-6 (3.1e-6)
    routes     outputs and input gradients 5.3e-7 (5.3e-7), parameter gradients 2.1e-6 (2.0e-6)
  MI355X (the cross products):
    attention  vector staging fwd 3.4e-7 (3.4e-7), bwd 7.1e-7 (8.3e-7); element-wise staging fwd 3.6e-7 (3.4e-7), bwd 9.5e-7 (8.3e-7);
               shifted by -9 / -14 (__expf of the hardware): fwd 1.0e-6, bwd 1.3e-6 in both stagings (torch's fp32: 7.6e-3, 2.0e-2): three times the
               emulator's figure, a thousand times inside the bound
    fused fwd  q 5.2e-7 (4.4e-7), k 6.2e-7 (5.5e-7), v 4.9e-7 (4.8e-7), att 3.4e-7 (2.7e-7), mpre 6.7e-7 (6.8e-7), stats 9.5e-7 (5.0e-7), msg 1.8e-7 (2.0e-7),
               hid 1.1e-6 (1.1e-6), m2pre 5.4e-7 (5.3e-7), out 1.4e-7 (1.5e-7)
    fused bwd  dm2pre 1.4e-7 (1.4e-7), dhid 4.5e-7 (5.7e-7), dmpre 4.5e-7 (5.6e-7), datt 4.4e-7 (5.3e-7), dq 4.9e-7 (5.9e-7), dk 2.7e-7 (2.4e-7),
               dv 2.3e-7 (2.3e-7), dx 3.2e-7 (2.8e-7), dsrc 8.0e-7 (7.5e-7), lnp 1.9e-5 (4.9e-7; flipped ties of 16-bit cases, as above), dg / db 9.9e-8 (1.2e-7)
    end to end out 2.3e-6 (3.7e-6), dx 2.0e-6 (4.8e-6), dsrc 6.3e-7 (1.0e-6), LayerNorm parameters 2.6e-6 (4.1e-6)
    routes     outputs and input gradients 5.8e-7 (5.6e-7), parameter gradients 2.7e-6 (2.5e-6)
  S = 1, pinned case (1, 32, 1, H = 1), of max|ref|: torch's fp32 dq 3.5, dk 5.6 (7.9 on another host); kernel dq 5.1, dk 5.2 on the MI355X, dq 5.1, dk 7.6
  on the emulator; of the cancelling terms the kernel is 1.0e-7 and 1.0e-7 (MI355X), 1.0e-7 and 1.5e-7 (emulator).
"""
import ctypes
import itertools

import numpy as np
import torch
import torch.nn.functional as F

import oracle.rcnet as O
from tests.parity_cases import TOL, bf16_mode
from tests.parity_cases_bn import _cover, _fp32_bound, _nanbuf
from tests.parity_cases_glue import BF16, EPS32, F16, F32, FLOOR_ULPS, MEASURED, TINY32, Buf, _bits, _call, _check, _dt, _E, _exact, _half_ulp, _P, _r, _randn, _refused, _rs, _S

NAN = float("nan")
DTYPES = (F32, BF16)
LENS = (1, 15, 16, 17, 21, 31, 32)
NH = ((1, 1), (2, 3), (3, 5), (1, 8), (3, 3))      # N * H mod 4 = 1, 2, 3, 0, 1 (the last: three blocks)
PTR_CAUSES, LD_CAUSES = ("q", "k", "v", "dout"), ("ldq", "ldk", "ldv", "ldo")
CAUSES = (None, "pad") + PTR_CAUSES + LD_CAUSES + ("ld4", "mixed")
DATA = ("normal", "x6", "shift9", "shift14", "zeros", "tiny_eps")
SWEEPS = ("lengths", "staging", "data")
EPS_A, EPS_LN = 1e-6, 1e-5
C, C2, HEADS = 128, 256, 8
EXTRA = 3                                           # rows allocated behind N * L in every saved / gradient buffer
S1_USED = []                                        # (what, torch fp32 error / max|ref|, kernel error / max|ref|, kernel error / scale): the S = 1 rule's uses


def report_attn():
    for k in sorted(MEASURED):
        if k.startswith(("attn ", "loftr ", "tf ")):
            print("attn parity %-34s torch fp32 error %.3e   kernel error %.3e   (relative to max|ref|)" % (k, MEASURED[k][0], MEASURED[k][1]))
    for what, et, ek, es in S1_USED[-8:]:
        print("attn parity S=1 rule %-40s torch fp32 %.3e, kernel %.3e of max|ref|; kernel %.3e of the cancelling terms" % (what, et, ek, es))


def _ve(dtype):
    return 4 if dtype == F32 else 8


class Mat(object):
    """rows x cols token matrix with row pitch ld inside a guarded Buf; pad columns NaN (init None: the whole matrix NaN, an output)"""

    def __init__(self, dev, rows, cols, ld, dtype, init=None, off=0):
        full = torch.full((max(rows, 1), ld), NAN)
        if init is not None and rows:
            full[:, :cols] = init.reshape(rows, cols)
        self.rows, self.cols, self.ld = max(rows, 1), cols, ld
        self.B = Buf(dev, full.numel(), dtype, full, off=off)
        self.p = _P(self.B.v)

    def data(self):
        return self.B.v.view(self.rows, self.ld)[:, :self.cols].detach().cpu()

    def check(self, what, unchanged=False):
        self.B.check(what, unchanged)
        if not unchanged and self.ld > self.cols:
            a = _bits(self.B.v).cpu().view(self.rows, self.ld)[:, self.cols:]
            b = _bits(self.B.snap[self.B.lo:self.B.hi]).cpu().view(self.rows, self.ld)[:, self.cols:]
            assert torch.equal(a, b), what + ": pad columns were overwritten"


# ---------------------------------------------------------------------------------------------------------------- 1. linear attention
def _lds(cause, Cc, ve):
    """(ldq, ldk, ldv, ldo)"""
    if cause == "pad":
        return (Cc + ve, Cc + 2 * ve, Cc, Cc + 3 * ve)
    if cause == "ld4":
        return (Cc + 4,) * 4
    if cause == "mixed":
        return (Cc + 1, Cc + 3, Cc + 5, Cc + 7)
    return tuple(Cc + 1 if cause == n else Cc for n in LD_CAUSES)


def _is_vec(cause, dtype, bwd):
    """the documented condition of the 16-byte staging path, restated for the causes above"""
    if cause in (None, "pad"):
        return True
    if cause == "ld4":
        return dtype == F32
    if cause in ("dout", "ldo"):
        return not bwd
    return False


def _attn_data(dtype, N, L, S, H, data, key):
    rs = _rs("attn", str(dtype), N, L, S, H, data, key)
    q, k, v, do = _randn(rs, N * L, H * 16), _randn(rs, N * S, H * 16), _randn(rs, N * S, H * 16), _randn(rs, N * L, H * 16)
    if data == "x6":
        q, k = q * 6, k * 6
    elif data in ("shift9", "shift14"):
        sh = 9.0 if data == "shift9" else 14.0
        q, k = q - sh, k - sh
    elif data == "zeros":
        q = torch.where(_randn(rs, N * L, H * 16) > 0.5, torch.zeros_like(q), q)
        k = torch.where(_randn(rs, N * S, H * 16) > 0.5, torch.zeros_like(k), k)
    return [_r(a, dtype) for a in (q, k, v, do)]


def _attn_ref(dt, q, k, v, do, N, L, S, H, eps):
    q_, k_, v_ = [a.to(dt).view(N, -1, H, 16).clone().requires_grad_() for a in (q, k, v)]
    out = O.linear_attention(q_, k_, v_, eps)
    out.backward(do.to(dt).view(N, L, H, 16))
    return [a.detach().reshape(a.shape[0] * a.shape[1], H * 16) for a in (out, q_.grad, k_.grad, v_.grad)]


def _cancel_scales(q, k, v, do, N, L, S, H, eps):
    """float64 magnitudes of the terms that cancel in dq and dk at S = 1, element-wise: (|dP KV^T| + |dden Ksum|) phi'(q) and
    (|V dKV^T| + |dKsum|) phi'(k), from the backward written out by hand (rd_attention_head.h's comments); the signed sums are returned too,
    so that the caller can hold the hand-written backward against autograd"""
    q, k, v, do = [a.double().view(N, -1, H, 16) for a in (q, k, v, do)]
    Q, K, V = F.elu(q) + 1, F.elu(k) + 1, v / S
    KV = torch.einsum("nshd,nshe->nhde", K, V)
    Ksum = K.sum(1)
    Z = 1 / (torch.einsum("nlhd,nhd->nlh", Q, Ksum) + eps)
    P = torch.einsum("nlhd,nhde->nlhe", Q, KV)
    dP = S * Z[..., None] * do
    dden = -Z * Z * S * (P * do).sum(-1)
    a1, a2 = torch.einsum("nlhe,nhde->nlhd", dP, KV), dden[..., None] * Ksum[:, None]
    dKV, dKsum = torch.einsum("nlhd,nlhe->nhde", Q, dP), torch.einsum("nlh,nlhd->nhd", dden, Q)
    b1, b2 = torch.einsum("nshe,nhde->nshd", V, dKV), dKsum[:, None].expand(N, S, H, 16)
    pq, pk = torch.where(q > 0, torch.ones_like(q), Q), torch.where(k > 0, torch.ones_like(k), K)
    flat = lambda a: a.reshape(-1, H * 16)      # noqa: E731
    return flat((a1.abs() + a2.abs()) * pq), flat((b1.abs() + b2.abs()) * pk), flat((a1 + a2) * pq), flat((b1 + b2) * pk)


def _check_s1(what, got, ref64, ref32, scale, group):
    """_check, except where torch's own fp32 error exceeds TOL * max|ref| (a reference that is pure cancellation: module docstring, 3): there
    the scale of the bound is `scale`, the float64 maximum of the summed magnitudes of the cancelling terms.  -> True where the rule was used"""
    r = ref64.double().reshape(-1)
    m = float(r.abs().max())
    ref_err = float((ref32.double().reshape(-1) - r).abs().max())
    if not ref_err > TOL * m:
        _check(what, got, ref64, ref32, group)
        return False
    assert ref_err > TOL * m, what + ": the S = 1 rule is for quantities torch's own fp32 cannot compute"
    g = got.detach().cpu()
    out_dt = g.dtype
    g = g.double().reshape(-1)
    assert g.shape == r.shape and bool(torch.isfinite(g).all()), what + ": shape / non-finite values"
    sm = float(scale)
    assert sm >= m
    bound = min(max(4.0 * ref_err, FLOOR_ULPS * EPS32 * sm, TINY32), max(TOL * sm, TINY32))
    diff = (g - r).abs()
    err = float(diff.max())
    S1_USED.append((what, ref_err / max(m, TINY32), err / max(m, TINY32), err / sm))
    assert bool((diff <= bound + _half_ulp(out_dt, r)).all()), "%s: kernel error %.3e, torch fp32's own error %.3e, bound %.3e at the scale %.3e of the cancelling terms (max|ref| %.3e)" % (
        what, err, ref_err, bound, sm, m)
    return True


def _attn_one(dev, dtype, N, L, S, H, cause=None, data="normal", key=0):
    Cc, ve = H * 16, _ve(dtype)
    eps = 1e-30 if data == "tiny_eps" else EPS_A
    ldq, ldk, ldv, ldo = _lds(cause, Cc, ve)
    q, k, v, do = _attn_data(dtype, N, L, S, H, data, key)
    what = "attention %s N=%d L=%d S=%d H=%d staging=%s data=%s" % (dtype, N, L, S, H, cause, data)
    Q = Mat(dev, N * L, Cc, ldq, dtype, q, off=1 if cause == "q" else 0)
    K = Mat(dev, N * S, Cc, ldk, dtype, k, off=1 if cause == "k" else 0)
    V = Mat(dev, N * S, Cc, ldv, dtype, v, off=1 if cause == "v" else 0)
    DO = Mat(dev, N * L, Cc, ldo, dtype, do, off=1 if cause == "dout" else 0)
    OUT, DQ, DK, DV = Mat(dev, N * L, Cc, ldo, dtype), Mat(dev, N * L, Cc, ldq, dtype), Mat(dev, N * S, Cc, ldk, dtype), Mat(dev, N * S, Cc, ldv, dtype)
    for bwd in (False, True):
        aligned = all(m_.B.v.data_ptr() % 16 == 0 for m_ in ((Q, K, V, DO) if bwd else (Q, K, V)))
        lds_ok = all(l_ % ve == 0 for l_ in ((ldq, ldk, ldv, ldo) if bwd else (ldq, ldk, ldv)))
        assert (aligned and lds_ok) == _is_vec(cause, dtype, bwd), what + ": the case is not in the staging class it is listed under"
    _call("rd_linear_attention_fwd", Q.p, K.p, V.p, OUT.p, N, L, S, H, ldq, ldk, ldv, ldo, eps, _dt(Q.B.v), _S(Q.B.v))
    _call("rd_linear_attention_bwd", Q.p, K.p, V.p, DO.p, DQ.p, DK.p, DV.p, N, L, S, H, ldq, ldk, ldv, ldo, eps, _dt(Q.B.v), _S(Q.B.v))
    for m_ in (Q, K, V, DO):
        m_.check(what, unchanged=True)
    for m_ in (OUT, DQ, DK, DV):
        m_.check(what, unchanged=(N == 0))
    if N == 0:
        return
    r64, r32 = _attn_ref(torch.float64, q, k, v, do, N, L, S, H, eps), _attn_ref(torch.float32, q, k, v, do, N, L, S, H, eps)
    sfx = " shifted" if data.startswith("shift") else ""
    gf = "attn %s fwd%s" % ("vec" if _is_vec(cause, dtype, False) else "scalar", sfx)
    gb = "attn %s bwd%s" % ("vec" if _is_vec(cause, dtype, True) else "scalar", sfx)
    _check(what + " out", OUT.data(), r64[0], r32[0], gf)
    _check(what + " dv", DV.data(), r64[3], r32[3], gb)
    if S == 1:
        cq, ck, sq, sk = _cancel_scales(q, k, v, do, N, L, S, H, eps)
        # the hand-written backward is the one autograd computes (to float64 rounding of the cancelling terms)
        assert float((sq - r64[1]).abs().max()) <= 1e-12 * float(cq.max()) and float((sk - r64[2]).abs().max()) <= 1e-12 * float(ck.max()), what
        uq = _check_s1(what + " dq", DQ.data(), r64[1], r32[1], cq.max(), gb + " S=1")
        uk = _check_s1(what + " dk", DK.data(), r64[2], r32[2], ck.max(), gb + " S=1")
        return uq, uk
    _check(what + " dq", DQ.data(), r64[1], r32[1], gb)
    _check(what + " dk", DK.data(), r64[2], r32[2], gb)


def _attn_configs(sweeps, dtypes):
    out = []
    for dtype in dtypes:
        if "lengths" in sweeps:
            for i, L in enumerate(LENS):
                for j, S in enumerate(LENS):
                    N, H = NH[(i * len(LENS) + j) % len(NH)]
                    out.append((dtype, N, L, S, H, (None, "ldv", "k")[(i + j) % 3], "normal"))
        if "staging" in sweeps:
            for cause in CAUSES:
                for (N, H) in NH[:4]:
                    for (L, S) in ((21, 21), (16, 17), (1, 32)):
                        out.append((dtype, N, L, S, H, cause, "normal"))
        if "data" in sweeps:
            for data in DATA[1:]:
                for cause in (None, "q", "ldk"):
                    for (L, S) in ((21, 21), (17, 16), (32, 32)):
                        out.append((dtype, 2, L, S, 3, cause, data))
    return out


def _attn_feats(c):
    dtype, N, L, S, H, cause, data = c
    lt, stl = (L + 15) >> 4, (S + 15) >> 4
    return [("L", L), ("S", S), ("tiles", (lt > stl) - (lt < stl)), ("res", (N * H) % 4), ("H", H), ("cause", dtype, cause), ("data", dtype, data),
            ("blocks", N * H > 4)]


def attention_case(dev, quick=False, dtypes=DTYPES, sweeps=SWEEPS):
    """rd_linear_attention_fwd / _bwd: lengths (every pair of LENS), staging causes, data kinds (module docstring, 1).  quick: a covering
    selection, whose coverage is asserted."""
    cfgs = _cover(_attn_configs(sweeps, dtypes), _attn_feats, quick, "attn")
    if set(sweeps) == set(SWEEPS):
        seen = set(itertools.chain.from_iterable(_attn_feats(c) for c in cfgs))
        for n in LENS:
            assert ("L", n) in seen and ("S", n) in seen, n
        assert {("tiles", -1), ("tiles", 0), ("tiles", 1)} <= seen and {("res", r) for r in range(4)} <= seen and {("H", h) for h in (1, 3, 5, 8)} <= seen
        for dtype in dtypes:
            assert {("cause", dtype, c) for c in CAUSES} <= seen and {("data", dtype, d) for d in DATA} <= seen, dtype
            for bwd in (False, True):      # both staging paths for each cause that can switch them
                assert {_is_vec(c, dtype, bwd) for c in CAUSES} == {True, False}
    for c in cfgs:
        _attn_one(dev, *c)
    return len(cfgs)


def attention_edges_case(dev, quick=False):
    """N = 0 (returns 0, writes nothing), one fp16 case per staging path, and the pinned S = 1 case, which must need the cancellation rule."""
    _attn_one(dev, F32, 0, 21, 17, 3)
    _attn_one(dev, BF16, 0, 1, 32, 8, "ldq")
    used = _attn_one(dev, F32, 1, 32, 1, 1)
    assert used == (True, True), "S = 1: torch's own fp32 error on dq / dk no longer exceeds TOL * max|ref|: %s" % (used,)
    _attn_one(dev, BF16, 2, 17, 1, 3, "ldk")
    with bf16_mode("fp16"):
        _attn_one(dev, F16, 2, 21, 17, 3)
        _attn_one(dev, F16, 1, 16, 32, 5, "v")


def attention_refusals_case(dev, quick=False):
    """by return code and message only; nothing is launched with L or S outside 1..32, and the outputs come back unchanged"""
    N, L, S, H = 1, 4, 4, 1
    q, k, v, do = _attn_data(F32, N, L, S, H, "normal", "refuse")
    Q, K, V, DO = (Mat(dev, 4, 16, 16, F32, a) for a in (q, k, v, do))
    outs = [Mat(dev, 4, 16, 16, F32) for _ in range(4)]
    OUT, DQ, DK, DV = outs
    st, dt = _S(Q.B.v), _dt(Q.B.v)
    for (l_, s_) in ((0, 4), (4, 0), (33, 4), (4, 33), (-1, 4)):
        _refused("rd_linear_attention_fwd", "L,S must be in 1..32", Q.p, K.p, V.p, OUT.p, N, l_, s_, H, 16, 16, 16, 16, EPS_A, dt, st)
        _refused("rd_linear_attention_bwd", "L,S must be in 1..32", Q.p, K.p, V.p, DO.p, DQ.p, DK.p, DV.p, N, l_, s_, H, 16, 16, 16, 16, EPS_A, dt, st)
    fa = [Q.p, K.p, V.p, OUT.p]
    for i in range(4):
        a = list(fa); a[i] = None
        _refused("rd_linear_attention_fwd", "linear_attention_fwd: bad args", *(a + [N, L, S, H, 16, 16, 16, 16, EPS_A, dt, st]))
    ba = [Q.p, K.p, V.p, DO.p, DQ.p, DK.p, DV.p]
    for i in range(7):
        a = list(ba); a[i] = None
        _refused("rd_linear_attention_bwd", "linear_attention_bwd: bad args", *(a + [N, L, S, H, 16, 16, 16, 16, EPS_A, dt, st]))
    for bad in (3, -1, 99):
        _refused("rd_linear_attention_fwd", "linear_attention_fwd: bad args", *(fa + [N, L, S, H, 16, 16, 16, 16, EPS_A, bad, st]))
        _refused("rd_linear_attention_bwd", "linear_attention_bwd: bad args", *(ba + [N, L, S, H, 16, 16, 16, 16, EPS_A, bad, st]))
    for m_ in (Q, K, V, DO) + tuple(outs):
        m_.check("refused attention", unchanged=True)


# ---------------------------------------------------------------------------------------------------------------- 2. fused LoFTR layer
SELF_SHAPES = ((2, 21), (1, 32), (1, 1), (3, 16), (1, 17))                                      # (N, L)
CROSS_LS = ((21, 21), (7, 30), (30, 7), (32, 1), (1, 32), (16, 17), (17, 16))
KINDS = ("self", "cross")
SAVED = ("q", "k", "v", "att", "mpre", "msg", "hid", "m2pre", "stats")
GRADS = ("dm2pre", "dhid", "dmpre", "datt", "dq", "dk", "dv", "dx", "dsrc")
WNAMES = ("wq", "wk", "wv", "wm", "w0", "w2")


def _rnd(z, dtype):
    return z if dtype == F32 else z.to(dtype).to(z.dtype)


def _tie_ulp(z64, z32, dtype):
    """one ulp of the 16-bit type at |z| where z lies within the fp32 bound (of z) of a rounding tie, else 0 (fp32: 0 everywhere)"""
    if dtype == F32:
        return torch.zeros_like(z64)
    hz = _half_ulp(dtype, z64)
    near = (hz - (z64 - z64.to(dtype).double()).abs()) <= _fp32_bound(z64.reshape(-1), z32.reshape(-1))[0]
    return torch.where(near, 2.0 * hz, torch.zeros_like(hz))


def _check_ties(what, got, ref64, ref32, extra, group):
    """_check plus `extra` (>= 0, element-wise): what flipped ties of an unstored rounded intermediate may add (module docstring, 2)"""
    if float(extra.max()) == 0.0:
        return _check(what, got, ref64, ref32, group)
    g = got.detach().cpu()
    out_dt = g.dtype
    g, r = g.double().reshape(-1), ref64.double().reshape(-1)
    assert g.shape == r.shape and bool(torch.isfinite(g).all()), what + ": shape / non-finite values"
    bound, ref_err, m = _fp32_bound(r, ref32.reshape(-1))
    diff = (g - r).abs()
    err = float(diff.max())
    if m > 0:
        cur = MEASURED.setdefault(group + (" 16-bit" if out_dt != F32 else ""), [0.0, 0.0])
        cur[0] = max(cur[0], ref_err / m); cur[1] = max(cur[1], err / m)
    assert bool((diff <= bound + _half_ulp(out_dt, r) + extra.reshape(-1)).all()), \
        "%s: kernel error %.3e, torch fp32's own error %.3e, fp32 bound %.3e (+ half an ulp of %s, + one ulp of the intermediate on %d near-ties)" % (
            what, err, ref_err, bound, out_dt, int((extra > 0).sum()))


def _ln_fwd(pre, g, b):
    mu = pre.mean(1, keepdim=True)
    d = pre - mu
    rs = 1.0 / torch.sqrt((d * d).mean(1, keepdim=True) + EPS_LN)
    return mu[:, 0], rs[:, 0], d * rs * g + b


def _ln_bwd(d, pre, mu, rs, gamma, N):
    """LayerNorm backward from the saved statistics, as documented above ln_bwd in rd_loftr.hip: -> (dpre, lnp [N][C][2] = per-sequence
    (sum d, sum d * xhat), xhat, rs)"""
    xh = (pre - mu[:, None]) * rs[:, None]
    g = d * gamma
    s1, s2 = g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)
    o = rs[:, None] * (g - s1 - xh * s2)
    lnp = torch.stack([d.view(N, -1, C).sum(1), (d * xh).view(N, -1, C).sum(1)], dim=2)
    return o, lnp, xh


def _attn128(q, k, v, N, L, S, datt=None):
    q_, k_, v_ = [a.view(N, -1, HEADS, 16).clone().requires_grad_(datt is not None) for a in (q, k, v)]
    out = O.linear_attention(q_, k_, v_, EPS_A)
    if datt is None:
        return out.reshape(N * L, C)
    out.backward(datt.view(N, L, HEADS, 16))
    return [a.reshape(-1, C) for a in (q_.grad, k_.grad, v_.grad)]


def _fused_data(dtype, kind, N, L, S, dead, key):
    rs = _rs("loftr", str(dtype), kind, N, L, S, dead, key)
    W = {n: _r(_randn(rs, C, C) / C ** 0.5, dtype) for n in WNAMES[:4]}
    W["w0"], W["w2"] = _r(_randn(rs, C2, C2) / 16.0, dtype), _r(_randn(rs, C, C2) / 16.0, dtype)
    ln = dict(g1=1.0 + 0.3 * _randn(rs, C), b1=0.2 * _randn(rs, C), g2=1.0 + 0.3 * _randn(rs, C), b2=0.2 * _randn(rs, C))
    x = _randn(rs, N * L, C)
    if dead:      # message > 0 everywhere (|LayerNorm| <= sqrt(127), |g1| <= 0.0045), W0 <= 0, x row 0 >= 0: the whole row 0 of hid is <= 0
        ln["g1"], ln["b1"] = (0.001 * _randn(rs, C)).clamp(-0.0045, 0.0045), 0.1 + 0.05 * _randn(rs, C).abs()
        W["w0"] = -W["w0"].abs()
        x[0] = x[0].abs()
    x = _r(x, dtype)
    src = x if kind == "self" else _r(_randn(rs, N * S, C), dtype)
    return W, ln, x, src, _r(_randn(rs, N * L, C), dtype), _r(_randn(rs, N * S, C), dtype), [_randn(rs, C) for _ in range(4)]


def _rows_buf(dev, rows, cols, dtype, init=None):
    """(rows + EXTRA) x cols, NaN (or `init` in the first rows)"""
    full = torch.full((rows + EXTRA, cols), NAN)
    if init is not None:
        full[:rows] = init
    return Buf(dev, full.numel(), dtype, full)


def _rows_of(b, rows, cols, what):
    """the first `rows` rows as fp32 CPU values; the EXTRA rows behind them must be untouched"""
    a, s = _bits(b.v).cpu().view(-1, cols), _bits(b.snap[b.lo:b.hi]).cpu().view(-1, cols)
    assert torch.equal(a[rows:], s[rows:]), what + ": rows behind the last sequence were overwritten"
    b.check(what)
    return b.v.detach().cpu().view(-1, cols)[:rows]


def _wstruct(Wd, lnd, mode, dt):
    from riders_amd import _lib
    w = _lib.LoftrWeights()
    packs = [_E().packed_weight(Wd[n], mode, dt) for n in WNAMES]
    w.wq, w.wk, w.wv, w.wm, w.w0, w.w2 = [b.data_ptr() for b in packs]
    w.g1, w.b1, w.g2, w.b2 = [lnd[n].v.data_ptr() for n in ("g1", "b1", "g2", "b2")]
    return w, packs


def _mm(a, w):
    """a . w^T.  float64: torch.  fp32: the yardstick of the token GEMMs, a restatement of the documented chain (tok_mma: one accumulator per
    output element through K / 4 dependent MFMA steps, k ascending) at its least accurate reading -- every product and every addition
    rounded to fp32, one k after the other -- NOT torch's blocked fp32 matmul, which a correct sequential chain over K = 256 does not match
    to 4 ulp (module docstring, "Finding 2")."""
    if a.dtype == torch.float64:
        return a @ w.t()
    an, wn = a.numpy(), w.numpy()
    acc = np.zeros((an.shape[0], wn.shape[0]), np.float32)
    for k in range(an.shape[1]):
        acc = acc + an[:, k:k + 1] * wn[None, :, k]
    return torch.from_numpy(acc)


def _fwd_stage_refs(dt, dtype, W, ln, x, src, st, N, L, S):
    Wt = {n: W[n].to(dt) for n in W}
    g = {n: ln[n].to(dt) for n in ln}
    x, src = x.to(dt), src.to(dt)
    s = {n: st[n].to(dt) for n in st}
    p = dict(q=_mm(x, Wt["wq"]), k=_mm(src, Wt["wk"]), v=_mm(src, Wt["wv"]))
    p["att"] = _attn128(s["q"], s["k"], s["v"], N, L, S)
    p["mpre"] = _mm(s["att"], Wt["wm"])
    p["mu1"], p["rs1"], p["msg"] = _ln_fwd(s["mpre"], g["g1"], g["b1"])
    p["hid"] = torch.relu(_mm(torch.cat([x, s["msg"]], 1), Wt["w0"]))
    p["m2pre"] = _mm(s["hid"], Wt["w2"])
    p["mu2"], p["rs2"], y2 = _ln_fwd(s["m2pre"], g["g2"], g["b2"])
    p["out"] = x + y2
    return p


def _bwd_stage_refs(dt, dtype, W, ln, kind, dout, prev, st, gs, N, L, S, dacc, rounded=None):
    """rounded: the 16-bit values of the unstored intermediates as the float64 pass rounded them.  The fp32 yardstick of a 16-bit case takes
    them over (they are exact in fp32), so that its error is that of the fp32 arithmetic and a tie that IT rounds the other way does not
    inflate the bound of the whole tensor; what the kernel's own ties may add is `_tie_ulp`'s business.  fp32 cases round nothing."""
    Wt = {n: W[n].to(dt) for n in W}
    g = {n: ln[n].to(dt) for n in ln}
    s = {n: st[n].to(dt) for n in st}
    d = {n: gs[n].to(dt) for n in gs}
    dout = dout.to(dt)
    p = {}
    p["dm2pre"], p["lnp2"], _ = _ln_bwd(dout, s["m2pre"], s["stats"][:, 2], s["stats"][:, 3], g["g2"], N)
    WT = {n: Wt[n].t().contiguous() for n in Wt}      # the backward's GEMMs contract over the output channels
    p["dhid"] = _mm(d["dm2pre"], WT["w2"]) * (s["hid"] > 0).to(dt)
    p["zcat"] = _mm(d["dhid"], WT["w0"])
    p["datt"] = _mm(d["dmpre"], WT["wm"])
    p["dq"], p["dk"], p["dv"] = _attn128(s["q"], s["k"], s["v"], N, L, S, d["datt"])
    p["zq"], p["zk"], p["zv"] = _mm(d["dq"], WT["wq"]), _mm(d["dk"], WT["wk"]), _mm(d["dv"], WT["wv"])
    if rounded is not None and dtype != F32:
        r = {n: rounded[n].to(dt) for n in rounded}
    else:
        r = {n: _rnd(p[n], dtype) for n in ("zcat", "zq", "zk", "zv")}
    p["rounded"] = r
    p["dmpre"], p["lnp1"], p["xh1"] = _ln_bwd(r["zcat"][:, C:], s["mpre"], s["stats"][:, 0], s["stats"][:, 1], g["g1"], N)
    p["dx"] = dout + r["zcat"][:, :C] + r["zq"]
    if kind == "self":
        p["dx"] = p["dx"] + r["zk"] + r["zv"]
    else:
        p["dsrc"] = r["zk"] + r["zv"]
        if dacc:
            p["dsrc"] = p["dsrc"] + prev.to(dt)
    return p


def _e2e_refs(dt, W, ln, kind, x, src, dout, N, L, S):
    sd = {"q_proj.weight": W["wq"], "k_proj.weight": W["wk"], "v_proj.weight": W["wv"], "merge.weight": W["wm"], "mlp.0.weight": W["w0"],
          "mlp.2.weight": W["w2"], "norm1.weight": ln["g1"], "norm1.bias": ln["b1"], "norm2.weight": ln["g2"], "norm2.bias": ln["b2"]}
    sd = {k_: v_.to(dt).clone().requires_grad_(k_.startswith("norm")) for k_, v_ in sd.items()}
    x_ = x.to(dt).view(N, L, C).clone().requires_grad_()
    s_ = x_ if kind == "self" else src.to(dt).view(N, S, C).clone().requires_grad_()
    out = O.loftr_layer(x_, s_, sd, "")
    out.backward(dout.to(dt).view(N, L, C))
    return dict(out=out.detach().reshape(-1, C), dx=x_.grad.reshape(-1, C), dsrc=None if kind == "self" else s_.grad.reshape(-1, C),
                dg1=sd["norm1.weight"].grad, db1=sd["norm1.bias"].grad, dg2=sd["norm2.weight"].grad, db2=sd["norm2.bias"].grad)


def _fused_one(dev, dtype, kind, N, L, S, defer_ln=1, accumulate=0, dacc=0, dead=False, key=0):
    from riders_amd import _lib
    ML, MS = N * L, N * S
    W, ln, x, src, dout, prev, lnprev = _fused_data(dtype, kind, N, L, S, dead, key)
    what = "loftr %s %s N=%d L=%d S=%d defer_ln=%d accumulate=%d dsrc_accumulate=%d%s" % (dtype, kind, N, L, S, defer_ln, accumulate, dacc, " dead-row" if dead else "")
    Wd = {n: W[n].to(dev) for n in W}
    lnd = {n: Buf(dev, C, F32, ln[n]) for n in ln}
    X = Buf(dev, ML * C, dtype, x)
    SRC = X if kind == "self" else Buf(dev, MS * C, dtype, src)
    DOUT = Buf(dev, ML * C, dtype, dout)
    dt, st_ = _dt(X.v), _S(X.v)
    # out: rows [2, 2 + ML) of a larger matrix
    OUTM = _nanbuf(dev, (2 + ML + EXTRA) * C, dtype)
    out_v = OUTM.v[2 * C:(2 + ML) * C]
    rows = dict(q=ML, k=MS, v=MS, att=ML, mpre=ML, msg=ML, hid=ML, m2pre=ML, stats=ML, dm2pre=ML, dhid=ML, dmpre=ML, datt=ML, dq=ML, dk=MS, dv=MS, dx=ML, dsrc=MS)
    cols = dict(hid=C2, dhid=C2, stats=4)
    SV = {n: _rows_buf(dev, rows[n], cols.get(n, C), F32 if n == "stats" else dtype) for n in SAVED}
    sv = _lib.LoftrSaved()
    for n in SAVED:
        setattr(sv, n, SV[n].v.data_ptr())
    wf, keep_f = _wstruct(Wd, lnd, 0, dt)
    _call("rd_loftr_layer_fwd", _P(X.v), _P(SRC.v), ctypes.byref(wf), _P(out_v), ctypes.byref(sv), N, L, S, EPS_A, EPS_LN, dt, st_)
    st = {n: _rows_of(SV[n], rows[n], cols.get(n, C), what + " " + n).float() for n in SAVED}
    OUTM.check(what + " out")
    om, os_ = _bits(OUTM.v).cpu().view(-1, C), _bits(OUTM.snap[OUTM.lo:OUTM.hi]).cpu().view(-1, C)
    assert torch.equal(om[:2], os_[:2]) and torch.equal(om[2 + ML:], os_[2 + ML:]), what + ": rows of the larger matrix around `out` were overwritten"
    out = out_v.detach().cpu().view(ML, C)
    p64, p32 = [_fwd_stage_refs(t_, dtype, W, ln, x, src, st, N, L, S) for t_ in (torch.float64, torch.float32)]
    for n in ("q", "k", "v", "att", "mpre", "msg", "hid", "m2pre"):
        _check("%s %s" % (what, n), SV[n].v.view(-1, cols.get(n, C))[:rows[n]], p64[n], p32[n], "loftr fwd " + n)
    for i, n in enumerate(("mu1", "rs1", "mu2", "rs2")):
        _check("%s stats %s" % (what, n), st["stats"][:, i], p64[n], p32[n], "loftr fwd stats")
    _check(what + " out", out_v.view(ML, C), p64["out"], p32["out"], "loftr fwd out")
    if dead:
        assert float(st["hid"][0].abs().max()) == 0.0 and float(st["hid"][1:].max()) > 0.0, what + ": the case has no dead row of hid beside live ones"

    # ---- backward (the saved tensors are its inputs from here on)
    for b_ in SV.values():
        b_.snap = b_.full.clone()
    GR ={n: _rows_buf(dev, rows[n], cols.get(n, C), dtype, prev if (n == "dsrc" and dacc) else None) for n in GRADS if not (n == "dsrc" and kind == "self")}
    LNP = [_nanbuf(dev, N * C * 2, F32), _nanbuf(dev, N * C * 2, F32)]
    DGB = [Buf(dev, C, F32, a) for a in lnprev]      # dg1, db1, dg2, db2 (previous contents)
    gr = _lib.LoftrGrads()
    gr.dout = DOUT.v.data_ptr()
    for n in GR:
        setattr(gr, n, GR[n].v.data_ptr())
    gr.dsrc = GR["dsrc"].v.data_ptr() if "dsrc" in GR else 0
    gr.lnp1, gr.lnp2 = LNP[0].v.data_ptr(), LNP[1].v.data_ptr()
    gr.dg1, gr.db1, gr.dg2, gr.db2 = [b.v.data_ptr() for b in DGB]
    gr.accumulate, gr.defer_ln, gr.dsrc_accumulate = accumulate, defer_ln, dacc
    wb, keep_b = _wstruct(Wd, lnd, 1, dt)
    _call("rd_loftr_layer_bwd", _P(X.v), _P(SRC.v), ctypes.byref(wb), ctypes.byref(sv), ctypes.byref(gr), N, L, S, EPS_A, dt, st_)
    for b_ in [X, SRC, DOUT] + list(lnd.values()) + list(SV.values()):
        b_.check(what + " (input of the backward)", unchanged=True)
    gs = {n: _rows_of(GR[n], rows[n], cols.get(n, C), what + " " + n).float() for n in GR}
    b64 = _bwd_stage_refs(torch.float64, dtype, W, ln, kind, dout, prev, st, gs, N, L, S, dacc)
    b32 = _bwd_stage_refs(torch.float32, dtype, W, ln, kind, dout, prev, st, gs, N, L, S, dacc, rounded=b64["rounded"])
    got = lambda n: GR[n].v.view(-1, cols.get(n, C))[:rows[n]]      # noqa: E731
    for n in ("dm2pre", "dhid", "datt", "dv"):
        _check("%s %s" % (what, n), got(n), b64[n], b32[n], "loftr bwd " + n)
    if S == 1:
        cq, ck, _, _ = _cancel_scales(st["q"], st["k"], st["v"], gs["datt"], N, L, S, HEADS, EPS_A)
        _check_s1(what + " dq", got("dq"), b64["dq"], b32["dq"], cq.max(), "loftr bwd dq S=1")
        _check_s1(what + " dk", got("dk"), b64["dk"], b32["dk"], ck.max(), "loftr bwd dk S=1")
    else:
        _check(what + " dq", got("dq"), b64["dq"], b32["dq"], "loftr bwd dq")
        _check(what + " dk", got("dk"), b64["dk"], b32["dk"], "loftr bwd dk")
    # stages behind an unstored rounded intermediate: near-tie allowance (module docstring, 2)
    tc = _tie_ulp(b64["zcat"], b32["zcat"], dtype)
    tq, tk, tv = (_tie_ulp(b64[n], b32[n], dtype) for n in ("zq", "zk", "zv"))
    rs1, xh = st["stats"][:, 1].double()[:, None], b64["xh1"].abs()
    w_ = tc[:, C:] * ln["g1"].double().abs()
    ex_dmpre = rs1 * (w_ + w_.mean(1, keepdim=True) + xh * (w_ * xh).mean(1, keepdim=True))
    ex_lnp1 = torch.stack([tc[:, C:].view(N, L, C).sum(1), (tc[:, C:] * xh).view(N, L, C).sum(1)], dim=2)
    _check_ties(what + " dmpre", got("dmpre"), b64["dmpre"], b32["dmpre"], ex_dmpre, "loftr bwd dmpre")
    lnp1, lnp2 = LNP[0].cpu().view(N, C, 2), LNP[1].cpu().view(N, C, 2)
    for n_ in range(N):      # per sequence
        _check_ties("%s lnp1[%d]" % (what, n_), lnp1[n_], b64["lnp1"][n_], b32["lnp1"][n_], ex_lnp1[n_], "loftr bwd lnp")
        _check("%s lnp2[%d]" % (what, n_), lnp2[n_], b64["lnp2"][n_], b32["lnp2"][n_], "loftr bwd lnp")
    ex_dx = tc[:, :C] + tq + ((tk + tv) if kind == "self" else 0.0)
    _check_ties(what + " dx", got("dx"), b64["dx"], b32["dx"], ex_dx, "loftr bwd dx")
    if kind == "cross":
        _check_ties(what + " dsrc", got("dsrc"), b64["dsrc"], b32["dsrc"], tk + tv, "loftr bwd dsrc")
    for b_ in LNP:
        b_.check(what + " lnp")
    # LayerNorm parameter gradients: the float64 sum of the kernel's own partials over N (on top of the previous contents when accumulating)
    for i, (b_, part, col) in enumerate(((DGB[0], lnp1, 1), (DGB[1], lnp1, 0), (DGB[2], lnp2, 1), (DGB[3], lnp2, 0))):
        name = ("dg1", "db1", "dg2", "db2")[i]
        if defer_ln:
            b_.check("%s %s (defer_ln)" % (what, name), unchanged=True)
            continue
        b_.check("%s %s" % (what, name))
        base = lnprev[i] if accumulate else torch.zeros(C)
        r64 = part[:, :, col].double().sum(0) + base.double()
        r32 = part[:, :, col].sum(0) + base
        _check("%s %s" % (what, name), b_.v, r64, r32, "loftr bwd ln params")

    # ---- end to end, fp32 only: two stages agreeing on a wrong convention would pass everything above
    if dtype == F32:
        e64, e32 = [_e2e_refs(t_, W, ln, kind, x, src, dout, N, L, S) for t_ in (torch.float64, torch.float32)]
        _check(what + " e2e out", out, e64["out"], e32["out"], "loftr e2e out")
        _check(what + " e2e dx", gs["dx"], e64["dx"], e32["dx"], "loftr e2e dx")
        if kind == "cross":
            add = prev if dacc else torch.zeros_like(prev)
            _check(what + " e2e dsrc", gs["dsrc"], e64["dsrc"] + add.double(), e32["dsrc"] + add, "loftr e2e dsrc")
        for name, part, col in (("dg1", lnp1, 1), ("db1", lnp1, 0), ("dg2", lnp2, 1), ("db2", lnp2, 0)):
            _check("%s e2e %s" % (what, name), part[:, :, col].double().sum(0).float(), e64[name], e32[name], "loftr e2e ln params")


def _fused_configs(kinds, dtypes):
    out = []
    for dtype in dtypes:
        if "self" in kinds:
            for (N, L) in SELF_SHAPES:
                for defer_ln, acc in itertools.product((0, 1), (0, 1)):
                    out.append((dtype, "self", N, L, L, defer_ln, acc, 0))
        if "cross" in kinds:
            for (L, S) in CROSS_LS:
                for N in (1, 3):
                    for defer_ln, acc, dacc in itertools.product((0, 1), (0, 1), (0, 1)):
                        out.append((dtype, "cross", N, L, S, defer_ln, acc, dacc))
    return out


def _fused_feats(c):
    dtype, kind, N, L, S, defer_ln, acc, dacc = c
    return [("shape", kind, L, S), ("N", kind, N), ("flags", kind, defer_ln, acc, dacc), ("dtype", dtype, kind), ("flags16", dtype, dacc, defer_ln)]


def fused_case(dev, quick=False, dtypes=DTYPES, kinds=KINDS):
    """rd_loftr_layer_fwd / _bwd stage by stage (module docstring, 2): every self and cross shape, every (defer_ln, accumulate, dsrc_accumulate);
    quick: a covering selection, whose coverage is asserted; and one case in which a whole row of hid is <= 0"""
    cfgs = _cover(_fused_configs(kinds, dtypes), _fused_feats, quick, "loftr")
    seen = set(itertools.chain.from_iterable(_fused_feats(c) for c in cfgs))
    if "self" in kinds:
        assert {("shape", "self", L, L) for _, L in SELF_SHAPES} <= seen and {("flags", "self", d_, a_, 0) for d_ in (0, 1) for a_ in (0, 1)} <= seen
    if "cross" in kinds:
        assert {("shape", "cross", L, S) for L, S in CROSS_LS} <= seen and {("N", "cross", 1), ("N", "cross", 3)} <= seen
        assert {("flags", "cross", d_, a_, s_) for d_ in (0, 1) for a_ in (0, 1) for s_ in (0, 1)} <= seen
    for dtype in dtypes:
        assert {("dtype", dtype, k_) for k_ in kinds} <= seen
    for c in cfgs:
        _fused_one(dev, *c)
    for dtype in dtypes:
        if "cross" in kinds:
            _fused_one(dev, dtype, "cross", 2, 21, 21, 1, 0, 1, dead=True)
        else:
            _fused_one(dev, dtype, "self", 2, 17, 17, 0, 0, 0, dead=True)
    return len(cfgs)


def fused_refusals_case(dev, quick=False):
    """L or S of 0 / 33, every null weight, saved buffer and gradient buffer, dsrc null with src != x, a self layer with dsrc_accumulate: refused
    by return code and message, nothing launched, every buffer unchanged"""
    from riders_amd import _lib
    N, L, S = 1, 2, 2
    W, ln, x, src, dout, prev, lnprev = _fused_data(F32, "cross", N, L, S, False, "refuse")
    Wd = {n: W[n].to(dev) for n in W}
    lnd = {n: Buf(dev, C, F32, ln[n]) for n in ln}
    X, SRC, DOUT, OUT = Buf(dev, L * C, F32, x), Buf(dev, S * C, F32, src), Buf(dev, L * C, F32, dout), _nanbuf(dev, L * C, F32)
    SV = {n: _nanbuf(dev, 2 * (C2 if n == "hid" else 4 if n == "stats" else C), F32) for n in SAVED}
    GR = {n: _nanbuf(dev, 2 * (C2 if n == "dhid" else C), F32) for n in GRADS}
    LN = {n: _nanbuf(dev, N * C * 2 if n.startswith("lnp") else C, F32) for n in ("lnp1", "lnp2", "dg1", "db1", "dg2", "db2")}
    dt, st_ = _dt(X.v), _S(X.v)
    wf, keep = _wstruct(Wd, lnd, 0, dt)

    def saved(skip=None):
        sv = _lib.LoftrSaved()
        for n in SAVED:
            setattr(sv, n, None if n == skip else SV[n].v.data_ptr())
        return sv

    def grads(skip=None, dacc=0):
        gr = _lib.LoftrGrads()
        gr.dout = None if skip == "dout" else DOUT.v.data_ptr()
        for n in GRADS:
            setattr(gr, n, None if n == skip else GR[n].v.data_ptr())
        for n in LN:
            setattr(gr, n, None if n == skip else LN[n].v.data_ptr())
        gr.accumulate, gr.defer_ln, gr.dsrc_accumulate = 0, 1, dacc
        return gr

    def weights(skip=None):
        w = _lib.LoftrWeights()
        for n in WNAMES + ("g1", "b1", "g2", "b2"):
            setattr(w, n, None if n == skip else getattr(wf, n))
        return w

    def fwd(w, sv, l_=L, s_=S, x_=X, dtype=dt):
        return ("rd_loftr_layer_fwd", _P(x_.v), _P(SRC.v), ctypes.byref(w), _P(OUT.v), ctypes.byref(sv), N, l_, s_, EPS_A, EPS_LN, dtype, st_)

    def bwd(w, sv, gr, l_=L, s_=S, src_=SRC, dtype=dt):
        return ("rd_loftr_layer_bwd", _P(X.v), _P(src_.v), ctypes.byref(w), ctypes.byref(sv), ctypes.byref(gr), N, l_, s_, EPS_A, dtype, st_)

    for (l_, s_) in ((0, 2), (2, 0), (33, 2), (2, 33)):
        a = fwd(weights(), saved(), l_, s_)
        _refused(a[0], "1..32 tokens", *a[1:])
        a = bwd(weights(), saved(), grads(), l_, s_)
        _refused(a[0], "1..32 tokens", *a[1:])
    for bad in (3, -1):
        a = fwd(weights(), saved(), dtype=bad)
        _refused(a[0], "bad dtype", *a[1:])
        a = bwd(weights(), saved(), grads(), dtype=bad)
        _refused(a[0], "bad dtype", *a[1:])
    for n in WNAMES + ("g1", "b1", "g2", "b2"):
        a = fwd(weights(n), saved())
        _refused(a[0], "null weight", *a[1:])
        if n not in ("b1", "b2"):      # (the backward does not read the LayerNorm biases)
            a = bwd(weights(n), saved(), grads())
            _refused(a[0], "null weight", *a[1:])
    for n in SAVED:
        a = fwd(weights(), saved(n))
        _refused(a[0], "null saved buffer", *a[1:])
        if n not in ("att", "msg"):    # (inputs of the weight gradients only: the backward kernel does not read them)
            a = bwd(weights(), saved(n), grads())
            _refused(a[0], "null saved buffer", *a[1:])
    for n in ("dout",) + GRADS:
        a = bwd(weights(), saved(), grads(n))
        _refused(a[0], "null gradient buffer", *a[1:])
    for n in LN:
        a = bwd(weights(), saved(), grads(n))
        _refused(a[0], "null LayerNorm gradient buffer", *a[1:])
    a = bwd(weights(), saved(), grads(dacc=1), src_=X)
    _refused(a[0], "dsrc_accumulate is for cross attention", *a[1:])
    for b_ in [X, SRC, DOUT, OUT] + list(lnd.values()) + list(SV.values()) + list(GR.values()) + list(LN.values()):
        b_.check("refused loftr layer", unchanged=True)


# ---------------------------------------------------------------------------------------------------------------- 4. module routes
ROUTES = ("default", "unmerged", "no_cross_inplace", "no_defer_wgrad", "cross_7_30", "unfused_7_30")
# bit-equal with the default route: "io" = outputs and input gradients, "all" = the parameter gradients too (module docstring, 4)
ROUTE_EXACT = {"unmerged": "io", "no_cross_inplace": "all", "no_defer_wgrad": "io"}


def _tf_inputs(L, S, N=2):
    rs = _rs("tf routes", L, S)
    return _randn(rs, N, L, C), _randn(rs, N, S, C), _randn(rs, N, L, C), _randn(rs, N, S, C)


def _tf_oracle(dt, sd, a, b, w0, w1, n_layers):
    sd = {k_: v_.detach().to(dt).clone().requires_grad_() for k_, v_ in sd.items()}
    a_, b_ = a.to(dt).clone().requires_grad_(), b.to(dt).clone().requires_grad_()
    r0, r1 = O.local_feature_transformer(a_, b_, sd, "", ("self", "cross") * n_layers)
    ((r0 * w0.to(dt)).sum() + (r1 * w1.to(dt)).sum()).backward()
    res = {"out0": r0.detach(), "out1": r1.detach(), "da": a_.grad, "db": b_.grad}
    res.update({"grad " + k_: v_.grad for k_, v_ in sd.items()})
    return res


def _tf_run(dev, route, a, b, w0, w1, n_layers):
    from riders_amd.linear_attention import LocalFeatureTransformer
    from tests.golden.fill import fill_state_dict
    E = _E()
    keep = {k_: E._state.get(k_, True) for k_ in ("merge_self_layers", "loftr_cross_inplace", "defer_wgrad", "fused_loftr")}
    try:
        if route == "unmerged":
            E._state["merge_self_layers"] = False
        elif route == "no_cross_inplace":
            E._state["loftr_cross_inplace"] = False
        elif route == "no_defer_wgrad":
            E.set_defer_wgrad(False)
        elif route == "unfused_7_30":
            E.set_fused_loftr(False)
        m = LocalFeatureTransformer(["self", "cross"], n_layers=n_layers, d_model=C).to(dev)
        sd = fill_state_dict(m, "attn.routes")
        ad, bd = a.to(dev).requires_grad_(), b.to(dev).requires_grad_()
        o0, o1 = m(ad, bd)
        ((o0 * w0.to(dev)).sum() + (o1 * w1.to(dev)).sum()).backward()
        res = {"out0": o0.detach().cpu(), "out1": o1.detach().cpu(), "da": ad.grad.cpu(), "db": bd.grad.cpu()}
        res.update({"grad " + k_: p.grad.detach().cpu() for k_, p in m.named_parameters()})
        return res, sd
    finally:
        for k_, v_ in keep.items():
            E._state[k_] = v_


_TF_CACHE = {}


def _tf_refs(L, S, sd, n_layers):
    """the float64 and fp32 oracle results, computed once per shape and left unchanged"""
    if (L, S, n_layers) not in _TF_CACHE:
        a, b, w0, w1 = _tf_inputs(L, S)
        _TF_CACHE[(L, S, n_layers)] = (_tf_oracle(torch.float64, sd, a, b, w0, w1, n_layers), _tf_oracle(torch.float32, sd, a, b, w0, w1, n_layers))
    return _TF_CACHE[(L, S, n_layers)]


def routes_case(dev, quick=False, routes=ROUTES):
    """LocalFeatureTransformer over its routes (module docstring, 4).  quick (the emulator twin, where a route costs half a minute per
    layer pair): one ('self', 'cross') pair instead of two."""
    default, n_layers = None, 1 if quick else 2
    for route in routes:
        L, S = (7, 30) if route.endswith("7_30") else (21, 21)
        a, b, w0, w1 = _tf_inputs(L, S)
        res, sd = _tf_run(dev, route, a, b, w0, w1, n_layers)
        r64, r32 = _tf_refs(L, S, sd, n_layers)
        assert set(res) == set(r64)
        for k_ in sorted(res):
            _check("transformer route %s: %s" % (route, k_), res[k_], r64[k_], r32[k_], "tf " + ("param grads" if k_.startswith("grad") else "outputs and input grads"))
        if route in ROUTE_EXACT:
            if default is None:
                default = _tf_run(dev, "default", a, b, w0, w1, n_layers)[0]
            for k_ in sorted(res):
                if ROUTE_EXACT[route] == "all" or not k_.startswith("grad"):
                    _exact("transformer route %s against the default route: %s" % (route, k_), res[k_], default[k_])
        if route == "default":
            default = res


def too_long_case(dev, quick=False):
    """L = 33 raises the library's 1..32 error and returns no tensor"""
    from riders_amd.linear_attention import LocalFeatureTransformer
    m = LocalFeatureTransformer(["self", "cross"], n_layers=1, d_model=C).to(dev)
    a, b = torch.zeros(1, 33, C, device=dev), torch.zeros(1, 33, C, device=dev)
    res = None
    try:
        res = m(a, b)
    except Exception as e:      # noqa: BLE001
        assert "1..32" in str(e), "L = 33: expected the library's 1..32 error, got %r" % (e,)
    assert res is None, "L = 33 returned a tensor"
