"""Pin tests/ref_full_attn.py (the torch restatement of softmax attention and of the token masks) against vectors the reference itself produced
in float64: tests/golden/g20_full_attention.npz, written by tests/golden/make_golden_full_attn.py, whose `recipe()` regenerates the inputs.
Every result array is stored as its flattened elements STRIDE apart (see the generator).  Bound: 1e-12 of max|reference|, float64."""
import os

import numpy as np
import pytest
import torch

from tests import ref_full_attn as R
from tests.golden.fill import fill_state_dict
from tests.golden.make_golden_full_attn import STRIDE, recipe

G = os.path.join(os.path.dirname(__file__), "golden", "g20_full_attention.npz")
TOL = 1e-12


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(G))


@pytest.fixture(scope="module")
def rec():
    return recipe()


def close(what, got, ref):
    g = got.detach().double().reshape(-1)[::STRIDE].numpy()
    assert g.shape == ref.shape, (what, g.shape, ref.shape)
    err, m = float(np.abs(g - ref).max()), float(np.abs(ref).max())
    print("%-28s error %.3e of max|ref| %.3e" % (what, err / max(m, 1e-300), m))
    assert np.isfinite(g).all() and err <= TOL * m, "%s: error %.3e, max|ref| %.3e" % (what, err, m)


def leaves(sd):
    return {k: v.double().clone().requires_grad_() for k, v in sd.items()}


def check_grads(gold, prefix, sd):
    n = 0
    for k, v in sd.items():
        ref_n = float(gold[prefix + k + "|norm"][0])
        g = v.grad.reshape(-1)
        assert abs(float(g.norm()) - ref_n) <= TOL * ref_n, (k, float(g.norm()), ref_n)
        head = gold[prefix + k + "|head"]
        assert float(np.abs(g[:16].numpy() - head).max()) <= TOL * max(float(g.abs().max()), ref_n), k
        n += 1
    assert n > 0


@pytest.mark.parametrize("case", ["a", "b", "d"])
def test_attention(gold, rec, case):
    c = rec[case]
    q, k, v = [c[n].clone().requires_grad_() for n in "qkv"]
    fn = R.linear_attention if case == "d" else R.full_attention
    out = fn(q, k, v, q_mask=c.get("q_mask"), kv_mask=c.get("kv_mask"))
    (out * c["w"]).sum().backward()
    for n, a in (("out", out), ("dq", q.grad), ("dk", k.grad), ("dv", v.grad)):
        close("%s.%s" % (case, n), a, gold["%s.%s" % (case, n)])
    if case == "b":      # masked keys: dk and dv exactly zero (the reference's, too)
        dead = ~c["kv_mask"]
        assert float(k.grad[dead].abs().max()) == 0.0 and float(v.grad[dead].abs().max()) == 0.0
    if case == "d":      # masked query rows come out exactly zero, nothing is NaN
        assert float(out.detach()[~c["q_mask"]].abs().max()) == 0.0 and float(q.grad[~c["q_mask"]].abs().max()) == 0.0


def test_attention_zero_rows_are_the_reference_nan_rows(gold, rec):
    c = rec["c"]
    q, k, v = [c[n].clone().requires_grad_() for n in "qkv"]
    out = R.full_attention(q, k, v, q_mask=c["q_mask"], kv_mask=c["kv_mask"])
    nan_rows = torch.from_numpy(gold["c.nan_rows"])
    assert bool(nan_rows.any()) and not bool(nan_rows.all())
    zero_rows = (out == 0).all(-1).all(-1)
    assert torch.equal(zero_rows, nan_rows), "the restatement's zero rows are not the reference's NaN rows"
    assert torch.equal(nan_rows, ~c["q_mask"])          # (every sequence of this case has a valid key)
    close("c.out", out, gold["c.out"])                  # stored with NaN -> 0: the zero rows compare as zeros, the others as they are
    (out * c["w"]).sum().backward()                     # and the gradients are finite, zero on the dead rows
    assert all(bool(torch.isfinite(a.grad).all()) for a in (q, k, v)) and float(q.grad[nan_rows].abs().max()) == 0.0


def test_quirks(rec):
    c = rec["b"]
    q, k, v = c["q"], c["k"], c["v"]
    part = rec["c"]["q_mask"]
    assert torch.equal(R.full_attention(q, k, v, q_mask=part), R.full_attention(q, k, v))       # q_mask alone is ignored
    with pytest.raises(TypeError):
        R.full_attention(q, k, v, kv_mask=c["kv_mask"])


def test_layer_full_with_source_mask(gold, rec):
    from riders_amd.linear_attention import LoFTREncoderLayer
    c = rec["e"]
    sd = leaves(fill_state_dict(LoFTREncoderLayer(128, 8, "full"), "g20.layer"))
    x, s = c["x"].clone().requires_grad_(), c["s"].clone().requires_grad_()
    o = R.loftr_layer(x, s, sd, "", "full", c["x_mask"], c["source_mask"])
    (o * c["w"]).sum().backward()
    close("e.out", o, gold["e.out"]); close("e.dx", x.grad, gold["e.dx"]); close("e.ds", s.grad, gold["e.ds"])
    check_grads(gold, "e.grad ", sd)


def test_transformer_full_with_masks(gold, rec):
    """mask1 partial: the reference's outputs are NaN on every row of the sequence that has a masked token (the generator says why); on the
    other rows the restatement agrees, and on the finite sequences alone it reproduces the reference's gradients."""
    from riders_amd.linear_attention import LocalFeatureTransformer
    c = rec["f"]
    sd = leaves(fill_state_dict(LocalFeatureTransformer(["self", "cross"], 1, 128, 8, "full"), "g20.tf"))
    with torch.no_grad():
        o0, o1 = R.local_feature_transformer(c["a"], c["b"], sd, "", ("self", "cross"), "full", c["mask0"], c["mask1"])
    assert bool(torch.isfinite(o0).all()) and bool(torch.isfinite(o1).all())
    nan0, nan1 = torch.from_numpy(gold["f.nan0"]), torch.from_numpy(gold["f.nan1"])
    close("f.out0", torch.where(nan0[..., None], torch.zeros_like(o0), o0), gold["f.out0"])
    close("f.out1", torch.where(nan1[..., None], torch.zeros_like(o1), o1), gold["f.out1"])
    fin = ~(nan0.any(1) | nan1.any(1))
    a, b = c["a"][fin].clone().requires_grad_(), c["b"][fin].clone().requires_grad_()
    p0, p1 = R.local_feature_transformer(a, b, sd, "", ("self", "cross"), "full", c["mask0"][fin], c["mask1"][fin])
    ((p0 * c["w0"][fin]).sum() + (p1 * c["w1"][fin]).sum()).backward()
    close("f.da", a.grad, gold["f.da"]); close("f.db", b.grad, gold["f.db"])
    check_grads(gold, "f.grad ", sd)


def test_transformer_linear_with_masks(gold, rec):
    from riders_amd.linear_attention import LocalFeatureTransformer
    c = rec["f"]
    sd = leaves(fill_state_dict(LocalFeatureTransformer(["self", "cross"], 1, 128, 8, "linear"), "g20.tf"))
    a, b = c["a"].clone().requires_grad_(), c["b"].clone().requires_grad_()
    o0, o1 = R.local_feature_transformer(a, b, sd, "", ("self", "cross"), "linear", c["mask0"], c["mask1"])
    ((o0 * c["w0"]).sum() + (o1 * c["w1"]).sum()).backward()
    close("g.out0", o0, gold["g.out0"]); close("g.out1", o1, gold["g.out1"])
    close("g.da", a.grad, gold["g.da"]); close("g.db", b.grad, gold["g.db"])
    check_grads(gold, "g.grad ", sd)
