"""Generate tests/golden/g20_full_attention.npz by IMPORTING THE REFERENCE's linear_attention.py (run in the build container only, as
make_golden.py):  python tests/golden/make_golden_full_attn.py

Softmax ('full') attention and token masks: FullAttention, masked LinearAttention, LoFTREncoderLayer(128, 8, 'full') with a source mask and
LocalFeatureTransformer(['self', 'cross'], 1, 128, 8, 'full') with masks.  The reference runs in float64 on inputs and weights regenerated
from names by tests/golden/fill.py (fp32 values), so that tests/test_golden_full_attn.py can hold the restatement to 1e-12.  Only recipes
(the `recipe()` below, imported by the tests) and results are stored.

Size: float64 results do not compress, and the full arrays of the six cases are 1.4 MB.  The fixture has to stay below the largest one
present (g9_sml.npz, 365 KB), so every result array is stored as its flattened elements STRIDE apart (the way g3 stores skip0_sub): every
sequence, token row and head is still sampled (the stride is coprime to 16 and 128), and N stays 4, which the four prefix lengths need.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))

STRIDE = 5
N, L, S, H, D = 4, 21, 17, 8, 16
KV_LENS = (17, 16, 5, 1)


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


def sub(a):
    return np.ascontiguousarray(a.detach().double().reshape(-1)[::STRIDE].numpy())


def recipe():
    """names -> inputs, masks and weights of every case; shared by the generator and the tests"""
    from tests.golden.fill import rand_array
    r = {}
    for c in "abcd":
        r[c] = dict(q=t64(rand_array("g20.%s.q" % c, (N, L, H, D), 1.0)), k=t64(rand_array("g20.%s.k" % c, (N, S, H, D), 1.0)),
                    v=t64(rand_array("g20.%s.v" % c, (N, S, H, D), 1.0)), w=t64(rand_array("g20.%s.w" % c, (N, L, H, D), 1.0)))
    prefix = torch.arange(S)[None, :] < torch.tensor(KV_LENS)[:, None]
    r["b"].update(q_mask=torch.ones(N, L, dtype=torch.bool), kv_mask=prefix)
    qpart = torch.from_numpy(rand_array("g20.c.qm", (N, L), 1.0) > -0.3)
    qpart[1] = False                                       # one sequence with no valid query at all
    r["c"].update(q_mask=qpart, kv_mask=prefix)
    r["d"].update(q_mask=torch.from_numpy(rand_array("g20.d.qm", (N, L), 1.0) > -0.3), kv_mask=torch.from_numpy(rand_array("g20.d.km", (N, S), 1.0) > -0.3))
    r["e"] = dict(x=t64(rand_array("g20.e.x", (3, 21, 128), 1.0)), s=t64(rand_array("g20.e.s", (3, 21, 128), 1.0)),
                  w=t64(rand_array("g20.e.w", (3, 21, 128), 1.0)), x_mask=torch.ones(3, 21, dtype=torch.bool),
                  source_mask=torch.arange(21)[None, :] < torch.tensor((21, 16, 3))[:, None])
    r["f"] = dict(a=t64(rand_array("g20.f.a", (2, 21, 128), 1.0)), b=t64(rand_array("g20.f.b", (2, 21, 128), 1.0)),
                  w0=t64(rand_array("g20.f.w0", (2, 21, 128), 1.0)), w1=t64(rand_array("g20.f.w1", (2, 21, 128), 1.0)),
                  mask0=torch.ones(2, 21, dtype=torch.bool), mask1=torch.arange(21)[None, :] < torch.tensor((21, 13))[:, None])
    return r


def grad_summary(named):
    out = {}
    for k, p in named:
        g = p.grad.detach().double().reshape(-1)
        out[k + "|norm"] = np.array([g.norm().item()], np.float64)
        out[k + "|head"] = g[:16].numpy().copy()
    return out


def main():
    sys.path[:0] = [ROOT, os.path.join(HERE, "stubs"), "/root/reference", "/root/reference/RCNet"]
    import linear_attention as la
    from tests.golden.fill import fill_state_dict
    torch.set_num_threads(8)
    r, arrs = recipe(), {}

    for c, cls in (("a", la.FullAttention), ("b", la.FullAttention), ("d", la.LinearAttention)):
        q, k, v = [r[c][n].clone().requires_grad_() for n in "qkv"]
        out = cls()(q, k, v, q_mask=r[c].get("q_mask"), kv_mask=r[c].get("kv_mask"))
        (out * r[c]["w"]).sum().backward()
        for n, a in (("out", out), ("dq", q.grad), ("dk", k.grad), ("dv", v.grad)):
            assert bool(torch.isfinite(a).all()), (c, n)
            arrs["%s.%s" % (c, n)] = sub(a)
    with torch.no_grad():
        out = la.FullAttention()(r["c"]["q"], r["c"]["k"], r["c"]["v"], q_mask=r["c"]["q_mask"], kv_mask=r["c"]["kv_mask"])
    nan_rows = torch.isnan(out).any(-1).any(-1)                      # [N, L]
    assert bool((torch.isnan(out).all(-1).all(-1) == nan_rows).all())   # a row is NaN as a whole or not at all
    arrs["c.nan_rows"] = nan_rows.numpy()
    arrs["c.out"] = sub(torch.nan_to_num(out, nan=0.0))

    layer = la.LoFTREncoderLayer(128, 8, "full").double()
    fill_state_dict(layer, "g20.layer")
    x, s = r["e"]["x"].clone().requires_grad_(), r["e"]["s"].clone().requires_grad_()
    o = layer(x, s, r["e"]["x_mask"], r["e"]["source_mask"])
    (o * r["e"]["w"]).sum().backward()
    for n, a in (("out", o), ("dx", x.grad), ("ds", s.grad)):
        assert bool(torch.isfinite(a).all()), ("e", n)
        arrs["e." + n] = sub(a)
    arrs.update({"e.grad " + k_: v_ for k_, v_ in grad_summary(layer.named_parameters()).items()})

    # (f) 'full' transformer.  Its 'self' layer calls layer(feat1, feat1, mask1, mask1), so a partial mask1 makes the masked QUERY rows of
    # feat1 NaN in the reference, and the following cross call spreads them over the whole sequence (0 * NaN in A V): every row of sequence 1
    # is NaN, in both outputs, and so is every parameter gradient.  Stored: the NaN row sets, the outputs with NaN -> 0, and the gradients
    # of the reference run on the sequences that stay finite (here sequence 0) alone.
    tf = la.LocalFeatureTransformer(["self", "cross"], 1, 128, 8, "full").double()
    fill_state_dict(tf, "g20.tf")
    with torch.no_grad():
        o0, o1 = tf(r["f"]["a"], r["f"]["b"], r["f"]["mask0"], r["f"]["mask1"])
    nan0, nan1 = torch.isnan(o0).any(-1), torch.isnan(o1).any(-1)
    arrs["f.nan0"], arrs["f.nan1"] = nan0.numpy(), nan1.numpy()
    arrs["f.out0"], arrs["f.out1"] = sub(torch.nan_to_num(o0, nan=0.0)), sub(torch.nan_to_num(o1, nan=0.0))
    fin = ~(nan0.any(1) | nan1.any(1))
    assert fin.tolist() == [True, False], fin
    a, b = r["f"]["a"][fin].clone().requires_grad_(), r["f"]["b"][fin].clone().requires_grad_()
    p0, p1 = tf(a, b, r["f"]["mask0"][fin], r["f"]["mask1"][fin])
    assert float((p0.detach() - o0[fin]).abs().max()) < 1e-13 and float((p1.detach() - o1[fin]).abs().max()) < 1e-13     # (GEMM blocking differs with the batch)
    ((p0 * r["f"]["w0"][fin]).sum() + (p1 * r["f"]["w1"][fin]).sum()).backward()
    for n, t_ in (("da", a.grad), ("db", b.grad)):
        assert bool(torch.isfinite(t_).all()), ("f", n)
        arrs["f." + n] = sub(t_)
    arrs.update({"f.grad " + k_: v_ for k_, v_ in grad_summary(tf.named_parameters()).items()})

    # (g) the same transformer with attention='linear', where masked rows are zeros instead of NaN: finite throughout, so the mask threading of
    # both layer kinds (the swapped order of the second cross call included) is pinned with gradients
    tf = la.LocalFeatureTransformer(["self", "cross"], 1, 128, 8, "linear").double()
    fill_state_dict(tf, "g20.tf")
    a, b = r["f"]["a"].clone().requires_grad_(), r["f"]["b"].clone().requires_grad_()
    o0, o1 = tf(a, b, r["f"]["mask0"], r["f"]["mask1"])
    ((o0 * r["f"]["w0"]).sum() + (o1 * r["f"]["w1"]).sum()).backward()
    for n, t_ in (("out0", o0), ("out1", o1), ("da", a.grad), ("db", b.grad)):
        assert bool(torch.isfinite(t_).all()), ("g", n)
        arrs["g." + n] = sub(t_)
    arrs.update({"g.grad " + k_: v_ for k_, v_ in grad_summary(tf.named_parameters()).items()})

    path = os.path.join(HERE, "g20_full_attention.npz")
    np.savez_compressed(path, **arrs)
    print("g20_full_attention %7.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
