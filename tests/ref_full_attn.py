"""Plain torch restatement (float64 or float32, CPU) of the reference's two attentions WITH masks and of the layer / transformer that thread
them, written from RCNet/linear_attention.py's lines; tests/test_golden_full_attn.py pins it against vectors the reference itself produced
(tests/golden/g20_full_attention.npz).  oracle/rcnet.py restates the mask-free path only and is left as it is.

Two deliberate, documented differences from the reference, both applied with torch.where and both invisible wherever the reference is finite:

  * full attention: a query row with no admissible key (q_mask false, or no valid key in the sequence) is NaN in the reference (softmax over
    a row of -inf).  Here, as in rd_attention_full.hip, its attention row is exactly 0: output row 0, dq row 0, no contribution to dk / dv.
  * linear attention: a masked query row has Q = 0, so its normaliser is 1 / eps.  The reference's backward squares it, which overflows in
    fp32 at eps = 1e-30 (0 * inf = NaN in dk).  Here, as in rd_attention_head.h, Z of a masked query row is 0: the row's output, its dq and its
    share of dk are the exact zeros the reference computes in float64.

Masks are torch.bool, q_mask [N, L], kv_mask [N, S], True = valid.
"""
import torch
import torch.nn.functional as F


def full_attention_abi(q, k, v, q_mask=None, kv_mask=None, scale=None):
    """The kernel's contract (rd_full_attention_fwd): either mask may be None = all valid; a pair (l, s) is admissible iff both are valid.
    q [N,L,H,D], k, v [N,S,H,D] -> [N,L,H,D].  Reference :68-78 with the zero-row rule."""
    N, L, H, D = q.shape
    S = k.shape[1]
    scale = 1.0 / D ** 0.5 if scale is None else scale
    QK = torch.einsum("nlhd,nshd->nlsh", q, k)
    if q_mask is None and kv_mask is None:
        A = torch.softmax(scale * QK, dim=2)
    else:
        qm = torch.ones(N, L, dtype=torch.bool) if q_mask is None else q_mask
        km = torch.ones(N, S, dtype=torch.bool) if kv_mask is None else kv_mask
        adm = qm[:, :, None, None] & km[:, None, :, None]                       # :70
        dead = ~adm.any(dim=2, keepdim=True)
        # (a dead row's scores are replaced BEFORE the softmax as well: a NaN in the unselected branch of a where() still poisons its gradient)
        QK = torch.where(dead, torch.zeros_like(QK), QK.masked_fill(~adm, float("-inf")))
        A = torch.where(dead, torch.zeros_like(QK), torch.softmax(scale * QK, dim=2))
    return torch.einsum("nlsh,nshd->nlhd", A, v)


def full_attention(q, k, v, q_mask=None, kv_mask=None):
    """FullAttention.forward with the reference's quirks (:69-70): q_mask alone is ignored, kv_mask without q_mask is a TypeError."""
    if kv_mask is None:
        return full_attention_abi(q, k, v)
    if q_mask is None:
        raise TypeError("FullAttention: kv_mask without q_mask (the reference indexes None)")
    return full_attention_abi(q, k, v, q_mask, kv_mask)


def linear_attention(q, k, v, q_mask=None, kv_mask=None, eps=1e-6):
    """LinearAttention.forward :29-45; each mask applied on its own, after the feature map; v_length stays S."""
    Q = F.elu(q) + 1
    K = F.elu(k) + 1
    if q_mask is not None:
        Q = Q * q_mask[:, :, None, None].to(Q.dtype)
    if kv_mask is not None:
        K = K * kv_mask[:, :, None, None].to(K.dtype)
        v = v * kv_mask[:, :, None, None].to(v.dtype)
    S = v.size(1)
    v = v / S
    KV = torch.einsum("nshd,nshv->nhdv", K, v)
    den = torch.einsum("nlhd,nhd->nlh", Q, K.sum(dim=1)) + eps
    if q_mask is not None:      # (the divisor is replaced BEFORE the division as well: the unselected branch's 0 * (1 / eps)^2 would be NaN)
        den = torch.where(q_mask[:, :, None], den, torch.ones_like(den))
    Z = 1 / den
    if q_mask is not None:
        Z = torch.where(q_mask[:, :, None], Z, torch.zeros_like(Z))
    return torch.einsum("nlhd,nhdv,nlh->nlhv", Q, KV, Z) * S


def loftr_layer(x, source, sd, prefix, attention="linear", x_mask=None, source_mask=None, nhead=8):
    """LoFTREncoderLayer.forward :112-135."""
    bs, _, C = x.shape
    dim = C // nhead
    q = F.linear(x, sd[prefix + "q_proj.weight"]).view(bs, -1, nhead, dim)
    k = F.linear(source, sd[prefix + "k_proj.weight"]).view(bs, -1, nhead, dim)
    v = F.linear(source, sd[prefix + "v_proj.weight"]).view(bs, -1, nhead, dim)
    att = linear_attention if attention == "linear" else full_attention
    m = att(q, k, v, q_mask=x_mask, kv_mask=source_mask)
    m = F.linear(m.reshape(bs, -1, C), sd[prefix + "merge.weight"])
    m = F.layer_norm(m, (C,), sd[prefix + "norm1.weight"], sd[prefix + "norm1.bias"], 1e-5)
    m = F.linear(F.relu(F.linear(torch.cat([x, m], dim=2), sd[prefix + "mlp.0.weight"])), sd[prefix + "mlp.2.weight"])
    m = F.layer_norm(m, (C,), sd[prefix + "norm2.weight"], sd[prefix + "norm2.bias"], 1e-5)
    return x + m


def local_feature_transformer(f0, f1, sd, prefix, layer_names, attention="linear", mask0=None, mask1=None):
    """LocalFeatureTransformer.forward :170-184 (the second cross call takes the masks in swapped order)."""
    for i, name in enumerate(layer_names):
        p = prefix + "layers.%d." % i
        if name == "self":
            f0 = loftr_layer(f0, f0, sd, p, attention, mask0, mask0)
            f1 = loftr_layer(f1, f1, sd, p, attention, mask1, mask1)
        elif name == "cross":
            f0 = loftr_layer(f0, f1, sd, p, attention, mask0, mask1)
            f1 = loftr_layer(f1, f0, sd, p, attention, mask1, mask0)
        else:
            raise KeyError(name)
    return f0, f1
