"""What softmax ('full') attention and the token masks cost at the workload's shape (N = 240 sequences, L = S = 21 tokens, H = 8 heads of 16):
rd_full_attention_{fwd,bwd} and rd_linear_attention_masked_{fwd,bwd} next to rd_linear_attention_{fwd,bwd} and next to torch's own eager
expression of FullAttention on the same device (what a user would run without the kernel: the baseline), in fp32 and bf16; and a whole
LocalFeatureTransformer(['self', 'cross'] * 4, d_model 128) training step with attention='full' (per-op route) against the default linear one
(fused route).  Protocol of tools/bench_loss_scale.py: device events on the stream after a warm-up; within one round every variant runs in
turn, `--inner` calls at a time, until each has filled `--seconds`; `--rounds` rounds; the minimum and the median over the rounds are printed.

python tools/bench_full_attn.py [--out profiles/full_attention.txt]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from riders_amd import engine  # noqa: E402
from riders_amd.linear_attention import LocalFeatureTransformer  # noqa: E402
from tools.bench_loss_scale import measure, median, spread  # noqa: E402

N, L, S, H, D = 240, 21, 21, 8, 16


def row(key, xs, against=None):
    text = "  %-34s min %8.2f us   median %8.2f us   spread between rounds %5.2f %%" % (key, min(xs), median(xs), spread(xs))
    if against is not None:
        text += "   %.2f x %s" % (min(xs) / min(against[1]), against[0])
    return text


def torch_full(q, k, v, q_mask=None, kv_mask=None):
    """the reference's FullAttention.forward, eager torch on the device (RCNet/linear_attention.py:68-78)"""
    QK = torch.einsum("nlhd,nshd->nlsh", q, k)
    if kv_mask is not None:
        QK.masked_fill_(~(q_mask[:, :, None, None] & kv_mask[:, None, :, None]), float("-inf"))
    A = torch.softmax(QK / D ** 0.5, dim=2)
    return torch.einsum("nlsh,nshd->nlhd", A, v).contiguous()


def kernels(dev, dtype, a):
    lib, C = engine.L(), H * D
    torch.manual_seed(0)
    q, k, v, do = [torch.randn(N * L, C, device=dev).to(dtype) for _ in range(4)]
    out, dq, dk, dv = [torch.empty_like(q) for _ in range(4)]
    qm = torch.ones(N, L, dtype=torch.bool, device=dev)
    km = (torch.arange(S, device=dev)[None, :] < torch.randint(1, S + 1, (N, 1), device=dev)).contiguous()
    p, dt, st = engine._p, engine.rd_of(q), engine._stream(q)
    dims = (N, L, S, H, C, C, C, C)
    q4, k4, v4 = [x.view(N, -1, H, D).clone().requires_grad_() for x in (q, k, v)]
    do4 = do.view(N, L, H, D)

    def eager_bwd(masks):
        def fn():
            o = torch_full(q4, k4, v4, *masks)
            torch.autograd.grad(o, (q4, k4, v4), do4)
            return 0
        return fn

    def eager_fwd(masks):
        def fn():
            with torch.no_grad():
                torch_full(q4, k4, v4, *masks)
            return 0
        return fn
    fwd = [("rd_linear_attention_fwd", lambda: lib.rd_linear_attention_fwd(p(q), p(k), p(v), p(out), *dims, 1e-6, dt, st)),
           ("rd_linear_attention_masked_fwd", lambda: lib.rd_linear_attention_masked_fwd(p(q), p(k), p(v), p(out), p(qm), p(km), *dims, 1e-6, dt, st)),
           ("rd_full_attention_fwd", lambda: lib.rd_full_attention_fwd(p(q), p(k), p(v), p(out), None, None, *dims, 0.25, dt, st)),
           ("rd_full_attention_fwd, masks", lambda: lib.rd_full_attention_fwd(p(q), p(k), p(v), p(out), p(qm), p(km), *dims, 0.25, dt, st)),
           ("torch eager FullAttention fwd", eager_fwd(())),
           ("torch eager fwd, masks", eager_fwd((qm, km)))]
    bwd = [("rd_linear_attention_bwd", lambda: lib.rd_linear_attention_bwd(p(q), p(k), p(v), p(do), p(dq), p(dk), p(dv), *dims, 1e-6, dt, st)),
           ("rd_linear_attention_masked_bwd", lambda: lib.rd_linear_attention_masked_bwd(p(q), p(k), p(v), p(do), p(dq), p(dk), p(dv), p(qm), p(km), *dims, 1e-6, dt, st)),
           ("rd_full_attention_bwd", lambda: lib.rd_full_attention_bwd(p(q), p(k), p(v), p(do), p(dq), p(dk), p(dv), None, None, *dims, 0.25, dt, st)),
           ("rd_full_attention_bwd, masks", lambda: lib.rd_full_attention_bwd(p(q), p(k), p(v), p(do), p(dq), p(dk), p(dv), p(qm), p(km), *dims, 0.25, dt, st)),
           ("torch eager fwd + bwd", eager_bwd(())),
           ("torch eager fwd + bwd, masks", eager_bwd((qm, km)))]
    lines = []
    for title, variants in (("forward", fwd), ("backward (the kernels recompute the forward; torch: forward + backward)", bwd)):
        res = measure(variants, a.seconds, a.rounds, a.inner)
        lines.append(" %s, %s" % (str(dtype).split(".")[-1], title))
        base = variants[4][0]
        for key, _ in variants:
            lines.append(row(key, res[key], None if key == base else (base, res[base])))
    # same seeded inputs, same results: the kernel against the eager expression at the size timed
    lib.rd_full_attention_fwd(p(q), p(k), p(v), p(out), p(qm), p(km), *dims, 0.25, dt, st)
    with torch.no_grad():
        ref = torch_full(q4.float(), k4.float(), v4.float(), qm, km).view(N * L, C)
    lines.append("  (kernel against eager fp32 torch on these inputs: max |difference| %.3e at max |out| %.3e)" % (
        float((out.float() - ref).abs().max()), float(ref.abs().max())))
    return lines


def step(dev, dtype_name, a):
    """a whole transformer step (forward, backward into inputs and weights) at the workload's shape, 'linear' (fused route) against 'full'"""
    engine.set_compute_dtype(dtype_name)
    torch.manual_seed(0)
    f0, f1 = torch.randn(N, L, 128, device=dev, requires_grad=True), torch.randn(N, S, 128, device=dev, requires_grad=True)
    w0, w1 = torch.randn(N, L, 128, device=dev), torch.randn(N, S, 128, device=dev)
    variants = []
    for att in ("linear", "full"):
        m = LocalFeatureTransformer(["self", "cross"], 4, 128, 8, att).to(dev)

        def fn(m=m):
            o0, o1 = m(f0, f1)
            ((o0 * w0).sum() + (o1 * w1).sum()).backward()
            return 0
        variants.append(("transformer step, '%s'" % att, fn))
    res = measure(variants, a.seconds, a.rounds, max(1, a.inner // 10))
    engine.set_compute_dtype("fp32")
    lines = [" %s, LocalFeatureTransformer(['self', 'cross'] * 4, 128, 8): forward + backward, issued from Python" % dtype_name]
    for key, _ in variants:
        lines.append(row(key, res[key], None if "linear" in key else (variants[0][0], res[variants[0][0]])))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.3, help="device time every variant fills per round")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--inner", type=int, default=50, help="calls of one variant between two events")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_full_attn.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    lines = ["Softmax ('full') attention and token masks, N = %d, L = S = %d, H = %d, D = %d: us per call, %d rounds of >= %.2f s per variant, variants "
             "alternating every %d calls" % (N, L, H, D, a.rounds, a.seconds, a.inner)]
    for dtype in (torch.float32, torch.bfloat16):
        lines += kernels(dev, dtype, a)
    for name in ("fp32", "bf16"):
        lines += step(dev, name, a)
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
