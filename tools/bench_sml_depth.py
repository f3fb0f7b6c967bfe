"""Timing of the Scale-Map-Learner options 'midas-small-depth' and ground_truth_dilation_kernel_size: sml_main.GraphedTrainStep (device pre-step +
forward + loss + backward replayed from a hipGraph, eager Adam) at B = 16, 288 x 384, bf16, for the two model types, each with and without a
3 x 3 ground-truth dilation -- four captured steps built in ONE process on one device and timed in interleaved rounds, so that clock and
neighbour noise hits them alike -- and the three kernels of rd_sml_depth.hip alone at 16 x 288 x 384 (each captured 20 x into a hipGraph and
replayed: device time per call without the host).

No condition is judged: the figures are reported (medians, and the spread (max - min) / median over the rounds).

    python tools/bench_sml_depth.py [--out profiles/sml_depth.txt] [--rounds 7] [--steps 40] [--small]
"""
import argparse
import contextlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, H, W, PER_GRAPH = 16, 288, 384, 20
VARIANTS = (("midas-small", -1), ("midas-small", 3), ("midas-small-depth", -1), ("midas-small-depth", 3))


def label(v):
    return "%s%s" % (v[0], ", dilation %d" % v[1] if v[1] > 1 else "")


def window(run, iters):
    import torch
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        run()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters      # ms per call


def steps(args, dev, b, h, w):
    import torch
    from riders_amd import engine, sml_main
    from riders_amd.optim import FlatAdam
    engine.set_compute_dtype("bf16")
    built = []
    for mt, k in VARIANTS:
        cfg = dict(sml_main.ZJU_SML_CONFIG, model_type=mt, ground_truth_dilation_kernel_size=k)
        torch.manual_seed(0)
        with contextlib.redirect_stdout(sys.stderr):
            model = sml_main.build_model(dev, cfg)
        model.train()
        opt = FlatAdam(model.parameters(), lr=cfg['learning_rate'])
        batch = sml_main.synthetic_batch(b, h, w, seed=1234, device=dev)
        step = sml_main.GraphedTrainStep(model, opt, batch, cfg, outlier=sml_main.make_outlier_removal(cfg))
        for _ in range(5):
            loss = step()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss)), (mt, k)
        built.append(step)
    ms = [[] for _ in VARIANTS]
    for r in range(args.rounds):
        order = list(range(len(VARIANTS)))
        order = order[r % len(order):] + order[:r % len(order)]      # every variant takes every position
        for i in order:
            ms[i].append(window(built[i], args.steps))
    engine.set_compute_dtype("fp32")
    return ms


def kernels(args, dev, b, h, w):
    import torch
    from riders_amd import engine
    lib, p = engine.L(), engine._p
    n = b * h * w
    g = torch.Generator().manual_seed(5)
    out32 = (torch.randn(n, generator=g) * 2.5).to(dev)
    out16 = out32.to(torch.bfloat16)
    dpred = torch.randn(n, generator=g).to(dev)
    pred = torch.empty(n, dtype=torch.float32, device=dev)
    do32, do16 = torch.empty_like(out32), torch.empty_like(out16)
    gt = (torch.rand((b, 1, h, w), generator=g) * 60.0 * (torch.rand((b, 1, h, w), generator=g) < 0.7)).to(dev)
    dil = torch.empty_like(gt)
    hi, lo = 1.0 / 0.1, 1.0 / 255.0
    side = torch.cuda.Stream()
    st = lambda: engine._stream(pred)      # noqa: E731
    calls = [
        ("rd_sml_depth_head_fwd fp32", 8 * n, lambda: lib.rd_sml_depth_head_fwd(p(out32), p(pred), n, hi, lo, 0, st())),
        ("rd_sml_depth_head_fwd bf16", 6 * n, lambda: lib.rd_sml_depth_head_fwd(p(out16), p(pred), n, hi, lo, 1, st())),
        ("rd_sml_depth_head_bwd fp32", 12 * n, lambda: lib.rd_sml_depth_head_bwd(p(out32), p(dpred), p(do32), n, hi, lo, 0, st())),
        ("rd_sml_depth_head_bwd bf16", 8 * n, lambda: lib.rd_sml_depth_head_bwd(p(out16), p(dpred), p(do16), n, hi, lo, 1, st())),
        ("rd_maxpool_dilate k=3", 8 * n, lambda: lib.rd_maxpool_dilate(p(gt), p(dil), b, h, w, 3, st())),
        ("rd_maxpool_dilate k=7", 8 * n, lambda: lib.rd_maxpool_dilate(p(gt), p(dil), b, h, w, 7, st())),
    ]
    res = []
    for name, nbytes, fn in calls:
        def run(fn=fn, name=name):
            engine._chk(fn(), name)
        run()
        torch.cuda.synchronize()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            run()
            with torch.cuda.graph(graph, stream=side):
                for _ in range(PER_GRAPH):
                    run()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph.replay()
        us = [window(graph.replay, 50) / PER_GRAPH * 1e3 for _ in range(args.rounds)]
        res.append((name, nbytes, us))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=40, help="training steps per timed window")
    ap.add_argument("--small", action="store_true", help="B = 2, 64 x 96 (rehearsal of the script, not a measurement)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_sml_depth: needs a GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    b, h, w = (2, 64, 96) if args.small else (B, H, W)
    ms = steps(args, dev, b, h, w)
    ks = kernels(args, dev, b, h, w)
    spread = lambda v: 100.0 * (max(v) - min(v)) / statistics.median(v)      # noqa: E731
    lines = ["Scale Map Learner, GraphedTrainStep (pre-step + forward + loss + backward in one hipGraph, eager Adam), B = %d, %d x %d, bf16; four steps "
             "built in one process, %d interleaved rounds of %d steps; ms per step" % (b, h, w, args.rounds, args.steps),
             "%-32s %10s %10s %9s %12s" % ("variant", "median ms", "min ms", "spread", "imgs/s")]
    med = {}
    for v, m in zip(VARIANTS, ms):
        med[v] = statistics.median(m)
        lines.append("%-32s %10.3f %10.3f %8.1f%% %12.1f" % (label(v), med[v], min(m), spread(m), b / med[v] * 1e3))
    base = med[VARIANTS[0]]
    lines.append("relative to midas-small: " + ", ".join("%s %+.2f%%" % (label(v), 100.0 * (med[v] / base - 1.0)) for v in VARIANTS[1:]))
    lines.append("")
    lines.append("the kernels alone, %d elements, device time per call from a hipGraph of %d calls, %d rounds of 50 replays; bytes = every operand once" % (
        b * h * w, PER_GRAPH, args.rounds))
    lines.append("%-32s %10s %10s %9s %10s" % ("kernel", "median us", "min us", "spread", "TB/s"))
    for name, nbytes, us in ks:
        m = statistics.median(us)
        lines.append("%-32s %10.2f %10.2f %8.1f%% %10.2f" % (name, m, min(us), spread(us), nbytes / (m * 1e-6) / 1e12))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out and not args.small:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
