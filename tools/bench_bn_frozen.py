"""Micro-benchmark of the frozen BatchNorm backward (rd_bn_act_bwd_frozen: one pass over dz and y, dy written -- three tensor passes) against
the unchanged training-mode backward at the same shape (rd_bn_act_bwd_recompute: reduce + finalize + apply -- five tensor passes), in bf16,
through the C ABI on one GPU.

The three variants -- training-mode, frozen without sums, frozen with sums -- run in ONE process and are ALTERNATED: each round times one window
of each (device events around `iters` back-to-back calls; `iters` is grown in the warm-up until a window exceeds --window seconds), and the
rounds' windows give a median and a spread (max - min over the rounds, relative to the median) per variant.  Bytes/s of the frozen forms are
3 x tensor bytes over the median time, printed next to the 6.29 TB/s measured-copy figure of SURVEY.md section 8d.

Condition checked per shape (exit status 1 if it fails anywhere): the form without sums is not slower than the training-mode backward beyond the
larger of the two measured spreads.  The form with sums is reported only.

    python tools/bench_bn_frozen.py [--out profiles/bn_frozen_bwd.txt] [--rounds 5] [--window 0.25]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_TBS = 6.29      # measured device-to-device copy, TB/s (read + write bytes)
# (pixels, channels, activation, what)
SHAPES = [
    (5760000, 16, 2, "RC-Net B=8 decoder 240x100 x 240 RoIs"),
    (1440000, 32, 2, "RC-Net B=8 decoder 120x50"),
    (345600, 64, 2, "RC-Net B=8 decoder 60x24"),
    (86400, 256, 2, "RC-Net B=8 decoder 30x12"),
    (663552, 144, 3, "SML B=16 expanded map 144x288 (narrow layer, wide map)"),
    (10368, 816, 3, "SML B=16 expanded map 18x36, 816 channels"),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25, help="least seconds per timed window")
    ap.add_argument("--shapes", type=int, default=len(SHAPES), help="only the first N shapes (rehearsal)")
    args = ap.parse_args()
    import torch
    from riders_amd.engine import L, _p, _stream
    if not torch.cuda.is_available():
        sys.exit("bench_bn_frozen: needs a GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    lib = L()
    dt, tdt, es = 1, torch.bfloat16, 2
    lines = ["frozen BatchNorm backward vs training-mode backward, bf16, %d alternated rounds, windows >= %.2f s; times are medians in us, spread = (max - min) / median over the rounds"
             % (args.rounds, args.window),
             "%-9s %5s  %-9s %18s  %18s %7s %6s  %18s %7s %6s  %s" % ("pixels", "C", "form", "train us (spread)", "frozen us (spread)", "TB/s", "x copy",
                                                                       "+sums us (spread)", "TB/s", "x copy", "no-sums <= train")]
    ok_all = True
    for pixels, C, act, what in SHAPES[:args.shapes]:
        g = torch.Generator(device="cpu").manual_seed(pixels + C)
        y = torch.randn((pixels, C), generator=g).to(dev).to(tdt)
        dz = torch.randn((pixels, C), generator=g).to(dev).to(tdt)
        dy = torch.empty_like(y)
        rows = lib.rd_bn_bwd_rows(pixels, C)
        part = torch.empty((rows, C, 2), dtype=torch.float32, device=dev)
        coef = torch.empty((4, C), dtype=torch.float32, device=dev)      # scale, shift, mean, rstd
        coef[0].fill_(0.8); coef[1].fill_(0.1); coef[2].fill_(0.05); coef[3].fill_(0.9)
        coef2 = torch.empty((2, C), dtype=torch.float32, device=dev)
        dg, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
        st = _stream(y)
        stat = (_p(coef[2]), _p(coef[3]), _p(coef[0]), _p(coef[1]))
        tail = (pixels, C, act, 0.2, dt, st)
        fns = {
            "train": lambda: lib.rd_bn_act_bwd_recompute(_p(dz), None, _p(y), *stat, _p(part), _p(coef2), _p(dg), _p(db), 0, _p(dy), None, *tail),
            "frozen": lambda: lib.rd_bn_act_bwd_frozen(_p(dz), None, _p(y), *stat, None, None, None, 0, _p(dy), None, *tail),
            "sums": lambda: lib.rd_bn_act_bwd_frozen(_p(dz), None, _p(y), *stat, _p(part), _p(dg), _p(db), 0, _p(dy), None, *tail),
        }

        def window(fn, iters):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(iters):
                fn()
            e.record()
            torch.cuda.synchronize()
            return s.elapsed_time(e) * 1e-3      # seconds

        iters = {}
        for k, fn in fns.items():      # warm-up of every variant at this shape, and the iteration count that fills a window
            assert fn() == 0, (k, lib.rd_last_error_string())
            n = 20
            while True:
                sec = window(fn, n)
                if sec >= args.window or n >= 1 << 20:
                    break
                n = max(n + 1, int(n * min(8.0, 1.2 * args.window / max(sec, 1e-6))))
            iters[k] = n
        times = {k: [] for k in fns}
        for _ in range(args.rounds):      # alternated: one window of each variant per round
            for k, fn in fns.items():
                times[k].append(window(fn, iters[k]) / iters[k] * 1e6)
        med = {k: statistics.median(v) for k, v in times.items()}
        spr = {k: (max(v) - min(v)) / med[k] for k, v in times.items()}
        tb = {k: 3.0 * pixels * C * es / (med[k] * 1e-6) / 1e12 for k in ("frozen", "sums")}
        ok = med["frozen"] <= med["train"] * (1.0 + max(spr["frozen"], spr["train"]))
        ok_all = ok_all and ok
        form = lib.rd_bn_kernel_name(3, C, dt, act, 0).decode().split("_kernel")[0].replace("bn_frozen_bwd_", "")
        lines.append("%-9d %5d  %-9s %10.1f (%4.1f%%)  %10.1f (%4.1f%%) %7.2f %6.2f  %10.1f (%4.1f%%) %7.2f %6.2f  %s   %s" % (
            pixels, C, form if form != "bn_frozen_bwd" else "scalar", med["train"], 100 * spr["train"], med["frozen"], 100 * spr["frozen"], tb["frozen"],
            tb["frozen"] / COPY_TBS, med["sums"], 100 * spr["sums"], tb["sums"], tb["sums"] / COPY_TBS, "yes" if ok else "NO", what))
        print(lines[-1], flush=True)
        del y, dz, dy, part
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    sys.exit(0 if ok_all else 1)


if __name__ == "__main__":
    main()
