"""Throughput of RC-Net inference (the step between the two stages, RCNet/run_rcnet_zju.py:204-271): rcnet_main.run_frame called frame by frame --
one forward per frame, a host read per retry -- against rcnet_main.run_frames over batches of F = 1, 4, 8, 16 frames, and the fusion kernels on
their own.  ZJU geometry: 256 x 512 frames, patch 240 x 100, the same 16 seeded frames with N_f drawn from 30..120 radar points in every variant,
compute modes bf16 and fp32 (the crops handed to the fusion are fp32 in both, as the model returns them; the kernel table also times bf16 crops).

Each (variant, mode) runs in a CHILD process of its own (fresh runtime, nothing shared but the GPU), the children one after the other, the whole
sequence `--repeats` times, so the variants alternate.  A child warms its variant up on all 16 frames and then times `--rounds` windows:
  frames   a host clock around passes over the 16 frames, ending in a device synchronise -> frames/s (inference here is bound by the host's launch
           rate, so the host clock is the figure a user sees);
  kernels  device events around back-to-back launches through the C ABI -> us per launch: rd_scatter_crops against rd_scatter_crops_frames on one
           frame of N = 30, 100, 300 points, on 8 frames of 100 points (eight launches of the old kernel against one of the new), and
           rd_frame_thresholds (both launches) on the same inputs.
The bar: run_frames at F = 8 ahead of the run_frame loop by more than the window spread (stated as met / NOT met; the figures are recorded either way).

    python tools/bench_infer.py [--out profiles/infer_frames.txt] [--rounds 5] [--passes 3] [--repeats 2]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NFRAMES, H, W = 16, 256, 512
BATCHES = (1, 4, 8, 16)
VARIANTS = ("frame_loop",) + tuple("frames%d" % f for f in BATCHES) + ("kernels",)
MODES = ("bf16", "fp32")
KERNEL_CASES = ((1, 30), (1, 100), (1, 300), (8, 100))      # (frames, points per frame)


def frames_child(variant, mode, rounds, passes, small):
    import numpy as np
    import torch
    from riders_amd import engine, rcnet_main
    dev = torch.device("cuda:0")
    engine.set_compute_dtype(mode)
    cfg = dict(rcnet_main.ZJU_CONFIG, patch_size=[64, 32]) if small else rcnet_main.ZJU_CONFIG
    h, w, lo, hi = (64, 96, 2, 6) if small else (H, W, 30, 120)
    torch.manual_seed(0)
    model = rcnet_main.build_model(dev, cfg)
    model.eval()
    rng = np.random.RandomState(3)
    images = torch.from_numpy(rng.randint(0, 256, (NFRAMES, 3, h, w)).astype(np.float32)).to(dev)
    counts = rng.randint(lo, hi + 1, NFRAMES)
    points = [torch.from_numpy(np.stack([rng.uniform(0, w - 0.01, n), rng.uniform(0, h - 0.01, n), rng.uniform(1.5, 100.0, n)], 1).astype(np.float32)).to(dev)
              for n in counts]
    retries = []
    if variant == "frame_loop":
        def one_pass():
            for f in range(NFRAMES):
                rcnet_main.run_frame(model, images[f:f + 1], points[f])
    else:
        F = int(variant[6:])

        def one_pass():
            for f in range(0, NFRAMES, F):
                out = rcnet_main.run_frames(model, images[f:f + F], points[f:f + F])
                retries.append(out[3])
    one_pass()      # warm-up: every shape of the timed window
    torch.cuda.synchronize()
    if variant != "frame_loop":
        rcnet_main.check_no_response()
    n_retry = int(torch.cat(retries).sum()) if retries else -1
    fps = []
    for _ in range(rounds):
        del retries[:]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(passes):
            one_pass()
        torch.cuda.synchronize()
        fps.append(NFRAMES * passes / (time.perf_counter() - t0))
    print("RESULT " + json.dumps(dict(variant=variant, mode=mode, fps=fps, points=int(counts.sum()), retries=n_retry)), flush=True)


def kernels_child(mode, rounds, small):
    import numpy as np
    import torch
    from riders_amd import engine, rcnet_main
    dev = torch.device("cuda:0")
    lib = engine.L()
    ph, pw, h, w = (64, 32, 64, 96) if small else (240, 100, H, W)
    dt = torch.bfloat16 if mode == "bf16" else torch.float32
    rng = np.random.RandomState(9)
    out = {}

    def timed(run, iters=50):
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        us = []
        for _ in range(rounds):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(iters):
                run()
            e.record()
            torch.cuda.synchronize()
            us.append(s.elapsed_time(e) * 1e3 / iters)
        return us
    for F, n in KERNEL_CASES:
        R = F * n
        crops = torch.from_numpy(rng.uniform(0, 1, (R, ph, pw)).astype(np.float32)).to(dt).to(dev)
        pts = torch.from_numpy(np.stack([rng.uniform(0, w - 0.01, R) + pw // 2, rng.uniform(0, h - 0.01, R) + ph // 2, rng.uniform(1.5, 100.0, R)], 1).astype(np.float32)).to(dev)
        fs = torch.arange(0, R + 1, n, dtype=torch.int32).to(dev)
        depth, resp = torch.empty((F, h, w), device=dev), torch.empty((F, h, w), device=dev)
        d1, r1 = torch.empty((F, h, w), device=dev), torch.empty((F, h, w), device=dev)
        thr = torch.full((F,), 0.5, device=dev)
        rmax, ret, flag = torch.empty(F, device=dev), torch.empty(F, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        ws = torch.empty(int(lib.rd_frame_thresholds_ws_bytes(R)) // 4, device=dev)
        st, code = engine._stream(crops), engine.rd_of(crops)

        def old():
            for f in range(F):
                engine._chk(lib.rd_scatter_crops(engine._p(crops[f * n:]), engine._p(pts[f * n:]), engine._p(d1[f]), engine._p(r1[f]), n, ph, pw, h, w,
                                                 ctypes.c_float(0.5), code, st), "rd_scatter_crops")

        def new():
            engine._chk(lib.rd_scatter_crops_frames(engine._p(crops), engine._p(pts), engine._p(fs), engine._p(thr), engine._p(depth), engine._p(resp), R, F,
                                                    ph, pw, h, w, code, st), "rd_scatter_crops_frames")

        def thresholds():
            engine._chk(lib.rd_frame_thresholds(engine._p(crops), engine._p(pts), engine._p(fs), R, F, ph, pw, h, w, 0.5, 0.05, engine._p(ws), engine._p(rmax),
                                                engine._p(thr), engine._p(ret), engine._p(flag), code, st), "rd_frame_thresholds")
        key = "F%d_N%d" % (F, n)
        out[key] = dict(old=timed(old), new=timed(new), thresholds=timed(thresholds))
        torch.cuda.synchronize()
        assert torch.equal(depth, d1) and torch.equal(resp, r1), "the two scatters disagree at " + key      # (thr is 0.5 again: uniform crops reach it)
    print("RESULT " + json.dumps(dict(variant="kernels", mode=mode, kernels=out)), flush=True)


def child(variant, mode, rounds, passes, small):
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_infer: needs a GPU (nothing is measured without one)")
    if variant == "kernels":
        return kernels_child(mode, rounds, small)
    return frames_child(variant, mode, rounds, passes, small)


def _ms(v):
    m = statistics.median(v)
    return m, (max(v) - min(v)) / m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--rounds", type=int, default=5, help="timed windows per child")
    ap.add_argument("--passes", type=int, default=3, help="passes over the 16 frames per window")
    ap.add_argument("--repeats", type=int, default=2, help="how often the sequence of children is run")
    ap.add_argument("--small", action="store_true", help="64 x 96 frames, patch 64 x 32 (rehearsal of the script, not a measurement)")
    ap.add_argument("--child", default=None, choices=VARIANTS)
    ap.add_argument("--mode", default="bf16", choices=MODES)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.mode, args.rounds, args.passes, args.small)
    fps = {(v, m): [] for v in VARIANTS[:-1] for m in MODES}
    kern = {m: {} for m in MODES}
    info = {}
    for _ in range(args.repeats):
        for m in MODES:
            for v in VARIANTS:
                cmd = [sys.executable, os.path.abspath(__file__), "--child", v, "--mode", m, "--rounds", str(args.rounds), "--passes", str(args.passes)]
                r = subprocess.run(cmd + (["--small"] if args.small else []), capture_output=True, text=True, cwd=ROOT, timeout=300)
                line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")]
                if r.returncode != 0 or not line:
                    sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                    sys.exit("bench_infer: child %s/%s failed (exit status %d)" % (v, m, r.returncode))
                d = json.loads(line[-1][7:])
                if v == "kernels":
                    for key, t in d["kernels"].items():
                        for k, us in t.items():
                            kern[m].setdefault(key, {}).setdefault(k, []).extend(us)
                else:
                    fps[(v, m)] += d["fps"]
                    info[(v, m)] = (d["points"], d["retries"])
                print("done %s/%s" % (v, m), flush=True)
    lines = ["RC-Net inference, %d frames of %d x %d, patch 240 x 100, N_f drawn from 30..120 (%d points in all); every (variant, mode) in children of its own, "
             "%d runs x %d windows of %d passes; frames/s by the host clock (synchronised), median and spread = (max - min) / median"
             % (NFRAMES, H, W, info[("frame_loop", MODES[0])][0], args.repeats, args.rounds, args.passes),
             "%-12s %-5s %20s %10s %10s" % ("variant", "mode", "frames/s (spread)", "vs loop", "retries")]
    verdict = []
    for m in MODES:
        base, base_s = _ms(fps[("frame_loop", m)])
        for v in VARIANTS[:-1]:
            md, sp = _ms(fps[(v, m)])
            lines.append("%-12s %-5s %12.1f (%4.1f%%) %9.2fx %10s" % (v, m, md, 100 * sp, md / base, "-" if v == "frame_loop" else info[(v, m)][1]))
            if v == "frames8":
                ok = md / base - 1.0 > max(sp, base_s)
                verdict.append("run_frames at F = 8 / run_frame loop (%s) = %.2f, spreads %.1f%% / %.1f%%; ahead by more than the spread: %s"
                               % (m, md / base, 100 * sp, 100 * base_s, "met" if ok else "NOT met"))
    lines += verdict
    lines.append("fusion kernels, device events around 50 back-to-back launches, us per launch (spread); crops in the mode's dtype; old = rd_scatter_crops "
                 "(one launch per frame), new = rd_scatter_crops_frames (one launch), thresholds = rd_frame_thresholds (two launches)")
    lines.append("%-10s %-5s %18s %18s %8s %18s" % ("case", "crops", "old us", "new us", "old/new", "thresholds us"))
    for m in MODES:
        for F, n in KERNEL_CASES:
            t = kern[m]["F%d_N%d" % (F, n)]
            (o, os_), (nw, ns), (th, ts) = _ms(t["old"]), _ms(t["new"]), _ms(t["thresholds"])
            lines.append("%-10s %-5s %10.1f (%4.1f%%) %10.1f (%4.1f%%) %7.2fx %10.1f (%4.1f%%)" % ("F=%d N=%d" % (F, n), m, o, 100 * os_, nw, 100 * ns, o / nw, th, 100 * ts))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out and not args.small:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
