"""Micro-benchmark of the Scale-Map-Learner batch augmentation (riders_amd.utv_dataset.augment: rd_sml_augment_geom + rd_sml_augment_noise
writing into a captured step's static batch) against what it replaces, GraphedStep.load_batch's device-to-device copies of the same six tensors
(six rd_cast launches), at the flagship shape: B = 16, 288 x 384, radar density 0.002, flip + noise on, with and without a (256, 352) crop.

Each variant runs in a CHILD process of its own (fresh runtime, nothing shared but the GPU), the children one after the other, the whole
sequence `--repeats` times.  A child warms its variant up and then times it two ways, each over `--rounds` windows of at least `--window` s:
  call    device events around back-to-back calls through the Python wrapper -- what a loop pays per call when nothing else overlaps the
          enqueue (max of host enqueue time and device time);
  device  the same calls captured once into a hipGraph of 20 and replayed -- device time per call without the host.
The condition of the issue is judged on the device figure (exit status 1 if it fails): augment(out=static) without crop takes no longer than
twice the copy.  Bytes: the geometry pass and the copy both read 8 planes and write 8 planes of B x H x W floats.

    python tools/bench_sml_augment.py [--out profiles/sml_augment.txt] [--rounds 5] [--window 0.25] [--repeats 2]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, H, W, CROP, DENSITY, PER_GRAPH = 16, 288, 384, (256, 352), 0.002, 20
VARIANTS = ("copy", "augment", "augment_crop")


def child(variant, rounds, window_s, small):
    import numpy as np
    import torch
    from riders_amd import sml_main
    from riders_amd import utv_dataset as U
    from riders_amd.rcnet_main import GraphedStep
    if not torch.cuda.is_available():
        sys.exit("bench_sml_augment: needs a GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    b, h, w, crop = (2, 32, 64, (24, 48)) if small else (B, H, W, CROP)
    batch = sml_main.synthetic_batch(b, h, w, seed=11, device=dev)      # radar density 0.002
    static = tuple(torch.empty_like(t) for t in batch)
    rs = np.random.RandomState(5)
    shape = crop if variant == "augment_crop" else None
    rows, vec, offsets = np.zeros((b, 8), np.float32), [], [0]
    radar = batch[2].cpu().numpy()
    for i in range(b):
        rows[i, 3] = i % 2
        rows[i, 4] = 1
        if shape is not None:
            rows[i, :3] = (1, rs.randint(0, w - shape[1]), rs.randint(0, h - shape[0]))
            n = U.count_positive_after_crop(radar[i, 0], int(rows[i, 2]), int(rows[i, 1]), shape, (U.bilinear_taps(shape[1], w), U.bilinear_taps(shape[0], h)))
        else:
            n = int((radar[i, 0] > 0).sum())
        vec.append(rs.normal(-0.01, 0.01, n))
        offsets.append(offsets[-1] + n)
    params, noise, off = torch.from_numpy(rows).to(dev), torch.from_numpy(np.concatenate(vec)).to(dev), torch.tensor(offsets, dtype=torch.int32, device=dev)
    if variant == "copy":
        holder = types.SimpleNamespace(static_batch=static)      # load_batch reads nothing else of a step
        fn = lambda: GraphedStep.load_batch(holder, batch)       # noqa: E731
    else:
        fn = lambda: U.augment(batch, params, noise, off, out=static, random_shape=shape)      # noqa: E731

    def window(run, iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            run()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) * 1e-3

    def measure(run, per):
        n = 5
        while True:
            sec = window(run, n)
            if sec >= window_s or n >= 1 << 18:
                break
            n = max(n + 1, int(n * min(8.0, 1.2 * window_s / max(sec, 1e-6))))
        return [window(run, n) / (n * per) * 1e6 for _ in range(rounds)]
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    if variant != "copy":
        U.check_noise_overflow()
    call_us = measure(fn, 1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        fn()
        with torch.cuda.graph(graph, stream=side):
            for _ in range(PER_GRAPH):
                fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    device_us = measure(graph.replay, PER_GRAPH)
    if variant != "copy":
        U.check_noise_overflow()
    print("RESULT " + json.dumps(dict(variant=variant, call_us=call_us, device_us=device_us, pixels=b * h * w)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25, help="least seconds per timed window")
    ap.add_argument("--repeats", type=int, default=2, help="how often the sequence of children is run")
    ap.add_argument("--small", action="store_true", help="B = 2, 32 x 64 (rehearsal of the script, not a measurement)")
    ap.add_argument("--child", default=None, choices=VARIANTS)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.rounds, args.window, args.small)
    res = {v: dict(call_us=[], device_us=[]) for v in VARIANTS}
    pixels = 0
    for _ in range(args.repeats):
        for v in VARIANTS:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", v, "--rounds", str(args.rounds), "--window", str(args.window)] + (["--small"] if args.small else [])
            r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=240)
            line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")]
            if r.returncode != 0 or not line:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                sys.exit("bench_sml_augment: child %s failed (exit status %d)" % (v, r.returncode))
            d = json.loads(line[-1][7:])
            pixels = d["pixels"]
            for k in ("call_us", "device_us"):
                res[v][k] += d[k]
    nbytes = 16 * pixels * 4      # 8 planes read + 8 planes written
    lines = ["SML batch augmentation vs GraphedStep.load_batch's device copies, %d pixels per plane x 8 planes, fp32; every variant in children of its own, "
             "%d runs x %d windows >= %.2f s; medians in us, spread = (max - min) / median" % (pixels, args.repeats, args.rounds, args.window),
             "bytes moved by the copy and by the geometry pass: %.1f MB (8 planes read, 8 written); the noise pass adds two reads of the radar plane (%.1f MB each, "
             "L2 / MALL resident) and the sparse writes" % (nbytes / 1e6, pixels * 4 / 1e6),
             "%-14s %22s %8s   %22s" % ("variant", "device us (spread)", "TB/s", "per call us (spread)")]
    med = {}
    for v in VARIANTS:
        m = {k: statistics.median(res[v][k]) for k in ("call_us", "device_us")}
        s = {k: (max(res[v][k]) - min(res[v][k])) / m[k] for k in m}
        med[v] = m["device_us"]
        lines.append("%-14s %14.1f (%4.1f%%) %8.2f   %14.1f (%4.1f%%)" % (v, m["device_us"], 100 * s["device_us"], nbytes / (m["device_us"] * 1e-6) / 1e12,
                                                                       m["call_us"], 100 * s["call_us"]))
    ok = med["augment"] <= 2.0 * med["copy"]
    lines.append("augment(out=static) without crop / copy = %.2f (device time); condition <= 2.00: %s" % (med["augment"] / med["copy"], "met" if ok else "NOT met"))
    lines.append("with the (%d, %d) crop / copy = %.2f (reported, no condition)" % (CROP[0], CROP[1], med["augment_crop"] / med["copy"]))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out and not args.small:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
