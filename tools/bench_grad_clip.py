"""What global-norm gradient clipping costs: rd_grad_norm_partial against rd_grad_finite_check on the same arena (both read 4 bytes per
parameter), rd_grad_clip_finalize alone, rd_adam_step_groups_clipped against rd_adam_step_groups and rd_adam_step_groups_scaled, and a whole
FlatAdam.step() with clipping off and on in the default and the dynamic loss-scale mode, on arenas of the two models' sizes.  Protocol of
tools/bench_loss_scale.py: device events after a warm-up; within one round every variant runs in turn, `--inner` calls at a time, until each has
filled `--seconds`; the alternation is repeated `--rounds` times; medians, each variant with its own spread between rounds.  The whole step is also
timed on the host clock, because a step is a handful of launches issued from Python.  The compiler's resource report of the new kernels and of the
two existing group kernels is appended when hipcc is at hand.

python tools/bench_grad_clip.py [--out profiles/grad_clip.txt]"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from riders_amd import _lib, build, engine  # noqa: E402
from riders_amd.optim import DynamicLossScale, FlatAdam  # noqa: E402
from tools.bench_adam import ARENAS, table  # noqa: E402
from tools.bench_loss_scale import measure, median, spread  # noqa: E402

KERNELS = (("adam_groups_kernel", "adam_groups_kernel (rd_adam_step_groups)"),
           ("adam_groups_scaled_kernel", "adam_groups_scaled_kernel (rd_adam_step_groups_scaled)"),
           ("adam_groups_clipped_kernel", "adam_groups_clipped_kernel (rd_adam_step_groups_clipped, static form)"),
           ("adam_groups_scaled_clipped_kernel", "adam_groups_scaled_clipped_kernel (rd_adam_step_groups_clipped, live-state form)"),
           ("grad_finite_kernel", "grad_finite_kernel (rd_grad_finite_check)"),
           ("grad_norm_kernelILb0EE", "grad_norm_kernel<L2> (rd_grad_norm_partial)"),
           ("grad_norm_kernelILb1EE", "grad_norm_kernel<inf> (rd_grad_norm_partial)"),
           ("grad_clip_finalize_kernel", "grad_clip_finalize_kernel (rd_grad_clip_finalize)"))


def resource_report():
    """-> lines: VGPRs / SGPRs / scratch / LDS / occupancy of the optimizer kernels, from -Rpass-analysis=kernel-resource-usage"""
    if not os.path.exists(build.HIPCC):
        return ["Compiler report: no hipcc here"]
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([build.HIPCC, "-x", "hip"] + build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(build.CSRC, "rd_optim.hip"),
                            "-o", os.path.join(tmp, "rd_optim.o")], capture_output=True, text=True)
    if r.returncode != 0:
        return ["Compiler report: hipcc failed: " + r.stderr[-300:]]
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([\w /\[\]]+?):\s+(\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    lines = ["Compiler report (gfx950, -Rpass-analysis=kernel-resource-usage):"]
    for key, label in KERNELS:
        for name, f in sorted(out.items()):
            if "rd_f16" in name or not re.search(r"\d" + re.escape(key) + r"(E|$)", name if "IL" in key else name.replace("IL", "\0")):
                continue
            lines.append("  %s: %d VGPRs, %d SGPRs, scratch %d bytes/lane, spills %d / %d, LDS %d bytes/block, occupancy %d waves per SIMD" % (
                label, f.get("VGPRs", -1), f.get("TotalSGPRs", -1), f.get("ScratchSize [bytes/lane]", -1), f.get("SGPRs Spill", -1), f.get("VGPRs Spill", -1),
                f.get("LDS Size [bytes/block]", -1), f.get("Occupancy [waves/SIMD]", -1)))
    return lines


def row(key, xs, nbytes=None, against=None):
    text = "  %-26s %s   median %.2f us" % (key, "  ".join("%.2f" % u for u in xs), median(xs))
    if nbytes:
        text += " (%.0f GB/s)" % (nbytes / median(xs) * 1e-3)
    text += "   own spread between rounds %.2f %%" % spread(xs)
    if against is not None:
        text += "   %+.2f us (%+.2f %%) against %s" % (median(xs) - median(against[1]), 100.0 * (median(xs) / median(against[1]) - 1.0), against[0])
    return text


def step_bench(dev, n, dynamic, seconds, rounds, inner):
    """a whole FlatAdam.step() on an arena of one n-element parameter, clipping off / on -> ({variant: device us per step}, {variant: host us per step})"""
    opts = {}
    for clip in (False, True):
        p = torch.nn.Parameter(torch.randn(n, device=dev))
        opt = FlatAdam([p], lr=2e-4)
        if dynamic:
            opt.loss_scale = DynamicLossScale(init_scale=1.0, growth_interval=1 << 30, device=dev)
        if clip:
            opt.set_grad_clip(1.0)
        opt._grad_view(p).normal_(std=1e-3)

        def step(o=opt):
            o.mark_touched([0])
            o.step()
            return 0
        opts["clip on" if clip else "clip off"] = step
    variants = sorted(opts.items())
    res = measure(variants, seconds, rounds, inner)
    host = {}
    for key, fn in variants:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(200):
            fn()
        torch.cuda.synchronize()
        host[key] = (time.perf_counter() - t0) / 200 * 1e6
    engine.set_param_grad_allocator(None)
    return res, host


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.3, help="device time every variant fills per round")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--inner", type=int, default=50, help="calls of one variant between two events")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_grad_clip.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    lib = engine.L()
    rows_ = _lib.RD_GRAD_NORM_ROWS
    lines = ["Global-norm gradient clipping: us per call, %d rounds of >= %.2f s per variant, variants alternating every %d calls" % (a.rounds, a.seconds, a.inner)]
    state = torch.zeros(8, dtype=torch.int32, device=dev)
    engine._chk(lib.rd_loss_scale_init(engine._p(state), 1.0, 0, engine._stream(state)), "rd_loss_scale_init")
    clip = torch.zeros(8, dtype=torch.int32, device=dev)
    engine._chk(lib.rd_grad_clip_init(engine._p(clip), engine._stream(clip)), "rd_grad_clip_init")
    partial = torch.zeros(rows_, dtype=torch.float64, device=dev)
    flag = torch.zeros(2, dtype=torch.int32, device=dev)
    for name, n, split in ARENAS:
        torch.manual_seed(0)
        p, g = torch.randn(n, device=dev), torch.randn(n, device=dev) * 1e-3
        m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        st = engine._stream(p)
        ptrs = (engine._p(p), engine._p(g), engine._p(m), engine._p(v))
        lines.append("%s arena, %d parameters" % (name, n))
        reads = [("finite check", lambda: lib.rd_grad_finite_check(engine._p(g), n, engine._p(flag), st)),
                 ("norm L2", lambda: lib.rd_grad_norm_partial(engine._p(g), n, 1.0, None, _lib.GRAD_NORM_L2, engine._p(partial), rows_, 0, None, st)),
                 ("norm L2 + flag + state", lambda: lib.rd_grad_norm_partial(engine._p(g), n, 1.0, engine._p(state), _lib.GRAD_NORM_L2, engine._p(partial), rows_, 0,
                                                                           engine._p(flag), st)),
                 ("norm inf", lambda: lib.rd_grad_norm_partial(engine._p(g), n, 1.0, None, _lib.GRAD_NORM_INF, engine._p(partial), rows_, 0, None, st))]
        res = measure(reads, a.seconds, a.rounds, a.inner)
        lines.append(" one read of the arena (4 bytes per parameter)")
        for key, _ in reads:
            lines.append(row(key, res[key], 4.0 * n, None if key == "finite check" else ("the finite check", res["finite check"])))
        t1 = table(n, [n], 10)
        adams = [("groups (skip flag)", lambda: lib.rd_adam_step_groups(*ptrs, n, t1, 1.0, engine._p(flag), st)),
                 ("clipped (skip flag)", lambda: lib.rd_adam_step_groups_clipped(*ptrs, n, t1, 1.0, engine._p(flag), None, 0, engine._p(clip), st)),
                 ("scaled", lambda: lib.rd_adam_step_groups_scaled(*ptrs, n, t1, 1.0, engine._p(state), 0, st)),
                 ("clipped (live state)", lambda: lib.rd_adam_step_groups_clipped(*ptrs, n, t1, 1.0, None, engine._p(state), 0, engine._p(clip), st))]
        res = measure(adams, a.seconds, a.rounds, a.inner)
        assert bool(torch.isfinite(p).all())
        lines.append(" the Adam launch (28 bytes per parameter, one group)")
        lines.append(row("groups (skip flag)", res["groups (skip flag)"], 28.0 * n))
        lines.append(row("clipped (skip flag)", res["clipped (skip flag)"], 28.0 * n, ("groups (skip flag)", res["groups (skip flag)"])))
        lines.append(row("scaled", res["scaled"], 28.0 * n))
        lines.append(row("clipped (live state)", res["clipped (live state)"], 28.0 * n, ("scaled", res["scaled"])))
        del p, g, m, v
        for dynamic in (False, True):
            res, host = step_bench(dev, n, dynamic, a.seconds, a.rounds, a.inner)
            lines.append(" FlatAdam.step(), %s mode (device events around %d steps issued from Python; host clock per step: off %.1f us, on %.1f us)" % (
                "dynamic loss-scale" if dynamic else "default", a.inner, host["clip off"], host["clip on"]))
            lines.append(row("clip off", res["clip off"]))
            lines.append(row("clip on", res["clip on"], None, ("clip off", res["clip off"])))
    st = engine._stream(clip)
    small = [("rd_grad_clip_finalize", lambda: lib.rd_grad_clip_finalize(engine._p(partial), rows_, 1.0, _lib.GRAD_NORM_L2, engine._p(clip), st)),
             ("rd_adam_skip_count", lambda: lib.rd_adam_skip_count(engine._p(flag), st))]
    res = measure(small, a.seconds / 3, a.rounds, a.inner)
    lines.append("the single-block launches, us per launch back to back")
    for key, _ in small:
        lines.append(row(key, res[key]))
    lines.append("")
    lines += resource_report()
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
