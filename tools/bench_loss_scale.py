"""What the dynamic loss scale costs per launch: rd_adam_step_groups_scaled against rd_adam_step_groups with a skip flag (the static fp16 mode's
launch) on arenas of the two models' sizes, and rd_loss_scale_update against rd_adam_skip_count.  The scaled kernel's extra work is per block
(two double-precision pow per group on eight threads, one barrier), not per element, so the expectation is equality within
rd_adam_step_groups' own spread between rounds.  Protocol of tools/bench_adam.py: device events after a warm-up; within one round every variant
runs in turn, `--inner` launches at a time, until each has filled `--seconds`; the alternation is repeated `--rounds` times.  The compiler's
resource report of both group kernels is appended when hipcc is at hand.

python tools/bench_loss_scale.py [--out profiles/loss_scale.txt]"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from riders_amd import _lib, build, engine  # noqa: E402
from tools.bench_adam import ARENAS, B1, B2, EPS, LR, table  # noqa: E402


def resource_report():
    """-> lines: VGPRs / SGPRs / scratch / LDS / occupancy of the two group kernels, from -Rpass-analysis=kernel-resource-usage"""
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
    for key, label in (("adam_groups_kernel", "adam_groups_kernel (rd_adam_step_groups)"), ("adam_groups_scaled_kernel", "adam_groups_scaled_kernel (rd_adam_step_groups_scaled)")):
        for name, f in sorted(out.items()):
            if "rd_f16" in name or key + "E" not in name:
                continue
            lines.append("  %s: %d VGPRs, %d SGPRs, scratch %d bytes/lane, spills %d / %d, LDS %d bytes/block, occupancy %d waves per SIMD" % (
                label, f.get("VGPRs", -1), f.get("TotalSGPRs", -1), f.get("ScratchSize [bytes/lane]", -1), f.get("SGPRs Spill", -1), f.get("VGPRs Spill", -1),
                f.get("LDS Size [bytes/block]", -1), f.get("Occupancy [waves/SIMD]", -1)))
    return lines


def measure(variants, seconds, rounds, inner):
    for _, fn in variants:      # warm-up: code objects, clocks
        for _ in range(20):
            engine._chk(fn(), "warm-up")
    torch.cuda.synchronize()
    res = {k: [] for k, _ in variants}
    for _ in range(rounds):
        tot = {k: [0.0, 0] for k, _ in variants}
        while min(t[0] for t in tot.values()) < seconds * 1e3:
            for key, fn in variants:
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(inner):
                    fn()
                e.record()
                e.synchronize()
                tot[key][0] += s.elapsed_time(e)
                tot[key][1] += inner
        for key in tot:
            res[key].append(tot[key][0] * 1e3 / tot[key][1])
    return res


def median(xs):
    return sorted(xs)[len(xs) // 2]


def spread(xs):
    return 100.0 * (max(xs) - min(xs)) / min(xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5, help="device time every variant fills per round")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--inner", type=int, default=50, help="launches of one variant between two events")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_loss_scale.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    lib = engine.L()
    lines = ["rd_adam_step_groups (skip flag, the static fp16 mode) vs rd_adam_step_groups_scaled (dynamic loss scale): us per launch (GB/s at 28 bytes per "
             "parameter), %d rounds of >= %.2f s per variant, variants alternating every %d launches" % (a.rounds, a.seconds, a.inner)]
    state = torch.zeros(8, dtype=torch.int32, device=dev)
    engine._chk(lib.rd_loss_scale_init(engine._p(state), 1.0, 0, engine._stream(state)), "rd_loss_scale_init")
    flag = torch.zeros(2, dtype=torch.int32, device=dev)
    for name, n, split in ARENAS:
        torch.manual_seed(0)
        p, g = torch.randn(n, device=dev), torch.randn(n, device=dev) * 1e-3
        m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        st = engine._stream(p)
        ptrs = (engine._p(p), engine._p(g), engine._p(m), engine._p(v))
        tabs = {1: table(n, [n], 10), 2: table(n, [split, n], 10)}
        variants = []
        for k in (1, 2):
            variants.append(("static x%d" % k, lambda t=tabs[k]: lib.rd_adam_step_groups(*ptrs, n, t, 1.0, engine._p(flag), st)))
            variants.append(("scaled x%d" % k, lambda t=tabs[k]: lib.rd_adam_step_groups_scaled(*ptrs, n, t, 1.0, engine._p(state), 0, st)))
        res = measure(variants, a.seconds, a.rounds, a.inner)
        assert bool(torch.isfinite(p).all())
        lines.append("%s arena, %d parameters (x2: 2 groups split at %d)" % (name, n, split))
        for k in (1, 2):
            base, us = res["static x%d" % k], res["scaled x%d" % k]
            lines.append("  static x%d    %s   median %.1f us (%.0f GB/s)   own spread between rounds %.2f %%" % (
                k, "  ".join("%.1f" % u for u in base), median(base), 28.0 * n / median(base) * 1e-3, spread(base)))
            lines.append("  scaled x%d    %s   median %.1f us (%.0f GB/s)   %+.2f %% against static x%d's median" % (
                k, "  ".join("%.1f" % u for u in us), median(us), 28.0 * n / median(us) * 1e-3, 100.0 * (median(us) / median(base) - 1.0), k))
    st = engine._stream(state)
    small = [("rd_adam_skip_count", lambda: lib.rd_adam_skip_count(engine._p(flag), st)),
             ("rd_loss_scale_update", lambda: lib.rd_loss_scale_update(engine._p(state), 2.0, 0.5, 2000, st))]
    res = measure(small, a.seconds / 5, a.rounds, a.inner)
    lines.append("the step's last launch (one thread), us per launch back to back")
    for key, _ in small:
        lines.append("  %-21s %s   median %.2f us   spread %.2f %%" % (key, "  ".join("%.2f" % u for u in res[key]), median(res[key]), spread(res[key])))
    lines.append("")
    lines += resource_report()
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
