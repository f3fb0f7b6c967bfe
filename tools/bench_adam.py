"""rd_adam_step against rd_adam_step_groups on arenas of the two models' sizes (RC-Net 5,892,272 and SML 21,320,635 parameters): does the
group lookup cost anything?  Both kernels move the same 28 bytes per parameter.  Variants: rd_adam_step; the grouped launch with 1 group, with 2
groups (RC-Net arena: encoder | decoder at 3,634,528; SML arena: backbone `first.*` + `pretrained.*` | `scratch.*` at 6,422,112) and with 8
groups of equal size.  Device events after a warm-up; within one round every variant runs in turn, `--inner` launches at a time, until each has
filled `--seconds`; the whole alternation is repeated `--rounds` times, which gives rd_adam_step's own spread to read the others against.

python tools/bench_adam.py [--out profiles/adam_groups.txt]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from riders_amd import _lib, engine  # noqa: E402

ARENAS = (("rcnet", 5892272, 3634528), ("sml", 21320635, 6422112))
LR, B1, B2, EPS = 2e-4, 0.9, 0.999, 1e-8


def table(n, ends, step):
    t = _lib.AdamGroups()
    t.count = len(ends)
    for k, e in enumerate(ends):
        t.end[k], t.flags[k], t.step[k] = e, _lib.ADAM_DECOUPLED if k % 2 else 0, step
        t.lr[k], t.beta1[k], t.beta2[k], t.eps[k], t.weight_decay[k] = LR * (1 + k), B1, B2, EPS, 1e-2 if k % 2 else 0.0
    assert ends[-1] == n and all(e % 4 == 0 for e in ends[:-1])
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5, help="device time every variant fills per round")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--inner", type=int, default=50, help="launches of one variant between two events")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_adam.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    lib = engine.L()
    lines = ["rd_adam_step vs rd_adam_step_groups: us per launch (GB/s at 28 bytes per parameter), %d rounds of >= %.2f s per variant, variants alternating "
             "every %d launches" % (a.rounds, a.seconds, a.inner)]
    for name, n, split in ARENAS:
        torch.manual_seed(0)
        p, g = torch.randn(n, device=dev), torch.randn(n, device=dev) * 1e-3
        m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        st = engine._stream(p)
        ptrs = (engine._p(p), engine._p(g), engine._p(m), engine._p(v))
        eight = [(n // 8 // 4 * 4) * (k + 1) for k in range(7)] + [n]
        tabs = {"groups x1": table(n, [n], 10), "groups x2": table(n, [split, n], 10), "groups x8": table(n, eight, 10)}
        variants = [("rd_adam_step", lambda: lib.rd_adam_step(*ptrs, n, LR, B1, B2, EPS, 0.0, 10, 1.0, st))]
        for key in ("groups x1", "groups x2", "groups x8"):
            variants.append((key, lambda t=tabs[key]: lib.rd_adam_step_groups(*ptrs, n, t, 1.0, None, st)))
        for _, fn in variants:      # warm-up: code objects, clocks
            for _ in range(20):
                engine._chk(fn(), "warm-up")
        torch.cuda.synchronize()
        res = {k: [] for k, _ in variants}
        for _ in range(a.rounds):
            tot = {k: [0.0, 0] for k, _ in variants}
            while min(t[0] for t in tot.values()) < a.seconds * 1e3:
                for key, fn in variants:
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record()
                    for _ in range(a.inner):
                        fn()
                    e.record()
                    e.synchronize()
                    tot[key][0] += s.elapsed_time(e)
                    tot[key][1] += a.inner
            for key in tot:
                res[key].append(tot[key][0] * 1e3 / tot[key][1])
        assert bool(torch.isfinite(p).all())
        base = res["rd_adam_step"]
        lines.append("%s arena, %d parameters (2 groups split at %d)" % (name, n, split))
        for key, _ in variants:
            us = res[key]
            mid = sorted(us)[len(us) // 2]
            lines.append("  %-13s %s   median %.1f us (%.0f GB/s)   %+.2f %% against rd_adam_step's median; rd_adam_step's own spread %.2f %%" % (
                key, "  ".join("%.1f" % u for u in us), mid, 28.0 * n / mid * 1e-3, 100.0 * (mid / sorted(base)[len(base) // 2] - 1.0),
                100.0 * (max(base) - min(base)) / min(base)))
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
