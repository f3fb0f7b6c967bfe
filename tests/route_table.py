"""The pinned kernel-route table: for a fixed list of convolution descriptors (and routing options), what every host-side routing query of the
C ABI answers -- kernel names, statistics rows, fusion / addend / gather support, workspace sizes.  Only host code runs, nothing is launched or
allocated, so the same table is checked against the emulator build on the CPU and against the GPU library (tests/test_route_table.py).

tests/route_table.jsonl was recorded at commit cd9c834 ("Direct parity tests for layout, LayerNorm, loss and Adam kernels"), the parent of the
change that gave rd_conv.hip one route function per side, with

    python -m tests.route_table            # writes tests/route_table.jsonl from the emulator build

Re-recording at a later commit must give no diff unless a route, a threshold or an option changed on purpose.
"""
import ctypes
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE = os.path.join(HERE, "route_table.jsonl")
FIELDS = ("dtype", "N", "Hin", "Win", "C1", "C2", "upsample", "H1", "W1", "Cout", "KH", "KW", "stride", "pad", "in_dilate", "OH", "OW", "act",
          "slope", "D1", "out_reduce2", "out_d2s", "in_s2d")
DTYPES = (0, 1, 2)      # RD_F32, RD_BF16, RD_F16


def D(dt, N, H, W, C1, Cout, k=3, s=1, pad=None, dil=1, C2=0, up=None, D1=None, OH=None, OW=None, d2s=0, s2d=0):
    """a descriptor as the engine builds it; up = (H1, W1) of the nearest-upsampled first source; dil = 2 with OH / OW given: a data gradient"""
    pad = k // 2 if pad is None else pad
    if OH is None:
        OH, OW = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    H1, W1 = up if up else (H, W)
    return dict(zip(FIELDS, (dt, N, H, W, C1, C2, 1 if up else 0, H1, W1, Cout, k, k, s, pad, dil, OH, OW, 0, 0.0, Cout if D1 is None else D1, 0, d2s, s2d)))


def entries():
    """[(descriptor, [option settings])]: a conditioned cross product built to reach every forward and weight-gradient route in all three dtypes"""
    out = []

    def add(d, *opts):
        out.append((d, [dict(o) for o in (opts or ({},))]))

    for dt in DTYPES:
        es = 4 if dt == 0 else 2
        ve = 16 // es
        # ---- 1x1 forms: skinny (C1 >= 1024, M x Cout <= 64 K; with pw_min_m = 0 and at M = 2048 it overlaps the pointwise kernel), direct, pw, GEMM
        add(D(dt, 1, 1, 48, 1024, 64, k=1), {}, {"pw_min_m": 0})
        add(D(dt, 1, 32, 64, 1024, 16, k=1), {}, {"pw_min_m": 0})
        add(D(dt, 1, 1, 240, 2688, 128, k=1))
        for C1 in (16, 64):
            add(D(dt, 2, 64, 64, C1, 48, k=1))                                         # natural M = 8192
            add(D(dt, 1, 8, 9, C1, 48, k=1), {}, {"conv1x1_min_m": 0}, {"pw_min_m": 0})
        for C1, Cout in ((136, 816), (816, 232)):
            add(D(dt, 2, 36, 36, C1, Cout, k=1))                                       # natural pw window (16-bit): M = 2592
            add(D(dt, 1, 8, 9, C1, Cout, k=1), {"pw_min_m": 0}, {"pw_min_m": 0, "pw_ks": 8})
        add(D(dt, 8, 36, 36, 136, 816, k=1))                                           # M = 10 368: 64-pixel tiles
        add(D(dt, 2, 16, 16, 256, 256, k=1))
        add(D(dt, 2, 8, 16, 512, 128, k=1))                                            # deep
        add(D(dt, 2, 16, 16, 64, 128, k=1, s=2, pad=0))
        add(D(dt, 2, 9, 7, 30, 20, k=1))                                               # scalar gather
        add(D(dt, 2, 8, 8, 128, 64, k=1, pad=0, dil=2, OH=16, OW=16))                  # data gradient of a 1x1 / stride-2 projection
        # ---- stems: 3 channels padded to the vector width
        for k in (3, 7):
            for Cout in (16, 32):
                add(D(dt, 1, 32, 32, ve, Cout, k=k, s=2), {"conv_stem_min_m": 0})
        add(D(dt, 1, 32, 32, ve, 32, k=7, s=2))
        add(D(dt, 4, 256, 256, ve, 32, k=7, s=2))                                      # natural M = 65 536
        add(D(dt, 4, 256, 256, ve, 32, k=3, s=2))
        # ---- few-channel streaming forms, the c1 head
        few = [D(dt, 1, 16, 20, 3, 3), D(dt, 1, 16, 20, 3, 4), D(dt, 1, 16, 20, 1, 32, k=1), D(dt, 1, 16, 20, 32, 1, k=1), D(dt, 1, 16, 20, 32, 4, k=1),
               D(dt, 1, 16, 16, 32, 3, pad=1, dil=2, OH=32, OW=32)]
        for d in few:
            add(d, {"conv_few_min_m": 0, "wgrad_tiny_min_m": 0})
        add(few[0])
        add(D(dt, 1, 256, 256, 3, 3))                                                  # natural M = 65 536
        add(D(dt, 1, 256, 256, 32, 1, k=1))
        add(D(dt, 1, 128, 128, 32, 3, pad=1, dil=2, OH=256, OW=256))
        add(D(dt, 1, 12, 20, 1, 16))
        add(D(dt, 1, 12, 20, 1, 64))
        # ---- 3x3 / stride 1: small, frag (both MFMA forms), patch, GEMM
        for cb in (32, 64, 128, 256, 512):
            for Cout in (16, 64, 128):
                add(D(dt, 2, 24, 40, cb // es, Cout), {}, {"conv3x3_min_blocks": 0}, {"conv3x3_frag": 0}, {"conv3x3_min_blocks": 0, "conv3x3_frag": 0})
        add(D(dt, 2, 24, 40, 256 // es, 128), {"conv3x3_min_blocks": 0, "frag32_v128": 2})
        add(D(dt, 2, 24, 40, 256 // es, 64), {"conv3x3_min_blocks": 0, "frag32_v64": 3})
        for C, Cout in ((32, 32), (128, 128), (128, 64), (64, 16), (128, 16)):
            add(D(dt, 8, 64, 128, C, Cout))                                            # natural M = 65 536 (Cout = 16: the patch-staged kernel)
        add(D(dt, 8, 13, 93, 128, 128))                                                # deep encoder stage: 9 672 pixels
        add(D(dt, 2, 9, 7, 30, 20))
        # ---- gather and store forms
        for C1, D1 in ((32, 16), (64, 32), (128, 64), (64, 16)):
            add(D(dt, 2, 16, 24, C1, 4 * D1, D1=D1, d2s=1), {}, {"conv3x3_frag": 0})
        add(D(dt, 8, 64, 128, 64, 128, D1=32, d2s=1))
        for C1, Cout in ((128, 64), (256, 128), (64, 32)):
            add(D(dt, 2, 16, 24, C1, Cout, s2d=1), {}, {"conv3x3_frag": 0})
        add(D(dt, 8, 64, 128, 128, 64, s2d=1))
        for C1, C2 in ((32, 0), (32, 32), (64, 64)):
            add(D(dt, 2, 16, 24, C1, 64, C2=C2, up=(8, 12)), {"conv3x3_min_blocks": 0})
        add(D(dt, 2, 17, 23, 32, 32, C2=32, up=(4, 3)))
        add(D(dt, 2, 32, 48, 64, 128, s=2))
        add(D(dt, 8, 128, 128, 64, 128, s=2))
        add(D(dt, 2, 16, 24, 3, 32, s=2))
        for C1, Cout in ((128, 64), (64, 64), (48, 24)):
            add(D(dt, 2, 8, 12, C1, Cout, pad=1, dil=2, OH=16, OW=24), {}, {"conv_par": 0})      # the parity-class walk
        add(D(dt, 8, 64, 64, 128, 64, pad=1, dil=2, OH=128, OW=128))
        add(D(dt, 2, 24, 40, 64, 96, D1=32), {}, {"conv3x3_min_blocks": 0})
        add(D(dt, 2, 16, 16, 256, 96, k=1, D1=64))
        # ---- weight gradient: tiny, transpose-read (8 x TW and map-fitted), halo, bf16 MFMA, generic
        add(D(dt, 1, 16, 20, 3, 4), {"wgrad_tiny_min_m": 0})
        for Cin, Cout in ((16, 16), (32, 32), (64, 16), (64, 32)):
            add(D(dt, 2, 24, 40, Cin, Cout))
        for Cin, Cout in ((128, 64), (384, 256)):
            add(D(dt, 2, 30, 40, Cin, Cout), {}, {"wgrad_fit": 1}, {"wgrad_tr_tw": 8})
        add(D(dt, 8, 60, 80, 256, 128), {}, {"wgrad_fit": 1})
        add(D(dt, 2, 5, 70, 128, 64))                                                   # poorly covered map: off the transpose-read kernels
        add(D(dt, 2, 32, 32, 8, 32, k=7, s=2))
        add(D(dt, 2, 16, 16, 33, 17))
        add(D(dt, 2, 16, 16, 36, 20, k=1))
    return out


# kernel families (regular expressions over the whole name) every dtype's part of the table must show: one per enumerator of ConvRoute / WgradRoute
# and per implicit-GEMM walk, so that a shrunken descriptor list fails here instead of hiding a route
FWD_ALL = (r"^linear_skinny_kernel<", r"^conv_stem_kernel$", r"^conv_few_kernel$", r"^conv1x1_direct_kernel$", r"^pw_gemm_kernel<", r"^conv3x3_c1_kernel$",
           r"^conv3x3_small_kernel<[^,]+, \d+, \d+, \w+, \w+>$", r"^conv3x3_frag_kernel<.*, false, false>$", r"^conv3x3_patch_kernel<",
           r"^conv_gemm_kernel<.*, false, false>$", r"^conv_gemm_kernel<.*, true, true>$", r"^conv_gemm_kernel<.*, true, false>$",
           r"^conv_gemm_kernel<.*, false, true>$")      # (implicit GEMM: plain, deep + parity walk, deep, parity walk)
FWD_16 = (r"^conv3x3_frag32_kernel<", r"^conv3x3_frag_kernel<.*, false, false, true>$", r"^conv3x3_frag_kernel<.*, false, true, false>$",
          r"^conv3x3_small_kernel<[^,]+, 4, 64, \w+, false, true>$")      # the 32x32x16 form; s2d, d2s (frag), d2s (small)
WG_ALL = (r"^conv_wgrad_tiny_kernel$", r"^conv_wgrad_kernel$")
WG_32 = (r"^conv_wgrad_halo_kernel$",)      # (16-bit: every shape the halo kernel takes goes to the transpose-read kernel first)
WG_16 = (r"^conv3x3_wgrad_tr_kernel<", r"^conv3x3_wgrad_fit_kernel<", r"^conv_wgrad_bf16_kernel<", r"^conv3x3_wgrad_tr_kernel<.*, 4, true>$")


def make_desc(fields):
    from riders_amd._lib import ConvDesc
    d = ConvDesc()
    for k, v in fields.items():
        setattr(d, k, v)
    return d


def answers(lib, fields, opts):
    """every routing query's answer for one descriptor under one option setting (options cleared afterwards)"""
    from riders_amd._lib import ConvFusion
    dummy = (ctypes.c_float * 4)()
    p = ctypes.cast(dummy, ctypes.c_void_p).value

    def fusion(want_in, want_bn):
        f = ConvFusion()
        if want_in:
            f.in_scale, f.in_shift = p, p
        if want_bn:
            f.bn_y, f.bn_scale, f.bn_shift, f.bn_mean, f.bn_rstd = p, p, p, p, p
        return f

    fus = {"in": fusion(True, False), "bn": fusion(False, True), "both": fusion(True, True)}
    d = ctypes.byref(make_desc(fields))
    lib.rd_clear_options()
    try:
        for k, v in opts.items():
            assert lib.rd_set_option(k.encode(), v) == 0, k
        a = {"fwd": lib.rd_conv_fwd_kernel_name(d).decode(), "stats_rows": lib.rd_conv_stats_rows(d), "add_ok": lib.rd_conv_add_ok(d),
             "reduce2_ok": lib.rd_conv_out_reduce2_ok(d), "up2_ok": lib.rd_conv_up2_ok(d), "up2_dgrad_ok": lib.rd_conv_up2_dgrad_ok(d),
             "fwd_streams": lib.rd_conv_fwd_streams(d), "wgrad": lib.rd_conv_wgrad_kernel_name(d).decode(), "wgrad_streams": lib.rd_conv_wgrad_streams(d),
             "wgrad_ws": lib.rd_conv_wgrad_workspace_bytes(d), "ws": [lib.rd_workspace_bytes(op, d) for op in range(4)]}
        for tag, f in fus.items():
            a["fused_" + tag] = lib.rd_conv_fused_kernel_name(d, ctypes.byref(f)).decode()
            a["fusion_ok_" + tag] = lib.rd_conv_fusion_ok(d, ctypes.byref(f))
            a["wgrad_fused_" + tag] = lib.rd_conv_wgrad_fused_kernel_name(d, ctypes.byref(f)).decode()
            a["wgrad_fusion_ok_" + tag] = lib.rd_conv_wgrad_fusion_ok(d, ctypes.byref(f))
        return a
    finally:
        lib.rd_clear_options()


# storage: one JSON line per descriptor, {"d": descriptor values in FIELDS order, "runs": [[options, answers in KEYS order], ...]}; a fused kernel
# name equal to the unfused one of its side is written "="
KEYS = ("fwd", "fused_in", "fused_bn", "fused_both", "wgrad", "wgrad_fused_in", "wgrad_fused_bn", "wgrad_fused_both", "stats_rows", "add_ok",
        "reduce2_ok", "up2_ok", "up2_dgrad_ok", "fwd_streams", "wgrad_streams", "fusion_ok_in", "fusion_ok_bn", "fusion_ok_both",
        "wgrad_fusion_ok_in", "wgrad_fusion_ok_bn", "wgrad_fusion_ok_both", "wgrad_ws", "ws")


def pack(a):
    base = {k: (a["wgrad"] if k.startswith("wgrad") else a["fwd"]) for k in KEYS if "fused" in k}
    return ["=" if k in base and a[k] == base[k] else a[k] for k in KEYS]


def unpack(v):
    a = dict(zip(KEYS, v))
    for k in KEYS:
        if "fused" in k and a[k] == "=":
            a[k] = a["wgrad"] if k.startswith("wgrad") else a["fwd"]
    return a


def record(lib):
    return [{"d": [f[k] for k in FIELDS], "runs": [[o, pack(answers(lib, f, o))] for o in opts]} for f, opts in entries()]


def load_table():
    with open(TABLE) as fh:
        rows = [json.loads(line) for line in fh if line.strip()]
    return [{"d": r["d"], "runs": [[o, unpack(a)] for o, a in r["runs"]]} for r in rows]


def dump(rows):
    return "".join(json.dumps(r, sort_keys=True, separators=(",", ":")) + "\n" for r in rows)


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.join(HERE, ".."))
    from riders_amd import _lib
    from tests.emu import build_emu
    rows = record(_lib._bind(ctypes.CDLL(build_emu.build())))
    with open(TABLE, "w") as fh:
        fh.write(dump(rows))
    print("%s: %d descriptors, %d entries" % (TABLE, len(rows), sum(len(r["runs"]) for r in rows)))
