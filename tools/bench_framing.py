#!/usr/bin/env python3
"""Device ms per launch of the resize passes with and without a framing (h263mi_framing), for SEVERAL builds of libh263mi.so
in one process (the way of tools/ab_inproc.py: one workload, one set of buffers, the builds interleaved round after round):
64 x 1080p, records resident as events (bench.py's Workload), H263MI_CFG_PIPELINE_POST, launch timing (h263mi_batch_timing_*).

  rgba_<W'>x<H'>, tensor_bf16_<W'>x<H'>      the unframed passes (k_rgba_resize, k_tensor_resize): every build
  ..._letterbox, ..._cover                   the framed passes (k_rgba_resize_framed, k_tensor_resize_framed): builds that
                                             export them; a framing that resolves to whole onto whole (1080p into 640 x 360)
                                             takes the unframed path and is marked "identity"

A pass's ms per launch is the timed post-processing time of its run less that of the default RGBA output of the same build
in the same round, over the GOP's launches.  Give the parent's library twice (two copies of the file) and this tree's once:
`spread_parent_vs_parent` is what the same code shows against itself, `this_vs_parent` must lie inside it for the unframed passes.
One warm-up round, then the mean and the extremes of --rounds.  Prints one JSON line.

    python tools/bench_framing.py [--gop 16] [--rounds 4] parent_a.so parent_b.so this.so
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "h263-rs_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import torch  # noqa: E402,F401  before h263mi: torch brings its own HIP runtime; the C-ABI library must share it (as in bench.py)
import bench  # noqa: E402
import h263mi  # noqa: E402

W, H, N = 1920, 1080, 64
SIZES = [(224, 224), (640, 360)]
SCALE = [1 / (255 * 0.229), 1 / (255 * 0.224), 1 / (255 * 0.225)]
BIAS = [-0.485 / 0.229, -0.456 / 0.224, -0.406 / 0.225]
MODES = {"letterbox": h263mi.FRAME_LETTERBOX, "cover": h263mi.FRAME_COVER}


def shapes(framed):
    out = [("rgba_default", None)]
    for ow, oh in SIZES:
        out.append(("rgba_%dx%d" % (ow, oh), ("rgba", ow, oh, None)))
        out.append(("tensor_bf16_%dx%d" % (ow, oh), ("tensor", ow, oh, None)))
        if framed:
            for mname, mode in MODES.items():
                out.append(("rgba_%dx%d_%s" % (ow, oh, mname), ("rgba", ow, oh, mode)))
                out.append(("tensor_bf16_%dx%d_%s" % (ow, oh, mname), ("tensor", ow, oh, mode)))
    return out


def post_ms(wl, shape, gop, out):
    """timed post-processing ms of one GOP under `shape` (None: the default RGBA output)"""
    b = h263mi.Batch(N, W, H, 0, None, pipeline_post=True)
    if shape is not None:
        kind, ow, oh, mode = shape
        f = h263mi.make_framing(mode, pad=(114, 114, 114)) if mode is not None else None
        if kind == "tensor":
            t = h263mi.make_tensor_out(ow, oh, h263mi.TENSOR_BF16, SCALE, BIAS)
            b.set_tensor_output_framed(t, f) if f is not None else b.set_tensor_output(t)
        else:
            b.set_rgba_resize_framed(f, ow, oh) if f is not None else b.set_rgba_resize(ow, oh)
    ms = None
    for r in range(2):                                       # (the first GOP touches the new frame store and scratch)
        b.timing_reserve(8 * gop)
        b.timing_begin()
        for k in range(gop):
            fr = wl.frames[k]
            if fr.get("first") is not None:
                b.decode_events(fr["ptype"], fr["mbs"].ptr, fr["first"].ptr, fr["ev"].ptr, fr["base"].ptr, 0, bench.STRENGTH, out.ptr, None)
            else:
                b.decode(fr["ptype"], fr["mbs"].ptr, fr["co"].ptr, fr["base"].ptr, 0, bench.STRENGTH, out.ptr, None)
        b.sync()
        ms = b.timing_end().post_ms
    b.close()
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gop", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("libs", nargs="+")
    args = ap.parse_args()
    handles = []
    for path in args.libs:
        h263mi._lib = None
        h263mi.LIB_PATH = os.path.abspath(path)
        handles.append((os.path.basename(path), h263mi.lib(), h263mi._has("h263mi_batch_set_rgba_resize_framed")))
    h263mi._lib = handles[0][1]
    wl = bench.Workload(h263mi, N, args.gop, 0, 0, None, events=True)
    out = h263mi.DeviceBuffer(N * W * H * 4)                 # (holds every shape)
    samples = {name: {} for name, _, _ in handles}
    for rnd in range(args.rounds + 1):                       # (round 0: warm-up)
        for name, L, framed in handles:
            h263mi._lib = L
            base = None
            for sname, shape in shapes(framed):
                ms = post_ms(wl, shape, args.gop, out)
                if shape is None:
                    base = ms
                elif rnd:
                    samples[name].setdefault(sname, []).append((ms - base) / args.gop)
    res = {"what": "64 x 1080p, events, pipeline_post, strength %d; one process, the builds interleaved; one warm-up round, %d rounds "
                   "of a %d-picture GOP; device ms per launch (64 pictures) of the pass behind k_frame: mean [min, max]"
                   % (bench.STRENGTH, args.rounds, args.gop),
           "identity": ["%s_640x360_%s" % (k, m) for k in ("rgba", "tensor_bf16") for m in MODES], "builds": {}}
    mean = lambda v: sum(v) / len(v)
    for name, _, _ in handles:
        res["builds"][name] = {s: [round(mean(v), 4), round(min(v), 4), round(max(v), 4)] for s, v in samples[name].items()}
    if len(handles) >= 3:
        a, b, c = (samples[h[0]] for h in handles[:3])
        res["spread_parent_vs_parent"] = {s: round(mean(b[s]) / mean(a[s]) - 1, 4) for s in a if s in b}
        res["this_vs_parent"] = {s: round(mean(c[s]) / (0.5 * (mean(a[s]) + mean(b[s]))) - 1, 4) for s in a if s in c}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
