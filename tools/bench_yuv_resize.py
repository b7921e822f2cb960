#!/usr/bin/env python3
"""Device ms per launch of k_plane_resize (h263mi_yuv_resize) beside k_rgba_resize at the same geometry, and of k_plane_filter
(h263mi_batch_set_yuv_resize_filtered) beside k_rgba_filter at the same geometry and kind, in one process, on the same buffers:
64 x 1080p, records resident as events (bench.py's Workload), H263MI_CFG_PIPELINE_POST, launch timing (h263mi_batch_timing_*).

  planes_default   d_deblocked without a YUV shape (tight full-size I420): the base of the plane resizes
  rgba_default     d_rgba without an RGBA shape: the base of the RGBA resizes
  yuv_<fmt>_<W'>x<H'>   k_frame into the plane scratch, then k_plane_resize
  rgba_<W'>x<H'>        k_frame into the RGBA scratch, then k_rgba_resize
  yuv_<fmt>_<kind>_<W'>x<H'>   k_frame into the plane scratch, then k_plane_filter (bilinear, bicubic)
  rgba_<kind>_<W'>x<H'>        k_frame into the RGBA scratch, then k_rgba_filter

A resize kernel's ms per launch is the timed post-processing time of its run less its base's, over the GOP's launches (both
resizes count as post-processing; the final flush k_post is the same in a run and its base).  Its bytes: what it reads
(1.5 wh per picture for the planes, 4 wh for RGBA) plus what it writes (1.5 W'H'; 4 W'H'), over that time, against the copy
ceiling of h263mi_probe_bandwidth measured in the same process.  One warm-up round, then the best of --rounds.  Prints one
JSON line.

    python tools/bench_yuv_resize.py [--gop 16] [--rounds 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "h263-rs_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import h263mi  # noqa: E402

W, H, N = 1920, 1080, 64
SIZES = [(640, 360), (1280, 720)]
FORMATS = [("i420", h263mi.YUV_I420), ("nv12", h263mi.YUV_NV12)]
KINDS = [("bilinear", h263mi.FILTER_BILINEAR), ("bicubic", h263mi.FILTER_BICUBIC)]


def time_shape(wl, shape, gop, rounds):
    """shape: ("planes",) | ("rgba",) | ("yuv", fmt, ow, oh[, kind]) | ("rgba", ow, oh[, kind]) -> best round's timings"""
    import bench
    b = h263mi.Batch(N, W, H, 0, None, pipeline_post=True)
    rgba = planes = None
    keep = None
    if shape[0] == "yuv" and len(shape) == 5:
        resize, keep = h263mi.make_yuv_resize(shape[2], shape[3], shape[1])
        b.set_yuv_resize_filtered(resize, h263mi.make_filter(shape[4]))
        planes = h263mi.DeviceBuffer(h263mi.yuv_resize_extent(N, shape[2], shape[3], shape[1]))
    elif shape[0] == "yuv":
        b.set_yuv_resize(shape[2], shape[3], shape[1])
        planes = h263mi.DeviceBuffer(h263mi.yuv_resize_extent(N, shape[2], shape[3], shape[1]))
    elif shape[0] == "planes":
        planes = h263mi.DeviceBuffer(h263mi.yuv_layout_extent(N, W, H, default=True))
    elif len(shape) == 4:
        b.set_rgba_resize_filtered(None, h263mi.make_filter(shape[3]), shape[1], shape[2])
        rgba = h263mi.DeviceBuffer(h263mi.rgba_resize_extent(N, shape[1], shape[2]))
    elif len(shape) == 3:
        b.set_rgba_resize(shape[1], shape[2])
        rgba = h263mi.DeviceBuffer(h263mi.rgba_resize_extent(N, shape[1], shape[2]))
    else:
        rgba = h263mi.DeviceBuffer(N * W * H * 4)
    best = None
    for r in range(rounds + 1):                              # (round 0: warm-up)
        b.timing_reserve(8 * gop)
        b.timing_begin()
        t0 = time.perf_counter()
        for f in range(gop):
            fr = wl.frames[f]
            if fr.get("first") is not None:
                b.decode_events(fr["ptype"], fr["mbs"].ptr, fr["first"].ptr, fr["ev"].ptr, fr["base"].ptr, 0, bench.STRENGTH,
                                rgba.ptr if rgba else None, planes.ptr if planes else None)
            else:
                b.decode(fr["ptype"], fr["mbs"].ptr, fr["co"].ptr, fr["base"].ptr, 0, bench.STRENGTH,
                         rgba.ptr if rgba else None, planes.ptr if planes else None)
        b.sync()
        wall = (time.perf_counter() - t0) * 1e3 / gop
        kt = b.timing_end()
        row = {"wall_ms": wall, "k_frame_ms": kt.frame_ms / max(kt.frame_launches, 1), "post_ms": kt.post_ms}
        if r and (best is None or row["post_ms"] < best["post_ms"]):
            best = row
    b.close()
    del keep
    for d in (rgba, planes):
        if d is not None:
            d.free()
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gop", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import bench
    wl = bench.Workload(h263mi, N, args.gop, 0, 0, None, events=True)
    copy_gbs = h263mi.probe_bandwidth(h263mi.PROBE_COPY)
    res = {"what": "64 x 1080p, events, pipeline_post, strength %d; one warm-up round, best of %d rounds of a %d-picture GOP; "
                   "resize kernels: device ms per launch (64 pictures)" % (bench.STRENGTH, args.rounds, args.gop),
           "copy_ceiling_GBps": round(copy_gbs, 1)}
    base_planes = time_shape(wl, ("planes",), args.gop, args.rounds)
    base_rgba = time_shape(wl, ("rgba",), args.gop, args.rounds)
    res["k_frame_ms_planes_default"] = round(base_planes["k_frame_ms"], 4)
    res["k_frame_ms_rgba_default"] = round(base_rgba["k_frame_ms"], 4)

    def record(name, row, base, bytes_per_picture):
        ms = (row["post_ms"] - base["post_ms"]) / args.gop
        moved = N * bytes_per_picture
        res[name + "_ms"] = round(ms, 4)
        res[name + "_bytes"] = moved
        res[name + "_GBps"] = round(moved / (ms * 1e-3) / 1e9, 1) if ms > 0 else None
        res[name + "_of_ceiling"] = round(moved / (ms * 1e-3) / 1e9 / copy_gbs, 3) if ms > 0 else None
        res[name + "_k_frame_ms"] = round(row["k_frame_ms"], 4)

    for ow, oh in SIZES:
        cw, ch, cow, coh = (W + 1) // 2, (H + 1) // 2, (ow + 1) // 2, (oh + 1) // 2
        for fname, fmt in FORMATS:
            row = time_shape(wl, ("yuv", fmt, ow, oh), args.gop, args.rounds)
            record("k_plane_resize_%s_%dx%d" % (fname, ow, oh), row, base_planes, W * H + 2 * cw * ch + ow * oh + 2 * cow * coh)
        row = time_shape(wl, ("rgba", ow, oh), args.gop, args.rounds)
        record("k_rgba_resize_%dx%d" % (ow, oh), row, base_rgba, 4 * W * H + 4 * ow * oh)
        # the filters: k_plane_filter against k_rgba_filter, a kernel of the same geometry and kind that reads 4 bytes per source
        # pixel where the planes hold 1.5
        for kname, kind in KINDS:
            for fname, fmt in FORMATS:
                row = time_shape(wl, ("yuv", fmt, ow, oh, kind), args.gop, args.rounds)
                record("k_plane_filter_%s_%s_%dx%d" % (fname, kname, ow, oh), row, base_planes,
                       W * H + 2 * cw * ch + ow * oh + 2 * cow * coh)
            row = time_shape(wl, ("rgba", ow, oh, kind), args.gop, args.rounds)
            record("k_rgba_filter_%s_%dx%d" % (kname, ow, oh), row, base_rgba, 4 * W * H + 4 * ow * oh)
            for fname, _ in FORMATS:
                a, r = res["k_plane_filter_%s_%s_%dx%d_ms" % (fname, kname, ow, oh)], res["k_rgba_filter_%s_%dx%d_ms" % (kname, ow, oh)]
                res["k_plane_filter_%s_%s_%dx%d_over_rgba_filter" % (fname, kname, ow, oh)] = round(a / r, 3) if r > 0 else None
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
