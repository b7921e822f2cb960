#!/usr/bin/env python3
"""ms per 64-picture frame index for the resized RGBA outputs (h263mi_rgba_resize), 64 x 1080p, records resident as events
(bench.py's Workload), H263MI_CFG_PIPELINE_POST, launch timing (h263mi_batch_timing_*):

  default      today's output (the default kernels)
  layout_f4    h263mi_rgba_layout scale_log2 = 2
  r480x270     a resize to 480 x 270: 1/4 of 1080p, routed to the layout kernels (should equal layout_f4)
  r640x360, r960x540, r1280x720   k_frame into the scratch, then k_rgba_resize

For each: wall-clock ms per frame index (the decode calls of a GOP and the sync behind them, over the GOP) and the k_frame ms
per launch.  For the resizes that need it, k_rgba_resize's own ms per launch -- the timed post-processing chains of the run
less the default's (the resize counts as post-processing; the final flush k_post is the same in both) -- and its bytes
(4wh read + 4W'H' written per picture) over that time, against the copy ceiling of h263mi_probe_bandwidth measured in the
same process.  Then the mixed wall: a mixed-size set of 64 streams (176x144, 320x240, 352x288, 1920x1080, 16 each) into
320 x 180 tiles, wall-clock ms per call, against the same set at full size.  Prints one JSON line.

    python tools/bench_rgba_resize.py [--gop 31] [--rounds 3]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "h263-rs_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

import h263mi  # noqa: E402

W, H, N = 1920, 1080, 64


def shapes():
    return {
        "default": None,
        "layout_f4": ("layout", 2),
        "r480x270": ("resize", 480, 270),
        "r640x360": ("resize", 640, 360),
        "r960x540": ("resize", 960, 540),
        "r1280x720": ("resize", 1280, 720),
    }


def time_shape(wl, shape, gop, rounds):
    import bench
    b = h263mi.Batch(N, W, H, 0, None, pipeline_post=True)
    if shape is None:
        nbytes = N * W * H * 4
    elif shape[0] == "layout":
        b.set_rgba_layout(shape[1])
        nbytes = h263mi.rgba_layout_extent(N, W, H, shape[1])[2]
    else:
        b.set_rgba_resize(shape[1], shape[2])
        nbytes = h263mi.rgba_resize_extent(N, shape[1], shape[2])
    out = h263mi.DeviceBuffer(nbytes)
    best = None
    for r in range(rounds + 1):                              # (round 0: warm-up)
        b.timing_reserve(8 * gop)
        b.timing_begin()
        t0 = time.perf_counter()
        for f in range(gop):
            fr = wl.frames[f]
            if fr.get("first") is not None:
                b.decode_events(fr["ptype"], fr["mbs"].ptr, fr["first"].ptr, fr["ev"].ptr, fr["base"].ptr, 0, bench.STRENGTH,
                                out.ptr, None)
            else:
                b.decode(fr["ptype"], fr["mbs"].ptr, fr["co"].ptr, fr["base"].ptr, 0, bench.STRENGTH, out.ptr, None)
        b.sync()
        wall = (time.perf_counter() - t0) * 1e3 / gop
        kt = b.timing_end()
        row = {"wall_ms": wall, "k_frame_ms": kt.frame_ms / max(kt.frame_launches, 1), "post_ms": kt.post_ms,
               "post_launches": kt.post_launches}
        if r and (best is None or row["wall_ms"] < best["wall_ms"]):
            best = row
    b.close()
    return best


def mixed_ms(resize, calls=8, reps=3):
    import fixture_enc
    sizes = [(176, 144), (320, 240), (352, 288), (1920, 1080)] * 16
    per_size = {}
    for w, h in set(sizes):
        per_size[(w, h)] = fixture_enc.corpus(7, sizes.count((w, h)), calls, w, h, [8] * 16)
    streams, k = [], {}
    for sz in sizes:
        i = k.get(sz, 0)
        k[sz] = i + 1
        streams.append(per_size[sz][i])
    m = h263mi.MixedBatch(len(sizes), pipeline_post=True)
    if resize:
        m.set_rgba_resize(320, 180)
        bufs = [h263mi.DeviceBuffer(320 * 180 * 4) for _ in sizes]
    else:
        bufs = [h263mi.DeviceBuffer(w * h * 4) for w, h in sizes]
    best = None
    for r in range(reps + 1):
        for s in range(len(sizes)):
            m.reset_stream(s)
        t0 = time.perf_counter()
        for f in range(calls):
            m.decode_next_pictures([st[f] for st in streams], strength=5, rgba=bufs)
        m.sync()
        ms = (time.perf_counter() - t0) * 1e3 / calls
        if r and (best is None or ms < best):
            best = ms
    m.close()
    return round(best, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gop", type=int, default=31)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-mixed", action="store_true")
    args = ap.parse_args()
    import bench
    wl = bench.Workload(h263mi, N, args.gop, 0, 0, None, events=True)
    copy_gbs = h263mi.probe_bandwidth(h263mi.PROBE_COPY)
    res = {"what": "64 x 1080p, events, pipeline_post, strength %d; best of %d rounds of a %d-picture GOP; ms per frame index"
                   % (bench.STRENGTH, args.rounds, args.gop), "copy_ceiling_GBps": round(copy_gbs, 1)}
    rows = {name: time_shape(wl, shape, args.gop, args.rounds) for name, shape in shapes().items()}
    for name, shape in shapes().items():
        row = rows[name]
        res["wall_ms_" + name] = round(row["wall_ms"], 4)
        res["k_frame_ms_" + name] = round(row["k_frame_ms"], 4)
        if shape is not None and shape[0] == "resize" and row["post_launches"] > rows["default"]["post_launches"] + 1:
            # gop resize launches: gop - 1 behind the k_frame launches, one behind the final flush
            ms = (row["post_ms"] - rows["default"]["post_ms"]) / args.gop
            moved = N * (4 * W * H + 4 * shape[1] * shape[2])
            res["k_rgba_resize_ms_" + name] = round(ms, 4)
            res["k_rgba_resize_GBps_" + name] = round(moved / (ms * 1e-3) / 1e9, 1)
            res["k_rgba_resize_of_ceiling_" + name] = round(moved / (ms * 1e-3) / 1e9 / copy_gbs, 3)
    if not args.no_mixed:
        res["mixed_wall_full_ms"] = mixed_ms(False)
        res["mixed_wall_320x180_ms"] = mixed_ms(True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
