#!/usr/bin/env python3
"""k_frame ms per launch for the RGBA output layouts (h263mi_rgba_layout), 64 x 1080p, records resident as events
(bench.py's Workload), H263MI_CFG_PIPELINE_POST, launch timing (h263mi_batch_timing_*):

  default   today's layout (the default kernels)
  f1_p8192  full size, rows 8 192 bytes apart (k_frame_layout<0>)
  f2        1/2, tight
  f4_4k     1/4 into one 3 840 x 2 160 canvas (8 x 8 mosaic)

plus host-to-host ms of h263mi_render_rgba_layout for one CIF state at a 1 536-byte pitch and one 1080p state at 1/4.
Prints one JSON line.

    python tools/bench_rgba_layout.py [--gop 31] [--rounds 3]
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


def layouts():
    return {
        "default": None,
        "f1_p8192": (0, 8192, None),
        "f2": (1, 0, None),
        "f4_4k": (2, 15360, [(s // 8) * 270 * 15360 + (s % 8) * 480 * 4 for s in range(N)]),
    }


def time_layout(wl, lay, gop, rounds):
    import bench
    b = h263mi.Batch(N, W, H, 0, None, pipeline_post=True)
    if lay is None:
        nbytes = N * W * H * 4
    else:
        b.set_rgba_layout(*lay)
        nbytes = h263mi.rgba_layout_extent(N, W, H, *lay)[2]
    out = h263mi.DeviceBuffer(nbytes)
    best = None
    for r in range(rounds + 1):                              # (round 0: warm-up)
        b.timing_reserve(4 * gop)
        b.timing_begin()
        for f in range(gop):
            fr = wl.frames[f]
            if fr.get("first") is not None:
                b.decode_events(fr["ptype"], fr["mbs"].ptr, fr["first"].ptr, fr["ev"].ptr, fr["base"].ptr, 0, bench.STRENGTH,
                                out.ptr, None)
            else:
                b.decode(fr["ptype"], fr["mbs"].ptr, fr["co"].ptr, fr["base"].ptr, 0, bench.STRENGTH, out.ptr, None)
        b.sync()
        kt = b.timing_end()
        ms = kt.frame_ms / max(kt.frame_launches, 1)
        if r and (best is None or ms < best):
            best = ms
    b.close()
    return round(best, 4)


def state_ms(w, h, scale, pitch, reps=20):
    import recgen
    st = h263mi.H263State(h263mi.SORENSON_SPARK_BITSTREAM, device_id=0)
    mbs, co = recgen.intra_picture(w, h, seed=1)
    st.submit_picture(w, h, mbs, co, h263mi.PICTURE_I, temporal_reference=0, pquant=8)
    ow, oh, nb = h263mi.rgba_layout_extent(1, w, h, scale, pitch)
    out = np.empty(oh * (pitch or 4 * ow), np.uint8)
    st.render_rgba_layout_into(5, out, scale, pitch)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        st.render_rgba_layout_into(5, out, scale, pitch)
        t.append((time.perf_counter() - t0) * 1e3)
    st.close()
    return round(float(np.median(t)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gop", type=int, default=31)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import bench
    wl = bench.Workload(h263mi, N, args.gop, 0, 0, None, events=True)
    res = {"what": "k_frame ms per launch, 64 x 1080p, events, pipeline_post, strength %d; best of %d rounds of a %d-picture GOP"
                   % (bench.STRENGTH, args.rounds, args.gop)}
    for name, lay in layouts().items():
        res["k_frame_ms_" + name] = time_layout(wl, lay, args.gop, args.rounds)
    res["state_cif_pitch1536_ms"] = state_ms(352, 288, 0, 1536)
    res["state_1080p_quarter_ms"] = state_ms(W, H, 2, 0)
    res["state_1080p_full_ms"] = state_ms(W, H, 0, 0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
