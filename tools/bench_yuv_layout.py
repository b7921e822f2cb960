#!/usr/bin/env python3
"""k_frame ms per launch for the deblocked-plane output (h263mi_yuv_layout) against the RGBA output, 64 x 1080p, records
resident as events (bench.py's Workload), H263MI_CFG_PIPELINE_POST, launch timing (h263mi_batch_timing_*):

  rgba_default    d_rgba, today's layout (the default kernels): the yardstick
  planes_legacy   d_rgba NULL, d_deblocked with no layout in force: tight I420 written by the default kernels' edge path
  nv12_p2048      d_rgba NULL, NV12 at 2 048-byte pitches, pictures back to back (k_frame_yuv, wide stores)
  i420_mosaic     d_rgba NULL, I420 as an 8 x 8 mosaic: luma tiles on a grid of 15 360 bytes, Cb and Cr tiles on one of 7 680

The four cases take turns inside every round of ONE process, so that they see the same clocks; per case the best round and
the spread (max - min) / min over the rounds are reported.  Plus host-to-host ms of h263mi_render_yuv (NV12 at 256-byte
multiples) for one CIF state and one 1080p state, with h263mi_render_rgba of the same states beside them.
Prints one JSON line.

    python tools/bench_yuv_layout.py [--gop 31] [--rounds 5]
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


def cases():
    """name -> (wants RGBA, YUV layout arguments or None)"""
    cw, ch = W // 2, H // 2
    luma_bytes = 8 * H * 8 * W                               # the 8 x 8 luma mosaic; the chroma mosaics follow it
    oy = [(s // 8) * H * 8 * W + (s % 8) * W for s in range(N)]
    ocb = [luma_bytes + (s // 8) * 2 * ch * 8 * cw + (s % 8) * cw for s in range(N)]
    ocr = [o + ch * 8 * cw for o in ocb]
    return {
        "rgba_default": (True, None),
        "planes_legacy": (False, None),
        "nv12_p2048": (False, (h263mi.YUV_NV12, 2048, 2048)),
        "i420_mosaic": (False, (h263mi.YUV_I420, 8 * W, 8 * cw, oy, ocb, ocr)),
    }


class Case:
    def __init__(self, rgba, lay):
        self.b = h263mi.Batch(N, W, H, 0, None, pipeline_post=True)
        self.rgba = h263mi.DeviceBuffer(N * W * H * 4) if rgba else None
        self.planes = None
        if not rgba:
            if lay is not None:
                self.b.set_yuv_layout(*lay)
                self.planes = h263mi.DeviceBuffer(h263mi.yuv_layout_extent(N, W, H, *lay))
            else:
                self.planes = h263mi.DeviceBuffer(h263mi.yuv_layout_extent(N, W, H, default=True))

    def run(self, wl, gop):
        import bench
        b = self.b
        rgba = self.rgba.ptr if self.rgba else None
        planes = self.planes.ptr if self.planes else None
        b.timing_reserve(4 * gop)
        b.timing_begin()
        for f in range(gop):
            fr = wl.frames[f]
            if fr.get("first") is not None:
                b.decode_events(fr["ptype"], fr["mbs"].ptr, fr["first"].ptr, fr["ev"].ptr, fr["base"].ptr, 0, bench.STRENGTH,
                                rgba, planes)
            else:
                b.decode(fr["ptype"], fr["mbs"].ptr, fr["co"].ptr, fr["base"].ptr, 0, bench.STRENGTH, rgba, planes)
        b.sync()
        kt = b.timing_end()
        return kt.frame_ms / max(kt.frame_launches, 1)


def state_ms(w, h, reps=20):
    import recgen
    st = h263mi.H263State(h263mi.SORENSON_SPARK_BITSTREAM, device_id=0)
    mbs, co = recgen.intra_picture(w, h, seed=1)
    st.submit_picture(w, h, mbs, co, h263mi.PICTURE_I, temporal_reference=0, pquant=8)
    py = pc = ((w + 255) // 256) * 256
    out = np.empty(h263mi.yuv_layout_extent(1, w, h, h263mi.YUV_NV12, py, pc), np.uint8)
    res = []
    for fn in (lambda: st.render_yuv_into(5, out, h263mi.YUV_NV12, py, pc), lambda: st.render_rgba(5)):
        fn()
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
        res.append(round(float(np.median(t)), 4))
    st.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gop", type=int, default=31)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import bench
    wl = bench.Workload(h263mi, N, args.gop, 0, 0, None, events=True)
    res = {"what": "k_frame ms per launch, 64 x 1080p, events, pipeline_post, strength %d; %d interleaved rounds of a %d-picture "
                   "GOP in one process: best round, and spread = (max - min) / min over the rounds" % (bench.STRENGTH, args.rounds, args.gop)}
    made = {name: Case(*c) for name, c in cases().items()}
    times = {name: [] for name in made}
    for r in range(args.rounds + 1):                         # (round 0: warm-up)
        for name, c in made.items():
            ms = c.run(wl, args.gop)
            if r:
                times[name].append(ms)
    for name, t in times.items():
        res["k_frame_ms_" + name] = round(min(t), 4)
        res["spread_" + name] = round((max(t) - min(t)) / min(t), 4)
        res["rounds_ms_" + name] = [round(v, 4) for v in t]
    for c in made.values():
        c.b.close()
    base = res["k_frame_ms_rgba_default"]
    for name in ("nv12_p2048", "i420_mosaic", "planes_legacy"):
        res["ratio_%s_to_rgba_default" % name] = round(res["k_frame_ms_" + name] / base, 4)
    for name in ("nv12_p2048", "i420_mosaic"):
        res["speedup_%s_over_planes_legacy" % name] = round(res["k_frame_ms_planes_legacy"] / res["k_frame_ms_" + name], 3)
    res["state_cif_render_yuv_ms"], res["state_cif_render_rgba_ms"] = state_ms(352, 288)
    res["state_1080p_render_yuv_ms"], res["state_1080p_render_rgba_ms"] = state_ms(W, H)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
