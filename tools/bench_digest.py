#!/usr/bin/env python3
"""What an on-device digest costs beside what a caller does without one, in one process: 64 x 1080p, records resident as events
(bench.py's Workload), one I and two P pictures decoded, then the legs in alternation, one warm-up round first.

  a  Batch.digest_yuv()                       all 64 pictures' Adler-32 in one call; bytes read = 64 x (w*h + 2*cw*ch)
  b  h263mi_probe_bandwidth, mode 1 (read)    the box's read ceiling over the same byte count
  c  64 x Batch.copy_yuv + zlib.adler32       what a caller does today
  d  Batch.adler32_spans over d_rgba          a full-size RGBA buffer of all 64 streams (64 x w*h*4 bytes)

a, c and d are host wall-clock times of complete calls (they return when the digests are on the host, so they include the
launches' and the copies' latencies); b is the library's own event timing of its probe.  The device time of k_digest alone
comes from a run of this tool under `rocprofv3 --kernel-trace --stats` (a run of its own).  Prints one JSON line and, with
--out, writes it to a file.

    python tools/bench_digest.py [--rounds 5] [--out profiles/rNN_digest.json]
"""
import argparse
import json
import os
import statistics
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "h263-rs_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import h263mi  # noqa: E402

W, H, N, GOP = 1920, 1080, 64, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bench
    cw, ch = (W + 1) // 2, (H + 1) // 2
    plane_bytes = N * (W * H + 2 * cw * ch)
    rgba_bytes = N * W * H * 4
    wl = bench.Workload(h263mi, N, GOP, 0, 0, None, events=True)
    b = h263mi.Batch(N, W, H, 0, None, pipeline_post=True)
    rgba = h263mi.DeviceBuffer(rgba_bytes)
    for f in range(GOP):
        fr = wl.frames[f]
        if fr.get("first") is not None:
            b.decode_events(fr["ptype"], fr["mbs"].ptr, fr["first"].ptr, fr["ev"].ptr, fr["base"].ptr, 0, bench.STRENGTH, rgba.ptr, None)
        else:
            b.decode(fr["ptype"], fr["mbs"].ptr, fr["co"].ptr, fr["base"].ptr, 0, bench.STRENGTH, rgba.ptr, None)
    b.sync()
    rgba_spans = h263mi.spans_of_rgba(N, W, H)

    def leg_a():
        t0 = time.perf_counter()
        d = b.digest_yuv(stream_rc=None)
        return time.perf_counter() - t0, d

    def leg_b():
        return h263mi.probe_bandwidth(h263mi.PROBE_READ, plane_bytes // 16 * 16, 10), None

    def leg_c():
        t0 = time.perf_counter()
        d = []
        for s in range(N):
            v = 1
            for p in b.copy_yuv(s):
                v = zlib.adler32(p, v)
            d.append(v)
        return time.perf_counter() - t0, d

    def leg_d():
        t0 = time.perf_counter()
        d = b.adler32_spans(rgba.ptr, rgba_bytes, rgba_spans)
        return time.perf_counter() - t0, d

    times = {"a": [], "b": [], "c": [], "d": []}
    digests = {}
    for r in range(args.rounds + 1):                         # (round 0: warm-up)
        for name, leg in (("a", leg_a), ("b", leg_b), ("c", leg_c), ("d", leg_d)):
            v, d = leg()
            if r:
                times[name].append(v)
            if d is not None:
                assert digests.setdefault(name, d) == d, "leg %s: a second call gave other digests" % name
    assert digests["a"] == digests["c"], "digest_yuv and zlib over copy_yuv disagree"
    a, c, d = (statistics.median(times[k]) for k in ("a", "c", "d"))
    read_gbs = statistics.median(times["b"])
    res = {"what": "64 x 1080p, events, pipeline_post, I + 2 P decoded; legs alternating, one warm-up round, medians of %d rounds; "
                   "a, c, d: host wall-clock of the complete call" % args.rounds,
           "plane_bytes": plane_bytes, "rgba_bytes": rgba_bytes,
           "a_digest_yuv_ms": round(a * 1e3, 4), "a_digest_yuv_min_ms": round(min(times["a"]) * 1e3, 4),
           "a_GBps": round(plane_bytes / a / 1e9, 1),
           "b_read_ceiling_GBps": round(read_gbs, 1), "b_read_ceiling_ms_for_plane_bytes": round(plane_bytes / read_gbs / 1e6, 4),
           "a_of_read_ceiling": round(plane_bytes / a / 1e9 / read_gbs, 3),
           "c_copy_yuv_zlib_ms": round(c * 1e3, 2), "c_over_a": round(c / a, 1),
           "d_adler32_spans_rgba_ms": round(d * 1e3, 4), "d_adler32_spans_rgba_min_ms": round(min(times["d"]) * 1e3, 4),
           "d_GBps": round(rgba_bytes / d / 1e9, 1), "d_of_read_ceiling": round(rgba_bytes / d / 1e9 / read_gbs, 3),
           "digests_equal_zlib": True}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    b.close()
    rgba.free()


if __name__ == "__main__":
    main()
