#!/usr/bin/env python3
"""Measures the plane histograms (the clearing + k_hist + k_hist_final + k_hist_select) against the box's own read ceiling and
against the change maps, in one process on one GPU.

Workload: 64 x 1920 x 1080 luma planes.  Variants:
  on         h263mi_hist_on without prev and without a list
  on_prev    h263mi_hist_on with prev, roll and a list
  last       h263mi_batch_hist_last, plane 0, with prev, roll and a list: the frame store's luma of a decoded synthetic I picture
Contents of the planes that `on` and `on_prev` count (the frame store holds what it holds):
  random     uniform bytes: a lane's 16 pixels are 16 runs, the lanes of a wave scatter over the bins
  flat       every picture one value: a lane's 16 pixels are one run, all 64 lanes meet in one bin, a wave adds one word
  decoded    the deblocked luma planes of the decoded synthetic I picture (the batch's default plane output)
  ramp16     every aligned 16 pixels one value, the value stepping from chunk to chunk: one run a lane as in `flat`, but the lanes
             scatter and a wave adds all 256 words as in `random`
  alt        two values alternating from pixel to pixel: 16 runs a lane AND all lanes in two bins, the worst case of the LDS scheme
random -> ramp16 changes the LDS additions alone (16 a chunk to 1); ramp16 -> flat changes the words a wave adds to the picture's
histogram (256 to 1) and how deep the LDS additions collide (1 to 8).
Yardsticks, same process, same bytes: the read mode of h263mi_probe_bandwidth, and h263mi_change_map_on with roll off, which
reads twice the bytes.  Every call is timed with device events on the calls' stream: warm-up, then --launches calls between one
pair of events, --rounds rounds per leg, the legs interleaved; the figure of a leg is the median of its rounds.

Prints one JSON line; --out FILE also writes it there.  No threshold: a record, not a gate."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "h263-rs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch  # (before the library is loaded: it brings the HIP runtime that the C-ABI library must share, as in bench.py)

import bench
import h263mi

N, W, H = 64, 1920, 1080
CONTENTS = ("random", "flat", "decoded", "ramp16", "alt")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.launches < 20:
        raise SystemExit("bench_hist: at least 20 launches per window")
    if h263mi.device_count() < 1:
        raise SystemExit("bench_hist: no HIP device -- nothing is measured without one")

    stream = torch.cuda.Stream(device=0)
    pixels = N * W * H
    picture = W * H + 2 * ((W + 1) // 2) * ((H + 1) // 2)

    # the frame store's leg and the decoded content: a batch on the same stream with one decoded picture per stream
    wl = bench.Workload(h263mi, N, 1, 0, 0, None)
    fr = wl.frames[0]
    b = h263mi.Batch(N, W, H, 0, stream.cuda_stream)
    deblocked = torch.empty(N * picture, dtype=torch.uint8, device="cuda")
    b.decode(fr["ptype"], fr["mbs"].ptr, fr["co"].ptr, fr["base"].ptr, 0, 5, None, deblocked.data_ptr())
    b.sync()

    g = torch.Generator(device="cuda").manual_seed(2026)
    x = torch.arange(W * H, dtype=torch.int64, device="cuda")
    planes = {
        "random": torch.randint(0, 256, (pixels,), dtype=torch.uint8, device="cuda", generator=g),
        "flat": (torch.arange(N, device="cuda") * 37 % 256).to(torch.uint8).repeat_interleave(W * H),
        "ramp16": ((x // 16 * 7) % 256).to(torch.uint8).repeat(N),
        "alt": torch.where((x % W + x // W) % 2 == 0, 60, 190).to(torch.uint8).repeat(N),
    }
    sets = {k: h263mi.PlaneSet(t.data_ptr(), pixels, W, W * H) for k, t in planes.items()}
    sets["decoded"] = h263mi.planes_default_set(deblocked.data_ptr(), N, W, H)
    other = torch.randint(0, 256, (pixels,), dtype=torch.uint8, device="cuda", generator=g)      # the change map's prev
    other_set = h263mi.PlaneSet(other.data_ptr(), pixels, W, W * H)

    plain = h263mi.make_hist(10, 990, 300, roll=0)
    rolling = h263mi.make_hist(10, 990, 300, roll=1)
    hist_bytes = h263mi.hist_extent(N, W, H, plain)
    d_hist = torch.empty(N * 256, dtype=torch.int32, device="cuda")
    d_stats = torch.empty(N * 8, dtype=torch.int32, device="cuda")
    d_list = torch.empty(N, dtype=torch.int32, device="cuda")
    d_count = torch.empty(1, dtype=torch.int32, device="cuda")
    d_prev = {k: torch.zeros(N * 256, dtype=torch.int32, device="cuda") for k in CONTENTS + ("last",)}
    keep = h263mi.make_change(4, 16 * 256, 1, roll=0)
    d_summary = torch.empty(N * 4, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def on(content, with_prev):
        prev = (d_prev[content].data_ptr(), hist_bytes, d_list.data_ptr(), d_count.data_ptr()) if with_prev else (None, 0, None, None)
        return lambda: h263mi.hist(sets[content], N, W, H, rolling if with_prev else plain, d_hist.data_ptr(), hist_bytes, d_stats.data_ptr(), *prev,
                                   stream=stream.cuda_stream)

    legs = {}
    for c in CONTENTS:
        legs["on/" + c] = on(c, False)
        legs["on_prev/" + c] = on(c, True)
    legs["last/decoded"] = lambda: b.hist_last(0, rolling, d_hist.data_ptr(), hist_bytes, d_stats.data_ptr(), d_prev["last"].data_ptr(), hist_bytes,
                                               d_list.data_ptr(), d_count.data_ptr())
    for c in ("random", "decoded"):
        legs["change_map/" + c] = (lambda c=c: h263mi.change_map(sets[c], other_set, N, W, H, keep, None, 0, d_summary.data_ptr(),
                                                                 d_list.data_ptr(), d_count.data_ptr(), stream=stream.cuda_stream))

    def window(call, launches):
        """us per call between two device events on the stream"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(launches):
            call()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / launches

    first = {}
    for k, call in legs.items():                                 # warm-up: every shape of the timed windows
        call()
        stream.synchronize()
        if not k.startswith("change_map"):
            hist = d_hist.cpu().numpy().view(np.uint32).reshape(N, 256)
            assert (hist.sum(axis=1) == W * H).all(), k        # every pixel counted once
            st = d_stats.cpu().numpy().view(h263mi.HIST_STATS_DTYPE)
            first[k] = {"bins_with_a_count": int((hist[0] > 0).sum()), "mean_of_picture_0": round(int(st["sum"][0]) / (W * H), 2)}
        window(call, 3)
    us = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, call in legs.items():
            us[k].append(window(call, a.launches))
    med = {k: statistics.median(v) for k, v in us.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in us.items()}

    read_gbs, read_shape = h263mi.probe_bandwidth(h263mi.PROBE_READ, pixels, 10, 0, stream.cuda_stream, with_shape=True)
    read_us = pixels / (read_gbs * 1e3)
    res = {
        "what": "histograms of %d x %d x %d luma planes: us per call (clearing + k_hist + k_hist_final [+ k_hist_select]), device events; "
                "change_map: h263mi_change_map_on, cell 16, roll off, a list, no grid, over the same planes and a second set" % (N, W, H),
        "method": "one process, legs interleaved, %d rounds of %d calls between one pair of events each; medians; spread = (max - min) / "
                  "median of a leg's rounds; read probe: h263mi_probe_bandwidth, read mode, over the same byte count" % (a.rounds, a.launches),
        "legs": {k: {"us_per_call": round(med[k], 2), "bytes_read": (2 if k.startswith("change_map") else 1) * pixels,
                     "gb_per_s": round((2 if k.startswith("change_map") else 1) * pixels / (med[k] * 1e3), 1),
                     "fraction_of_read_probe": round((2 if k.startswith("change_map") else 1) * pixels / (med[k] * 1e3) / read_gbs, 4),
                     "spread": round(spread[k], 4), "rounds_us": [round(x, 2) for x in us[k]], **({"first_call": first[k]} if k in first else {})}
                 for k in legs},
        "ratios_to_random": {v: {c: round(med["%s/%s" % (v, c)] / med[v + "/random"], 4) for c in CONTENTS if c != "random"} for v in ("on", "on_prev")},
        "probe_read": {"gb_per_s": round(read_gbs, 1), "bytes": pixels, "us": round(read_us, 2), "shape": read_shape},
        "kernel_source_hash": bench.kernel_source_hash(),
    }
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    b.close()


if __name__ == "__main__":
    main()
