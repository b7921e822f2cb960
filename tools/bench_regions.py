#!/usr/bin/env python3
"""Measures the motion regions (k_regions + k_regions_pack) beside the change-map call that produces their grids, in one process on
one GPU.

Workload: 64 pictures of 1920 x 1080 geometry at cell_log2 = 4 (a grid of 120 x 68) and 3 (240 x 135, 32 400 cells: next to the cap),
connectivity 4, min_cells 1, max_per_picture 16, a table of 1024 entries, stats wanted.  Inputs:
  still         all-zero grids, skipped through summaries without changed cells: no grid is read
  decoded       the grids h263mi_batch_change_last gives for a synthetic P picture against the I picture in front of it
  checkerboard  every other cell changed: the most components there can be (connectivity 4)
  serpentine    full rows joined at alternating ends: one component, one path through half the grid
Yardstick, same process: the h263mi_batch_change_last call (roll off) that writes the decoded grids at that cell size.
Every call is timed with device events on the calls' stream: warm-up, then --launches calls between one pair of events, --rounds
rounds per leg, the legs interleaved; the figure of a leg is the median of its rounds.

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
MAX_PER, MAX_ROIS = 16, 1024
ON = 1 << 12                                                       # the SAD of a changed cell of the synthetic grids


def serpentine(gh, gw):
    m = np.zeros((gh, gw), bool)
    m[0::2] = True
    for k, y in enumerate(range(1, gh - 1, 2)):
        m[y, gw - 1 if k % 2 == 0 else 0] = True
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.launches < 20:
        raise SystemExit("bench_regions: at least 20 launches per window")
    if h263mi.device_count() < 1:
        raise SystemExit("bench_regions: no HIP device -- nothing is measured without one")

    stream = torch.cuda.Stream(device=0)
    # two decoded pictures per stream: the I picture goes to prev, the P picture is compared with it
    wl = bench.Workload(h263mi, N, 2, 0, 0, None)
    b = h263mi.Batch(N, W, H, 0, stream.cuda_stream)
    prev = torch.zeros(N * W * H, dtype=torch.uint8, device="cuda")
    prev_set = h263mi.PlaneSet(prev.data_ptr(), N * W * H, W, W * H)

    legs, keep, first = {}, [], {}
    for cl in (4, 3):
        tag = "c%d" % (1 << cl)
        thr = 4 << (2 * cl)                                         # changed: a mean difference above 4 a pixel
        regions = h263mi.make_regions(cl, thr, connectivity=4, margin_cells=1, min_cells=1, max_per_picture=MAX_PER)
        gw, gh, cells_bytes, work_bytes = h263mi.regions_extent(N, W, H, regions)
        outs = dict(work=torch.empty(work_bytes, dtype=torch.uint8, device="cuda"), rois=torch.empty(MAX_ROIS * 4, dtype=torch.int32, device="cuda"),
                    stats=torch.empty(MAX_ROIS * 2, dtype=torch.int64, device="cuda"), info=torch.empty(N * 4, dtype=torch.int32, device="cuda"),
                    count=torch.empty(2, dtype=torch.int32, device="cuda"))
        keep.append(outs)

        def regions_call(d_cells, d_summary, regions=regions, outs=outs, cells_bytes=cells_bytes, work_bytes=work_bytes):
            h263mi.regions(d_cells.data_ptr(), cells_bytes, N, W, H, regions, outs["work"].data_ptr(), work_bytes, outs["rois"].data_ptr(),
                           MAX_ROIS, outs["info"].data_ptr(), outs["count"].data_ptr(), d_stats=outs["stats"].data_ptr(),
                           d_summary=d_summary.data_ptr() if d_summary is not None else None, stream=stream.cuda_stream)

        # decoded: I into prev (roll on), then P against it (roll off: the yardstick call, repeatable)
        d_cells = torch.empty(cells_bytes // 4, dtype=torch.int32, device="cuda")
        d_summary = torch.empty(N * 2, dtype=torch.int64, device="cuda")
        roll, anchor = h263mi.make_change(cl, thr, 1, roll=1), h263mi.make_change(cl, thr, 1, roll=0)
        b.reset()
        fr = wl.frames[0]
        b.decode(fr["ptype"], fr["mbs"].ptr, fr["co"].ptr, fr["base"].ptr, 0, 0, None, None)
        b.change_last(prev_set, roll, d_cells.data_ptr(), cells_bytes, d_summary.data_ptr())
        fr = wl.frames[1]
        b.decode(fr["ptype"], fr["mbs"].ptr, fr["co"].ptr, fr["base"].ptr, 0, 0, None, None)
        change_call = lambda anchor=anchor, d_cells=d_cells, d_summary=d_summary, cells_bytes=cells_bytes: b.change_last(
            prev_set, anchor, d_cells.data_ptr(), cells_bytes, d_summary.data_ptr())
        change_call()
        b.sync()
        # synthetic grids
        checker = np.indices((gh, gw)).sum(0) % 2 == 0
        grids = {"still": np.zeros((gh, gw), bool), "checkerboard": checker, "serpentine": serpentine(gh, gw)}
        dev = {"decoded": (d_cells, d_summary)}
        for name, mask in grids.items():
            g = torch.from_numpy(np.tile(np.where(mask, ON << (2 * cl - 6), 0).astype(np.int32), (N, 1, 1))).cuda()
            s = np.zeros(N, h263mi.CHANGE_SUMMARY_DTYPE)
            s["changed_cells"] = int(mask.sum())
            dev[name] = (g, torch.from_numpy(s.view(np.int64).copy()).cuda())
        keep.append(dev)
        legs["change_last_" + tag] = change_call
        for name, (g, s) in dev.items():
            legs["%s_%s" % (name, tag)] = lambda g=g, s=s, call=regions_call: call(g, s)
        first[tag] = {"grid": [gw, gh], "outs": outs}

    def window(call, launches):
        """us per call between two device events on the stream"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(launches):
            call()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / launches

    seen = {}
    for k, call in legs.items():                                 # warm-up: every shape of the timed windows
        call()
        stream.synchronize()
        if not k.startswith("change_last"):
            outs = first[k.rsplit("_", 1)[1]]["outs"]
            info = outs["info"].cpu().numpy().view(h263mi.REGION_INFO_DTYPE)
            seen[k] = {"components": int(info["components"].sum()), "kept": int(info["kept"].sum()),
                       "count": [int(v) for v in outs["count"].cpu()]}
        window(call, 3)
    us = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, call in legs.items():
            us[k].append(window(call, a.launches))
    res = {
        "what": "motion regions of %d grids of %d x %d geometry, connectivity 4, margin 1, min_cells 1, max_per_picture %d, a table of %d "
                "entries with stats: us per call (k_regions + k_regions_pack), device events; change_last_*: the h263mi_batch_change_last "
                "call (roll off) that writes the decoded grids" % (N, W, H, MAX_PER, MAX_ROIS),
        "method": "one process, legs interleaved, %d rounds of %d calls between one pair of events each; medians" % (a.rounds, a.launches),
        "grids": {tag: v["grid"] for tag, v in first.items()},
        "legs": {k: dict({"us_per_call": round(statistics.median(v), 2), "rounds_us": [round(x, 2) for x in v]}, **seen.get(k, {}))
                 for k, v in us.items()},
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
