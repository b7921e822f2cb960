#!/usr/bin/env python3
"""Measures the change maps (k_change + k_change_select and the clearing in front of them) against the box's own streaming
ceilings, in one process on one GPU.

Workload: 64 x 1920 x 1080 luma planes, cell_log2 = 4, a list wanted, no grid unless --cells.  Three variants:
  on_keep    h263mi_change_map_on, roll off: reads 2 bytes a pixel (cur, prev), writes next to nothing
  on_roll    h263mi_change_map_on, roll on:  reads 2 bytes a pixel, writes 1 (prev takes cur)
  last_roll  h263mi_batch_change_last, roll on: cur is the frame store's luma of a decoded synthetic I picture, read in place
Yardsticks, same process: h263mi_probe_bandwidth over the same byte count -- read mode for roll off, copy mode for roll on (the copy
probe moves half of its bytes in each direction, the rolled map a third out: the nearer of the two probes, not the same mix).
Every call is timed with device events on the calls' stream: warm-up, then --launches calls between one pair of events, --rounds
rounds per variant, the variants interleaved; the figure of a variant is the median of its rounds.

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
CELL_LOG2 = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--cells", action="store_true", help="write the grids too")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.launches < 20:
        raise SystemExit("bench_change: at least 20 launches per window")
    if h263mi.device_count() < 1:
        raise SystemExit("bench_change: no HIP device -- nothing is measured without one")

    stream = torch.cuda.Stream(device=0)
    pixels = N * W * H
    g = torch.Generator(device="cuda").manual_seed(2026)
    planes = [torch.randint(0, 256, (pixels,), dtype=torch.uint8, device="cuda", generator=g) for _ in range(3)]
    cur, prev_keep, prev_roll = [h263mi.PlaneSet(t.data_ptr(), pixels, W, W * H) for t in planes]
    keep = h263mi.make_change(CELL_LOG2, 16 * 256, 1, roll=0)          # changed: a mean difference above 16 a pixel
    roll = h263mi.make_change(CELL_LOG2, 16 * 256, 1, roll=1)
    gw, gh, cells_bytes = h263mi.change_extent(N, W, H, keep)
    d_cells = torch.empty(cells_bytes // 4, dtype=torch.int32, device="cuda") if a.cells else None
    d_summary = torch.empty(N * 4, dtype=torch.int32, device="cuda")
    d_list = torch.empty(N, dtype=torch.int32, device="cuda")
    d_count = torch.empty(1, dtype=torch.int32, device="cuda")
    outs = (d_cells.data_ptr() if a.cells else None, cells_bytes if a.cells else 0, d_summary.data_ptr(), d_list.data_ptr(), d_count.data_ptr())

    # the frame store's leg: a batch on the same stream with one decoded picture per stream
    wl = bench.Workload(h263mi, N, 1, 0, 0, None)
    fr = wl.frames[0]
    b = h263mi.Batch(N, W, H, 0, stream.cuda_stream)
    b.decode(fr["ptype"], fr["mbs"].ptr, fr["co"].ptr, fr["base"].ptr, 0, 0, None, None)
    b.sync()
    prev_last = torch.zeros(pixels, dtype=torch.uint8, device="cuda")
    prev_last_set = h263mi.PlaneSet(prev_last.data_ptr(), pixels, W, W * H)
    torch.cuda.synchronize()

    legs = {
        "on_keep": lambda: h263mi.change_map(cur, prev_keep, N, W, H, keep, *outs, stream=stream.cuda_stream),
        "on_roll": lambda: h263mi.change_map(cur, prev_roll, N, W, H, roll, *outs, stream=stream.cuda_stream),
        "last_roll": lambda: b.change_last(prev_last_set, roll, *outs),
    }

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
        s = d_summary.cpu().numpy().view(h263mi.CHANGE_SUMMARY_DTYPE)
        first[k] = {"sad_total": int(s["sad"].sum()), "changed_cells_total": int(s["changed_cells"].sum()), "selected": int(d_count.cpu()[0])}
        window(call, 3)
    us = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, call in legs.items():
            us[k].append(window(call, a.launches))
    med = {k: statistics.median(v) for k, v in us.items()}

    moved = {"on_keep": 2 * pixels, "on_roll": 3 * pixels, "last_roll": 3 * pixels}
    read_gbs, read_shape = h263mi.probe_bandwidth(h263mi.PROBE_READ, 2 * pixels, 10, 0, stream.cuda_stream, with_shape=True)
    # (the copy probe counts what it reads and what it writes: half of 3 bytes a pixel in, half out)
    copy_gbs, copy_shape = h263mi.probe_bandwidth(h263mi.PROBE_COPY, (3 * pixels // 2) // 16 * 16, 10, 0, stream.cuda_stream, with_shape=True)
    ceiling = {"on_keep": read_gbs, "on_roll": copy_gbs, "last_roll": copy_gbs}
    res = {
        "what": "change maps of %d x %d x %d luma planes, cell_log2 %d, a list wanted, %s: us per call (clearing + k_change + "
                "k_change_select), device events" % (N, W, H, CELL_LOG2, "grids written" if a.cells else "no grid"),
        "method": "one process, variants interleaved, %d rounds of %d calls between one pair of events each; medians; ceilings: "
                  "h263mi_probe_bandwidth over the same byte count in the same process" % (a.rounds, a.launches),
        "variants": {k: {"us_per_launch": round(med[k], 2), "bytes_moved": moved[k], "gb_per_s": round(moved[k] / (med[k] * 1e3), 1),
                         "ceiling": "read" if k == "on_keep" else "copy", "ceiling_gb_per_s": round(ceiling[k], 1),
                         "fraction_of_ceiling": round(moved[k] / (med[k] * 1e3) / ceiling[k], 4),
                         "rounds_us": [round(x, 2) for x in us[k]], "first_call": first[k]} for k in legs},
        "probe_read": {"gb_per_s": round(read_gbs, 1), "bytes": 2 * pixels, "shape": read_shape},
        "probe_copy": {"gb_per_s": round(copy_gbs, 1), "bytes_in_plus_out": 2 * ((3 * pixels // 2) // 16 * 16), "shape": copy_shape},
        "grid": [gw, gh],
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
