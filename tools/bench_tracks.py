#!/usr/bin/env python3
"""Measures the region tracks (k_tracks + k_tracks_pack) beside the regions call and the change-map call in front of them, in one
process on one GPU.

Workload: 64 pictures of 1920 x 1080 geometry, iou_permille 300, max_missed 2, min_hits 2, emit_period 0, a table of 1024 entries with
refs.  Legs:
  empty         16 slots, empty states, no detections
  decoded_16    16 slots; the table h263mi_batch_regions gives (max_per_picture 16, its threshold at the 60th percentile of the cell
                SADs: 16 boxes a picture) for a synthetic P picture against the I picture in front of it, call after call: 16 tracks
                and 16 detections a picture, every track finds its own box again
  random_256    256 slots; two tables of 256 random boxes a picture, the second the first moved by a few pixels, in turns: crowded,
                several rounds
  chain_256     256 slots; a chain as in tests/tracks_cases.py (track k prefers detection k - 1 and settles for k), tracks and
                detections in turns, iou_permille 100 (a link's IoU is 1/7): 256 rounds, the most there can be
Yardsticks, same process: the h263mi_batch_regions call that writes the decoded table, and the h263mi_batch_change_last call (roll
off) in front of it.  Every call is timed with device events on the calls' stream: warm-up, then --launches calls between one pair
of events, --rounds rounds per leg, the legs interleaved; the figure of a leg is the median of its rounds.

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
MAX_PER, MAX_ROIS, MAX_OUT, CL = 16, 1024, 1024, 4


def chain_tables():
    """boxes 4 wide, 3 apart (neighbours share one column), heights falling along the chain: S_0 = T_0, S_1 = D_0, S_2 = T_1, ..."""
    s = [(3 * m, 0, 4, 1000 - m) for m in range(512)]
    return s[0::2], s[1::2]


def table_of(per_picture):
    """the boxes of every picture -> (rois, info) as regions lays them out"""
    rois = np.zeros(sum(len(b) for b in per_picture), h263mi.ROI_DTYPE)
    info = np.zeros(len(per_picture), h263mi.REGION_INFO_DTYPE)
    at = 0
    for p, boxes in enumerate(per_picture):
        info[p] = (len(boxes), len(boxes), at, len(boxes))
        for b in boxes:
            rois[at] = (p,) + tuple(b) + (0,)
            at += 1
    return rois, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.launches < 20:
        raise SystemExit("bench_tracks: at least 20 launches per window")
    if h263mi.device_count() < 1:
        raise SystemExit("bench_tracks: no HIP device -- nothing is measured without one")

    stream = torch.cuda.Stream(device=0)
    dev = lambda arr: torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()).cuda()
    # the yardsticks and the decoded table: I into prev (roll on), then P against it (roll off), then regions
    wl = bench.Workload(h263mi, N, 2, 0, 0, None)
    b = h263mi.Batch(N, W, H, 0, stream.cuda_stream)
    prev = torch.zeros(N * W * H, dtype=torch.uint8, device="cuda")
    prev_set = h263mi.PlaneSet(prev.data_ptr(), N * W * H, W, W * H)
    thr = 4 << (2 * CL)
    regions = h263mi.make_regions(CL, thr, connectivity=4, margin_cells=1, min_cells=1, max_per_picture=MAX_PER)
    gw, gh, cells_bytes, work_bytes = h263mi.regions_extent(N, W, H, regions)
    d_cells = torch.empty(cells_bytes // 4, dtype=torch.int32, device="cuda")
    d_summary = torch.empty(N * 2, dtype=torch.int64, device="cuda")
    r_work = torch.empty(work_bytes, dtype=torch.uint8, device="cuda")
    r_rois = torch.empty(MAX_ROIS * 16, dtype=torch.uint8, device="cuda")
    r_info = torch.empty(N * 16, dtype=torch.uint8, device="cuda")
    r_count = torch.empty(2, dtype=torch.int32, device="cuda")
    roll, anchor = h263mi.make_change(CL, thr, 1, roll=1), h263mi.make_change(CL, thr, 1, roll=0)
    fr = wl.frames[0]
    b.decode(fr["ptype"], fr["mbs"].ptr, fr["co"].ptr, fr["base"].ptr, 0, 0, None, None)
    b.change_last(prev_set, roll, d_cells.data_ptr(), cells_bytes, d_summary.data_ptr())
    fr = wl.frames[1]
    b.decode(fr["ptype"], fr["mbs"].ptr, fr["co"].ptr, fr["base"].ptr, 0, 0, None, None)
    change_call = lambda: b.change_last(prev_set, anchor, d_cells.data_ptr(), cells_bytes, d_summary.data_ptr())
    regions_call = lambda: b.regions(d_cells.data_ptr(), cells_bytes, regions, r_work.data_ptr(), work_bytes, r_rois.data_ptr(), MAX_ROIS,
                                     r_info.data_ptr(), r_count.data_ptr(), d_summary=d_summary.data_ptr())
    change_call()
    b.sync()
    # the regions' own threshold: the 60th percentile of the cell SADs, so that two cells in five are changed and every picture
    # has far more than MAX_PER components -- the synthetic P pictures differ from their I pictures in every cell, and at the change
    # map's threshold regions would write one box a picture
    region_thr = int(np.percentile(d_cells.cpu().numpy().view(np.uint32), 60))
    regions = h263mi.make_regions(CL, region_thr, connectivity=4, margin_cells=1, min_cells=1, max_per_picture=MAX_PER)
    regions_call()
    b.sync()

    rng = np.random.default_rng(7)
    xy = rng.integers(0, [W - 64, H - 64], (N, 256, 2))
    wh = rng.integers(16, 64, (N, 256, 2))
    moved = np.clip(xy + rng.integers(-6, 7, xy.shape), 0, [W - 64, H - 64])
    random_a = table_of([[tuple(int(v) for v in (*xy[p, k], *wh[p, k])) for k in range(256)] for p in range(N)])
    random_b = table_of([[tuple(int(v) for v in (*moved[p, k], *wh[p, k])) for k in range(256)] for p in range(N)])
    ct, cd = chain_tables()
    chain_a, chain_b = table_of([ct] * N), table_of([cd] * N)
    none = table_of([[]] * N)

    legs, keep, shown = {"change_last": change_call, "regions": regions_call}, [], {}

    def tracks_leg(name, max_tracks, tables, permille=300):
        """the tables in turns over one state, which the warm-up fills"""
        t = h263mi.make_tracks(max_tracks, permille, 2, 2, 0)
        state_bytes = h263mi.tracks_extent(N, W, H, t)
        outs = dict(state=torch.zeros(state_bytes, dtype=torch.uint8, device="cuda"), rois=torch.empty(MAX_OUT * 16, dtype=torch.uint8, device="cuda"),
                    refs=torch.empty(MAX_OUT * 16, dtype=torch.uint8, device="cuda"), info=torch.empty(N * 32, dtype=torch.uint8, device="cuda"),
                    count=torch.empty(2, dtype=torch.int32, device="cuda"))
        turn = [0]

        def call():
            d_rois, n_rois, d_info = tables[turn[0] % len(tables)]
            turn[0] += 1
            h263mi.tracks(d_rois, n_rois, d_info, N, W, H, t, outs["state"].data_ptr(), state_bytes, outs["rois"].data_ptr(), MAX_OUT,
                          outs["info"].data_ptr(), outs["count"].data_ptr(), d_out_refs=outs["refs"].data_ptr(), stream=stream.cuda_stream)
        keep.append((outs, tables))
        legs[name] = call
        shown[name] = outs

    def on_device(tab):
        rois, info = dev(tab[0]), dev(tab[1])
        keep.append((rois, info))
        return (rois.data_ptr() if tab[0].size else None, int(tab[0].size), info.data_ptr())

    tracks_leg("empty", 16, [on_device(none)])
    tracks_leg("decoded_16", 16, [(r_rois.data_ptr(), MAX_ROIS, r_info.data_ptr())])
    tracks_leg("random_256", 256, [on_device(random_a), on_device(random_b)])
    tracks_leg("chain_256", 256, [on_device(chain_a), on_device(chain_b)], permille=100)

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
    for k, call in legs.items():                                 # warm-up: every shape of the timed windows; the states fill
        window(call, 4)
        if k in shown:
            info = shown[k]["info"].cpu().numpy().view(h263mi.TRACK_INFO_DTYPE)
            seen[k] = {f: int(info[f].sum()) for f in ("detections", "matched", "born", "died", "dropped")}
            seen[k]["count"] = [int(v) for v in shown[k]["count"].cpu()]
    us = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, call in legs.items():
            us[k].append(window(call, a.launches))
    res = {
        "what": "region tracks of %d pictures of %d x %d geometry, iou_permille 300, max_missed 2, min_hits 2, emit_period 0, a table of %d "
                "entries with refs: us per call (k_tracks + k_tracks_pack), device events; regions: the h263mi_batch_regions call that "
                "writes the decoded table (cells of %d, max_per_picture %d, cell_threshold %d); change_last: the h263mi_batch_change_last call (roll off) in "
                "front of it" % (N, W, H, MAX_OUT, 1 << CL, MAX_PER, region_thr),
        "method": "one process, legs interleaved, %d rounds of %d calls between one pair of events each; medians" % (a.rounds, a.launches),
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
