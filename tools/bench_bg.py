#!/usr/bin/env python3
"""Measures one call of the background model (k_bg_begin + k_bg + k_change_select) beside two yardsticks, in one process on one GPU.

Workload: 64 luma planes of 1920 x 1080 (tight, 16-byte aligned), cells of 16, the grid and the list wanted, no mask; the states are
past their initialisation, so every call reads 1 byte and reads and writes 2 bytes of state a pixel: 5 bytes x 132.7 M pixels =
663.6 MB.  Two sets of planes take turns as cur, and the sets (133 MB of planes, 265 MB of state) are larger than the Infinity Cache.
Yardsticks, same process, same stream:
  copy          a device-to-device copy of 331.8 MB: the same bytes read plus written
  change_map    h263mi_change_map_on with roll = 1 on the same planes (2 bytes read, 1 written a pixel: 398 MB)
Every call is timed on its own with a pair of device events: --warmup calls, then --calls timed ones (at least 20), the three legs
interleaved; the figure of a leg is the median.

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

import torch  # (before the library is loaded: it brings the HIP runtime that the C-ABI library must share, as in bench.py)

import h263mi

N, W, H, CL = 64, 1920, 1080, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.calls < 20:
        raise SystemExit("bench_bg: at least 20 timed calls")
    if h263mi.device_count() < 1:
        raise SystemExit("bench_bg: no HIP device -- nothing is measured without one")

    stream = torch.cuda.Stream(device=0)
    pixels = N * W * H
    gen = torch.Generator(device="cuda").manual_seed(1)
    base = torch.randint(0, 256, (pixels,), dtype=torch.uint8, device="cuda", generator=gen)
    # the second set: the first with noise of a few grey levels, and every fourth picture replaced (foreground everywhere)
    noise = torch.randint(0, 7, (pixels,), dtype=torch.uint8, device="cuda", generator=gen)
    other = torch.clamp(base.to(torch.int16) + noise.to(torch.int16) - 3, 0, 255).to(torch.uint8)
    other.view(N, W * H)[::4] = torch.randint(0, 256, (N // 4, W * H), dtype=torch.uint8, device="cuda", generator=gen)
    del noise
    sets = [h263mi.PlaneSet(t.data_ptr(), pixels, W, W * H) for t in (base, other)]

    bg = h263mi.make_background(CL, learn_shift=4, fg_learn_shift=6, pixel_threshold=24, warmup=0, cell_threshold=64, min_changed_cells=1)
    gw, gh, cells_bytes, state_bytes = h263mi.background_extent(N, W, H, bg)
    state = torch.zeros(state_bytes, dtype=torch.uint8, device="cuda")
    cells = torch.empty(cells_bytes, dtype=torch.uint8, device="cuda")
    summary = torch.empty(N * 16, dtype=torch.uint8, device="cuda")
    lst = torch.empty(N * 4, dtype=torch.uint8, device="cuda")
    count = torch.empty(4, dtype=torch.uint8, device="cuda")
    prev = base.clone()
    prev_set = h263mi.PlaneSet(prev.data_ptr(), pixels, W, W * H)
    change = h263mi.make_change(CL, 64 * 24, 1, roll=1)
    copy_bytes = 5 * pixels // 2
    src = torch.randint(0, 256, (copy_bytes,), dtype=torch.uint8, device="cuda", generator=gen)
    dst = torch.empty_like(src)
    torch.cuda.synchronize()

    def leg_background(k):
        h263mi.background_on(sets[k & 1], N, W, H, bg, state.data_ptr(), state_bytes, cells.data_ptr(), cells_bytes, summary.data_ptr(),
                             lst.data_ptr(), count.data_ptr(), stream=stream.cuda_stream)

    def leg_copy(k):
        dst.copy_(src, non_blocking=True)

    def leg_change(k):
        h263mi.change_map(sets[k & 1], prev_set, N, W, H, change, cells.data_ptr(), cells_bytes, summary.data_ptr(), lst.data_ptr(),
                          count.data_ptr(), stream=stream.cuda_stream)

    legs = {"background": leg_background, "copy": leg_copy, "change_map": leg_change}
    times = {name: [] for name in legs}
    with torch.cuda.stream(stream):
        for k in range(a.warmup + a.calls):
            for name, leg in legs.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(stream)
                leg(k)
                t1.record(stream)
                t1.synchronize()
                if k >= a.warmup:
                    times[name].append(t0.elapsed_time(t1) * 1e3)
    head = state[:64].cpu().numpy().view(h263mi.BACKGROUND_HEAD_DTYPE)[0]
    selected = int(count.cpu().numpy().view("uint32")[0])
    moved = {"background": 5 * pixels, "copy": 2 * copy_bytes, "change_map": 3 * pixels}
    out = {"what": "bench_bg", "commit": a.commit, "pictures": N, "width": W, "height": H, "cell": 1 << CL, "calls": a.calls,
           "age_at_the_end": int(head["age"]), "selected_at_the_end": selected}
    for name in legs:
        us = statistics.median(times[name])
        out[name] = {"median_us": round(us, 1), "min_us": round(min(times[name]), 1), "max_us": round(max(times[name]), 1),
                     "bytes_moved": moved[name], "tb_per_s": round(moved[name] / us / 1e6, 3)}
    out["background_over_copy"] = round(out["background"]["median_us"] / out["copy"]["median_us"], 3)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
