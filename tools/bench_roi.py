#!/usr/bin/env python3
"""Measures k_roi_tensor (h263mi_roi_tensor_on) against the kernel it was cut from, in one process on one GPU.

Workload: 64 x 1080p full-size RGBA on the device (a batch's own rendering of a synthetic I picture, strength 5) and 1 024 seeded
ROIs of mixed sizes, 32 to 600 pixels a side, anywhere in any picture, into 224 x 224 binary16 with ImageNet's normalisation: ONE
launch.  Yardstick: k_tensor_resize_framed through h263mi_batch_set_tensor_output_framed with one WINDOW of the median ROI size --
64 crops per launch, one per picture.  That kernel cannot be launched alone: a rendering is k_post into the batch's scratch, then
the framed kernel; so the yardstick is the time of a rendering in that shape LESS the time of the same rendering in the default
shape (k_post alone, into a buffer of the caller), both measured here.  The three legs are interleaved round by round; each window is
a host clock around `--launches` calls that ends in a device synchronise; the figure of a leg is the median of its rounds.

Prints one JSON line; --out FILE also writes it there.  No threshold: a record, not a gate."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "h263-rs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch  # noqa: F401  (before the library is loaded: it brings the HIP runtime that the C-ABI library must share, as in bench.py)

import bench
import h263mi

N, W, H = 64, 1920, 1080
OW, OH = 224, 224
IMAGENET = ([1 / (255 * 0.229), 1 / (255 * 0.224), 1 / (255 * 0.225)], [-0.485 / 0.229, -0.456 / 0.224, -0.406 / 0.225])


def make_rois(k, seed):
    rng = np.random.default_rng(seed)
    w = rng.integers(32, 601, k)
    h = rng.integers(32, 601, k)
    x = (rng.random(k) * (W - w + 1)).astype(np.int64)
    y = (rng.random(k) * (H - h + 1)).astype(np.int64)
    p = rng.integers(0, N, k)
    return [(int(p[i]), int(x[i]), int(y[i]), int(w[i]), int(h[i])) for i in range(k)]


def window(call, launches):
    """ms per call: `launches` calls, then a device synchronise, under a host clock"""
    h263mi.synchronize(0)
    t0 = time.perf_counter()
    for _ in range(launches):
        call()
    h263mi.synchronize(0)
    return (time.perf_counter() - t0) * 1e3 / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rois", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--seed", type=int, default=2025)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if h263mi.device_count() < 1:
        raise SystemExit("bench_roi: no HIP device -- nothing is measured without one")

    wl = bench.Workload(h263mi, N, 1, 0, 0, None)
    fr = wl.frames[0]
    rois = make_rois(a.rois, a.seed)
    med_w, med_h = int(np.median([r[3] for r in rois])), int(np.median([r[4] for r in rois]))
    t = h263mi.make_tensor_out(OW, OH, h263mi.TENSOR_F16, *IMAGENET)

    # the ROI leg's pictures: a batch's rendering in the default shape
    b = h263mi.Batch(N, W, H, 0, None)
    rgba = h263mi.DeviceBuffer(N * W * H * 4)
    b.decode(fr["ptype"], fr["mbs"].ptr, fr["co"].ptr, fr["base"].ptr, 0, 5, rgba.ptr, None)
    b.sync()
    d_rois = h263mi.DeviceBuffer(16 * len(rois))
    d_rois.upload(h263mi.roi_table(rois))
    status = h263mi.DeviceBuffer(4 * len(rois))
    out_bytes = h263mi.tensor_extent(len(rois), t)
    out = h263mi.DeviceBuffer(out_bytes)
    rgba_again = h263mi.DeviceBuffer(N * W * H * 4)             # what the default-shape leg renders into

    # the yardstick's batch: the same pictures, one WINDOW of the median size in the middle of each
    b2 = h263mi.Batch(N, W, H, 0, None)
    b2.decode(fr["ptype"], fr["mbs"].ptr, fr["co"].ptr, fr["base"].ptr, 0, 5, None, None)
    b2.sync()
    f = h263mi.make_framing(h263mi.FRAME_WINDOW, src=((W - med_w) // 2, (H - med_h) // 2, med_w, med_h), dst=(0, 0, OW, OH))
    b2.set_tensor_output_framed(t, f)
    out2 = h263mi.DeviceBuffer(h263mi.tensor_extent(N, t))

    legs = {
        "roi": lambda: h263mi.roi_tensor(rgba.ptr, rgba.nbytes, N, W, H, d_rois.ptr, len(rois), t, out.ptr, out_bytes, status.ptr),
        "framed_render": lambda: b2.render_rgba(5, out2.ptr),
        "default_render": lambda: b.render_rgba(5, rgba_again.ptr),
    }
    for call in legs.values():                                   # warm-up: every shape of the timed windows
        window(call, 3)
    assert int(status.download(dtype=np.uint32).sum()) == 0      # every ROI was valid
    ms = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, call in legs.items():
            ms[k].append(window(call, a.launches))
    med = {k: statistics.median(v) for k, v in ms.items()}
    framed_kernel = med["framed_render"] - med["default_render"]
    read = sum(4 * r[3] * r[4] for r in rois)
    written = len(rois) * 3 * OW * OH * 2
    res = {
        "what": "k_roi_tensor: %d ROIs (32..600 a side, seed %d) of 64 x 1080p RGBA -> %d x %d f16, one launch; yardstick "
                "k_tensor_resize_framed, one WINDOW %d x %d per picture = 64 crops per launch, as (rendering in that shape) - "
                "(rendering in the default shape)" % (len(rois), a.seed, OW, OH, med_w, med_h),
        "method": "one process, legs interleaved, %d rounds of %d calls each under a host clock ending in a device synchronise; medians"
                  % (a.rounds, a.launches),
        "roi_ms_per_launch": round(med["roi"], 4),
        "roi_us_per_crop": round(1e3 * med["roi"] / len(rois), 3),
        "roi_source_bytes": read,                                  # 4 * w * h summed over the table: what the rectangles hold
        "roi_tensor_bytes": written,
        "roi_gb_per_s_source_plus_tensor": round((read + written) / (med["roi"] * 1e6), 1),
        "framed_render_ms": round(med["framed_render"], 4),
        "default_render_ms": round(med["default_render"], 4),
        "framed_kernel_ms_per_launch": round(framed_kernel, 4),
        "framed_us_per_crop": round(1e3 * framed_kernel / N, 3),
        "framed_source_bytes": 4 * med_w * med_h * N,
        "ratio_per_crop_roi_over_framed": round((med["roi"] / len(rois)) / (framed_kernel / N), 3) if framed_kernel > 0 else None,
        "rounds_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()},
        "kernel_source_hash": bench.kernel_source_hash(),
    }
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    b.close()
    b2.close()


if __name__ == "__main__":
    main()
