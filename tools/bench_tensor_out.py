#!/usr/bin/env python3
"""Device ms per launch of k_tensor_resize (h263mi_tensor_out) beside k_rgba_resize at the same geometry, in one process:
64 x 1080p, records resident as events (bench.py's Workload), H263MI_CFG_PIPELINE_POST, launch timing (h263mi_batch_timing_*).

  rgba_default            d_rgba without a shape: the base of every resize
  rgba_<W'>x<H'>          k_frame into the RGBA scratch, then k_rgba_resize (the yardstick)
  tensor_<dt>_<W'>x<H'>   k_frame into the RGBA scratch, then k_tensor_resize (contiguous NCHW, ImageNet's scale and bias)

A resize kernel's ms per launch is the timed post-processing time of its run less the base's, over the GOP's launches (the
final flush k_post is the same in a run and its base).  Both kernels read the same 64 * w*h*4 bytes; they differ in the bytes
written per output pixel (4; 12 for float32, 6 for the 16-bit types): `bytes_ratio` is (read + written) of the tensor over the
same of the RGBA resize, `time_ratio` the same of their times.  `torch_second_pass_ms` is what the tensor output saves a caller
of the RGBA resize: one framework pass (permute, to(dtype), mul, add) over the [64, H', W', 4] bytes, timed with torch's own
events -- for information, where torch sees the device.  One warm-up round, then the best of --rounds.  Prints one JSON line.

    python tools/bench_tensor_out.py [--gop 16] [--rounds 3]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "h263-rs_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

try:
    import torch  # before h263mi: torch brings its own HIP runtime; the C-ABI library must share it (as in bench.py)
except ImportError:
    torch = None
import h263mi  # noqa: E402

W, H, N = 1920, 1080, 64
SIZES = [(224, 224), (640, 360)]
DTYPES = [("f32", h263mi.TENSOR_F32, 4), ("bf16", h263mi.TENSOR_BF16, 2)]
SCALE = [1 / (255 * 0.229), 1 / (255 * 0.224), 1 / (255 * 0.225)]
BIAS = [-0.485 / 0.229, -0.456 / 0.224, -0.406 / 0.225]


def time_shape(wl, shape, gop, rounds):
    """shape: ("rgba",) | ("rgba", ow, oh) | ("tensor", dtype, ow, oh) -> best round's timings"""
    import bench
    b = h263mi.Batch(N, W, H, 0, None, pipeline_post=True)
    if shape[0] == "tensor":
        t = h263mi.make_tensor_out(shape[2], shape[3], shape[1], SCALE, BIAS)
        b.set_tensor_output(t)
        out = h263mi.DeviceBuffer(h263mi.tensor_extent(N, t))
    elif len(shape) == 3:
        b.set_rgba_resize(shape[1], shape[2])
        out = h263mi.DeviceBuffer(h263mi.rgba_resize_extent(N, shape[1], shape[2]))
    else:
        out = h263mi.DeviceBuffer(N * W * H * 4)
    best = None
    for r in range(rounds + 1):                              # (round 0: warm-up)
        b.timing_reserve(8 * gop)
        b.timing_begin()
        t0 = time.perf_counter()
        for f in range(gop):
            fr = wl.frames[f]
            if fr.get("first") is not None:
                b.decode_events(fr["ptype"], fr["mbs"].ptr, fr["first"].ptr, fr["ev"].ptr, fr["base"].ptr, 0, bench.STRENGTH, out.ptr, None)
            else:
                b.decode(fr["ptype"], fr["mbs"].ptr, fr["co"].ptr, fr["base"].ptr, 0, bench.STRENGTH, out.ptr, None)
        b.sync()
        wall = (time.perf_counter() - t0) * 1e3 / gop
        kt = b.timing_end()
        row = {"wall_ms": wall, "k_frame_ms": kt.frame_ms / max(kt.frame_launches, 1), "post_ms": kt.post_ms}
        if r and (best is None or row["post_ms"] < best["post_ms"]):
            best = row
    b.close()
    out.free()
    return best


def torch_second_pass(ow, oh, dtype_name, rounds):
    """ms of permute / to(dtype) / mul / add over [N, H', W', 4] uint8, or None where torch sees no device"""
    if torch is None or not torch.cuda.is_available():
        return None
    dt = {"f32": torch.float32, "bf16": torch.bfloat16}[dtype_name]
    x = torch.randint(0, 256, (N, oh, ow, 4), dtype=torch.uint8, device="cuda")
    scale = torch.tensor(SCALE, dtype=torch.float32, device="cuda").view(1, 3, 1, 1)
    bias = torch.tensor(BIAS, dtype=torch.float32, device="cuda").view(1, 3, 1, 1)
    best = None
    for r in range(rounds + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        y = (x[..., :3].permute(0, 3, 1, 2).to(torch.float32) * scale + bias).to(dt).contiguous()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        if r >= 2 and (best is None or ms < best):
            best = ms
        del y
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gop", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import bench
    wl = bench.Workload(h263mi, N, args.gop, 0, 0, None, events=True)
    copy_gbs = h263mi.probe_bandwidth(h263mi.PROBE_COPY)
    res = {"what": "64 x 1080p, events, pipeline_post, strength %d; one warm-up round, best of %d rounds of a %d-picture GOP; "
                   "resize kernels: device ms per launch (64 pictures)" % (bench.STRENGTH, args.rounds, args.gop),
           "copy_ceiling_GBps": round(copy_gbs, 1)}
    base = time_shape(wl, ("rgba",), args.gop, args.rounds)
    res["k_frame_ms_rgba_default"] = round(base["k_frame_ms"], 4)
    for ow, oh in SIZES:
        row = time_shape(wl, ("rgba", ow, oh), args.gop, args.rounds)
        rgba_ms = (row["post_ms"] - base["post_ms"]) / args.gop
        rgba_bytes = N * (4 * W * H + 4 * ow * oh)
        name = "k_rgba_resize_%dx%d" % (ow, oh)
        res[name + "_ms"] = round(rgba_ms, 4)
        res[name + "_GBps"] = round(rgba_bytes / (rgba_ms * 1e-3) / 1e9, 1) if rgba_ms > 0 else None
        for dname, dtype, elt in DTYPES:
            row = time_shape(wl, ("tensor", dtype, ow, oh), args.gop, args.rounds)
            ms = (row["post_ms"] - base["post_ms"]) / args.gop
            moved = N * (4 * W * H + 3 * elt * ow * oh)
            name = "k_tensor_resize_%s_%dx%d" % (dname, ow, oh)
            res[name + "_ms"] = round(ms, 4)
            res[name + "_GBps"] = round(moved / (ms * 1e-3) / 1e9, 1) if ms > 0 else None
            res[name + "_of_ceiling"] = round(moved / (ms * 1e-3) / 1e9 / copy_gbs, 3) if ms > 0 else None
            res[name + "_bytes_ratio"] = round(moved / rgba_bytes, 3)
            res[name + "_time_ratio"] = round(ms / rgba_ms, 3) if rgba_ms > 0 else None
            res[name + "_k_frame_ms"] = round(row["k_frame_ms"], 4)
            second = torch_second_pass(ow, oh, dname, args.rounds)
            res["torch_second_pass_%s_%dx%d_ms" % (dname, ow, oh)] = round(second, 4) if second is not None else None
    print(json.dumps(res))


if __name__ == "__main__":
    main()
