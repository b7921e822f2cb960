#!/usr/bin/env python3
"""bench.py -- decoded megapixels/s of the MI355X macroblock back-end (BASELINE.json metric).

Workload (config.workload): BASELINE configs[3] -- a batch of 64 independent 1080p streams on each GPU.
A STEP is one pass over the resident synthetic input of the batch: GOPS_PER_STEP GOPs of 31 frame indices (1 I
picture with mixed block classes, then 30 P pictures: half-pel vectors in [-32, 31], 25 % coded blocks, quant 10)
for all 64 streams, i.e. 64 x 124 pictures per step.  Per frame index: k_recon (dequant + IDCT + half-pel MC +
residual add/clip) and k_post (deblock strength 5 + BT.601 -> RGBA) over the 64 pictures.  Records are generated on
the device beforehand (counter-based splitmix64), so inputs are resident in HBM when the timed region
starts.  With --gpus N every rank decodes its own 64 streams (weak scaling, no data-path collective); RCCL only
carries the barrier and the max-over-ranks reduction.  `python bench.py --gpus N` launches the N ranks itself
(torch.distributed.run); under an external launcher (WORLD_SIZE set) it is one of the ranks.

A plain run sets up, warms up, times the steps, writes --dump-outputs if asked and prints the line: nothing else.
Everything else the benchmark measures or checks runs with --full (each part can be left out there with its --no-*
option):
  * a PARITY GATE after the timed region, and outside it: the last picture (Y, Cb, Cr and RGBA) of streams 0, 31 and
    63 of the 64-stream batch is compared with the CPU oracle run from the GOP's I picture; a mismatch makes the run fail;
  * the box's copy / read / write ceilings (roofline.peak_measured*, bound_observed) and roofline.trusted_mode;
  * the `extra` legs (dense transport, dense I pictures, sustained, end to end from bitstreams, latencies);
  * `cpu_baseline`: the C oracle (a port of the reference CPU path, not the Rust binary) built natively on this box
    (-O3 -march=native -ffp-contract=off) and timed on its host cores with one stream per thread.

One JSON line is printed by rank 0.  `roofline` is for the kernel with the larger share of the timed region; its launch
times are the HIP events of the timed steps themselves, so a plain run reports them too.
"""
import argparse
import hashlib
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "h263-rs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

W, H = 1920, 1080
MBS_PP = 120 * 68
MP_PER_PICTURE = W * H / 1e6
Y_BYTES, C_BYTES = W * H, 960 * 540
YUV_BYTES = Y_BYTES + 2 * C_BYTES            # 3 110 400
RGBA_BYTES = W * H * 4                       # 8 294 400
HDR_BYTES = MBS_PP * 32                      # 261 120
HBM_PEAK_GBS = 8000.0                        # MI355X_MICROARCH.md: 8.0 TB/s spec
STRENGTH = 5                                 # QUANT_TO_STRENGTH[10] (deblock.rs:5-8)
GOP = 31
GOPS_PER_STEP = 4                            # 124 frame indices per step: >= 0.5 s of device time in 12+ steps
PARITY_STREAMS = (0, 31, 63)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--streams", type=int, default=64, help="streams per GPU")
    ap.add_argument("--total-streams", type=int, default=0,
                    help="strong scaling (SURVEY 8d config 5, second form): this many streams in total, split evenly over "
                         "the GPUs; 0 = off (weak scaling, --streams per GPU)")
    ap.add_argument("--gop", type=int, default=GOP)
    ap.add_argument("--gops-per-step", type=int, default=GOPS_PER_STEP)
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also run the parity gate, the measured ceilings, the extra legs and the CPU "
                         "baseline (the --no-* options below leave parts of that out)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the cpu_baseline object")
    ap.add_argument("--cpu-baseline-only", action="store_true", help="print the cpu_baseline object and exit (no GPU needed)")
    ap.add_argument("--no-extra", action="store_true", help="--full without the extra legs and roofline.trusted_mode")
    ap.add_argument("--no-e2e", action="store_true", help="--full without the extra.e2e_bitstream* legs")
    ap.add_argument("--sustained-seconds", type=float, default=10.0,
                    help="--full: length of extra.sustained (the headline loop, >= 10 s)")
    ap.add_argument("--no-parity-gate", action="store_true", help="--full without the parity gate (profiling runs only: "
                                                                   "the line then says so)")
    ap.add_argument("--dense-coeffs", action="store_true",
                    help="coefficients as dense 128-byte blocks in HBM (h263mi_batch_decode) instead of the sparse events the "
                         "host parser emits (h263mi_batch_decode_events)")
    ap.add_argument("--no-pipeline", action="store_true",
                    help="two launches per frame index (k_recon, then k_post) instead of the frame-pipelined single launch")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last step computed (a fixed, seeded sample of every stream's "
                         "Y, Cb, Cr planes and RGBA frame) as DIR/<name>.npy in float32, the sampled positions as "
                         "DIR/<name>_index.npy in float64, for output-for-output comparison of two builds")
    ap.add_argument("--overlap", action="store_true",
                    help="k_post on a second stream (post of picture i beside recon of picture i+1); measured: no gain")
    return ap.parse_args(argv)


# ---------------------------------------------------------------------------------------------------------------
# N-rank launch: one process per GPU.  Runs BEFORE anything touches the GPU (a process that has initialised HIP
# must never be replaced or forked into ranks).
# ---------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def visible_gpus():
    """Devices visible to this process, WITHOUT initialising the runtime (torch.cuda.device_count() does not, on
    this image).  H263MI_BENCH_STUB: CPU stand-in workload over gloo (tests/test_bench_launcher.py), any N."""
    if os.environ.get("H263MI_BENCH_STUB"):
        return 1 << 10
    import torch
    return torch.cuda.device_count()


def launch_ranks(args, argv):
    """`bench.py --gpus N` without a launcher around it: start N ranks of this file and return their exit code."""
    have = visible_gpus()
    if have < args.gpus:
        sys.stderr.write("bench.py: --gpus %d but only %d device(s) visible; refusing to report a smaller job as "
                         "n_gpus=%d\n" % (args.gpus, have, args.gpus))
        return 2
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + list(argv)
    return subprocess.run(cmd, env=env).returncode


# ---------------------------------------------------------------------------------------------------------------
# workload
# ---------------------------------------------------------------------------------------------------------------
class Workload:
    """Device-resident records of `gop` frame indices for `n` streams."""

    def __init__(self, h263mi, n, gop, first_stream, device_id, stream, i_kind=None, p_frames=True, events=False, stream_stride=1):
        """picture p of the batch is stream first_stream + p * stream_stride (strong scaling deals stream s to GPU s mod N)"""
        i_kind = h263mi.SYNTH_I_MIXED if i_kind is None else i_kind
        self.n, self.frames, self.h263mi, self.events = n, [], h263mi, events
        for f in range(gop):
            kind = i_kind if (f == 0 or not p_frames) else h263mi.SYNTH_P
            cap = n * MBS_PP * (6 if kind != h263mi.SYNTH_P else 2)
            d_mbs = h263mi.DeviceBuffer(n * MBS_PP * 32, device_id)
            d_co = h263mi.DeviceBuffer(cap * 128, device_id)
            d_base = h263mi.DeviceBuffer(n * 8, device_id)
            blocks = h263mi.synth_batch_device(kind, W, H, n, first_stream, f, d_mbs.ptr, d_co.ptr, cap, d_base.ptr,
                                               device_id, stream, stream_stride)
            ptype = h263mi.PICTURE_I if kind != h263mi.SYNTH_P else h263mi.PICTURE_P
            fr = dict(kind=kind, ptype=ptype, mbs=d_mbs, co=d_co, base=d_base, blocks=blocks)
            if events:
                fr.update(self.to_events(fr, device_id))
            self.frames.append(fr)

    def to_events(self, fr, device_id):
        """The same coefficients as sparse events (h263mi_submit_picture_events: one 32-bit word per non-zero LEVEL, an
        intra block's DC stays in its record), the transport form of the host parser: converted once, on the host, from
        the dense pool the generator wrote; the dense pool is freed."""
        import numpy as np
        h263mi, n = self.h263mi, self.n
        h263mi.synchronize(device_id)
        rec = fr["mbs"].download(n * MBS_PP * 32).view(h263mi.MB_RECORD_DTYPE)
        base = fr["base"].download(n * 8).view(np.uint64)
        blocks = fr["blocks"]
        co = fr["co"].download(blocks * 128).view(np.int16).reshape(-1, 64)
        cbp = rec["cbp"].astype(np.uint32)
        npop = np.zeros(len(rec), np.int64)
        for b in range(6):
            npop += (cbp >> b) & 1
        pool_index = np.repeat(base.astype(np.int64), MBS_PP) + rec["coeff_index"].astype(np.int64)
        intra_mb = (rec["mb_type"] == 3) | (rec["mb_type"] == 4)
        sel = intra_mb & (npop > 0)
        starts, lens = pool_index[sel], npop[sel]
        intra_block = np.zeros(blocks, bool)
        if lens.size:
            within = np.arange(int(lens.sum())) - np.repeat(np.cumsum(lens) - lens, lens)
            intra_block[np.repeat(starts, lens) + within] = True
        first, ev = h263mi.events_from_dense(co, intra_block)
        ev = np.concatenate([ev, np.zeros(8, np.uint32)])
        # The transport is chosen per picture: events pay off for sparse blocks (a P picture's 4 LEVELs per block); a
        # picture that averages more than 8 events per coded block (the GOP's I picture) stays dense -- rebuilding its
        # blocks from events takes the reconstruction waves eight trips per round.
        if int(first[-1]) > 8 * max(blocks, 1) and not os.environ.get("H263MI_BENCH_EVENTS_ALWAYS"):   # (the switch: probes only)
            return dict(first=None, ev=None, n_events=int(first[-1]))
        d_first = h263mi.DeviceBuffer(first.nbytes, device_id)
        d_first.upload(first)
        d_ev = h263mi.DeviceBuffer(ev.nbytes, device_id)
        d_ev.upload(ev)
        fr["co"].free()
        return dict(co=None, first=d_first, ev=d_ev, n_events=int(first[-1]))

    def recon_bytes(self, f, survey_8d=False):
        """algorithmic bytes of one k_recon launch: headers + coefficients + reference read (P only) + reconstructed
        planes written.  The coefficients count as what the transport of the picture MOVES: a picture sent as events is
        its block index (4 bytes per coded block + 4) and one 32-bit word per non-zero LEVEL; a dense picture 128 bytes
        per coded block.  survey_8d: SURVEY 8(d)'s figure, 128 bytes per coded block whatever the transport (what rounds
        1-3 reported; with events that counts ~89 MB per launch which are never read)."""
        fr = self.frames[f]
        coef = fr["blocks"] * 128
        if not survey_8d and fr.get("first") is not None:
            coef = (fr["blocks"] + 1) * 4 + fr["n_events"] * 4
        b = self.n * HDR_BYTES + coef + self.n * YUV_BYTES
        if fr["ptype"] == self.h263mi.PICTURE_P:
            b += self.n * YUV_BYTES
        return b

    def recon_write_bytes(self):
        """the part of recon_bytes that is written (the reconstructed planes)"""
        return self.n * YUV_BYTES

    def post_bytes(self):
        """algorithmic bytes of one k_post launch: the RGBA frames written.  Re-reading the reconstructed planes is
        the price of running deblock + convert as a second kernel and is NOT counted (a fully fused pipeline would
        keep them on chip)."""
        return self.n * RGBA_BYTES


def run_frames(batch, wl, d_rgba, n_frames, pipeline=False, checked=True):
    """n_frames frame indices starting at a GOP boundary (every GOP re-starts all streams with an I picture).
    pipeline: h263mi_batch_decode on a H263MI_CFG_PIPELINE_POST batch -- one launch per frame index reconstructs
    picture f and post-processes picture f - 1; the last picture's post-processing runs at the next sync.
    checked (the default, and what the headline runs): the calls say how large their arrays are (coeff_pool_blocks,
    n_events), as every host entry point does: the waves refuse to read a coded block outside the pool / an event list whose
    bounds do not ascend or reach beyond the events (include/h263mi.h).  checked=False is for a batch made with
    trusted_arrays (H263MI_CFG_TRUSTED_ARRAYS): the caller vouches, the waves check nothing (roofline.trusted_mode)."""
    g = len(wl.frames)
    for i in range(n_frames):
        fr = wl.frames[i % g]
        pool = fr["blocks"] if checked else 0
        if pipeline and wl.events and fr.get("first") is not None:
            batch.decode_events(fr["ptype"], fr["mbs"].ptr, fr["first"].ptr, fr["ev"].ptr, fr["base"].ptr, pool, STRENGTH,
                                d_rgba.ptr, None, n_events=fr["n_events"] if checked else 0)
        elif pipeline:
            batch.decode(fr["ptype"], fr["mbs"].ptr, fr["co"].ptr, fr["base"].ptr, pool, STRENGTH, d_rgba.ptr, None)
        else:
            batch.submit(fr["ptype"], fr["mbs"].ptr, fr["co"].ptr, fr["base"].ptr)
            batch.render_rgba(STRENGTH, d_rgba.ptr, None)


DUMP_SEED = 20260
DUMP_SAMPLES = {"y": 32768, "cb": 8192, "cr": 8192, "rgba": 131072}    # positions per stream and array
DUMP_MAX_BYTES = 64 << 20


def dump_outputs(h263mi, batch, d_rgba, n, out_dir, prefix=""):
    """The arrays a caller of the timed path receives after its last step -- each stream's decoded Y, Cb, Cr planes
    (h263mi_batch_copy_yuv) and its RGBA frame -- sampled at fixed positions (DUMP_SEED, the same positions for every
    stream and every run) and written as float32 <prefix><name>.npy of shape (n, k); <prefix><name>_index.npy (float64)
    holds the byte positions sampled within one stream's array.  Outside the timed region."""
    import numpy as np
    sizes = {"y": Y_BYTES, "cb": C_BYTES, "cr": C_BYTES, "rgba": RGBA_BYTES}
    rng = np.random.default_rng(DUMP_SEED)
    index = {k: np.sort(rng.choice(sizes[k], DUMP_SAMPLES[k], replace=False)) for k in sizes}
    total = sum(n * len(i) * 4 + len(i) * 8 for i in index.values())
    if total > DUMP_MAX_BYTES:
        raise SystemExit("--dump-outputs: %d bytes for %d streams exceeds the %d byte limit" % (total, n, DUMP_MAX_BYTES))
    out = {k: np.empty((n, len(i)), np.float32) for k, i in index.items()}
    for s in range(n):
        for k, plane in zip(("y", "cb", "cr"), batch.copy_yuv(s)):
            out[k][s] = plane[index[k]]
        out["rgba"][s] = d_rgba.download(RGBA_BYTES, s * RGBA_BYTES)[index["rgba"]]
    os.makedirs(out_dir, exist_ok=True)
    for k in sizes:
        np.save(os.path.join(out_dir, prefix + k + ".npy"), out[k])
        np.save(os.path.join(out_dir, prefix + k + "_index.npy"), index[k].astype(np.float64))
    return sorted(prefix + k + sfx + ".npy" for k in sizes for sfx in ("", "_index"))


def parity_gate(h263mi, batch, d_rgba, first_stream, n, gop, streams=PARITY_STREAMS, stream_stride=1):
    """BASELINE.md section 3 "parity gate": the batch has just decoded whole GOPs; its last picture (frame index
    gop-1, after gop-1 chained P pictures) of a few streams must equal the oracle's, planes and RGBA, bit for bit.
    The oracle is the checker here -- it is never on the timed or shipped path."""
    import numpy as np
    from oracle import oracle as orc
    checked = []
    for s in streams:
        if s >= n:
            continue
        ref = None
        for f in range(gop):
            kind = h263mi.SYNTH_I_MIXED if f == 0 else h263mi.SYNTH_P
            mbs, co = h263mi.synth_picture_host(kind, W, H, first_stream + s * stream_stride, f)
            rc, ref = orc.decode_picture(W, H, mbs, co, ref)
            if rc != 0:
                return "oracle error %d (stream %d frame %d)" % (rc, s, f), checked
        got = batch.copy_yuv(s)
        for name, g, e in zip(("Y", "Cb", "Cr"), got, ref):
            if not np.array_equal(g, e):
                return "stream %d: %s plane differs from the oracle in %d bytes" % (s, name, int((g != e).sum())), checked
        filt = tuple(orc.deblock(p, pw, STRENGTH) for p, pw in zip(ref, (W, 960, 960)))
        want = orc.yuv420_to_rgba(*filt, W)
        rgba = d_rgba.download(RGBA_BYTES, s * RGBA_BYTES)
        if not np.array_equal(rgba, want):
            return "stream %d: RGBA differs from the oracle in %d bytes" % (s, int((rgba != want).sum())), checked
        checked.append(first_stream + s * stream_stride)
    return "ok", checked


def kernel_source_hash():
    """identifies the kernel code a committed PMC traffic figure belongs to"""
    h = hashlib.sha256()
    d = os.path.join(ROOT, "h263-rs_amd", "csrc")
    for name in sorted(os.listdir(d)):
        if name.endswith((".inl", ".hip", ".h")):
            h.update(open(os.path.join(d, name), "rb").read())
    return h.hexdigest()[:16]


# ---------------------------------------------------------------------------------------------------------------
# CPU baseline: the oracle, built natively on this box, one stream per thread (pthreads inside the C library)
# ---------------------------------------------------------------------------------------------------------------
def cpu_quota():
    """CPUs' worth of time the cgroup of this container may use (cpu.max), or None when unlimited / unknown"""
    for path, parse in (("/sys/fs/cgroup/cpu.max", lambda t: (t.split()[0], t.split()[1])),):
        try:
            quota, period = parse(open(path).read())
            if quota != "max":
                return max(1, int(int(quota) / int(period)))
        except Exception:
            pass
    try:
        q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
        per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        if q > 0:
            return max(1, q // per)
    except Exception:
        pass
    return None


def physical_cores():
    """(threads to use, physical cores of the host, logical CPUs in the affinity mask, cgroup quota, model name):
    one thread per physical core (lscpu's cores x sockets), capped by the affinity mask and by the CPU quota of the
    container -- more runnable threads than the quota allows only get throttled (measured on the GPU box: 16 CPUs of
    quota on a 128-core host; 16 threads reach 1 744 MP/s, 128 threads 1 294 MP/s)."""
    model, cores = "unknown", None
    try:
        txt = subprocess.run(["lscpu"], capture_output=True, text=True, timeout=10).stdout
        kv = dict((k.strip(), v.strip()) for k, v in (ln.split(":", 1) for ln in txt.splitlines() if ":" in ln))
        model = kv.get("Model name", model)
        cores = int(kv["Core(s) per socket"]) * int(kv["Socket(s)"])
    except Exception:
        pass
    avail = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    if not cores:
        cores = max(1, avail // 2)
    quota = cpu_quota()
    use = max(1, min(cores, avail, quota or cores))
    return use, cores, avail, quota, model


def cpu_baseline(h263mi, budget_s=12.0):
    from oracle import native_bench       # checker/baseline only: never on the product path
    t_build = time.perf_counter()
    nb = native_bench.NativeOracle()      # gcc -O3 -march=native -ffp-contract=off, on this box
    t_build = time.perf_counter() - t_build
    cores, host_cores, logical, quota, model = physical_cores()
    n_distinct = min(cores, 4)
    streams = []
    for s in range(n_distinct):
        pics = []
        for f in range(GOP):
            kind = h263mi.SYNTH_I_MIXED if f == 0 else h263mi.SYNTH_P
            pics.append(h263mi.synth_picture_host(kind, W, H, 100 + s, f))
        streams.append(pics)
    nb.check_against_portable(W, H, streams[0][:3], STRENGTH)      # byte-equal to the -O2 oracle before timing
    nb.check_simd_stages(W, H, streams[0][:2], STRENGTH)           # ... and the explicit-SIMD deblock / BT.601 to the oracle
    # The headline: what a consumer of the reference runs per picture -- reconstruction, deblock() x 3 planes and
    # yuv420_to_rgba -- with deblock and BT.601 in the reference's own explicit 128-bit SIMD shape (oracle/simd_stages.c;
    # gcc does not vectorise the oracle's one-lane-at-a-time restatement of them, see `autovectorised`).
    one = nb.run(W, H, streams[:1], 1, 1, STRENGTH, simd=True)     # 1 thread, one GOP
    one_mp = GOP * MP_PER_PICTURE / one
    # T threads, one stream each, whole GOPs; bounded to ~budget_s of wall clock
    gops = max(1, min(24, int(budget_s / (1.3 * one))))
    wall = nb.run(W, H, streams, cores, gops, STRENGTH, simd=True)
    value = cores * gops * GOP * MP_PER_PICTURE / wall
    # "recon / deblock / yuv->rgba individually and end-to-end", 1 thread and T threads.  A stage
    # on its own works on one fixed picture (the GOP's second), 31 times over per "GOP".
    stages = {}
    for name, bits, reps in (("recon", nb.RECON, 1), ("deblock_x3_planes", nb.DEBLOCK, 4), ("yuv420_to_rgba", nb.RGBA, 2)):
        row = {}
        for simd in ((False,) if bits == nb.RECON else (False, True)):
            t1 = nb.run(W, H, streams[:1], 1, reps, STRENGTH, stages=bits, simd=simd)
            tt = nb.run(W, H, streams, cores, reps, STRENGTH, stages=bits, simd=simd)
            key = "" if bits == nb.RECON else ("_simd128" if simd else "_scalar")
            row["one_thread_mp_s" + key] = round(reps * GOP * MP_PER_PICTURE / t1, 1)
            row["%d_threads_mp_s%s" % (cores, key)] = round(cores * reps * GOP * MP_PER_PICTURE / tt, 1)
        stages[name] = row
    scalar_one = nb.run(W, H, streams[:1], 1, 1, STRENGTH, simd=False)
    stages["end_to_end"] = {"one_thread_mp_s_simd128": round(one_mp, 1), "%d_threads_mp_s_simd128" % cores: round(value, 1),
                            "one_thread_mp_s_scalar": round(GOP * MP_PER_PICTURE / scalar_one, 1)}
    return {"value": round(value, 2), "unit": "MP/s", "cores": cores, "kind": "port",
            "cores_physical": host_cores, "cpus_logical": logical, "cpu_quota": quota, "cpu_model": model,
            "flags": nb.flags, "one_thread_mp_s": round(one_mp, 2),
            "parallel_efficiency": round(value / (cores * one_mp), 3),
            "stages": stages,
            "autovectorised": nb.vectorisation_report(),
            "simd_note": "deblock / BT.601 of `value` and of the *_simd128 rows are oracle/simd_stages.c: the reference's explicit "
                         "128-bit shape (8 x i16 quartets, deblock.rs:99-127; 4 x i32 pixels, bt601.rs:12-59) on gcc vector types, "
                         "byte-checked against the oracle before timing; *_scalar rows are the oracle's own loops, which gcc "
                         "leaves scalar (`autovectorised`).  The reconstruction has no SIMD in the reference either "
                         "(idct.rs / gather.rs are scalar Rust): its f32 matrix loops are what the compiler makes of them.",
            "sample": "%d threads (one per physical core the container may use) x 1 stream x %d GOP(s) of 31 pictures (1 I + 30 P) of the bench "
                      "workload at 1920x1080, recon + deblock(%d) x3 planes + BT.601; C port of the h263-rs CPU "
                      "path (not the Rust binary) with pthreads, %d distinct streams shared read-only; %.1f s wall, "
                      "built in %.1f s; per-stage rows: 1-4 x 31 passes each" % (cores, gops, STRENGTH, n_distinct, wall, t_build)}


# ---------------------------------------------------------------------------------------------------------------
# end to end: Sorenson Spark bitstreams -> host parser threads -> events over PCIe -> k_frame (k_recon / k_post at the ends)
# ---------------------------------------------------------------------------------------------------------------
def e2e_bitstream(h263mi, n, device_id, stream, d_rgba, corpus="kinds", n_distinct=8, n_frames=8, gop=GOP, parser_threads=None,
                  min_seconds=1.5):
    """The north star's end-to-end figure (never the headline `value`: the host parser and the PCIe link are in it).
    n streams of 1920x1080 Sorenson Spark pictures, one h263mi_batch_decode_next_pictures_ex per frame index on a
    frame-pipelined batch: host parser threads -> sparse records + events over PCIe -> k_frame (reconstruction of this picture +
    deblock / RGBA of the previous one).  Every stream has its OWN picture quantiser and asks for the deblocker in its header;
    the call renders each with H263MI_STRENGTH_FROM_HEADER = QUANT_TO_STRENGTH[its PQUANT] (deblock.rs:5-8), as a consumer of
    the reference picks it per picture (picture.rs:61-64).  The corpus:
      "dense"    the bench workload's records (every macroblock coded, random half-pel vectors: ~35 Mbit/s per stream, ten
                 times a typical Spark stream), `n_distinct` streams x `n_frames` pictures, PQUANT 10; a GOP's P pictures cycle
                 through the n_frames - 1 encoded ones (each is a valid P picture on whatever reference precedes it);
      "kinds"    pictures shaped like real content (tests/fixture_enc: ~2/3 of the macroblocks not coded, slow global motion,
                 few small residuals; key frames of ~150 KB), `n_distinct` different streams dealt to the n by a seeded draw,
                 P pictures cycling as above, PQUANT 4 .. 20 by stream kind -- round 5's definition of the realistic leg: a
                 parser thread meets each of 64 pictures ~560 times in the run, which flatters its branch predictor;
      "distinct" the same content, ALL DISTINCT: n streams x one whole GOP, every one of the n x gop pictures different
                 (VERDICT r5 next 3b); the timed GOPs re-decode that corpus (1 984 pictures, ~35 MB of bitstream per pass).
    The streams are written by the C++ fixture writer (tests/fixture_enc, byte for byte tests/sorenson_enc.py's output:
    tests/test_fixture_enc.py) in a second or two; the oracle decodes the same records for the parity check."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import fixture_enc as fx
    from oracle import oracle as orc
    t_enc = time.perf_counter()
    q2s = [int(v) for v in h263mi.quant_to_strength()]
    cores = parser_threads or physical_cores()[0]
    seed = 20261004
    if corpus == "distinct":
        n_distinct, n_frames = n, gop
    quants = [10] * n_distinct if corpus == "dense" else [4 + (7 * s) % 17 for s in range(n_distinct)]
    dense_recs = {}
    if corpus == "dense":
        from test_bitstream_e2e import make_codable
        streams = []
        for s in range(n_distinct):
            pics = []
            for f in range(n_frames):
                mbs, co = h263mi.synth_picture_host(h263mi.SYNTH_I_MIXED if f == 0 else h263mi.SYNTH_P, W, H, 200 + s, f)
                mbs = make_codable(mbs, quants[s], s * 100 + f, 0 if f == 0 else 1)
                pics.append(fx.encode_picture(W, H, 0 if f == 0 else 1, quants[s], mbs, co, temporal_reference=f, deblock_flag=1))
                dense_recs[(s, f)] = (mbs, co)
            streams.append(pics)
    else:
        streams = fx.corpus(seed, n_distinct, n_frames, W, H, quants, deblock_flag=1, threads=max(2, min(cores, 16)))

    def records(v, f):
        """what the oracle decodes for picture f of distinct stream v: the records the writer serialised"""
        if corpus == "dense":
            return dense_recs[(v, f)]
        _, mbs, co = fx.picture(seed, v, f, W, H, f == 0, quants[v], 1, with_records=True)
        return mbs, co

    t_enc = time.perf_counter() - t_enc
    batch = h263mi.Batch(n, W, H, device_id, stream, pipeline_post=True)
    # which of the distinct streams each of the n is: a seeded draw, not s % n_distinct -- a parser thread takes the streams
    # t, t + T, t + 2T, ..., and with T a multiple of n_distinct it would meet ONE picture again and again and have its branches
    # predicted from history (tools/probes/e2e_distinct_streams.py)
    if corpus == "distinct":
        variant = list(range(n))
    else:
        variant = [int(v) for v in np.random.default_rng(20261004).integers(0, n_distinct, n)]
        for s in range(min(n, n_distinct)):
            variant[s] = s                                       # (the parity check below reads streams 0 .. n_distinct - 1)
    prepared = [batch.prepare_pictures([streams[variant[s]][f] for s in range(n)]) for f in range(n_frames)]
    # picture of the stream at each frame index of a GOP
    order = list(range(gop)) if corpus == "distinct" else [0] + [1 + k % (n_frames - 1) for k in range(gop - 1)]

    def run_gop(threads, sync=True):
        for f in order:
            used, rcs = batch.decode_next_pictures_ex(None, n_threads=threads, prepared=prepared[f],
                                                      strength=h263mi.STRENGTH_FROM_HEADER, d_rgba=d_rgba.ptr)
            if any(rcs):
                raise RuntimeError("e2e: stream errors %s" % [r for r in rcs if r][:4])
        if sync:
            batch.sync()

    run_gop(cores)                                               # warm-up: staging buffers, parser tables ...
    t_warm = time.perf_counter()
    run_gop(cores)                                               # ... of BOTH staging slots (a GOP has an odd number of calls)
    t_warm = time.perf_counter() - t_warm
    # as many GOPs as fill about min_seconds (3 at least): three GOPs of the realistic streams are 70 ms, and the figure moved
    # by 10 % from run to run on one box
    reps = max(3, min(400, int(min_seconds / max(t_warm, 1e-3))))
    batch.timing_reserve(2 * len(order) * reps + 8)
    batch.timing_begin()
    t0 = time.perf_counter()
    for k in range(reps):
        # a server does not drain the pipeline between two GOPs of a stream: the key frames of the next GOP are parsed while
        # the GPU finishes the last pictures of this one; everything queued is waited for inside the timed region
        run_gop(cores, sync=k == reps - 1)
    dt = time.perf_counter() - t0
    kt = batch.timing_end()
    # parity of what just ran: last picture (planes and RGBA) of a few streams against the oracle
    ok = True
    check = sorted({0, n // 2, n - 1}) if corpus == "distinct" else sorted(set(range(min(n, n_distinct, 3))) | {n - 1})
    for s in check:
        ref = None
        for f in order:
            mbs, co = records(variant[s], f)
            rc, ref = orc.decode_picture(W, H, mbs, co, ref)
        ok = ok and all(np.array_equal(g, e) for g, e in zip(batch.copy_yuv(s), ref))
        filt = tuple(orc.deblock(p, pw, q2s[quants[variant[s]]]) for p, pw in zip(ref, (W, 960, 960)))
        ok = ok and np.array_equal(d_rgba.download(RGBA_BYTES, s * RGBA_BYTES), orc.yuv420_to_rgba(*filt, W))
    # the stages on their own: the same call with one parser thread
    p_bytes = sum(len(p) for p in streams[0][1:])
    i_bytes = len(streams[0][0])
    # (the first GOP behind the many-thread run finds every stream's buffers in other cores' caches: best of the two behind it)
    run_gop(1)
    dt1 = 1e9
    for _ in range(2):
        t1 = time.perf_counter()
        run_gop(1)
        dt1 = min(dt1, time.perf_counter() - t1)
    placement = batch.host_placement()
    batch.close()
    pics = n * len(order) * reps
    pps = pics / dt
    gop_bytes = sum(len(streams[variant[s]][f]) for s in range(n) for f in order)
    p_mean = int(p_bytes / max(n_frames - 1, 1))
    what = {"dense": "the bench workload's records (every macroblock coded); %d distinct streams, the P pictures cycle through %d "
                     "encoded ones" % (n_distinct, n_frames - 1),
            "kinds": "pictures shaped like real content; %d distinct streams dealt to the %d at random, the P pictures cycle through "
                     "%d encoded ones (round 5's definition)" % (n_distinct, n, n_frames - 1),
            "distinct": "pictures shaped like real content, ALL DISTINCT: %d streams x %d pictures = %d different pictures, "
                        "%.1f MB of bitstream per GOP pass" % (n, gop, n * gop, gop_bytes / 1e6)}[corpus]
    return {"_pictures": pics, "_seconds": dt, "corpus": corpus, "picture_quantisers": sorted(set(quants)),
            "distinct_pictures": n_distinct * n_frames,
            "pictures_per_s": round(pps, 1), "mp_per_s": round(pps * MP_PER_PICTURE, 1),
            "realtime_1080p30_streams": round(pps / 30.0, 1), "parity_vs_oracle": "ok" if ok else "MISMATCH",
            "parity_streams": check,
            "parser_threads": cores, "gops_timed": reps, "timed_seconds": round(dt, 3),
            "bitstream_mb_per_s": round(gop_bytes * reps / dt / 1e6, 1),
            "one_parser_thread_pictures_per_s": round(n * len(order) / dt1, 1),
            "one_parser_thread_bitstream_mb_per_s": round(gop_bytes / dt1 / 1e6, 1),
            "bytes_per_picture": {"I": i_bytes, "P_mean": p_mean},
            "p_picture_mbit_per_s_at_30fps": round(p_mean * 8 * 30 / 1e6, 2),
            "gop_mbit_per_s_at_30fps": round((i_bytes + p_mean * (len(order) - 1)) / len(order) * 8 * 30 / 1e6, 2),
            "k_frame_avg_ms": round(kt.frame_ms / max(kt.frame_launches, 1), 4), "k_frame_launches": kt.frame_launches,
            "k_recon_launches": kt.recon_launches, "k_post_launches": kt.post_launches,
            "host_placement": {"device_numa_node": placement[0], "staging_numa_node": placement[1], "pool_cpus": len(placement[2])},
            "what": "%d streams x GOPs of %d pictures (1 I + %d P) of 1920x1080 Sorenson Spark: %s; "
                    "h263mi_batch_decode_next_pictures_ex on a frame-pipelined batch (host parser on %d threads -> sparse records + "
                    "events -> H2D -> k_frame: reconstruction from the events + deblock(strength from each picture's own header: "
                    "PQUANT %s) + BT.601 of the previous picture in one launch) per frame index; streams written by "
                    "tests/fixture_enc in %.1f s" % (n, len(order), len(order) - 1, what, cores, sorted(set(quants)), t_enc),
            "limit": "host parser: the container's CPU-time quota (cpu_quota_per_rank CPUs; %d threads that park when they are "
                     "out of work share it, include/h263mi.h: h263mi_default_parser_threads); the device-resident rate of the "
                     "same kernels is the headline value" % cores}


class GpuSampler:
    """Shader clock, socket power, temperature and busy share of ONE device, sampled from sysfs on a side thread while a leg
    runs (extra.sustained): /sys/bus/pci/devices/<bdf>/pp_dpm_sclk (the level marked `*`), hwmon power1_average / power1_input,
    temp1_input, gpu_busy_percent.  Whatever the container does not show stays None."""

    def __init__(self, pci_bdf, period=0.25):
        import threading
        self.base = "/sys/bus/pci/devices/%s" % pci_bdf if pci_bdf else None
        self.period, self.samples, self._stop = period, [], threading.Event()
        self._thread = threading.Thread(target=self._run, daemon=True)

    @staticmethod
    def _read(path):
        try:
            return open(path).read()
        except Exception:
            return None

    def sample(self):
        import glob
        out = {"t": time.perf_counter(), "sclk_mhz": None, "power_w": None, "temp_c": None, "busy_pct": None}
        if not self.base:
            return out
        txt = self._read(self.base + "/pp_dpm_sclk")
        if txt:
            for ln in txt.splitlines():
                if "*" in ln:
                    try:
                        out["sclk_mhz"] = int("".join(ch for ch in ln.split(":")[1].split("M")[0] if ch.isdigit()))
                    except Exception:
                        pass
        for name, key, scale in (("power1_average", "power_w", 1e-6), ("power1_input", "power_w", 1e-6), ("temp1_input", "temp_c", 1e-3)):
            if out[key] is None:
                for pth in glob.glob(self.base + "/hwmon/hwmon*/" + name):
                    v = self._read(pth)
                    if v and v.strip().lstrip("-").isdigit():
                        out[key] = round(int(v) * scale, 1)
                        break
        v = self._read(self.base + "/gpu_busy_percent")
        if v and v.strip().isdigit():
            out["busy_pct"] = int(v)
        return out

    def _run(self):
        while not self._stop.is_set():
            self.samples.append(self.sample())
            self._stop.wait(self.period)

    def __enter__(self):
        self._thread.start()
        return self

    def __exit__(self, *exc):
        self._stop.set()
        self._thread.join()

    def window(self, t0, t1, key):
        v = [s[key] for s in self.samples if t0 <= s["t"] <= t1 and s[key] is not None]
        return round(sum(v) / len(v), 1) if v else None


def sustained_run(torch, batch, wl, d_rgba, frames_per_step, pipeline, n, pci_bdf, seconds=10.0):
    """the headline loop for >= `seconds` instead of 0.64 s -- "N x real-time" is a sustained
    claim.  Steps back to back, one sync per step (a step is ~32 ms of launches: the sync is a 20 us bubble in it); the rate of
    the first second against the last, and what the device's clock, power and temperature did meanwhile (sysfs)."""
    run_frames(batch, wl, d_rgba, frames_per_step, pipeline)
    batch.sync()
    torch.cuda.synchronize()
    stamps = []
    with GpuSampler(pci_bdf) as gs:
        t0 = time.perf_counter()
        stamps.append(t0)
        while stamps[-1] - t0 < seconds:
            run_frames(batch, wl, d_rgba, frames_per_step, pipeline)
            batch.sync()
            stamps.append(time.perf_counter())
    total = stamps[-1] - t0
    mp_step = n * frames_per_step * MP_PER_PICTURE

    def rate(lo, hi):
        k = [i for i in range(1, len(stamps)) if lo <= stamps[i] - t0 <= hi]
        return round(len(k) * mp_step / (stamps[k[-1]] - stamps[k[0] - 1]), 1) if k else None

    first, last = rate(0.0, 1.0), rate(total - 1.0, total + 1.0)
    return {"seconds": round(total, 3), "steps": len(stamps) - 1, "mp_per_s": round((len(stamps) - 1) * mp_step / total, 1),
            "first_second_mp_per_s": first, "last_second_mp_per_s": last,
            "last_over_first": round(last / first, 4) if first and last else None,
            "slowest_step_ms": round(max(b - a for a, b in zip(stamps, stamps[1:])) * 1e3, 3),
            "fastest_step_ms": round(min(b - a for a, b in zip(stamps, stamps[1:])) * 1e3, 3),
            "device": {"pci": pci_bdf, "samples": len(gs.samples),
                       "sclk_mhz_first_second": gs.window(t0, t0 + 1.0, "sclk_mhz"), "sclk_mhz_last_second": gs.window(stamps[-1] - 1.0, stamps[-1], "sclk_mhz"),
                       "power_w_first_second": gs.window(t0, t0 + 1.0, "power_w"), "power_w_last_second": gs.window(stamps[-1] - 1.0, stamps[-1], "power_w"),
                       "temp_c_first_second": gs.window(t0, t0 + 1.0, "temp_c"), "temp_c_last_second": gs.window(stamps[-1] - 1.0, stamps[-1], "temp_c"),
                       "busy_pct_mean": gs.window(t0, stamps[-1], "busy_pct")},
            "what": "the headline loop (checked calls, %d frame indices per step, one sync per step) for %.0f s; rates over the steps "
                    "that end inside the first and the last second; device clock / power / temperature from sysfs (null: not visible "
                    "in this container; the shader clock from the GRBM counter is in profiles/README.md)" % (frames_per_step, seconds)}


def plain_function_latency(h263mi, reps=10):
    """host-to-host latency of the drop-in plain functions on one 1080p picture (deblock.rs:305, bt601.rs:105): the
    device scratch is kept per thread, so every call after the first allocates nothing"""
    import numpy as np
    rng = np.random.default_rng(3)
    y = rng.integers(0, 256, W * H, dtype=np.uint8)
    cb = rng.integers(0, 256, C_BYTES, dtype=np.uint8)
    cr = rng.integers(0, 256, C_BYTES, dtype=np.uint8)
    out = {}
    for name, fn in (("deblock_luma_ms", lambda: h263mi.deblock(y, W, STRENGTH)),
                     ("yuv420_to_rgba_ms", lambda: h263mi.yuv420_to_rgba(y, cb, cr, W))):
        t_first = time.perf_counter()
        fn()
        t_first = time.perf_counter() - t_first
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        out[name] = round((time.perf_counter() - t0) / reps * 1e3, 3)
        out[name.replace("_ms", "_first_call_ms")] = round(t_first * 1e3, 3)
    out["what"] = "one 1920x1080 plane / picture from host memory and back (PCIe both ways), mean of %d calls after the first" % reps
    return out


def single_stream_latency(h263mi, device_id, stream, n_p=12, reps=3):
    """The drop-in caller's own number: ONE H263State, one picture at a time, as a Ruffle-style consumer runs it
    (state.rs:138-141 decode_next_picture -> picture.rs:140-142 as_yuv -> deblock -> bt601.rs:105 yuv420_to_rgba): the
    host-to-host latency per 1080p picture of h263mi_decode_next_picture + the RGBA rendering, for a key frame and for
    P pictures shaped like real content, with the RGBA going to pageable memory (h263mi_render_rgba), to the caller's
    pinned buffer through a device buffer and a copy (h263mi_render_rgba on pinned memory) and straight into the pinned
    buffer (h263mi_render_rgba_pinned: the kernel's stores cross the link themselves).  Beside it: the C port of the
    reference CPU path on one thread for the same pictures (reconstruction + deblock x 3 + BT.601, explicit-SIMD
    post-processing; no bitstream parsing in it: the oracle has no parser), and this library's host parser alone."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import fixture_enc as fx
    from oracle import oracle as orc
    from oracle import native_bench
    pics, recs = [], []
    for f in range(1 + n_p):
        data, mbs, co = fx.picture(20261004, 900, f, W, H, f == 0, 10, 1, with_records=True)
        pics.append(data)
        recs.append((mbs, co))
    st = h263mi.H263State(h263mi.SORENSON_SPARK_BITSTREAM, device_id, stream)
    pinned = h263mi.PinnedBuffer(RGBA_BYTES)
    pageable = np.empty(RGBA_BYTES, np.uint8)
    lib = h263mi.lib()

    def render(mode):
        if mode == "pageable":
            h263mi._check(lib.h263mi_render_rgba(st._h, STRENGTH, h263mi._p(pageable)), "render_rgba")
            return pageable
        if mode == "pinned_copy":
            h263mi._check(lib.h263mi_render_rgba(st._h, STRENGTH, h263mi._p(pinned.array)), "render_rgba")
            return pinned.array
        return st.render_rgba_pinned(STRENGTH, pinned)

    out, ok = {}, True
    for mode in ("pageable", "pinned_copy", "pinned_direct"):
        t_i, t_p, t_dec_i, t_dec_p = [], [], [], []
        for rep_ in range(reps + 1):
            st.reset()
            for f, data in enumerate(pics):
                t0 = time.perf_counter()
                st.decode_next_picture(data)
                t1 = time.perf_counter()
                got = render(mode)
                t2 = time.perf_counter()
                if rep_:                                  # the first pass allocates staging and frame store
                    (t_i if f == 0 else t_p).append(t2 - t0)
                    (t_dec_i if f == 0 else t_dec_p).append(t1 - t0)
        # parity of what was timed: the last picture of the chain, planes and RGBA
        ref = None
        for mbs, co in recs:
            rc, ref = orc.decode_picture(W, H, mbs, co, ref)
        filt = tuple(orc.deblock(p, pw, STRENGTH) for p, pw in zip(ref, (W, 960, 960)))
        ok = ok and np.array_equal(np.asarray(got)[:RGBA_BYTES], orc.yuv420_to_rgba(*filt, W))
        ok = ok and all(np.array_equal(g, e) for g, e in zip(st.get_last_picture().as_yuv(), ref))
        med = lambda v: round(float(np.median(v)) * 1e3, 3)
        out[mode] = {"I_picture_ms": med(t_i), "P_picture_ms": med(t_p), "P_picture_ms_p90": round(float(np.percentile(t_p, 90)) * 1e3, 3),
                     "of_which_decode_call_ms": {"I": med(t_dec_i), "P": med(t_dec_p)}}
    nb = native_bench.NativeOracle()
    cw = 960
    t_cpu_i, t_cpu_p = [], []
    for rep_ in range(2):
        ref = None
        for f, (mbs, co) in enumerate(recs):
            t0 = time.perf_counter()
            rc, ref = orc.decode_picture(W, H, mbs, co, ref, L=nb.L)
            filt = tuple(nb.deblock_simd(p, pw, STRENGTH) for p, pw in zip(ref, (W, cw, cw)))
            nb.yuv420_to_rgba_simd(*filt, W)
            (t_cpu_i if f == 0 else t_cpu_p).append(time.perf_counter() - t0)
    st.close()
    pinned.free()
    out["cpu_port_one_thread"] = {"I_picture_ms": round(float(np.median(t_cpu_i)) * 1e3, 3),
                                  "P_picture_ms": round(float(np.median(t_cpu_p)) * 1e3, 3),
                                  "what": "C port of the reference CPU path (oracle, native build) from RECORDS: reconstruction + "
                                          "deblock x 3 + BT.601 (explicit 128-bit SIMD forms), one thread, no bitstream parsing"}
    out["parity_vs_oracle"] = "ok" if ok else "MISMATCH"
    out["bytes_per_picture"] = {"I": len(pics[0]), "P_mean": int(sum(len(p) for p in pics[1:]) / n_p)}
    out["what"] = ("one H263State, 1920x1080 Sorenson Spark pictures shaped like real content (1 I + %d P), one call of "
                   "h263mi_decode_next_picture (host parse -> events -> H2D -> k_recon) + one RGBA rendering (deblock %d + BT.601) "
                   "per picture, host to host, median of %d passes; pageable = h263mi_render_rgba into ordinary memory, "
                   "pinned_copy = the same into h263mi_host_alloc memory, pinned_direct = h263mi_render_rgba_pinned" % (n_p, STRENGTH, reps))
    return out


# ---------------------------------------------------------------------------------------------------------------
def stub_main(args, rank, world):
    """CPU stand-in for the launcher test: same rendezvous, barrier and aggregation code over gloo, no GPU work."""
    import torch.distributed as dist
    import shard
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo")
        side = dist.new_group(backend="gloo")        # (the side group main() makes for its long host-side waits)
        dist.barrier(group=side)
    else:
        dist = None
    elapsed = shard.timed_region(dist, lambda: time.sleep(0.01 * args.steps))
    strong = args.total_streams > 0
    mine = shard.streams_of_rank(rank, world, args.streams, total_streams=args.total_streams if strong else None)
    pictures = shard.aggregate_pictures(dist, len(mine) * args.steps * args.gop * args.gops_per_step)
    # the end-to-end leg of every rank (stand-in: rank r "decodes" 100 * (r + 1) pictures in 0.1 * (r + 1) s) and the host
    # thread budget of a rank, through the same functions main() uses
    threads = shard.parser_threads_for_rank(physical_cores()[0], world)
    e2e_rate, e2e_units, e2e_seconds = shard.aggregate_rate(dist, 100 * (rank + 1), 0.1 * (rank + 1))
    all_streams = [None] * world
    if dist is not None:
        dist.all_gather_object(all_streams, mine)
    else:
        all_streams = [mine]
    # where the library would place this rank's host side (NUMA node of its GPU, its slice of that node's cores): the real
    # code path of a batch (worker_pool.cpp: host_placement) on the topology H263MI_SYSFS_ROOT / H263MI_STUB_PCI_IDS describe
    placement = None
    if os.environ.get("H263MI_STUB_PCI_IDS"):
        import h263mi
        node, cpus = h263mi.debug_host_placement(os.environ["H263MI_STUB_PCI_IDS"].split(","), rank, shard.local_world_size(world))
        placement = [None] * world
        mine_pl = {"rank": rank, "node": node, "cpus": cpus}
        if dist is not None:
            dist.all_gather_object(placement, mine_pl)
        else:
            placement = [mine_pl]
    if rank == 0:
        print(json.dumps({"metric": "stub", "value": pictures * MP_PER_PICTURE / elapsed, "unit": "MP/s", "n_gpus": world,
                          "steps": args.steps, "warmup": args.warmup, "data": "stub (no GPU work)",
                          "pictures": pictures, "scaling": "strong" if strong else "weak",
                          "streams_of_rank": all_streams, "parser_threads_per_rank": threads,
                          "cpu_budget": physical_cores()[0], "local_world_size": shard.local_world_size(world),
                          "placement_per_rank": placement,
                          "e2e": {"pictures_per_s": e2e_rate, "pictures": e2e_units, "seconds": e2e_seconds}}), flush=True)
    if dist is not None:
        dist.destroy_process_group()
    return 0


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    args = parse_args(argv)
    if args.dump_outputs and args.steps < 1:
        raise SystemExit("--dump-outputs needs --steps >= 1: it writes what the last timed step computed")
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        return launch_ranks(args, argv)                 # first thing, before torch.cuda.* or any h263mi call

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit("WORLD_SIZE %d != --gpus %d" % (world, args.gpus))
    if os.environ.get("H263MI_BENCH_STUB"):
        return stub_main(args, rank, world)
    if args.cpu_baseline_only:
        import h263mi
        print(json.dumps(cpu_baseline(h263mi)), flush=True)
        return 0

    import torch  # before h263mi: torch brings its own HIP runtime; the C-ABI library must share it
    import h263mi
    import shard

    # how many ranks of this job share the node (its CPUs, its CPU quota, the cores of each socket): said outright, not left to
    # the launcher's LOCAL_WORLD_SIZE -- before any batch is made (a batch looks up its host placement when it is created)
    h263mi.set_ranks_per_node(shard.local_world_size(world))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the MI355X back-end has no CPU fallback")
    if torch.cuda.device_count() <= local_rank:
        raise SystemExit("rank %d: no device %d (%d visible)" % (rank, local_rank, torch.cuda.device_count()))
    torch.cuda.set_device(local_rank)
    dist = None
    if world > 1 or os.environ.get("H263MI_FORCE_DIST"):      # (the env switch exercises the RCCL path on one GPU)
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        # "nccl" is RCCL on ROCm; rank / world size are passed explicitly so that the forced single-rank form needs no
        # launcher environment
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
    # waits that may last seconds (another rank is busy on its HOST) go through a gloo group: a socket wait, where a RCCL
    # barrier spins a host thread per waiting rank
    host_pg = None
    if dist is not None and world > 1:
        try:
            host_pg = dist.new_group(backend="gloo")
        except Exception as e:          # (no gloo in this build: the long waits fall back to the RCCL barrier)
            sys.stderr.write("bench.py: no gloo side group (%s): waiting on RCCL barriers\n" % e)

    stream = torch.cuda.current_stream().cuda_stream
    strong = args.total_streams > 0
    if strong and args.total_streams % world:
        raise SystemExit("--total-streams %d is not a multiple of %d GPUs" % (args.total_streams, world))
    n = args.total_streams // world if strong else args.streams
    # weak scaling: rank r owns the 64 streams r * 64 ...; strong: stream s of the T is pinned to GPU s mod N
    my_streams = shard.streams_of_rank(rank, world, n, total_streams=args.total_streams if strong else None)
    stride = world if strong else 1
    assert len(my_streams) == n and all(my_streams[k] == my_streams[0] + k * stride for k in range(n))
    pipeline = not args.no_pipeline and not args.overlap
    use_events = pipeline and not args.dense_coeffs
    extras = args.full and not args.no_extra        # the legs after the headline (a plain run stops at the line)
    wl = Workload(h263mi, n, args.gop, my_streams[0], local_rank, stream, events=use_events, stream_stride=stride)
    batch = h263mi.Batch(n, W, H, local_rank, stream, overlap_post=args.overlap, pipeline_post=pipeline)
    d_rgba = h263mi.DeviceBuffer(n * RGBA_BYTES, local_rank)
    frames_per_step = args.gop * args.gops_per_step

    batch.timing_reserve(2 * frames_per_step * max(args.steps, 1))   # no event is created inside the timed region
    run_frames(batch, wl, d_rgba, frames_per_step * args.warmup, pipeline)
    batch.sync()
    batch.timing_begin()

    def timed_steps():
        run_frames(batch, wl, d_rgba, frames_per_step * args.steps, pipeline)
        batch.sync()                                  # (pipeline mode: the last picture's post-processing is part of the work)

    # barrier + synchronize | exactly K steps | synchronize + barrier; MAX over ranks
    elapsed = shard.timed_region(dist, timed_steps, torch.cuda.synchronize)
    kt = batch.timing_end()
    batch.sync()

    pictures = shard.aggregate_pictures(dist, n * frames_per_step * args.steps)
    value = pictures * MP_PER_PICTURE / elapsed

    # ---- parity gate (--full, outside the timed region): every rank checks its own streams; any failure fails the job
    gate, gate_streams, gate_bad = ("not run (--full runs it)", [], 0)
    if args.full:
        gate = "skipped"
        if not args.no_parity_gate:
            gate, gate_streams = parity_gate(h263mi, batch, d_rgba, my_streams[0], n, args.gop, stream_stride=stride)
        gate_bad = 0 if gate in ("ok", "skipped") else 1
        if dist is not None:
            t = torch.tensor([gate_bad], dtype=torch.int32, device="cuda")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            gate_bad = int(t.item())
        if gate_bad and gate == "ok":
            gate = "failed on another rank"

    # ---- what the last timed step computed, before any later leg reuses the batch
    dumped = None
    if args.dump_outputs:
        dumped = dump_outputs(h263mi, batch, d_rgba, n, args.dump_outputs, prefix="rank%d_" % rank if world > 1 else "")

    # ---- roofline of the dominant kernel (HIP events on the launch stream, timed region only)
    g = len(wl.frames)
    recon_alg = sum(wl.recon_bytes(i % g) for i in range(frames_per_step)) / frames_per_step
    recon_alg_8d = sum(wl.recon_bytes(i % g, survey_8d=True) for i in range(frames_per_step)) / frames_per_step
    recon_alg_p = wl.recon_bytes(1) if g > 1 else recon_alg
    post_alg = wl.post_bytes()
    recon_avg_ms = kt.recon_ms / max(kt.recon_launches, 1)
    post_avg_ms = kt.post_ms / max(kt.post_launches, 1)
    frame_avg_ms = kt.frame_ms / max(kt.frame_launches, 1)
    kernels = {
        "k_recon": {"avg_ms": recon_avg_ms, "launches": kt.recon_launches, "alg_bytes_per_launch": recon_alg},
        "k_post": {"avg_ms": post_avg_ms, "launches": kt.post_launches, "alg_bytes_per_launch": post_alg},
        # k_frame = k_recon of picture f and k_post of picture f - 1 in one launch: the algorithmic bytes of both
        "k_frame": {"avg_ms": frame_avg_ms, "launches": kt.frame_launches, "alg_bytes_per_launch": recon_alg + post_alg},
    }
    for k in kernels.values():
        k["achieved_gbs"] = k["alg_bytes_per_launch"] / (k["avg_ms"] * 1e-3) / 1e9 if k["avg_ms"] > 0 else 0.0
    spent = {"k_recon": kt.recon_ms, "k_post": kt.post_ms, "k_frame": kt.frame_ms}
    dom = max(spent, key=spent.get)

    # HBM traffic of that kernel: FETCH_SIZE + WRITE_SIZE from the separate rocprofv3 --pmc passes of
    # tools/prof_final.sh, committed under profiles/.  It cannot be measured from inside this process, so it is
    # reported only when the committed figure was taken on exactly this kernel source.
    traffic, traffic_source, valu_pmc = None, None, None
    try:
        tr = json.load(open(os.path.join(ROOT, "profiles", "traffic_latest.json")))
        if n == 64 and tr.get("kernel_source_hash") == kernel_source_hash():
            traffic = tr["kernels"][dom]["hbm_bytes_per_launch"]
            valu_pmc = (tr.get("valu") or {}).get(dom)
            traffic_source = "profiles/traffic_latest.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this " \
                             "workload, %s, kernel sources %s)" % (tr.get("tag", "?"), tr["kernel_source_hash"])
        else:
            traffic_source = "none for this kernel source (profiles/traffic_latest.json is from other kernel code)"
    except Exception:
        traffic_source = "profiles/traffic_latest.json missing"
    ach = kernels[dom]["achieved_gbs"]
    roofline = {"bound": "hbm", "kernel": dom, "achieved": round(ach, 1),
                "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 4),
                "traffic": traffic, "traffic_source": traffic_source,
                # the box's own ceilings take runs of their own: --full only (filled in below)
                "peak_measured": None, "frac_measured": None, "peak_measured_what": None,
                "peak_measured_mix": None, "frac_measured_mix": None, "peak_measured_mix_what": None,
                "avg_launch_ms": round(kernels[dom]["avg_ms"], 4),
                "alg_bytes_per_launch": int(kernels[dom]["alg_bytes_per_launch"]),
                "alg_bytes_what": "bytes the coefficient transport that ran really moves (events: 4 B per coded block of index + 4 B "
                                  "per non-zero LEVEL; dense: 128 B per coded block) + headers + reference read + planes and RGBA "
                                  "written; `achieved`, `frac`, `frac_measured*` and `pipeline_*` are on these bytes",
                # SURVEY 8(d) prices a coded block at 128 bytes whatever the transport: the figure of rounds 1-3, kept
                # beside the honest one (with events it counts bytes that are never read)
                "survey_8d": {"alg_bytes_per_launch": int(kernels[dom]["alg_bytes_per_launch"] + (recon_alg_8d - recon_alg if dom != "k_post" else 0)),
                              "achieved": round((kernels[dom]["alg_bytes_per_launch"] + (recon_alg_8d - recon_alg if dom != "k_post" else 0))
                                                / (kernels[dom]["avg_ms"] * 1e-3) / 1e9, 1) if kernels[dom]["avg_ms"] > 0 else 0.0,
                              "frac": round((kernels[dom]["alg_bytes_per_launch"] + (recon_alg_8d - recon_alg if dom != "k_post" else 0))
                                            / (kernels[dom]["avg_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if kernels[dom]["avg_ms"] > 0 else 0.0},
                "traffic_over_algorithmic": round(traffic / kernels[dom]["alg_bytes_per_launch"], 3) if traffic else None,
                "pipeline_achieved": round((recon_alg + post_alg) * frames_per_step * args.steps / elapsed / 1e9, 1),
                "pipeline_frac": round((recon_alg + post_alg) * frames_per_step * args.steps / elapsed / 1e9 / HBM_PEAK_GBS, 4),
                "kernels": {k: {"avg_ms": round(v["avg_ms"], 4), "launches": v["launches"],
                                "alg_bytes_per_launch": int(v["alg_bytes_per_launch"]),
                                "achieved_gbs": round(v["achieved_gbs"], 1)} for k, v in kernels.items()},
                "k_recon_p_alg_bytes_per_launch": int(recon_alg_p)}
    peak_copy = None
    if args.full:
        # on-box ceilings, measured in this run: plain copy / read / write kernels over 1 GiB
        peak_copy, copy_shape = h263mi.probe_bandwidth(h263mi.PROBE_COPY, 1 << 30, 10, local_rank, stream, True)
        peak_read, read_shape = h263mi.probe_bandwidth(h263mi.PROBE_READ, 1 << 30, 10, local_rank, stream, True)
        peak_write, write_shape = h263mi.probe_bandwidth(h263mi.PROBE_WRITE, 1 << 30, 10, local_rank, stream, True)
        # A ceiling that knows the kernel's mix of reads and writes: on this part a stream of reads and a stream of writes
        # take as long together as one after the other (copy of 1 GiB = read of 1 GiB + write of 1 GiB, in time, within
        # 3 %), and writes are the slower of the two.  The time the ALGORITHMIC bytes of the dominant kernel need at the
        # read-only and write-only rates measured in this run, and the rate that corresponds to.
        alg_w = {"k_recon": wl.recon_write_bytes(), "k_post": post_alg, "k_frame": wl.recon_write_bytes() + post_alg}[dom]
        alg_r = kernels[dom]["alg_bytes_per_launch"] - alg_w
        mix_ms = (alg_r / (peak_read * 1e9) + alg_w / (peak_write * 1e9)) * 1e3 if peak_read and peak_write else 0.0
        peak_mix = kernels[dom]["alg_bytes_per_launch"] / (mix_ms * 1e-3) / 1e9 if mix_ms else 0.0
        roofline.update({
            "peak_measured": round(peak_copy, 1), "frac_measured": round(ach / peak_copy, 4) if peak_copy else None,
            "peak_measured_what": "copy kernel (read + write counted) over 1 GiB on this device, in this run: the fastest of "
                                  "the tuned launch shapes (%s) -- the MI355X guide's 6.29 TB/s float4 copy is what this "
                                  "probe is held against; read-only %.0f GB/s (%s), write-only %.0f GB/s (%s)"
                                  % (copy_shape, peak_read, read_shape, peak_write, write_shape),
            "peak_measured_mix": round(peak_mix, 1), "frac_measured_mix": round(ach / peak_mix, 4) if peak_mix else None,
            "peak_measured_mix_what": "algorithmic bytes / (bytes read / measured read-only rate + bytes written / "
                                      "measured write-only rate): %.0f MB read, %.0f MB written per launch, %.3f ms"
                                      % (alg_r / 1e6, alg_w / 1e6, mix_ms)})
    # What bounds the launch in fact: the vector ALUs' issue slots, not HBM.  From the committed PMC passes of
    # tools/prof_final.sh over exactly these kernel sources (hash-tied like `traffic`): vector instructions per launch, the
    # lane operations that is per output pixel, the share of the launch's cycles the vector ALUs were busy -- and the time
    # that share is of THIS run's launches.  `bound` stays "hbm" (the byte roofline this line is quoted on); `bound_observed`
    # says which unit is nearest its limit.
    pixels_per_launch = n * W * H
    if valu_pmc:
        busy = valu_pmc["busy_frac"]
        roofline["valu"] = {"insts_per_launch": int(valu_pmc["insts_per_launch"]),
                            "lane_ops_per_pixel": round(valu_pmc["insts_per_launch"] * 64.0 / pixels_per_launch, 2),
                            "busy_frac": round(busy, 4),
                            "alu_time_ms": round(busy * kernels[dom]["avg_ms"], 4),
                            "hbm_busy_frac": round(ach / peak_copy, 4) if peak_copy else None,
                            "source": "profiles/traffic_latest.json `valu` (rocprofv3 --pmc SQ_INSTS_VALU / VALUBusy passes of "
                                      "tools/prof_final.sh, %s, kernel sources %s): mean over the launches of the profiled GOPs; "
                                      "alu_time_ms = busy_frac x this run's avg_launch_ms; hbm_busy_frac = achieved / this box's copy "
                                      "ceiling" % (tr.get("tag", "?"), tr["kernel_source_hash"])}
        # (without --full there is no copy ceiling to hold `achieved` against)
        roofline["bound_observed"] = ("valu" if busy > ach / peak_copy else "hbm") if peak_copy else None
    else:
        roofline["valu"] = None
        roofline["bound_observed"] = None

    def ms_per_frame_index(bt, workload, n_frames, checked):
        run_frames(bt, workload, d_rgba, args.gop, pipeline, checked)
        bt.sync()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        run_frames(bt, workload, d_rgba, n_frames, pipeline, checked)
        bt.sync()
        torch.cuda.synchronize()
        return (time.perf_counter() - t1) / n_frames * 1e3

    if extras and pipeline:
        # The timed region runs CHECKED (ABI 7: the default): every call says how large its arrays are and the waves
        # bounds-check every coded block and event list they read -- the path real streams take.  What the opt-out would buy
        # (H263MI_CFG_TRUSTED_ARRAYS: the caller vouches, the waves check nothing): the same frames on a second batch made that
        # way, interleaved with the checked batch, right here:
        trusted_batch = h263mi.Batch(n, W, H, local_rank, stream, pipeline_post=True, trusted_arrays=True)
        pairs = [(ms_per_frame_index(trusted_batch, wl, 2 * frames_per_step, False), ms_per_frame_index(batch, wl, 2 * frames_per_step, True))
                 for _ in range(2)]
        trusted_batch.close()
        vouched = sum(p_[0] for p_ in pairs) / len(pairs)
        checked_ms = sum(p_[1] for p_ in pairs) / len(pairs)
        roofline["trusted_mode"] = {"ms_per_frame_index": round(vouched, 4), "checked_ms_per_frame_index": round(checked_ms, 4),
                                    "gain": round(checked_ms / vouched - 1.0, 4),
                                    "mp_per_s": round(n * MP_PER_PICTURE / (vouched * 1e-3), 1),
                                    "what": "the timed workload on a H263MI_CFG_TRUSTED_ARRAYS batch with no sizes given (the caller "
                                            "vouches, the waves check nothing) against the headline's checked calls; 2 x %d frame "
                                            "indices each, interleaved twice, wall clock; gain = checked / trusted - 1"
                                            % (2 * frames_per_step)}
    else:
        roofline["trusted_mode"] = None

    extra = {}
    # (the extra legs run on EVERY rank -- each on its own GPU and its own share of the host -- so that no rank sits in a
    # collective while another measures; rank 0 reports its own figures, the end-to-end leg the sum over the ranks)
    if extras and use_events:
        # the same workload with the coefficients as dense 128-byte blocks in HBM (round 1-2's transport)
        wld = Workload(h263mi, n, args.gop, my_streams[0], local_rank, stream, events=False, stream_stride=stride)
        run_frames(batch, wld, d_rgba, args.gop, pipeline)
        batch.sync()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        run_frames(batch, wld, d_rgba, 2 * frames_per_step, pipeline)
        batch.sync()
        torch.cuda.synchronize()
        dtd = time.perf_counter() - t1
        extra["dense_coefficient_transport"] = {
            "ms_per_frame_index": round(dtd / (2 * frames_per_step) * 1e3, 4),
            "mp_per_s": round(n * 2 * frames_per_step * MP_PER_PICTURE / dtd, 1),
            "what": "the same pictures with h263mi_batch_decode: coefficients as dense int16[64] blocks in HBM (%.0f MB per "
                    "P frame index) instead of events (%.1f MB)" % (wld.frames[1]["blocks"] * 128 / 1e6,
                                                                    wl.frames[1]["n_events"] * 4 / 1e6)}
        for fr in wld.frames:
            for k in ("mbs", "co", "base"):
                fr[k].free()
        del wld
    if extras:
        # BASELINE configs[1]: dense 1080p I pictures (every block Full): dequant + IDCT + YUV->RGBA, no deblock
        del wl
        dense = Workload(h263mi, n, 1, 0, local_rank, stream, i_kind=h263mi.SYNTH_I_DENSE, p_frames=False)
        fr = dense.frames[0]

        def dense_pictures(reps, fused):
            for it in range(reps):
                if fused:                              # one launch: I picture f + post-processing of I picture f - 1
                    batch.decode(fr["ptype"], fr["mbs"].ptr, fr["co"].ptr, fr["base"].ptr, 0, 0, d_rgba.ptr, None)
                else:
                    batch.submit(fr["ptype"], fr["mbs"].ptr, fr["co"].ptr, fr["base"].ptr)
                    batch.render_rgba(0, d_rgba.ptr, None)
            batch.sync()

        reps = 200
        alg = dense.recon_bytes(0) + dense.post_bytes()
        res = {"alg_bytes_per_picture": int(alg / n)}
        for fused in ([False, True] if pipeline else [False]):
            dense_pictures(3, fused)
            batch.timing_reserve(2 * reps)
            batch.timing_begin()
            t1 = time.perf_counter()
            dense_pictures(reps, fused)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t1
            kd = batch.timing_end()
            if fused:
                res.update({"mp_per_s": round(n * reps * MP_PER_PICTURE / dt, 1),
                            "k_frame_avg_ms": round(kd.frame_ms / max(kd.frame_launches, 1), 4),
                            "pipeline_gbs": round(alg * reps / dt / 1e9, 1),
                            "pipeline_frac": round(alg * reps / dt / 1e9 / HBM_PEAK_GBS, 4)})
            else:
                res.update({"two_launches_mp_per_s": round(n * reps * MP_PER_PICTURE / dt, 1),
                            "k_recon_avg_ms": round(kd.recon_ms / max(kd.recon_launches, 1), 4),
                            "k_post_avg_ms": round(kd.post_ms / max(kd.post_launches, 1), 4)})
                if not pipeline:
                    res.update({"mp_per_s": res["two_launches_mp_per_s"], "pipeline_gbs": round(alg * reps / dt / 1e9, 1),
                                "pipeline_frac": round(alg * reps / dt / 1e9 / HBM_PEAK_GBS, 4)})
        extra["config2_dense_iframe"] = res
        # BASELINE's second single-GPU configuration where the driver keeps it: inside `roofline`
        if "k_frame_avg_ms" in res:
            roofline["config2_dense_i"] = {
                "ms_per_64": res["k_frame_avg_ms"] * 64.0 / n, "pictures_per_launch": n,
                "alg_bytes_per_launch": int(alg),
                "achieved": round(alg / (res["k_frame_avg_ms"] * 1e-3) / 1e9, 1),
                "frac": round(alg / (res["k_frame_avg_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                "mp_per_s": res["mp_per_s"],
                "what": "BASELINE configs[1]: %d dense 1920x1080 I pictures (every block Full) per launch, dequant + IDCT + "
                        "BT.601 RGBA (no deblock), k_frame: HIP-event mean over %d launches; algorithmic bytes = records + "
                        "128 B per coded block + planes + RGBA written" % (n, reps)}
    roofline.setdefault("config2_dense_i", None)

    if extras and rank == 0 and world == 1 and pipeline:
        # (needs the workload `wl`, which the dense-I leg above has freed: made again here, 2 GB)
        wl2 = Workload(h263mi, n, args.gop, my_streams[0], local_rank, stream, events=use_events, stream_stride=stride)
        try:
            pr = torch.cuda.get_device_properties(local_rank)
            bdf = "%04x:%02x:%02x.0" % (getattr(pr, "pci_domain_id", 0), pr.pci_bus_id, pr.pci_device_id)
        except Exception:
            bdf = None
        extra["sustained"] = sustained_run(torch, batch, wl2, d_rgba, frames_per_step, pipeline, n, bdf, seconds=args.sustained_seconds)
        for fr in wl2.frames:
            for k in ("mbs", "co", "base", "first", "ev"):
                if fr.get(k) is not None:
                    fr[k].free()
        del wl2

    e2e_bad = 0
    if extras and not args.no_e2e:
        # every rank runs its own 64 streams end to end, on ITS share of the container's CPUs, all at the same time
        # ... as many parser threads as the LIBRARY chooses for that share (h263mi_default_parser_threads: under a CPU-time
        # quota more threads than the quota has CPUs, parked the moment they run out of work -- include/h263mi.h)
        threads, quota_per_rank = h263mi.default_parser_threads(n)
        if dist is not None:
            dist.barrier()
        for key, corpus, kinds in (("e2e_bitstream", "dense", 4), ("e2e_bitstream_realistic", "kinds", 8),
                                   ("e2e_bitstream_distinct", "distinct", n)):
            # (a parser thread that meets the same picture again and again has its branches predicted from history -- one
            # thread parses 10.8 k pictures/s of ONE realistic stream repeated, 7.2-7.4 k of 8 or 16 different ones,
            # tools/probes/e2e_distinct_streams.py: the "distinct" corpus repeats nothing inside a GOP pass)
            e = e2e_bitstream(h263mi, n, local_rank, stream, d_rgba, corpus=corpus, n_distinct=kinds, parser_threads=threads)
            mine = {"rank": rank, "device": local_rank, "pictures_per_s": e["pictures_per_s"], "parser_threads": threads,
                    "host_placement": e["host_placement"]}
            rate, units, seconds = shard.aggregate_rate(dist, e.pop("_pictures"), e.pop("_seconds"))
            e["cpu_quota_per_rank"] = quota_per_rank or None
            if world > 1:
                per_rank = [None] * world
                dist.all_gather_object(per_rank, mine, group=host_pg)       # (host_pg None: the default group)
                e["all_ranks"] = {"pictures_per_s": round(rate, 1), "realtime_1080p30_streams": round(rate / 30.0, 1),
                                  "pictures": units, "seconds_slowest_rank": round(seconds, 4), "ranks": world,
                                  "parser_threads_per_rank": threads, "per_rank": per_rank,
                                  "what": "every rank its own %d streams on its own GPU and %d parser threads, all ranks at the "
                                          "same time: pictures of all ranks / the slowest rank's time; per_rank: each rank's own "
                                          "rate, the NUMA node of its GPU, the node its pinned staging memory lies on and the CPUs "
                                          "its parser threads are confined to; the other fields of this object are rank 0's own"
                                          % (n, threads)}
            e2e_bad |= e["parity_vs_oracle"] != "ok"
            extra[key] = e
        if rank == 0:
            extra["plain_functions_1080p"] = plain_function_latency(h263mi)
            extra["single_stream_1080p"] = single_stream_latency(h263mi, local_rank, stream)
            e2e_bad |= extra["single_stream_1080p"]["parity_vs_oracle"] != "ok"
        if host_pg is not None:
            dist.barrier(group=host_pg)          # (rank 0's single-stream leg: the others wait on a socket)
        elif dist is not None:
            dist.barrier()
    if dist is not None:
        t = torch.tensor([int(e2e_bad)], dtype=torch.int32, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        e2e_bad = int(t.item())

    out = {
        "metric": "decoded megapixels/sec (IDCT+MC+YUV->RGB)",
        "value": round(value, 1), "unit": "MP/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(elapsed / max(args.steps, 1) * 1e3, 4), "higher_is_better": True,
        "scaling": "strong" if strong else "weak",
        "vs_baseline": None, "dtype": "u8/i16/i32 integer + f32 (IDCT, un-fused)", "data": "synthetic",
        "config": {"workload": "BASELINE configs[3]: batch of %d independent 1920x1080 streams per GPU; step = one pass "
                               "over the resident input = %d GOPs x %d frame indices = %d pictures per stream (%d per "
                               "step and GPU); GOP = 1 I (mixed block classes) + %d P (half-pel MVs in [-32,31], 25%% "
                               "coded blocks, quant 10); dequant+IDCT+MC+add/clip, deblock strength %d, BT.601 RGBA; "
                               "records pre-generated in HBM (checked calls: pool size and event count given, the waves "
                               "bounds-check what they read; roofline.trusted_mode has the opt-out), coefficients %s" % (
                                   n, args.gops_per_step, args.gop, frames_per_step, n * frames_per_step, args.gop - 1, STRENGTH,
                                   "as sparse events (one 32-bit word per non-zero LEVEL: the host parser's transport form, "
                                   "h263mi_batch_decode_events) for the P pictures, dense blocks for the GOP's I picture" if use_events else "as dense int16[64] blocks (h263mi_batch_decode)"),
                   "coefficient_transport": "events" if use_events else "dense",
                   "streams_per_gpu": n, "width": W, "height": H, "gop": args.gop, "gops_per_step": args.gops_per_step,
                   "pictures_per_step": n * frames_per_step * world,
                   "parallelism": "streams sharded per GPU, no data-path collective"},
        "timed_region_s": round(elapsed, 4),
        "ms_per_frame_index": round(elapsed / max(args.steps * frames_per_step, 1) * 1e3, 4),
        "realtime_1080p30_streams": round(value / (MP_PER_PICTURE * 30), 1),
        "parity_gate": gate, "parity_gate_streams": gate_streams,
        "e2e_parity": None if (not extras or args.no_e2e) else ("MISMATCH" if e2e_bad else "ok"),
        "roofline": roofline,
    }
    if extra:
        out["extra"] = extra
    if dumped is not None:
        out["dumped_outputs"] = dumped
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(h263mi)
    elif rank == 0:
        # a plain run times the GPU only.  N > 1: the CPU baseline is a property of the box, not of the job; it is timed
        # at N = 1 only (there the host is idle beside it -- with N ranks their threads would compete with its `cores`
        # threads)
        out["cpu_baseline"] = None
    if rank == 0:
        print(json.dumps(out), flush=True)
    batch.close()
    if dist is not None:
        if host_pg is not None:
            dist.barrier(group=host_pg)
        else:
            dist.barrier()
        dist.destroy_process_group()
    # a mismatch anywhere -- the main gate or an end-to-end leg, on any rank -- fails the run
    return 1 if (gate_bad or e2e_bad) else 0


if __name__ == "__main__":
    sys.exit(main())
