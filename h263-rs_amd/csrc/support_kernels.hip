// support_kernels.hip -- kernels that serve bench.py and the tests, not decoding: the synthetic record generators and the
// memory-ceiling probes.  Built with the flags of decode_kernels.hip.
#include "kernels.h"

#include "synth.inl"

namespace h263mi {

// ---------------------------------------------------------------------------------------
// synthetic record generators (bench / test support)
// ---------------------------------------------------------------------------------------
__global__ void k_synth_headers(SynthArgs a)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.n_streams * a.mbs_per_picture) return;
    const uint32_t p = g / a.mbs_per_picture, mb = g % a.mbs_per_picture;
    MbRecord r = synth_mb_header(a.kind, a.first_stream_id + p * a.stream_stride, a.frame_idx, mb);
    a.mbs[g] = r;
    a.counts[g] = (uint32_t)__popc(r.cbp);
}

// exclusive scan of the per-macroblock coded-block counts of one picture -> coeff_index
__global__ __launch_bounds__(1024) void k_synth_scan(SynthArgs a)
{
    __shared__ uint32_t sums[1024];
    const uint32_t p = blockIdx.x, tid = threadIdx.x;
    const uint32_t n = a.mbs_per_picture, chunk = (n + 1023) / 1024;
    const uint32_t lo = tid * chunk, hi = lo + chunk < n ? lo + chunk : n;
    uint32_t local = 0;
    for (uint32_t i = lo; i < hi; i++) local += a.counts[p * n + i];
    sums[tid] = local;
    __syncthreads();
    for (uint32_t off = 1; off < 1024; off <<= 1) {
        uint32_t v = tid >= off ? sums[tid - off] : 0;
        __syncthreads();
        sums[tid] += v;
        __syncthreads();
    }
    uint32_t run = sums[tid] - local;     // exclusive prefix of this thread's chunk
    for (uint32_t i = lo; i < hi; i++) {
        a.mbs[p * n + i].coeff_index = run;
        run += a.counts[p * n + i];
    }
    if (tid == 1023) a.totals[p] = sums[1023];
}

__global__ void k_synth_coeffs(SynthArgs a)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.n_streams * a.mbs_per_picture * 6) return;
    const uint32_t blk = g % 6, gm = g / 6, p = gm / a.mbs_per_picture, mb = gm % a.mbs_per_picture;
    const MbRecord r = a.mbs[gm];
    if (!((r.cbp >> blk) & 1)) return;
    int16_t c[64];
    synth_block_coeffs(a.kind, a.first_stream_id + p * a.stream_stride, a.frame_idx, mb, (int)blk, c);
    const uint64_t idx = a.coeff_base[p] + r.coeff_index + (uint64_t)__popc(r.cbp & ((1u << blk) - 1u));
    uint4 *dst = reinterpret_cast<uint4 *>(a.coeffs + idx * 64);
#pragma unroll
    for (int q = 0; q < 8; q++) {
        uint32_t w[4];
        for (int k = 0; k < 4; k++) w[k] = (uint16_t)c[q * 8 + 2 * k] | ((uint32_t)(uint16_t)c[q * 8 + 2 * k + 1] << 16);
        dst[q] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

hipError_t launch_synth_headers(const SynthArgs &a, hipStream_t stream)
{
    const uint32_t n = a.n_streams * a.mbs_per_picture;
    hipLaunchKernelGGL(k_synth_headers, dim3((n + 255) / 256), dim3(256), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_synth_scan, dim3(a.n_streams), dim3(1024), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_synth_coeffs(const SynthArgs &a, hipStream_t stream)
{
    const uint32_t n = a.n_streams * a.mbs_per_picture * 6;
    hipLaunchKernelGGL(k_synth_coeffs, dim3((n + 255) / 256), dim3(256), 0, stream, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// on-box memory ceilings (bench support: roofline.peak_measured).  Streaming kernels with 16-byte accesses: the rate the
// HBM system of THIS box sustains for a copy, a pure read and a pure write.  Round 2's plain grid-stride probes
// (2 048 workgroups, one access per iteration) reported 4.8 TB/s for a copy where the MI355X guide measures 6.29:
// tools/probes/ceiling.hip swept the launch shape (profiles/r03_a_ceiling_probe.txt) -- what reaches 6.2 TB/s is
// non-temporal accesses, four of them in flight per lane (copy); a read wants non-temporal loads, a write is fastest
// with few (256) workgroups of plain stores.  `shape` selects among the winners; the C entry point reports the best.
// ---------------------------------------------------------------------------------------
typedef uint32_t probe_u32x4 __attribute__((ext_vector_type(4)));
template <int MODE, int U, bool NT>
__global__ __launch_bounds__(1024) void k_probe(const probe_u32x4 *__restrict__ in, probe_u32x4 *__restrict__ out, size_t n)
{
    // a workgroup walks the buffer in steps of gridDim * blockDim * U elements; its U accesses of a step are blockDim apart
    const size_t step = (size_t)gridDim.x * blockDim.x * U;
    probe_u32x4 acc = {0, 0, 0, 0};
    for (size_t base = (size_t)blockIdx.x * blockDim.x * U + threadIdx.x; base < n; base += step) {
        probe_u32x4 v[U];
        if (MODE != 2) {
#pragma unroll
            for (int u = 0; u < U; u++) {
                const size_t i = base + (size_t)u * blockDim.x;
                v[u] = i < n ? (NT ? __builtin_nontemporal_load(in + i) : in[i]) : acc;
            }
        }
        if (MODE == 1) {
#pragma unroll
            for (int u = 0; u < U; u++) acc ^= v[u];
        } else {
#pragma unroll
            for (int u = 0; u < U; u++) {
                const size_t i = base + (size_t)u * blockDim.x;
                if (MODE == 2) v[u] = probe_u32x4{(uint32_t)i, 1, 2, 3};
                if (i < n) {
                    if (NT) __builtin_nontemporal_store(v[u], out + i);
                    else out[i] = v[u];
                }
            }
        }
    }
    if (MODE == 1 && (acc.x ^ acc.y ^ acc.z ^ acc.w) == 0x12345678u) out[0] = acc;      // never true for the probe's fill pattern
}

int probe_shapes(int mode) { return mode == 0 ? 2 : mode == 1 ? 2 : 3; }
const char *probe_shape_name(int mode, int shape)
{
    static const char *names[3][3] = {
        {"non-temporal, 4 accesses in flight, 4096 x 256 threads", "non-temporal, 4 accesses in flight, 256 x 512 threads", ""},
        {"non-temporal loads, 4 in flight, 256 x 512 threads", "non-temporal loads, 512 x 1024 threads", ""},
        {"plain stores, 256 x 256 threads", "plain stores, 8 per iteration, 256 x 1024 threads", "non-temporal stores, 256 x 256 threads"}};
    return names[mode][shape];
}

hipError_t launch_probe(int mode, int shape, const void *in, void *out, size_t bytes, hipStream_t stream)
{
    const size_t n = bytes / 16;
    const probe_u32x4 *pi = (const probe_u32x4 *)in;
    probe_u32x4 *po = (probe_u32x4 *)out;
    if (mode == 0 && shape == 0) hipLaunchKernelGGL((k_probe<0, 4, true>), dim3(4096), dim3(256), 0, stream, pi, po, n);
    else if (mode == 0) hipLaunchKernelGGL((k_probe<0, 4, true>), dim3(256), dim3(512), 0, stream, pi, po, n);
    else if (mode == 1 && shape == 0) hipLaunchKernelGGL((k_probe<1, 4, true>), dim3(256), dim3(512), 0, stream, pi, po, n);
    else if (mode == 1) hipLaunchKernelGGL((k_probe<1, 1, true>), dim3(512), dim3(1024), 0, stream, pi, po, n);
    else if (shape == 0) hipLaunchKernelGGL((k_probe<2, 1, false>), dim3(256), dim3(256), 0, stream, pi, po, n);
    else if (shape == 1) hipLaunchKernelGGL((k_probe<2, 8, false>), dim3(256), dim3(1024), 0, stream, pi, po, n);
    else hipLaunchKernelGGL((k_probe<2, 1, true>), dim3(256), dim3(256), 0, stream, pi, po, n);
    return hipGetLastError();
}

}  // namespace h263mi
