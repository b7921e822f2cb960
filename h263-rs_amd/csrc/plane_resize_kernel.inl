// plane_resize_kernel.inl -- k_plane_resize: full-size deblocked planes -> W' x H' I420 or NV12 by area averaging
// (h263mi_yuv_resize, ABI 7).
//
// The contract (include/h263mi.h): every plane is resized on its own by the formula of h263mi_rgba_resize applied to one 8-bit
// channel -- for a plane P of pw x ph and an output of pw' x ph'
//     out[Y][X] = (sum_j sum_i oy(Y, j) * ox(X, i) * P[j][i] + floor(pw*ph / 2)) div (pw*ph)
// with luma (w, h, W', H') and Cb, Cr (cw, ch, cW', cH'), c* = ceil(* / 2).  ResizeSpan, resize_weight and resize_div are the
// ones of resize_kernel.inl; the host makes one pair of span tables for luma and one for chroma.
//
// The source is the tightly packed I420 that the rendering kernels write by default (picture p at + p * (w*h + 2*cw*ch)); the
// destinations are three DEVICE pointers per picture (Y; Cb or the CbCr plane; Cr), a null Y pointer skips the picture.
//
// One wave per workgroup, no barrier.  A wave = PLANE_OUT output columns (PLANE_PX adjacent ones per lane, stored as one word)
// x PLANE_ROWS output rows of one plane JOB of one picture.  A job is the luma plane (one channel) or the chroma pair (two
// channels: Cb and Cr have one geometry, are resized at the same output positions and, for NV12, leave interleaved in one
// store).  blockIdx.y = picture, blockIdx.z = column segment -- the luma segments first, the chroma segments behind them --,
// blockIdx.x = band in XCD order (output_kernels.hip: k_plane_resize): ONE launch serves all planes of all pictures.
// Per output row the wave walks the source columns that its output columns cover in chunks of PLANE_CHUNK: each lane sums
// PLANE_SRC adjacent source samples down the row's source rows (one 16-byte load per row where the plane's start and width are
// multiples of 16, bytes otherwise), the wave hands the column sums through LDS, and each lane weighs the ones its output
// columns cover.  The vertical sums are at most 255 * ph < 2^24; the accumulators are 64-bit (255 * pw * ph).
//
// Written in the H263_HD style of the other kernels: tests/sim_yuv_resize/ runs plane_resize_item lane by lane under g++
// (ASan / UBSan), with the same PlaneResizeArgs and the same arithmetic.
#pragma once

#include "resize_kernel.inl"

namespace h263mi {

constexpr uint32_t PLANE_ROWS = 4;                       // output rows per wave
constexpr uint32_t PLANE_PX = 4;                         // adjacent output samples per lane: one word of a plane
constexpr uint32_t PLANE_OUT = 64 * PLANE_PX;            // output columns per wave
constexpr uint32_t PLANE_SRC = 16;                       // adjacent source samples per lane: one 16-byte load
constexpr uint32_t PLANE_CHUNK = 64 * PLANE_SRC;         // source columns per LDS hand-off

// where picture p's planes go: Y, Cb (NV12: the CbCr plane), Cr (NV12: unused).  p[0] == nullptr: the picture is skipped
struct PlaneDst {
    uint8_t *p[3];
};

struct PlaneResizeArgs {
    const uint8_t *src;          // tight I420, picture p at + p * (d_y + 2 * d_c)
    const PlaneDst *dst;         // DEVICE array, one entry per picture
    const ResizeSpan *cols_y;    // W' entries
    const ResizeSpan *rows_y;    // H'
    const ResizeSpan *cols_c;    // cW'
    const ResizeSpan *rows_c;    // cH'
    uint32_t w, h, cw, ch;       // source planes
    uint32_t ow, oh, cow, coh;   // output planes
    uint32_t pitch_y, pitch_c;   // destination row pitches (plane spans < 2^32: h263mi_yuv_resize_extent)
    uint32_t nv12;               // 1: Cb, Cr interleaved at p[1]
    uint32_t wide;               // 1: both pitches and every destination pointer are multiples of 4: word stores
    uint32_t d_y, d_c;           // w*h, cw*ch (< 2^30: layout_fits)
    float inv_d_y, inv_d_c;      // 1.0f / d, rounded to nearest
    uint32_t bands;              // ceil(H' / PLANE_ROWS): bands of output rows per picture (the chroma planes use the first half)
    uint32_t chunk;              // bands per picture and XCD: ceil(bands / 8)
    uint32_t segs_y;             // ceil(W' / PLANE_OUT): blockIdx.z below it is a luma segment
    uint32_t n_pictures;
};

// the launch of k_plane_resize (HOST): the luma segments, then the chroma segments, in z
inline bool plane_resize_plan(PlaneResizeArgs &a, LaunchDims &d)
{
    if (a.n_pictures > 65535) return false;
    a.segs_y = (a.ow + PLANE_OUT - 1) / PLANE_OUT;
    d = band_grid(a.oh, PLANE_ROWS, a.n_pictures, a.segs_y + (a.cow + PLANE_OUT - 1) / PLANE_OUT, a.bands, a.chunk);
    return true;
}

// what a wave hands between its lanes: the column sums of one chunk, per channel
struct PlaneLds {
    uint32_t v[2][PLANE_CHUNK];
};

// what a lane keeps: the spans of its output columns for all rows of the wave, the sums across the phases of one output row
struct PlaneLane {
    ResizeSpan cs[PLANE_PX];
    uint64_t acc[2][PLANE_PX];
};

// one plane (NCH = 1) or two planes of one geometry resized together (NCH = 2), as a wave sees it
struct PlaneJob {
    const uint8_t *src[2];
    uint8_t *dst[2];             // (interleave: dst[0] alone)
    const ResizeSpan *cols, *rows;
    uint32_t pw, ph, ow, oh, pitch, d;
    float inv_d;
    bool wide_src;               // every source row starts on a 16-byte boundary
    bool wide_dst;
    bool interleave;             // NCH = 2: the two channels leave as byte pairs in one plane
};

H263_HD void plane_unpack_add(uint32_t word, uint32_t wt, uint32_t *v)
{
    v[0] += wt * (word & 0xffu);
    v[1] += wt * ((word >> 8) & 0xffu);
    v[2] += wt * ((word >> 16) & 0xffu);
    v[3] += wt * (word >> 24);
}

// Phase 1: the lane's 16 source columns c0 + 16*lane .. +15 summed down the output row's source rows (weights oy), into LDS
template <int NCH>
H263_HD void plane_phase_vertical(const PlaneJob &j, PlaneLds &s, int lane, const ResizeSpan &rs, uint32_t c0, uint32_t c_end)
{
    const uint32_t x = c0 + PLANE_SRC * (uint32_t)lane;
    // (c0 is a multiple of 16: in a plane whose start and width are too, the lane's 16 samples are one aligned load in the row)
    const bool full = j.wide_src && x + PLANE_SRC <= j.pw;
#pragma unroll
    for (int c = 0; c < NCH; c++) {                           // (unrolled: j.src[c] stays in registers)
        uint32_t v[PLANE_SRC];
        for (uint32_t e = 0; e < PLANE_SRC; e++) v[e] = 0;
        if (x < c_end) {
            for (uint32_t k = 0; k < rs.count; k++) {
                const uint32_t wt = resize_weight(rs, k, j.oh);
                const uint8_t *row = j.src[c] + (size_t)(rs.first + k) * j.pw + x;
                if (full) {
                    const uint4 p = *reinterpret_cast<const uint4 *>(row);
                    plane_unpack_add(p.x, wt, v + 0);
                    plane_unpack_add(p.y, wt, v + 4);
                    plane_unpack_add(p.z, wt, v + 8);
                    plane_unpack_add(p.w, wt, v + 12);
                } else {
                    for (uint32_t e = 0; e < PLANE_SRC; e++)
                        if (x + e < j.pw) v[e] += wt * row[e];
                }
            }
        }
        for (uint32_t e = 0; e < PLANE_SRC; e++) s.v[c][PLANE_SRC * (uint32_t)lane + e] = v[e];
    }
}

// Phase 2: the lane's output columns X .. X + 3 (up to X1) weigh the column sums of the chunk [c0, c0 + PLANE_CHUNK) they cover
template <int NCH>
H263_HD void plane_phase_horizontal(const PlaneJob &j, const PlaneLds &s, PlaneLane &t, uint32_t X, uint32_t X1, uint32_t c0)
{
#pragma unroll
    for (uint32_t e = 0; e < PLANE_PX; e++) {                 // (unrolled: the lane's spans and sums stay in registers)
        if (X + e > X1) continue;
        const ResizeSpan cs = t.cs[e];
        const uint32_t b = cs.first > c0 ? cs.first : c0;
        const uint32_t e0 = cs.first + cs.count, e1 = c0 + PLANE_CHUNK, en = e0 < e1 ? e0 : e1;
        for (uint32_t i = b; i < en; i++) {
            const uint64_t wt = resize_weight(cs, i - cs.first, j.ow);
            for (int c = 0; c < NCH; c++) t.acc[c][e] += wt * s.v[c][i - c0];
        }
    }
}

H263_HD void plane_store4(uint8_t *p, const uint32_t *q, uint32_t n, bool wide)
{
    if (wide && n == PLANE_PX) {
        *reinterpret_cast<uint32_t *>(p) = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
    } else {
        for (uint32_t e = 0; e < PLANE_PX; e++)     // (a constant trip count: q stays in registers)
            if (e < n) p[e] = (uint8_t)q[e];
    }
}

// Phase 3: round, divide and store the lane's samples of row Y
template <int NCH>
H263_HD void plane_phase_store(const PlaneJob &j, const PlaneLane &t, uint32_t X, uint32_t X1, uint32_t Y)
{
    if (X > X1) return;
    const uint32_t n = X1 + 1 - X < PLANE_PX ? X1 + 1 - X : PLANE_PX, half = j.d >> 1;
    uint32_t q[NCH][PLANE_PX];
    for (int c = 0; c < NCH; c++)
        for (uint32_t e = 0; e < PLANE_PX; e++) q[c][e] = e < n ? resize_div(t.acc[c][e] + half, j.d, j.inv_d) : 0u;
    if (NCH == 2 && j.interleave) {
        // Cb, Cr pairs: the lane's 8 bytes as two words
        uint8_t *p = j.dst[0] + (size_t)Y * j.pitch + (size_t)X * 2u;
        const uint32_t pairs[2 * PLANE_PX] = {q[0][0], q[NCH - 1][0], q[0][1], q[NCH - 1][1], q[0][2], q[NCH - 1][2], q[0][3], q[NCH - 1][3]};
        plane_store4(p, pairs, n < 2 ? 2 * n : 4u, j.wide_dst);
        if (n > 2) plane_store4(p + 4, pairs + 4, 2 * (n - 2), j.wide_dst);
    } else {
        for (int c = 0; c < NCH; c++) plane_store4(j.dst[c] + (size_t)Y * j.pitch + X, q[c], n, j.wide_dst);
    }
}

// One wave's work on one job: the PLANE_OUT output columns of segment `seg` in band `band`
template <int NCH, class EachLane>
H263_HD void plane_resize_job(const PlaneJob &j, PlaneLds &s, uint32_t band, uint32_t seg, EachLane each)
{
    const uint32_t X0 = seg * PLANE_OUT, X1 = (X0 + PLANE_OUT < j.ow ? X0 + PLANE_OUT : j.ow) - 1u;
    const uint32_t c0 = j.cols[X0].first & ~(PLANE_SRC - 1u), c_end = j.cols[X1].first + j.cols[X1].count;
    const uint32_t Y0 = band * PLANE_ROWS, Y1 = Y0 + PLANE_ROWS < j.oh ? Y0 + PLANE_ROWS : j.oh;
    each([&](int lane, PlaneLane &t) {                        // (read once for the wave's rows)
#pragma unroll
        for (uint32_t e = 0; e < PLANE_PX; e++) {
            const uint32_t X = X0 + PLANE_PX * (uint32_t)lane + e;
            t.cs[e] = j.cols[X <= X1 ? X : X1];
        }
    });
    for (uint32_t Y = Y0; Y < Y1; Y++) {
        const ResizeSpan rs = j.rows[Y];
        each([&](int lane, PlaneLane &t) {
            for (int c = 0; c < NCH; c++)
                for (uint32_t e = 0; e < PLANE_PX; e++) t.acc[c][e] = 0;
        });
        for (uint32_t c = c0; c < c_end; c += PLANE_CHUNK) {
            each([&](int lane, PlaneLane &) { plane_phase_vertical<NCH>(j, s, lane, rs, c, c_end); });
            wave_fence();
            each([&](int lane, PlaneLane &t) { plane_phase_horizontal<NCH>(j, s, t, X0 + PLANE_PX * (uint32_t)lane, X1, c); });
            wave_fence();                                     // (the next chunk's column sums overwrite these)
        }
        each([&](int lane, PlaneLane &t) { plane_phase_store<NCH>(j, t, X0 + PLANE_PX * (uint32_t)lane, X1, Y); });
    }
}

H263_HD bool plane_aligned16(const uint8_t *p, uint32_t pw) { return (((uintptr_t)p | pw) & 15u) == 0; }

// One wave's work: segment `seg` (luma segments first, then chroma) in band `band` of picture `pic`.  `each(f)` runs
// f(lane, lane_state) for the lanes this thread stands for: the one of its hardware lane on the GPU, all 64 in turn in the CPU
// checker.  Everything outside `each` is wave-uniform.
template <class EachLane>
H263_HD void plane_resize_item(const PlaneResizeArgs &a, PlaneLds &s, uint32_t band, uint32_t seg, uint32_t pic, EachLane each)
{
    uint8_t *const dst_y = a.dst[pic].p[0];
    if (!dst_y) return;                                       // a stream with nothing to render: untouched
    const uint8_t *const pic_src = a.src + (size_t)pic * ((size_t)a.d_y + 2u * (size_t)a.d_c);
    PlaneJob j;
    j.wide_dst = a.wide != 0;
    if (seg < a.segs_y) {
        j.src[0] = j.src[1] = pic_src;
        j.dst[0] = j.dst[1] = dst_y;
        j.cols = a.cols_y;
        j.rows = a.rows_y;
        j.pw = a.w, j.ph = a.h, j.ow = a.ow, j.oh = a.oh, j.pitch = a.pitch_y, j.d = a.d_y, j.inv_d = a.inv_d_y;
        j.wide_src = plane_aligned16(j.src[0], j.pw);
        j.interleave = false;
        plane_resize_job<1>(j, s, band, seg, each);
    } else {
        if (band * PLANE_ROWS >= a.coh) return;               // (the chroma planes have half the bands)
        j.src[0] = pic_src + a.d_y;
        j.src[1] = j.src[0] + a.d_c;
        j.dst[0] = a.dst[pic].p[1];
        j.dst[1] = a.nv12 ? j.dst[0] : a.dst[pic].p[2];
        j.cols = a.cols_c;
        j.rows = a.rows_c;
        j.pw = a.cw, j.ph = a.ch, j.ow = a.cow, j.oh = a.coh, j.pitch = a.pitch_c, j.d = a.d_c, j.inv_d = a.inv_d_c;
        j.wide_src = plane_aligned16(j.src[0], j.pw) && plane_aligned16(j.src[1], j.pw);
        j.interleave = a.nv12 != 0;
        plane_resize_job<2>(j, s, band, seg - a.segs_y, each);
    }
}

}  // namespace h263mi
