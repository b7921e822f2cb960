// plane_filter_kernel.inl -- k_plane_filter: full-size deblocked planes -> W' x H' I420 or NV12 with Pillow's bilinear or bicubic
// filter (h263mi_batch_set_yuv_resize_filtered, ABI 7).
//
// The contract (include/h263mi.h): every plane is resampled on its own by the two passes that h263mi_filter documents, applied to
// one 8-bit channel -- for a plane P of pw x ph and an output of pw' x ph'
//     horizontal   t[j][X]   = clamp((2^21 + sum_i kx[X][i] * P[j][fx(X) + i]) >> 22, 0, 255)      the first rounding
//     vertical     out[Y][X] = clamp((2^21 + sum_j ky[Y][j] * t[fy(Y) + j][X]) >> 22, 0, 255)      the second rounding
// with luma (w, h, W', H') and Cb, Cr (cw, ch, cW', cH'), c* = ceil(* / 2): it is Image.fromarray(P, "L").resize((pw', ph')).
// The host makes one tap table for luma and one for chroma (filter_taps.h: filter_table; filter_kernel.inl: filter_axes); a pass
// whose sizes agree has the identity table, which the same arithmetic hands through bit for bit.  filter_round_h,
// filter_round_v, FilterSpan and FilterAxis are the ones of filter_kernel.inl: the two mutants of mutants.h apply unchanged.
//
// Source, destinations and jobs are those of k_plane_resize (plane_resize_kernel.inl: PlaneDst, the null-Y-pointer skip, the
// luma plane as one channel and the chroma pair as two channels of one geometry, interleaved in one store for NV12;
// plane_store4).  One wave per workgroup, no barrier.  A wave = PLANE_OUT output columns (PLANE_PX adjacent ones per lane,
// stored as one word) x PFILTER_ROWS output rows of one job of one picture; blockIdx.y = picture, blockIdx.z = column segment --
// the luma segments first, the chroma segments behind them --, blockIdx.x = band in XCD order: ONE launch serves all planes of
// all pictures.
// The intermediate picture t never reaches memory: the wave walks the source rows that its rows' vertical taps cover ONCE.  Per
// source row it stages the samples that its columns' horizontal taps cover into LDS in chunks of PFILTER_CHUNK columns -- lane l
// loads 16 samples of channel l / 16 (one 16-byte load where the plane's start and width are multiples of 16, bytes otherwise;
// the chunks start at multiples of 16 in plane coordinates) --, every lane sums the taps of its PLANE_PX columns in int32 and
// rounds and clamps them to bytes -- the horizontal pass of that row --, and adds ky * value into one int32 accumulator per
// output row, column and channel.  A tap window of thousands of rows or columns (1080p -> 1 x 1) takes no more registers or LDS
// than a small one.  255 * sum |k| + 2^21 < 2^31 for every row of every table: int32 holds every sum, whatever the channel count.
// The coefficient rows of a lane's columns are held in LDS, lane-major per tap and column (no bank conflict), where a row has at
// most PFILTER_LDS_TAPS entries; longer rows are read from the table.  LDS per workgroup: 512 bytes hand-off + 16 KB coefficients.
//
// Written in the H263_HD style of the other kernels: tests/sim_plane_filter/ runs plane_filter_item lane by lane under g++
// (ASan / UBSan), also with the two mutants.
#pragma once

#include "filter_kernel.inl"
#include "plane_resize_kernel.inl"

namespace h263mi {

constexpr uint32_t PFILTER_ROWS = 4;                     // output rows per wave
constexpr uint32_t PFILTER_SRC = 16;                     // adjacent source samples per loading lane: one 16-byte load
constexpr uint32_t PFILTER_CHUNK = 256;                  // source columns per LDS hand-off: 16 lanes per channel load them
constexpr uint32_t PFILTER_LDS_TAPS = 16;                // horizontal coefficient rows up to this length are held in LDS

struct PlaneFilterArgs {
    const uint8_t *src;          // tight I420, picture p at + p * (d_y + 2 * d_c)
    const PlaneDst *dst;         // DEVICE array, one entry per picture
    FilterAxis xy, yy;           // the tables of w -> W' and h -> H'
    FilterAxis xc, yc;           // ... of cw -> cW' and ch -> cH'
    uint32_t w, h, cw, ch;       // source planes
    uint32_t ow, oh, cow, coh;   // output planes
    uint32_t pitch_y, pitch_c;   // destination row pitches
    uint32_t nv12;               // 1: Cb, Cr interleaved at p[1]
    uint32_t wide;               // 1: both pitches and every destination pointer are multiples of 4: word stores
    uint32_t d_y, d_c;           // w*h, cw*ch
    uint32_t bands;              // ceil(H' / PFILTER_ROWS): bands of output rows per picture (the chroma planes use the first half)
    uint32_t chunk;              // bands per picture and XCD: ceil(bands / 8)
    uint32_t segs_y;             // ceil(W' / PLANE_OUT): blockIdx.z below it is a luma segment
    uint32_t n_pictures;
};

// the axes of the luma and the chroma table, which lie back to back at `base`, the luma table first (filter_taps.h: filter_table)
H263_HD void plane_filter_axes(const void *base, PlaneFilterArgs &a, uint32_t ksx_y, uint32_t ksy_y, uint32_t ksx_c, uint32_t ksy_c)
{
    filter_axes(base, a.ow, a.oh, ksx_y, ksy_y, a.xy, a.yy);
    filter_axes(a.yy.coeff + (size_t)a.oh * ksy_y, a.cow, a.coh, ksx_c, ksy_c, a.xc, a.yc);
}

// the launch of k_plane_filter (HOST): k_plane_resize's shape; tables, planes and chroma sizes that are the luma's halves
inline bool plane_filter_plan(PlaneFilterArgs &a, LaunchDims &d)
{
    const FilterAxis *const ax[4] = {&a.xy, &a.yy, &a.xc, &a.yc};
    for (const FilterAxis *x : ax)
        if (!x->span || !x->coeff || !x->ksize) return false;
    if (!a.src || !a.dst || !a.w || !a.h || !a.ow || !a.oh || a.cw != (a.w + 1) / 2 || a.ch != (a.h + 1) / 2 ||
        a.cow != (a.ow + 1) / 2 || a.coh != (a.oh + 1) / 2 || a.n_pictures > 65535)
        return false;
    a.segs_y = (a.ow + PLANE_OUT - 1) / PLANE_OUT;
    d = band_grid(a.oh, PFILTER_ROWS, a.n_pictures, a.segs_y + (a.cow + PLANE_OUT - 1) / PLANE_OUT, a.bands, a.chunk);
    return true;
}

struct PlaneFilterLds {
    uint32_t v[2][PFILTER_CHUNK / 4];                    // the staged samples of a chunk, per channel, four to a word
    int32_t kx[PFILTER_LDS_TAPS][PLANE_PX][64];
};

// what a lane keeps across a band
struct PlaneFilterLane {
    FilterSpan cs[PLANE_PX];                             // its columns' horizontal taps
    int32_t h[2][PLANE_PX];                              // the horizontal sums of the source row at hand
    filter_acc_t acc[2][PLANE_PX][PFILTER_ROWS];
};

// one plane (NCH = 1) or two planes of one geometry resampled together (NCH = 2), as a wave sees it
struct PlaneFilterJob {
    const uint8_t *src[2];
    uint8_t *dst[2];             // (interleave: dst[0] alone)
    FilterAxis x, y;
    uint32_t pw, ow, oh, pitch;
    bool wide_src;               // every source row starts on a 16-byte boundary
    bool wide_dst;
    bool interleave;             // NCH = 2: the two channels leave as byte pairs in one plane
};

// One source row's staging: lane l holds the 16 samples c + 16 * (l % 16) .. + 15 of channel l / 16 (c is a multiple of 16: in a
// plane whose start and width are too, they are one aligned load inside the row)
template <int NCH>
H263_HD void pfilter_phase_stage(const PlaneFilterJob &j, PlaneFilterLds &s, int lane, uint32_t row, uint32_t c, uint32_t c_end)
{
    const uint32_t ch = (uint32_t)lane >> 4, x = c + PFILTER_SRC * ((uint32_t)lane & 15u);
    if (ch >= (uint32_t)NCH || x >= c_end) return;       // (what no tap reads is not staged)
    const uint8_t *const p = (ch ? j.src[NCH - 1] : j.src[0]) + (size_t)row * j.pw + x;      // (a select: j stays in registers)
    uint32_t *const out = &s.v[ch][(x - c) / 4u];
    if (j.wide_src && x + PFILTER_SRC <= j.pw) {
        const uint4 q = *reinterpret_cast<const uint4 *>(p);
        out[0] = q.x, out[1] = q.y, out[2] = q.z, out[3] = q.w;
    } else {
        for (uint32_t g = 0; g < PFILTER_SRC / 4u; g++) {
            uint32_t word = 0;
            for (uint32_t e = 0; e < 4; e++)
                if (x + 4u * g + e < c_end) word |= (uint32_t)p[4u * g + e] << (8u * e);
            out[g] = word;
        }
    }
}

// The taps of the lane's columns that lie in the chunk [c, c + PFILTER_CHUNK), weighed into its horizontal sums.  kx: the
// coefficient row of its first column in the table (used where the rows are not in LDS)
template <int NCH>
H263_HD void pfilter_phase_horizontal(const PlaneFilterLds &s, PlaneFilterLane &t, int lane, const int32_t *kx, uint32_t ksx, bool in_lds,
                                      uint32_t c)
{
    const uint8_t *const v0 = reinterpret_cast<const uint8_t *>(s.v[0]);
    const uint8_t *const v1 = reinterpret_cast<const uint8_t *>(s.v[NCH - 1]);
#pragma unroll
    for (uint32_t e = 0; e < PLANE_PX; e++) {                 // (unrolled: the lane's spans and sums stay in registers)
        const FilterSpan cs = t.cs[e];
        const uint32_t b = cs.first > c ? cs.first : c;
        const uint32_t e0 = cs.first + cs.count, e1 = c + PFILTER_CHUNK, en = e0 < e1 ? e0 : e1;
        for (uint32_t i = b; i < en; i++) {
            const uint32_t k = i - cs.first;
            const int32_t wt = in_lds ? s.kx[k][e][lane] : kx[(size_t)e * ksx + k];
            t.h[0][e] += wt * (int32_t)v0[i - c];
            if (NCH == 2) t.h[1][e] += wt * (int32_t)v1[i - c];
        }
    }
}

// the lane's samples of output row r of the band, rounded and stored
template <int NCH>
H263_HD void pfilter_phase_store(const PlaneFilterJob &j, const PlaneFilterLane &t, uint32_t r, uint32_t X, uint32_t X1, uint32_t Y)
{
    if (X > X1) return;
    const uint32_t n = X1 + 1 - X < PLANE_PX ? X1 + 1 - X : PLANE_PX;
    uint32_t q[NCH][PLANE_PX];
    for (int c = 0; c < NCH; c++)
        for (uint32_t e = 0; e < PLANE_PX; e++) q[c][e] = e < n ? filter_round_v(t.acc[c][e][r]) : 0u;
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
H263_HD void plane_filter_job(const PlaneFilterJob &j, PlaneFilterLds &s, uint32_t band, uint32_t seg, EachLane each)
{
    const uint32_t X0 = seg * PLANE_OUT, X1 = (X0 + PLANE_OUT < j.ow ? X0 + PLANE_OUT : j.ow) - 1u;
    const uint32_t Y0 = band * PFILTER_ROWS, Y1 = Y0 + PFILTER_ROWS < j.oh ? Y0 + PFILTER_ROWS : j.oh;
    const uint32_t ksx = j.x.ksize, ksy = j.y.ksize;
    const bool in_lds = ksx <= PFILTER_LDS_TAPS;
    // the lanes' columns, their coefficient rows
    each([&](int lane, PlaneFilterLane &t) {
#pragma unroll
        for (uint32_t e = 0; e < PLANE_PX; e++) {
            const uint32_t X = X0 + PLANE_PX * (uint32_t)lane + e;
            const bool valid = X <= X1;
            t.cs[e] = valid ? j.x.span[X] : FilterSpan{0, 0};
            for (int c = 0; c < NCH; c++)
                for (uint32_t r = 0; r < PFILTER_ROWS; r++) t.acc[c][e][r] = 0;
            if (valid && in_lds) {
                const int32_t *kx = j.x.coeff + (size_t)X * ksx;
                for (uint32_t k = 0; k < ksx; k++) s.kx[k][e][lane] = kx[k];
            }
        }
    });
    // (a lane reads back its own coefficients only: no fence)
    const FilterSpan ca = j.x.span[X0], cb = j.x.span[X1];
    const uint32_t c0 = ca.first & ~(PFILTER_SRC - 1u), c_end = cb.first + cb.count;
    // the band's rows: their vertical taps (wave-uniform)
    FilterSpan ys[PFILTER_ROWS];
#pragma unroll
    for (uint32_t r = 0; r < PFILTER_ROWS; r++) ys[r] = Y0 + r < Y1 ? j.y.span[Y0 + r] : FilterSpan{0, 0};
    const FilterSpan rb = j.y.span[Y1 - 1u];
    const uint32_t j0 = ys[0].first, j1 = rb.first + rb.count;
    for (uint32_t row = j0; row < j1; row++) {
        each([&](int lane, PlaneFilterLane &t) {
            for (int c = 0; c < NCH; c++)
                for (uint32_t e = 0; e < PLANE_PX; e++) t.h[c][e] = 0;
        });
        for (uint32_t c = c0; c < c_end; c += PFILTER_CHUNK) {
            each([&](int lane, PlaneFilterLane &) { pfilter_phase_stage<NCH>(j, s, lane, row, c, c_end); });
            wave_fence();
            each([&](int lane, PlaneFilterLane &t) {
                const uint32_t X = X0 + PLANE_PX * (uint32_t)lane;
                if (X > X1) return;
                pfilter_phase_horizontal<NCH>(s, t, lane, j.x.coeff + (size_t)X * ksx, ksx, in_lds, c);
            });
            wave_fence();                                     // (the next chunk's samples overwrite these)
        }
        // the weights of this source row in the band's output rows (wave-uniform: scalar loads)
        int32_t kv[PFILTER_ROWS];
#pragma unroll
        for (uint32_t r = 0; r < PFILTER_ROWS; r++) {
            const bool holds = row >= ys[r].first && row - ys[r].first < ys[r].count;
            kv[r] = holds ? j.y.coeff[(size_t)(Y0 + r) * ksy + (row - ys[r].first)] : 0;
        }
        each([&](int lane, PlaneFilterLane &t) {
#pragma unroll
            for (int c = 0; c < NCH; c++)
#pragma unroll
                for (uint32_t e = 0; e < PLANE_PX; e++) {
                    const int32_t v = filter_round_h(t.h[c][e]);
#pragma unroll
                    for (uint32_t r = 0; r < PFILTER_ROWS; r++) t.acc[c][e][r] += (filter_acc_t)kv[r] * v;
                }
        });
    }
#pragma unroll
    for (uint32_t r = 0; r < PFILTER_ROWS; r++) {
        if (Y0 + r >= Y1) break;
        each([&](int lane, PlaneFilterLane &t) { pfilter_phase_store<NCH>(j, t, r, X0 + PLANE_PX * (uint32_t)lane, X1, Y0 + r); });
    }
}

// One wave's work: segment `seg` (luma segments first, then chroma) in band `band` of picture `pic`.  `each(f)` runs
// f(lane, lane_state) for the lanes this thread stands for: the one of its hardware lane on the GPU, all 64 in turn in the CPU
// checker.  Everything outside `each` is wave-uniform.
template <class EachLane>
H263_HD void plane_filter_item(const PlaneFilterArgs &a, PlaneFilterLds &s, uint32_t band, uint32_t seg, uint32_t pic, EachLane each)
{
    uint8_t *const dst_y = a.dst[pic].p[0];
    if (!dst_y) return;                                       // a stream with nothing to render: untouched
    const uint8_t *const pic_src = a.src + (size_t)pic * ((size_t)a.d_y + 2u * (size_t)a.d_c);
    PlaneFilterJob j;
    j.wide_dst = a.wide != 0;
    if (seg < a.segs_y) {
        j.src[0] = j.src[1] = pic_src;
        j.dst[0] = j.dst[1] = dst_y;
        j.x = a.xy, j.y = a.yy;
        j.pw = a.w, j.ow = a.ow, j.oh = a.oh, j.pitch = a.pitch_y;
        j.wide_src = plane_aligned16(j.src[0], j.pw);
        j.interleave = false;
        plane_filter_job<1>(j, s, band, seg, each);
    } else {
        if (band * PFILTER_ROWS >= a.coh) return;             // (the chroma planes have half the bands)
        j.src[0] = pic_src + a.d_y;
        j.src[1] = j.src[0] + a.d_c;
        j.dst[0] = a.dst[pic].p[1];
        j.dst[1] = a.nv12 ? j.dst[0] : a.dst[pic].p[2];
        j.x = a.xc, j.y = a.yc;
        j.pw = a.cw, j.ow = a.cow, j.oh = a.coh, j.pitch = a.pitch_c;
        j.wide_src = plane_aligned16(j.src[0], j.pw) && plane_aligned16(j.src[1], j.pw);
        j.interleave = a.nv12 != 0;
        plane_filter_job<2>(j, s, band, seg - a.segs_y, each);
    }
}

}  // namespace h263mi
