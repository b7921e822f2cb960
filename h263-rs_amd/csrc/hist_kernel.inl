// hist_kernel.inl -- k_hist, k_hist_final, k_hist_select: grey-level histograms of 8-bit planes in device memory, their statistics
// and the list of scene cuts (h263mi_hist_on, h263mi_batch_hist, h263mi_batch_hist_last, h263mi_hist_last; ABI 7).
//
// The contract (include/h263mi.h): a set of W x H planes; hist[p][v] is the number of pixels of picture p with value v; a
// picture's statistics are the sums, the range, the mode and two percentiles of its histogram and its L1 distance to `prev`'s;
// a picture is a CUT when distance * 1000 > cut_permille * 2 * W*H.  Integers only: no result depends on the order of anything.
//
// k_hist.  One wave per workgroup, no barrier.  A work ITEM is a band of HIST_ROWS = 8 picture rows (fewer at the bottom) times a
// column SEGMENT of HIST_SEG = 1024 pixels; lane l takes the CHUNK of 16 pixels at picture column 1024 * segment + 16 * l of every
// row of the band -- k_change's addressing, with its three access paths (change_load): 16-byte loads where base, pitch and stride
// are multiples of 16, words on multiples of 4, bytes otherwise and always for the chunk that the right edge cuts short.  No byte
// outside the W x H rows is read.  A wave counts into a private histogram in LDS over items_per_wave items of one picture
// (hist_items_per_wave: one in a small launch, up to 16 in a large one) and then adds its non-zero bins to the picture's 256 words
// with 32-bit integer atomics, 64 consecutive words an instruction; the words are cleared in stream order in front of the launch.
//
// What keeps the content from deciding the time: (1) the LDS histogram is HIST_COPIES = 16 histograms interleaved, bin v of copy c
// at word 16 * v + c with c = lane & 15: lanes that meet in one bin spread over sixteen words in sixteen banks, so one instruction
// serialises 4 deep at the worst (all 64 lanes in one bin) instead of 64; (2) a lane whose 16 pixels are all one value adds 16
// once, not 1 sixteen times -- flat areas, of which decoded video is full, are the cheapest content, not the dearest.  The worst
// content is one whose lanes all meet in a bin without any chunk being flat, such as two values alternating from pixel to pixel:
// 16 additions a chunk, each 4 deep.  (Merging every run of equal neighbours inside a chunk was tried first: its compares and
// branches, some 12 instructions a pixel, bound the kernel at three times the read probe whatever the content was.)
//
// k_hist_final.  One wave per picture: lane l holds the counts 4 l .. 4 l + 3, the cumulative count comes from a prefix sum of the
// lanes' totals through LDS, lane 0 reduces the lanes' terms and writes the 32 bytes; the lanes compare with and roll `prev`.
// k_hist_select is k_change_select's shape with the cut as its predicate.
//
// Nothing wraps: a copy's bin is at most 4 lanes x 16 items x 8 rows x 16 pixels = 2^13; a count is at most W*H < 2^30; sum_sq < 2^46;
// distance <= 256 * 2^32; distance * 1000 and 1000 * C(v), q * P, cut_permille * 2 P lie in 64 bits.
//
// Written in the H263_HD style of change_kernel.inl: tests/sim_hist/ runs hist_wave, hist_final and hist_select lane by lane under
// g++ (ASan / UBSan) over planes of exactly the set's bytes.
#pragma once

#include "change_kernel.inl"
#include "dev_common.h"
#include "mutants.h"

namespace h263mi {

constexpr uint32_t HIST_SEG = 1024u;                     // pixels of a segment: 64 lanes x 16
constexpr uint32_t HIST_ROWS = 8u;                       // rows of a work item
constexpr uint32_t HIST_COPIES = 16u;                    // interleaved copies of a wave's LDS histogram
constexpr uint32_t HIST_MAX_PICTURES = 65535u;
enum : uint32_t {
    HIST_VALID = 1u,             // the picture exists: a stream without a last picture lacks it
    HIST_SET1 = 2u,              // its plane lies `set1` bytes further (the frame store's second set)
};

static_assert(sizeof(h263mi_hist_stats) == 32, "the statistics are written as 32-byte records");

struct HistArgs {
    const uint8_t *src;
    uint64_t pitch, stride;
    uint64_t set1;               // bytes from a picture to the same picture in the second set (HIST_SET1)
    const uint32_t *words;       // one HIST_* word per picture (device), or nullptr: every picture is valid and in set 0
    uint32_t *hist;              // picture p's 256 counts at + 256 * p; cleared in front of the launch
    uint32_t w, h, n_pictures;
    uint32_t align;              // 16, 4 or 1: what base, pitch, stride (and set1) are all multiples of (change_align)
    uint32_t segs;               // ceil(w / HIST_SEG)
    uint32_t bands;              // ceil(h / HIST_ROWS)
    uint32_t p0;                 // the launch's first picture (set by the launcher)
    uint32_t items_per_wave;     // work items a wave takes, one after the other (set by the plan: hist_items_per_wave)
};

struct HistFinalArgs {
    const uint32_t *hist;
    uint32_t *prev;              // as hist, or nullptr: distance 0; written under roll only
    h263mi_hist_stats *stats;
    const uint32_t *words;       // as HistArgs::words
    uint64_t pixels;             // W * H
    uint32_t n_pictures, lo_permille, hi_permille, roll;
};

struct HistSelectArgs {
    const h263mi_hist_stats *stats;
    const uint32_t *words;       // as HistArgs::words
    uint32_t *selected, *count;
    uint64_t pixels;             // W * H
    uint32_t n_pictures, cut_permille;
};

// what a wave hands between its lanes
struct HistLds {
    uint32_t bins[256 * HIST_COPIES];    // k_hist: bin v of copy c at 16 v + c
};
struct HistFinalLds {
    uint32_t total[64];                  // k_hist_final: every lane's terms
    uint64_t sum[64], sum_sq[64], distance[64];
    uint32_t min[64], max[64], mode[64], mode_count[64], p_lo[64], p_hi[64];
    unsigned long long vote;             // k_hist_select: the lanes that select their picture
};

struct HistLane {
    uint32_t c[4];
    bool sel;
};

H263_HD void hist_lds_add(uint32_t *p, uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#else
    *p += v;
#endif
}

// the first nb (1..16) bytes of v into the lane's copy of the LDS histogram; a whole chunk of one value is one addition of 16
H263_HD void hist_count(uint32_t *mine, const uint4 &v, uint32_t nb)
{
    if (mutants::kHistCutChunkFull) nb = 16u;
    // (all 16 bytes equal: the four words are equal and one of them equals itself rotated by a byte)
    if (nb == 16u && v.x == v.y && v.x == v.z && v.x == v.w && v.x == ((v.x >> 8) | (v.x << 24))) {
        hist_lds_add(mine + HIST_COPIES * (v.x & 0xffu), 16u);
        return;
    }
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (uint32_t k = 0; k < 16u; k++) {
        if (k >= nb) break;
        hist_lds_add(mine + HIST_COPIES * ((w[k >> 2] >> (8u * (k & 3u))) & 0xffu), 1u);
    }
}

// R rows of a whole chunk on 16-byte accesses: the R loads are in flight together
template <uint32_t R>
H263_HD void hist_rows_wide(const uint8_t *p, uint64_t pitch, uint32_t *mine)
{
    uint4 v[R];
#pragma unroll
    for (uint32_t k = 0; k < R; k++) v[k] = *reinterpret_cast<const uint4 *>(p + (uint64_t)k * pitch);
#pragma unroll
    for (uint32_t k = 0; k < R; k++) hist_count(mine, v[k], 16u);
}

// Work items one wave takes (HistArgs::items_per_wave) of a launch of `items` in all: a wave ends in up to 256 atomics on the 16
// cache lines of its picture's histogram, so a large launch gives each wave several items before it adds (a 1080p picture's 270
// items go to 34 waves in a call of 64: 8 700 words a picture at the most) -- but keeps some thousand waves, enough to fill the device
inline uint32_t hist_items_per_wave(uint64_t items)
{
    const uint64_t k = items / 2048u;
    return k < 1u ? 1u : (k > 16u ? 16u : (uint32_t)k);
}

// The launches of k_hist (HOST): a call goes out `pictures` whole pictures at a time from p0 = 0 on, the last launch the rest,
// `waves` workgroups a picture -- at most HIST_GRID_MAX workgroups a launch.  items_per_wave: 0 = hist_items_per_wave's (the
// launcher), another value the checker's.
constexpr uint64_t HIST_GRID_MAX = 1u << 24;

struct HistLaunch {
    uint32_t waves, pictures;
};

inline bool hist_plan(HistArgs &a, HistLaunch &l, uint32_t items_per_wave = 0)
{
    if (a.n_pictures > HIST_MAX_PICTURES || !a.w || !a.h || a.w > 65535 || a.h > 65535 || (uint64_t)a.w * a.h >= (1ull << 30) || !a.src ||
        !a.hist || (a.align != 16u && a.align != 4u && a.align != 1u) || a.segs != (a.w + HIST_SEG - 1u) / HIST_SEG ||
        a.bands != (a.h + HIST_ROWS - 1u) / HIST_ROWS)
        return false;
    const uint32_t items = a.bands * a.segs;                           // of a picture (below 2^18: w * h < 2^30)
    a.items_per_wave = items_per_wave ? items_per_wave : hist_items_per_wave((uint64_t)items * a.n_pictures);
    l.waves = (items + a.items_per_wave - 1u) / a.items_per_wave;
    l.pictures = (uint32_t)(HIST_GRID_MAX / l.waves);
    return true;
}

// One wave's work: the items first .. first + items_per_wave - 1 of picture p, an item being segment seg of band `band` and their
// number band * segs + seg.  `each(f)` runs f(lane, lane_state) for the lanes this thread stands for: the one of its hardware lane
// on the GPU, all 64 in turn in the CPU checker.  Everything outside `each` is wave-uniform.
template <class EachLane>
H263_HD void hist_wave(const HistArgs &a, HistLds &s, uint32_t p, uint32_t first, EachLane each)
{
    const uint32_t word = a.words ? a.words[p] : (uint32_t)HIST_VALID;
    if (!(word & HIST_VALID)) return;
    const uint8_t *const src_p = a.src + (uint64_t)p * a.stride + ((word & HIST_SET1) ? a.set1 : 0u);
    each([&](int lane, HistLane &) {
        for (uint32_t k = 0; k < 256u * HIST_COPIES / (64u * 4u); k++)     // (four words a lane and turn)
            *reinterpret_cast<uint4 *>(&s.bins[4u * (64u * k + (uint32_t)lane)]) = make_uint4(0u, 0u, 0u, 0u);
    });
    wave_fence();
    uint32_t band = first / a.segs, seg = first - band * a.segs;
    for (uint32_t i = 0; i < a.items_per_wave && band < a.bands; i++) {
        const uint32_t y0 = band * HIST_ROWS, rows = a.h - y0 < HIST_ROWS ? a.h - y0 : HIST_ROWS, seg_x = seg * HIST_SEG;
        const uint8_t *const src = src_p + (uint64_t)y0 * a.pitch;
        each([&](int lane, HistLane &) {
            const uint32_t x = seg_x + 16u * (uint32_t)lane;
            if (x >= a.w) return;
            const uint32_t nb = a.w - x < 16u ? a.w - x : 16u;
            const uint8_t *const q = src + x;
            uint32_t *const mine = s.bins + ((uint32_t)lane & (HIST_COPIES - 1u));
            uint32_t r = 0;
            if (nb == 16u && a.align == 16u) {
                if (rows == HIST_ROWS) {
                    hist_rows_wide<HIST_ROWS>(q, a.pitch, mine);
                    r = HIST_ROWS;
                } else if (rows >= 4u) {
                    hist_rows_wide<4>(q, a.pitch, mine);
                    r = 4u;
                }
            }
            for (; r < rows; r++) hist_count(mine, change_load(q + (uint64_t)r * a.pitch, nb, a.align), nb);
        });
        if (++seg == a.segs) seg = 0, band++;
    }
    wave_fence();
    // the wave's counts: bins j * 64 + lane, the copies summed, zeros left out
    uint32_t *const out = a.hist + (size_t)p * 256u;
    each([&](int lane, HistLane &) {
        for (uint32_t j = 0; j < 4u; j++) {
            const uint32_t v = 64u * j + (uint32_t)lane;
            uint32_t n = 0;
            for (uint32_t c = 0; c < HIST_COPIES; c++) n += s.bins[HIST_COPIES * v + c];
            if (n) change_add32(out + v, n);
        }
    });
}

// is 1000 * C >= q * P (hist_final's percentile test; C >= 1 is the caller's)
H263_HD bool hist_reached(uint64_t cum, uint32_t permille, uint64_t pixels)
{
    if (mutants::kHistPercentileStrict) return 1000u * cum > (uint64_t)permille * pixels;
    return 1000u * cum >= (uint64_t)permille * pixels;
}

// The one wave of picture p of k_hist_final
template <class EachLane>
H263_HD void hist_final(const HistFinalArgs &f, HistFinalLds &s, uint32_t p, EachLane each)
{
    const bool valid = !f.words || (f.words[p] & HIST_VALID);
    h263mi_hist_stats *const out = f.stats + p;
    if (!valid) {                                            // (its histogram was cleared; its prev is not touched)
        each([&](int lane, HistLane &) {
            if (lane < 8) reinterpret_cast<uint32_t *>(out)[lane] = 0u;
        });
        return;
    }
    const uint32_t *const hist = f.hist + (size_t)p * 256u;
    uint32_t *const prev = f.prev ? f.prev + (size_t)p * 256u : nullptr;
    each([&](int lane, HistLane &t) {
        uint64_t sum = 0, sum_sq = 0, distance = 0;
        uint32_t total = 0, mn = 256u, mx = 0, mode = 0, mode_count = 0;
        for (uint32_t k = 0; k < 4u; k++) {
            const uint32_t v = 4u * (uint32_t)lane + k, c = hist[v];
            t.c[k] = c;
            total += c;
            sum += (uint64_t)v * c;
            sum_sq += (uint64_t)(v * v) * c;
            if (c && mn == 256u) mn = v;
            if (c) mx = v;
            if (c > mode_count) mode_count = c, mode = v;
            if (prev) {
                const uint32_t q = prev[v];
                distance += c > q ? c - q : q - c;
                if (f.roll) prev[v] = c;
            }
        }
        s.total[lane] = total;
        s.sum[lane] = sum, s.sum_sq[lane] = sum_sq, s.distance[lane] = distance;
        s.min[lane] = mn, s.max[lane] = mx, s.mode[lane] = mode, s.mode_count[lane] = mode_count;
    });
    wave_fence();
    // the prefix sum: the count below the lane's first value; then the first of its values that reaches each percentile
    each([&](int lane, HistLane &t) {
        uint64_t cum = 0;
        for (int k = 0; k < lane; k++) cum += s.total[k];
        uint32_t lo = 256u, hi = 256u;
        for (uint32_t k = 0; k < 4u; k++) {
            cum += t.c[k];
            if (!cum) continue;
            if (lo == 256u && hist_reached(cum, f.lo_permille, f.pixels)) lo = 4u * (uint32_t)lane + k;
            if (hi == 256u && hist_reached(cum, f.hi_permille, f.pixels)) hi = 4u * (uint32_t)lane + k;
        }
        s.p_lo[lane] = lo, s.p_hi[lane] = hi;
    });
    wave_fence();
    each([&](int lane, HistLane &) {
        if (lane != 0) return;
        uint64_t sum = 0, sum_sq = 0, distance = 0;
        uint32_t mn = 256u, mx = 0, mode = 0, mode_count = 0, lo = 256u, hi = 256u;
        for (int k = 0; k < 64; k++) {
            sum += s.sum[k], sum_sq += s.sum_sq[k], distance += s.distance[k];
            mn = s.min[k] < mn ? s.min[k] : mn;
            mx = s.max[k] > mx ? s.max[k] : mx;
            if (s.mode_count[k] > mode_count) mode_count = s.mode_count[k], mode = s.mode[k];
            lo = s.p_lo[k] < lo ? s.p_lo[k] : lo;
            hi = s.p_hi[k] < hi ? s.p_hi[k] : hi;
        }
        // (a picture has a pixel, so min and, with the strict mutant aside, both percentiles exist: 255 stands for "none reached")
        out->sum = sum, out->sum_sq = sum_sq, out->distance = distance;
        out->min = (uint8_t)(mn & 255u), out->max = (uint8_t)mx;
        out->p_lo = (uint8_t)(lo > 255u ? 255u : lo), out->p_hi = (uint8_t)(hi > 255u ? 255u : hi);
        out->mode = (uint8_t)mode;
        out->reserved[0] = out->reserved[1] = out->reserved[2] = 0;
    });
}

// is the picture a cut?
H263_HD bool hist_is_cut(uint64_t distance, uint32_t cut_permille, uint64_t pixels) { return distance * 1000u > (uint64_t)cut_permille * 2u * pixels; }

// One lane's vote, collected for the wave: the GPU's ballot, the checker's bit by bit (s.vote cleared in front)
H263_HD void hist_vote(HistFinalLds &s, int lane, bool sel)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const unsigned long long m = __builtin_amdgcn_ballot_w64(sel);
    if (lane == 0) s.vote = m;
#else
    if (sel) s.vote |= 1ull << lane;
#endif
}

// The one wave of k_hist_select: the valid pictures that are cuts, ascending, 64 per step -- a picture's place in the list is the
// count so far plus the votes of the lanes below its own (change_select with another predicate).
template <class EachLane>
H263_HD void hist_select(const HistSelectArgs &f, HistFinalLds &s, EachLane each)
{
    uint32_t count = 0;
    for (uint32_t base = 0; base < f.n_pictures; base += 64u) {
#if !defined(__HIP_DEVICE_COMPILE__)
        s.vote = 0;
#endif
        each([&](int lane, HistLane &t) {
            const uint32_t p = base + (uint32_t)lane;
            t.sel = p < f.n_pictures && (!f.words || (f.words[p] & HIST_VALID)) && hist_is_cut(f.stats[p].distance, f.cut_permille, f.pixels);
            hist_vote(s, lane, t.sel);
        });
        wave_fence();
        const unsigned long long vote = s.vote;
        each([&](int lane, HistLane &t) {
            if (t.sel) f.selected[count + (uint32_t)__builtin_popcountll(vote & ((1ull << lane) - 1ull))] = base + (uint32_t)lane;
        });
        wave_fence();                                        // (the next step overwrites the votes)
        count += (uint32_t)__builtin_popcountll(vote);
    }
    each([&](int lane, HistLane &) {
        if (lane == 0) *f.count = count;
    });
}

}  // namespace h263mi
