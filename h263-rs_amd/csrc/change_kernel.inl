// change_kernel.inl -- k_change, k_change_select: change maps of 8-bit planes in device memory (h263mi_change_map_on,
// h263mi_batch_change_map, h263mi_batch_change_last, h263mi_change_last; ABI 7).
//
// The contract (include/h263mi.h): two sets of W x H planes, `cur` and `prev`, compared picture by picture over a grid of square
// cells of c = 1 << cell_log2 pixels anchored at the origin, gw = ceil(W / c) by gh = ceil(H / c), edge cells partial.  A cell's
// SAD is the sum of |cur - prev| over its pixels; it is CHANGED when sad * c*c > cell_threshold * pixels(cell), in 64 bits; a
// picture's summary is the sum of its cells' SADs, the count of changed cells and the largest raw SAD.  Integers only: the
// results do not depend on the order in which anything is summed.
//
// One wave per workgroup, no barrier.  A work ITEM is one cell row of one picture (c picture rows, fewer at the bottom) times a
// column SEGMENT of CHANGE_SEG = 1024 pixels.  Lane l takes the CHUNK of 16 pixels at picture column 1024 * segment + 16 * l of
// every row: chunks start at multiples of 16 in PICTURE coordinates, so one never straddles a cell when c >= 16 and holds exactly
// two when c = 8 -- a lane keeps one sum per 8-pixel half.  |a - b| is summed four bytes per instruction (v_sad_u8).  The halves
// go through LDS; lane j sums the c / 8 of cell j of the segment (the halves of 1, 2 or 4 lanes; c = 8: lane j has cells j and
// j + 64), judges it, and the 64 lanes store 64 consecutive cell SADs.  A wave takes items_per_wave items of one picture, one
// after the other (change_items_per_wave: one in a small launch, up to 16 in a large one); its total, changed count and maximum
// then go to the picture's summary with integer atomics (64-bit add, 32-bit add, 32-bit max), zeros left out; the summaries are
// cleared in stream order in front of the launch.  Under roll the lane that loaded a chunk of cur stores it to prev.
//
// Accesses: a set whose base, pitch and picture stride are all multiples of 16 is read (and rolled) with 16-byte accesses, one
// whose are multiples of 4 with 4-byte ones, any other byte by byte; a chunk that the picture's right edge cuts short always goes
// byte by byte.  On every path a wave reads and writes no byte outside the W x H rows of its pictures.  A picture whose word
// (ChangeArgs::words) lacks CHANGE_VALID is not touched at all: nothing read, nothing written.
//
// Nothing wraps: a half's sum is at most 8 * 64 * 255 < 2^17, a cell's at most 64 * 64 * 255 < 2^20, a wave's 16 * 1024 * 64 * 255
// < 2^28; a picture's lies in 64 bits; sad << 12 and cell_threshold * 4096 lie in 64 bits.
//
// Written in the H263_HD style of digest_kernel.inl: tests/sim_change/ runs change_wave and change_select lane by lane under g++
// (ASan / UBSan) over planes of exactly the sets' bytes.
#pragma once

#include "dev_common.h"
#include "mutants.h"

namespace h263mi {

constexpr uint32_t CHANGE_SEG = 1024u;                   // pixels of a segment: 64 lanes x 16
constexpr uint32_t CHANGE_MAX_PICTURES = 65535u;
enum : uint32_t {
    CHANGE_VALID = 1u,           // the picture exists: a stream without a last picture lacks it
    CHANGE_SET1 = 2u,            // its cur plane lies cur_set1 bytes further (the frame store's second set)
};

static_assert(sizeof(h263mi_change_summary) == 16, "the summaries are cleared and read as 16-byte records");

struct ChangeArgs {
    const uint8_t *cur;
    uint8_t *prev;               // written under roll only
    uint64_t cur_pitch, cur_stride, prev_pitch, prev_stride;
    uint64_t cur_set1;           // bytes from a picture of cur to the same picture in the second set (CHANGE_SET1)
    const uint32_t *words;       // one CHANGE_* word per picture (device), or nullptr: every picture is valid and in set 0
    uint32_t *cells;             // picture p's grid at + p * gw * gh, or nullptr
    h263mi_change_summary *summary;
    uint32_t w, h, gw, gh;
    uint32_t cell_log2, roll, threshold, n_pictures;
    uint32_t cur_align, prev_align;      // 16, 4 or 1: what base, pitch and stride of the set are all multiples of
    uint32_t segs;               // ceil(w / CHANGE_SEG)
    uint32_t p0;                 // the launch's first picture (set by the launcher)
    uint32_t items_per_wave;     // work items a wave takes, one after the other (set by the launcher: change_items_per_wave)
    uint32_t pad;
};

// what a set's base, pitch and picture stride (and `more`) are all multiples of: 16, 4 or 1 (cur_align, prev_align)
inline uint32_t change_align(const void *base, uint64_t pitch, uint64_t stride, uint64_t more = 0)
{
    const uint64_t m = (uint64_t)(uintptr_t)base | pitch | stride | more;
    return m % 16 == 0 ? 16u : (m % 4 == 0 ? 4u : 1u);
}

struct ChangeSelectArgs {
    const h263mi_change_summary *summary;
    const uint32_t *words;       // as ChangeArgs::words
    uint32_t *selected, *count;
    uint32_t n_pictures, min_changed;
};

// what a wave hands between its lanes: the sums of every lane's two halves, then per lane and per eight lanes the wave's terms
struct ChangeLds {
    uint32_t half[128];
    uint32_t sad[64], changed[64], max[64];
    uint32_t sad8[8], changed8[8], max8[8];
    unsigned long long vote;     // k_change_select: the lanes that select their picture
};

struct ChangeLane {
    uint32_t sad, changed, max;
    bool sel;
};

// acc + the sum of |byte k of a - byte k of b|
H263_HD uint32_t change_sad4(uint32_t a, uint32_t b, uint32_t acc)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_sad_u8(a, b, acc);
#else
    for (int k = 0; k < 4; k++) {
        const int d = (int)((a >> (8 * k)) & 0xffu) - (int)((b >> (8 * k)) & 0xffu);
        acc += (uint32_t)(d < 0 ? -d : d);
    }
    return acc;
#endif
}

// the nb (1..16) bytes at p as four words, the missing ones 0; align: what p is a multiple of when nb == 16
H263_HD uint4 change_load(const uint8_t *p, uint32_t nb, uint32_t align)
{
    if (nb == 16u && align == 16u) return *reinterpret_cast<const uint4 *>(p);
    if (nb == 16u && align == 4u) {
        const uint32_t *q = reinterpret_cast<const uint32_t *>(p);
        return make_uint4(q[0], q[1], q[2], q[3]);
    }
    uint32_t v[4] = {0u, 0u, 0u, 0u};
    for (uint32_t k = 0; k < nb; k++) v[k >> 2] |= (uint32_t)p[k] << (8u * (k & 3u));
    return make_uint4(v[0], v[1], v[2], v[3]);
}

H263_HD void change_store(uint8_t *p, const uint4 &v, uint32_t nb, uint32_t align)
{
    if (nb == 16u && align == 16u) {
        *reinterpret_cast<uint4 *>(p) = v;
        return;
    }
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    if (nb == 16u && align == 4u) {
        uint32_t *q = reinterpret_cast<uint32_t *>(p);
        for (int k = 0; k < 4; k++) q[k] = w[k];
        return;
    }
    for (uint32_t k = 0; k < nb; k++) p[k] = (uint8_t)(w[k >> 2] >> (8u * (k & 3u)));
}

H263_HD void change_add64(uint64_t *p, uint64_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v);
#else
    *p += v;
#endif
}
H263_HD void change_add32(uint32_t *p, uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(p, v);
#else
    *p += v;
#endif
}
H263_HD void change_max32(uint32_t *p, uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMax(p, v);
#else
    if (v > *p) *p = v;
#endif
}

// is the cell changed?  pixels: the picture pixels it holds (c*c for a full cell)
H263_HD bool change_judge(uint32_t sad, uint32_t cell_log2, uint32_t threshold, uint32_t pixels)
{
    if (mutants::kChangeEdgeAsFull) pixels = 1u << (2u * cell_log2);
    return ((uint64_t)sad << (2u * cell_log2)) > (uint64_t)threshold * pixels;
}

// R rows of a whole chunk, both sets on 16-byte accesses: the 2 R loads are in flight together
template <uint32_t R>
H263_HD void change_rows_wide(const ChangeArgs &a, const uint8_t *pc, uint8_t *pp, uint32_t &lo, uint32_t &hi)
{
    uint4 vc[R], vp[R];
#pragma unroll
    for (uint32_t k = 0; k < R; k++) vc[k] = *reinterpret_cast<const uint4 *>(pc + (uint64_t)k * a.cur_pitch);
#pragma unroll
    for (uint32_t k = 0; k < R; k++) vp[k] = *reinterpret_cast<const uint4 *>(pp + (uint64_t)k * a.prev_pitch);
#pragma unroll
    for (uint32_t k = 0; k < R; k++) {
        lo = change_sad4(vc[k].x, vp[k].x, change_sad4(vc[k].y, vp[k].y, lo));
        hi = change_sad4(vc[k].z, vp[k].z, change_sad4(vc[k].w, vp[k].w, hi));
    }
    if (a.roll) {
#pragma unroll
        for (uint32_t k = 0; k < R; k++) *reinterpret_cast<uint4 *>(pp + (uint64_t)k * a.prev_pitch) = vc[k];
    }
}

// Work items one wave takes (ChangeArgs::items_per_wave) of a launch of `items` in all: the summaries take three atomics per WAVE,
// and the waves of a picture meet in one 16-byte record, so a large launch gives each wave several items to sum before it adds --
// but keeps some thousand waves, enough to fill the device
inline uint32_t change_items_per_wave(uint64_t items)
{
    const uint64_t k = items / 2048u;
    return k < 1u ? 1u : (k > 16u ? 16u : (uint32_t)k);
}

// The launches of k_change (HOST): a call goes out `pictures` whole pictures at a time from p0 = 0 on, the last launch the rest,
// `waves` workgroups a picture -- at most CHANGE_GRID_MAX workgroups a launch.  items_per_wave: 0 = change_items_per_wave's (the
// launcher), another value the checker's.
constexpr uint64_t CHANGE_GRID_MAX = 1u << 24;

struct ChangeLaunch {
    uint32_t waves, pictures;
};

inline bool change_plan(ChangeArgs &a, ChangeLaunch &l, uint32_t items_per_wave = 0)
{
    if (a.n_pictures > CHANGE_MAX_PICTURES || a.cell_log2 < 3 || a.cell_log2 > 6 || !a.w || !a.h || a.w > 65535 || a.h > 65535 ||
        (uint64_t)a.w * a.h >= (1ull << 30) || !a.cur || !a.prev || !a.summary || a.gw != ((a.w - 1u) >> a.cell_log2) + 1u ||
        a.gh != ((a.h - 1u) >> a.cell_log2) + 1u || a.segs != (a.w + CHANGE_SEG - 1u) / CHANGE_SEG)
        return false;
    const uint32_t items = a.gh * a.segs;                              // of a picture (below 2^19: w * h < 2^30)
    a.items_per_wave = items_per_wave ? items_per_wave : change_items_per_wave((uint64_t)items * a.n_pictures);
    l.waves = (items + a.items_per_wave - 1u) / a.items_per_wave;
    l.pictures = (uint32_t)(CHANGE_GRID_MAX / l.waves);
    return true;
}

// One wave's work: the items first .. first + items_per_wave - 1 of picture p, an item being segment seg of cell row cy and
// their number cy * segs + seg.  `each(f)` runs f(lane, lane_state) for the lanes this thread stands for: the one of its hardware
// lane on the GPU, all 64 in turn in the CPU checker.  Everything outside `each` is wave-uniform.
template <class EachLane>
H263_HD void change_wave(const ChangeArgs &a, ChangeLds &s, uint32_t p, uint32_t first, EachLane each)
{
    const uint32_t word = a.words ? a.words[p] : (uint32_t)CHANGE_VALID;
    if (!(word & CHANGE_VALID)) return;
    const uint32_t c = 1u << a.cell_log2, halves = c >> 3, in_seg = CHANGE_SEG >> a.cell_log2;
    const uint8_t *const cur_p = a.cur + (uint64_t)p * a.cur_stride + ((word & CHANGE_SET1) ? a.cur_set1 : 0u);
    uint8_t *const prev_p = a.prev + (uint64_t)p * a.prev_stride;
    each([&](int, ChangeLane &t) { t.sad = t.changed = t.max = 0; });
    uint32_t cy = first / a.segs, seg = first - cy * a.segs;
    for (uint32_t i = 0; i < a.items_per_wave && cy < a.gh; i++) {
        const uint32_t y0 = cy << a.cell_log2, rows = a.h - y0 < c ? a.h - y0 : c, seg_x = seg * CHANGE_SEG;
        const uint8_t *const cur = cur_p + (uint64_t)y0 * a.cur_pitch;
        uint8_t *const prev = prev_p + (uint64_t)y0 * a.prev_pitch;
        each([&](int lane, ChangeLane &) {
            const uint32_t x = seg_x + 16u * (uint32_t)lane;
            uint32_t lo = 0, hi = 0;                          // pixels x .. x + 7 and x + 8 .. x + 15 of the item's rows
            if (x < a.w) {
                const uint32_t nb = a.w - x < 16u ? a.w - x : 16u;
                const uint8_t *const pc = cur + x;
                uint8_t *const pp = prev + x;
                uint32_t r = 0;
                if (nb == 16u && a.cur_align == 16u && a.prev_align == 16u) {
                    for (; r + 8u <= rows; r += 8u) change_rows_wide<8>(a, pc + (uint64_t)r * a.cur_pitch, pp + (uint64_t)r * a.prev_pitch, lo, hi);
                    if (r + 4u <= rows) {
                        change_rows_wide<4>(a, pc + (uint64_t)r * a.cur_pitch, pp + (uint64_t)r * a.prev_pitch, lo, hi);
                        r += 4u;
                    }
                }
                for (; r < rows; r++) {
                    uint8_t *const qp = pp + (uint64_t)r * a.prev_pitch;
                    const uint4 vc = change_load(pc + (uint64_t)r * a.cur_pitch, nb, a.cur_align);
                    const uint4 vp = change_load(qp, nb, a.prev_align);
                    lo = change_sad4(vc.x, vp.x, change_sad4(vc.y, vp.y, lo));
                    hi = change_sad4(vc.z, vp.z, change_sad4(vc.w, vp.w, hi));
                    if (a.roll) change_store(qp, vc, nb, a.prev_align);
                }
            }
            s.half[2 * lane] = lo;
            s.half[2 * lane + 1] = hi;
        });
        wave_fence();
        // the segment's cells: cell j is made of the halves j * c/8 ...; its picture column is cell0 + j
        const uint32_t cell0 = (mutants::kChangeSegmentCell && seg ? seg_x - 1u : seg_x) >> a.cell_log2;
        const uint32_t n_cells = a.gw - cell0 < in_seg ? a.gw - cell0 : in_seg;
        uint32_t *const row = a.cells ? a.cells + (size_t)p * a.gw * a.gh + (size_t)cy * a.gw + cell0 : nullptr;
        each([&](int lane, ChangeLane &t) {
            for (uint32_t j = (uint32_t)lane; j < n_cells; j += 64u) {            // (a second turn when c = 8 only)
                uint32_t sad = 0;
                for (uint32_t k = 0; k < halves; k++) sad += s.half[j * halves + k];
                const uint32_t cx = cell0 + j, cw = a.w - (cx << a.cell_log2) < c ? a.w - (cx << a.cell_log2) : c;
                if (row) row[j] = sad;
                t.sad += sad;
                t.changed += change_judge(sad, a.cell_log2, a.threshold, cw * rows) ? 1u : 0u;
                t.max = sad > t.max ? sad : t.max;
            }
        });
        wave_fence();                                        // (the next item overwrites the halves)
        if (++seg == a.segs) seg = 0, cy++;
    }
    // the wave's terms: every lane's, then the sums of eight lanes each, then lane 0 adds
    each([&](int lane, ChangeLane &t) {
        s.sad[lane] = t.sad;
        s.changed[lane] = t.changed;
        s.max[lane] = t.max;
    });
    wave_fence();
    each([&](int lane, ChangeLane &) {
        if (lane < 8) {
            uint32_t sad = 0, changed = 0, mx = 0;
            for (int k = 0; k < 8; k++) {
                sad += s.sad[8 * lane + k];
                changed += s.changed[8 * lane + k];
                mx = s.max[8 * lane + k] > mx ? s.max[8 * lane + k] : mx;
            }
            s.sad8[lane] = sad;
            s.changed8[lane] = changed;
            s.max8[lane] = mx;
        }
    });
    wave_fence();
    each([&](int lane, ChangeLane &) {
        if (lane == 0) {
            uint32_t sad = 0, changed = 0, mx = 0;
            for (int k = 0; k < 8; k++) {
                sad += s.sad8[k];
                changed += s.changed8[k];
                mx = s.max8[k] > mx ? s.max8[k] : mx;
            }
            h263mi_change_summary *const out = a.summary + p;
            if (sad) change_add64(&out->sad, sad);               // (sad == 0: max is 0 too)
            if (changed) change_add32(&out->changed_cells, changed);
            if (mx) change_max32(&out->max_cell_sad, mx);
        }
    });
}

// One lane's vote, collected for the wave: the GPU's ballot, the checker's bit by bit (s.vote cleared in front)
H263_HD void change_vote(ChangeLds &s, int lane, bool sel)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const unsigned long long m = __builtin_amdgcn_ballot_w64(sel);
    if (lane == 0) s.vote = m;
#else
    if (sel) s.vote |= 1ull << lane;
#endif
}

// The one wave of k_change_select: the valid pictures with changed_cells >= min_changed, ascending, 64 per step -- a picture's
// place in the list is the count so far plus the votes of the lanes below its own.
template <class EachLane>
H263_HD void change_select(const ChangeSelectArgs &f, ChangeLds &s, EachLane each)
{
    uint32_t count = 0;
    for (uint32_t base = 0; base < f.n_pictures; base += 64u) {
#if !defined(__HIP_DEVICE_COMPILE__)
        s.vote = 0;
#endif
        each([&](int lane, ChangeLane &t) {
            const uint32_t p = base + (uint32_t)lane;
            t.sel = p < f.n_pictures && (!f.words || (f.words[p] & CHANGE_VALID)) && f.summary[p].changed_cells >= f.min_changed;
            change_vote(s, lane, t.sel);
        });
        wave_fence();
        const unsigned long long vote = s.vote;
        each([&](int lane, ChangeLane &t) {
            if (t.sel) f.selected[count + (uint32_t)__builtin_popcountll(vote & ((1ull << lane) - 1ull))] = base + (uint32_t)lane;
        });
        wave_fence();                                        // (the next step overwrites the votes)
        count += (uint32_t)__builtin_popcountll(vote);
    }
    each([&](int lane, ChangeLane &) {
        if (lane == 0) *f.count = count;
    });
}

}  // namespace h263mi
