// background_kernel.inl -- k_bg_begin, k_bg: the background model of 8-bit planes in device memory, a running average per pixel and
// the map of foreground cells (h263mi_background_on, h263mi_batch_background, h263mi_batch_background_last, h263mi_background_last;
// ABI 7).  The selection is change_select's (change_kernel.inl).
//
// The contract (include/h263mi.h, BACKGROUND MODEL): every picture of a set of W x H planes, `cur`, has a STATE in device memory
// that the caller owns: a 64-byte head {age, mode} and H rows of uint16 background words b in 8.7 fixed point (0 .. 255 << 7), a
// row padded to whole 16-pixel chunks (bpitch = 32 * ceil(W / 16) bytes).  A call judges every pixel c against its word BEFORE the
// update -- r = (b + 64) >> 7, foreground when |c - r| > pixel_threshold -- and then moves the word towards c << 7 by
// d >> shift, at least by one while d != 0, the shift chosen by the verdict (fg_learn_shift 255 freezes a foreground pixel's
// word).  A picture whose age is 0, or that the cut list names, is INITIALISED (b = c << 7, nothing is foreground); one younger than
// `warmup` calls LEARNS and nothing is foreground.  The foreground pixels of a cell are counted into a grid laid out as the
// change maps' and summed up as theirs (count in the place of the SAD), so regions and tracks consume both alike.  Integers only:
// no result depends on the order of anything.
//
// Two kernels.  k_bg_begin, one lane per picture: reads the head, the picture's word and the cut list, writes the mode and the
// new age into the head and clears the picture's summary -- no memset in front.  k_bg, one wave per workgroup, no barrier: the work
// items of k_change (a cell row x a segment of 1024 pixels; lane l takes the 16-pixel chunk of every row; items_per_wave items are
// summed before the three summary atomics).  Per chunk and row: 16 bytes of cur (change_load's paths; the right edge by bytes, the
// missing ones 0), two 16-byte loads and two 16-byte stores of state -- always whole and aligned, the reason for the padded row --
// and the pixel rule on packed 16-bit halves, two pixels per instruction: (c << 7) - b lies in -32640 .. 32640.  Rows go two at a
// time, their six loads in flight together.  A lane's counts per 8-pixel half go through LDS to the cell's lane as in change_wave.
// An initialising picture's state is not read at all.
//
// Padding words (columns W .. 16 * ceil(W / 16) - 1) see c = 0: written as 0 by an initialisation, and a 0 word under c = 0 never
// moves and is never foreground.  Whatever the words hold, the addresses depend on the geometry alone.
//
// Nothing wraps: a half's count is at most 8 * 64, a cell's 64 * 64, a wave's 16 * 1024 * 64 = 2^20; a packed accumulator's half
// at most 4 * 64.
//
// Written in the H263_HD style of change_kernel.inl: tests/sim_bg/ runs bg_begin, bg_wave and change_select lane by lane under g++
// (ASan / UBSan) over buffers of exactly the extents.
#pragma once

#include "change_kernel.inl"

namespace h263mi {

constexpr uint32_t BG_HEAD_BYTES = 64u;
constexpr uint32_t BG_KEEP = 255u;                       // fg_learn_shift: a foreground pixel keeps its word
constexpr uint64_t BG_GRID_MAX = 1u << 24;
enum : uint32_t {
    BG_MODE_VALID = 1u,
    BG_MODE_INIT = 2u,           // initialised in this call
    BG_MODE_WARM = 4u,           // warm-up: learning, nothing is foreground
};

static_assert(sizeof(h263mi_background_head) == BG_HEAD_BYTES, "the state's rows start 64 bytes behind its head");

struct BgArgs {
    const uint8_t *cur;
    uint8_t *state;              // picture p's at + p * state_stride: the head, then h rows of bpitch bytes
    uint8_t *mask;               // or nullptr
    uint64_t cur_pitch, cur_stride;
    uint64_t cur_set1;           // as ChangeArgs::cur_set1
    uint64_t state_stride;       // 64 + h * bpitch
    uint64_t mask_pitch, mask_stride;
    const uint32_t *words;       // one CHANGE_* word per picture (device), or nullptr: every picture is valid and in set 0
    const uint32_t *cut, *cut_count;     // both or neither
    uint32_t *cells;             // picture p's grid at + p * gw * gh, or nullptr
    h263mi_change_summary *summary;
    uint32_t w, h, gw, gh;
    uint32_t bpitch;             // 32 * ceil(w / 16)
    uint32_t cell_log2, threshold, n_pictures;
    uint32_t learn_shift, fg_learn_shift, pixel_threshold, warmup;
    uint32_t cur_align, mask_align;      // 16, 4 or 1 (change_align)
    uint32_t segs;               // ceil(w / CHANGE_SEG)
    uint32_t p0;                 // the launch's first picture (set by the launcher)
    uint32_t items_per_wave;     // (set by the launcher: change_items_per_wave)
    uint32_t pad;
};

inline uint32_t bg_pitch(uint32_t w) { return 32u * ((w + 15u) / 16u); }
inline uint64_t bg_stride(uint32_t w, uint32_t h) { return BG_HEAD_BYTES + (uint64_t)h * bg_pitch(w); }

// The launches of k_bg (HOST), as change_plan: `pictures` whole pictures at a time from p0 = 0 on, `waves` workgroups a picture,
// at most BG_GRID_MAX workgroups a launch.  items_per_wave: 0 = change_items_per_wave's (the launcher), another value the checker's.
struct BgLaunch {
    uint32_t waves, pictures;
};

inline bool bg_plan(BgArgs &a, BgLaunch &l, uint32_t items_per_wave = 0)
{
    if (a.n_pictures > CHANGE_MAX_PICTURES || a.cell_log2 < 3 || a.cell_log2 > 6 || !a.w || !a.h || a.w > 65535 || a.h > 65535 ||
        (uint64_t)a.w * a.h >= (1ull << 30) || !a.cur || !a.state || !a.summary || (uintptr_t)a.state % 32 || a.bpitch != bg_pitch(a.w) ||
        a.state_stride != bg_stride(a.w, a.h) || a.learn_shift > 7 || (a.fg_learn_shift > 7 && a.fg_learn_shift != BG_KEEP) ||
        a.pixel_threshold > 255 || !a.cut != !a.cut_count || a.gw != ((a.w - 1u) >> a.cell_log2) + 1u ||
        a.gh != ((a.h - 1u) >> a.cell_log2) + 1u || a.segs != (a.w + CHANGE_SEG - 1u) / CHANGE_SEG)
        return false;
    const uint32_t items = a.gh * a.segs;                              // of a picture (below 2^19: w * h < 2^30)
    a.items_per_wave = items_per_wave ? items_per_wave : change_items_per_wave((uint64_t)items * a.n_pictures);
    l.waves = (items + a.items_per_wave - 1u) / a.items_per_wave;
    l.pictures = (uint32_t)(BG_GRID_MAX / l.waves);
    return true;
}

// k_bg_begin's lane of picture p: the mode of this call and the new age into the head, the summary cleared
H263_HD void bg_begin(const BgArgs &a, uint32_t p)
{
    h263mi_change_summary *const out = a.summary + p;
    out->sad = 0;
    out->changed_cells = 0;
    out->max_cell_sad = 0;
    const uint32_t word = a.words ? a.words[p] : (uint32_t)CHANGE_VALID;
    if (!(word & CHANGE_VALID)) return;
    h263mi_background_head *const head = reinterpret_cast<h263mi_background_head *>(a.state + (uint64_t)p * a.state_stride);
    const uint32_t age = head->age;
    bool init = age == 0u;
    if (a.cut) {
        const uint32_t listed = a.cut_count[0] < a.n_pictures ? a.cut_count[0] : a.n_pictures;
        for (uint32_t k = 0; k < listed; k++) init |= a.cut[k] == p;
    }
    const bool warm = !init && age < a.warmup;
    head->age = init ? 1u : (age == 0xFFFFFFFFu ? age : age + 1u);
    head->mode = BG_MODE_VALID | (init ? (uint32_t)BG_MODE_INIT : 0u) | (warm ? (uint32_t)BG_MODE_WARM : 0u);
    for (int k = 0; k < 14; k++) head->reserved[k] = 0;
}

// arithmetic shift right of both halves by n (0 .. 15), a value of the wave
H263_DEV uint32_t bg_pk_ashr(uint32_t x, uint32_t n)
{
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t r;
    asm("v_pk_ashrrev_i16 %0, %1, %2 op_sel_hi:[0,1]" : "=v"(r) : "v"(n), "v"(x));
    return r;
#else
    const uint32_t lo = (uint32_t)((int16_t)(x & 0xffffu) >> n) & 0xffffu, hi = (uint32_t)((int16_t)(x >> 16) >> n) & 0xffffu;
    return lo | (hi << 16);
#endif
}

// what a wave's picture asks of every pixel (wave-uniform)
struct BgRule {
    uint32_t init;               // b' = c << 7, nothing is foreground, the state is not read
    uint32_t thr2;               // the pixel threshold in both halves; 255 in warm-up, which no |c - r| exceeds
    uint32_t s_bg, s_fg;         // the shifts
    uint32_t keep_fg;            // 0: a foreground pixel keeps its word; else all ones
    uint32_t want_mask;
};

// d >> s, but at least one towards c while d != 0: max(d >> s, min(d, 1)) -- a negative d never shifts to 0
H263_DEV uint32_t bg_step(uint32_t d, uint32_t s)
{
    const uint32_t floor = bg_pk_ashr(d, s);
    if (mutants::kBgStepFloor) return floor;
    return pk_max_i16(floor, pk_min_i16(d, 0x00010001u));
}

// two pixels: c2 their bytes and b2 their words, a half each -> the new words; fg01: 1 in the half of a foreground pixel
H263_DEV uint32_t bg_pair(uint32_t c2, uint32_t b2, const BgRule &q, uint32_t &fg01)
{
    const uint32_t d = pk_sub_u16(pk_lshl_u16(c2, 7), b2);
    const uint32_t step_bg = bg_step(d, q.s_bg);
    const uint32_t judged = mutants::kBgJudgeAfter ? pk_add_u16(b2, step_bg) : b2;
    const uint32_t r = pk_lshr_u16(pk_add_u16(judged, 0x00400040u), 7);
    const uint32_t dist = pk_max_i16(pk_sub_u16(c2, r), pk_sub_u16(r, c2));
    fg01 = pk_min_i16(pk_max_i16(pk_sub_u16(dist, q.thr2), 0u), 0x00010001u);
    const uint32_t full = pk_sub_u16(0u, fg01);                          // all ones in a foreground half
    const uint32_t step_fg = bg_step(d, q.s_fg) & q.keep_fg;
    return pk_add_u16(b2, (step_fg & full) | (step_bg & ~full));
}

// four pixels: c4 their bytes, b01 and b23 their words; acc += the verdicts (packed), -> their mask bytes
H263_DEV uint32_t bg_quad(uint32_t c4, uint32_t &b01, uint32_t &b23, const BgRule &q, uint32_t &acc)
{
    const uint32_t c01 = (c4 & 0xffu) | ((c4 & 0xff00u) << 8), c23 = ((c4 >> 16) & 0xffu) | ((c4 >> 8) & 0xff0000u);
    if (q.init) {
        b01 = pk_lshl_u16(c01, 7);
        b23 = pk_lshl_u16(c23, 7);
        return 0u;
    }
    uint32_t f01, f23;
    b01 = bg_pair(c01, b01, q, f01);
    b23 = bg_pair(c23, b23, q, f23);
    acc = pk_add_u16(acc, pk_add_u16(f01, f23));
    return ((f01 & 1u) | ((f01 >> 8) & 0x100u) | ((f23 & 1u) << 16) | ((f23 << 8) & 0x01000000u)) * 255u;
}

// the 16 pixels of a chunk: vc their bytes, s0 and s1 the words of pixels 0 .. 7 and 8 .. 15 -> the mask bytes
H263_DEV uint4 bg_chunk(const uint4 &vc, uint4 &s0, uint4 &s1, const BgRule &q, uint32_t &lo, uint32_t &hi)
{
    uint4 m;
    m.x = bg_quad(vc.x, s0.x, s0.y, q, lo);
    m.y = bg_quad(vc.y, s0.z, s0.w, q, lo);
    m.z = bg_quad(vc.z, s1.x, s1.y, q, hi);
    m.w = bg_quad(vc.w, s1.z, s1.w, q, hi);
    return m;
}

// R rows of a whole chunk, cur (and the mask) on 16-byte accesses: the 3 R loads are in flight together
template <uint32_t R>
H263_DEV void bg_rows_wide(const BgArgs &a, const BgRule &q, const uint8_t *pc, uint8_t *ps, uint8_t *pm, uint32_t &lo, uint32_t &hi)
{
    uint4 vc[R], s0[R], s1[R];
#pragma unroll
    for (uint32_t k = 0; k < R; k++) vc[k] = *reinterpret_cast<const uint4 *>(pc + (uint64_t)k * a.cur_pitch);
    if (!q.init) {
#pragma unroll
        for (uint32_t k = 0; k < R; k++) {
            s0[k] = *reinterpret_cast<const uint4 *>(ps + (uint64_t)k * a.bpitch);
            s1[k] = *reinterpret_cast<const uint4 *>(ps + (uint64_t)k * a.bpitch + 16u);
        }
    }
#pragma unroll
    for (uint32_t k = 0; k < R; k++) {
        const uint4 m = bg_chunk(vc[k], s0[k], s1[k], q, lo, hi);
        *reinterpret_cast<uint4 *>(ps + (uint64_t)k * a.bpitch) = s0[k];
        *reinterpret_cast<uint4 *>(ps + (uint64_t)k * a.bpitch + 16u) = s1[k];
        if (q.want_mask) *reinterpret_cast<uint4 *>(pm + (uint64_t)k * a.mask_pitch) = m;
    }
}

// One wave's work: the items first .. first + items_per_wave - 1 of picture p, numbered as change_wave's.  `each` as there.
template <class EachLane>
H263_HD void bg_wave(const BgArgs &a, ChangeLds &s, uint32_t p, uint32_t first, EachLane each)
{
    const uint32_t word = a.words ? a.words[p] : (uint32_t)CHANGE_VALID;
    if (!(word & CHANGE_VALID)) return;
    const uint32_t c = 1u << a.cell_log2, halves = c >> 3, in_seg = CHANGE_SEG >> a.cell_log2;
    const uint8_t *const cur_p = a.cur + (uint64_t)p * a.cur_stride + ((word & CHANGE_SET1) ? a.cur_set1 : 0u);
    uint8_t *const state_p = a.state + (uint64_t)p * a.state_stride;
    uint8_t *const mask_p = a.mask ? a.mask + (uint64_t)p * a.mask_stride : nullptr;
    const uint32_t mode = reinterpret_cast<const h263mi_background_head *>(state_p)->mode;       // (k_bg_begin's)
    BgRule q;
    q.init = (mode & BG_MODE_INIT) ? 1u : 0u;
    q.thr2 = ((mode & BG_MODE_WARM) ? 255u : a.pixel_threshold) * 0x00010001u;
    q.s_bg = a.learn_shift;
    q.s_fg = a.fg_learn_shift == BG_KEEP ? 0u : a.fg_learn_shift;
    q.keep_fg = a.fg_learn_shift == BG_KEEP ? 0u : 0xFFFFFFFFu;
    q.want_mask = mask_p ? 1u : 0u;
    const bool wide = a.cur_align == 16u && (!mask_p || a.mask_align == 16u);
    each([&](int, ChangeLane &t) { t.sad = t.changed = t.max = 0; });
    uint32_t cy = first / a.segs, seg = first - cy * a.segs;
    for (uint32_t i = 0; i < a.items_per_wave && cy < a.gh; i++) {
        const uint32_t y0 = cy << a.cell_log2, rows = a.h - y0 < c ? a.h - y0 : c, seg_x = seg * CHANGE_SEG;
        const uint8_t *const cur = cur_p + (uint64_t)y0 * a.cur_pitch;
        uint8_t *const state = state_p + BG_HEAD_BYTES + (uint64_t)y0 * a.bpitch;
        uint8_t *const mask = mask_p ? mask_p + (uint64_t)y0 * a.mask_pitch : nullptr;
        each([&](int lane, ChangeLane &) {
            const uint32_t x = seg_x + 16u * (uint32_t)lane;
            uint32_t lo = 0, hi = 0;                          // the verdicts of pixels x .. x + 7 and x + 8 .. x + 15, two sums each
            if (x < a.w) {
                const uint32_t nb = a.w - x < 16u ? a.w - x : 16u;
                const uint8_t *const pc = cur + x;
                uint8_t *const ps = state + 2u * x;
                uint8_t *const pm = mask ? mask + x : nullptr;
                uint32_t r = 0;
                if (nb == 16u && wide)
                    for (; r + 2u <= rows; r += 2u)
                        bg_rows_wide<2>(a, q, pc + (uint64_t)r * a.cur_pitch, ps + (uint64_t)r * a.bpitch,
                                        pm ? pm + (uint64_t)r * a.mask_pitch : nullptr, lo, hi);
                for (; r < rows; r++) {
                    uint4 *const qs = reinterpret_cast<uint4 *>(ps + (uint64_t)r * a.bpitch);
                    const uint4 vc = change_load(pc + (uint64_t)r * a.cur_pitch, nb, a.cur_align);
                    uint4 s0 = make_uint4(0u, 0u, 0u, 0u), s1 = s0;
                    if (!q.init) s0 = qs[0], s1 = qs[1];
                    const uint4 m = bg_chunk(vc, s0, s1, q, lo, hi);
                    qs[0] = s0;
                    qs[1] = s1;
                    if (pm) change_store(pm + (uint64_t)r * a.mask_pitch, m, nb, a.mask_align);
                }
            }
            s.half[2 * lane] = (lo & 0xffffu) + (lo >> 16);
            s.half[2 * lane + 1] = (hi & 0xffffu) + (hi >> 16);
        });
        wave_fence();
        // the segment's cells: cell j is made of the halves j * c/8 ...; its picture column is cell0 + j
        const uint32_t cell0 = seg_x >> a.cell_log2;
        const uint32_t n_cells = a.gw - cell0 < in_seg ? a.gw - cell0 : in_seg;
        uint32_t *const row = a.cells ? a.cells + (size_t)p * a.gw * a.gh + (size_t)cy * a.gw + cell0 : nullptr;
        each([&](int lane, ChangeLane &t) {
            for (uint32_t j = (uint32_t)lane; j < n_cells; j += 64u) {            // (a second turn when c = 8 only)
                uint32_t count = 0;
                for (uint32_t k = 0; k < halves; k++) count += s.half[j * halves + k];
                const uint32_t cx = cell0 + j, cw = a.w - (cx << a.cell_log2) < c ? a.w - (cx << a.cell_log2) : c;
                if (row) row[j] = count;
                t.sad += count;
                t.changed += change_judge(count, a.cell_log2, a.threshold, cw * rows) ? 1u : 0u;
                t.max = count > t.max ? count : t.max;
            }
        });
        wave_fence();                                        // (the next item overwrites the halves)
        if (++seg == a.segs) seg = 0, cy++;
    }
    // the wave's terms: every lane's, then the sums of eight lanes each, then lane 0 adds (as change_wave)
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
            if (sad) change_add64(&out->sad, sad);               // (no foreground pixel: no changed cell, no maximum)
            if (changed) change_add32(&out->changed_cells, changed);
            if (mx) change_max32(&out->max_cell_sad, mx);
        }
    });
}

}  // namespace h263mi
