// regions_kernel.inl -- k_regions, k_regions_pack: the changed cells of a change map's grids as a device table of ROI boxes
// (h263mi_regions_on, h263mi_batch_regions; ABI 7).
//
// The contract (include/h263mi.h): a grid of gw x gh uint32 cell SADs per picture, as k_change writes them; a cell is CHANGED by
// change_judge (change_kernel.inl); a COMPONENT is a maximal set of changed cells connected over edges (connectivity 4) or edges
// and corners (8); its label is its smallest raster index, its cells their count, its sad their sum.  Components of at least
// min_cells cells are KEPT, the first max_per_picture of them in label order are EMITTED as boxes (cell bounding box, grown by
// margin_cells, clipped, in pixels) with their stats.
//
// k_regions: one workgroup of REGIONS_THREADS threads per picture, the whole grid in LDS: a 16-bit parent per cell (REGIONS_NONE:
// not changed) and a 16-bit count per cell -- 128 KiB at the cap of 2^15 cells.  The labelling is union-find, not propagation, so a
// path of thousands of cells costs no more than a blob:
//   1. judge: thread t takes the cells t, t + 1024, ...; within the 64 cells of a wave a changed cell's parent is the first cell of
//      its row run inside those 64 (a ballot of the run starts), so runs are flat from the start;
//   2. hook: a run that goes on across a wave's 64 cells is united with its left part, a changed cell with its changed neighbours
//      in the row above -- only those that the cell's and the neighbour's runs do not connect already.  regions_union finds both
//      roots (halving the paths it walks) and hooks the larger root under the smaller with a 16-bit atomic minimum (a compare-and-
//      swap of the 32-bit word that holds it); parents only ever decrease, so a root is the smallest index of its tree;
//   3. flatten and count: every changed cell walks to its root, points every cell on its way at it and adds one to the root's
//      count;
//   4. rank: the roots, 1024 cells a step in raster order, are counted by ballots; a kept root's rank among the kept ones is its
//      place in label order; one of the first max_per_picture takes a slot, and its count cell now holds the slot's number;
//   5. every changed cell of an emitted component adds its SAD and its column and row to the slot (LDS atomics);
//   6. thread k writes slot k's box and stat to the picture's staging slice of d_work, thread 0 the picture's components and kept.
// A picture whose summary has changed_cells == 0 is not read: its info is zero.
//
// k_regions_pack: one wave.  The exclusive prefix of min(kept, max_per_picture) over the pictures, 64 a step, gives first and
// written; the staged entries are copied to their places, the rest of the table is written as invalid entries, the two count words
// last.
//
// Nothing wraps: a cell index and a count are at most 2^15; a component's sad is summed in 64 bits; (cx1 + 1) * c <= 65536 + 63.
//
// Written in the H263_HD style of change_kernel.inl: tests/sim_regions/ runs regions_picture and regions_pack thread by thread
// under g++ (ASan / UBSan) over buffers of exactly their extents.  `each(f)` runs f(thread, thread_state) for the threads this
// thread stands for: its own on the GPU, all of the workgroup in turn in the CPU checker -- one interleaving of the many the
// device may take, every phase being correct under any.  Everything outside `each` is uniform over the workgroup.
#pragma once

#include "change_kernel.inl"

namespace h263mi {

constexpr uint32_t REGIONS_MAX_CELLS = H263MI_REGIONS_MAX_CELLS;
constexpr uint32_t REGIONS_THREADS = 1024u, REGIONS_WAVES = REGIONS_THREADS / 64u;
constexpr uint32_t REGIONS_MAX_PER_PICTURE = 256u, REGIONS_MAX_MARGIN = 8u, REGIONS_MAX_ROIS = 65535u;
constexpr uint32_t REGIONS_NONE = 0xFFFFu;               // a parent: the cell is not changed; a count cell: no slot
constexpr uint32_t REGIONS_ENTRY = 32u;                  // bytes of a staged entry in d_work: the h263mi_roi, then the h263mi_region_stat

static_assert(REGIONS_MAX_CELLS <= 32768u && REGIONS_MAX_CELLS % 2u == 0, "parents and counts are 16-bit, two to a word");
static_assert(sizeof(h263mi_roi) == 16 && sizeof(h263mi_region_stat) == 16 && sizeof(h263mi_region_info) == 16,
              "a staged entry is two 16-byte records");

struct RegionsArgs {
    const uint32_t *cells;                   // picture p's grid at + p * gw * gh
    const h263mi_change_summary *summary;    // or nullptr
    uint8_t *work;                           // picture p's staging slice at + p * max_per * REGIONS_ENTRY
    h263mi_region_info *info;
    uint32_t w, h, gw, gh;
    uint32_t cell_log2, connectivity, margin, threshold;
    uint32_t min_cells, max_per, n_pictures, pad;
};

struct RegionsPackArgs {
    const h263mi_change_summary *summary;    // or nullptr
    const uint8_t *work;
    h263mi_roi *rois;
    h263mi_region_stat *stats;               // or nullptr
    h263mi_region_info *info;
    uint32_t *count;
    uint32_t n_pictures, max_per, max_rois, pad;
};

// two 16-bit values to a word: the halves are read and written as such, the atomics work on the words
union RegionsHalves {
    uint16_t h[REGIONS_MAX_CELLS];
    uint32_t w[REGIONS_MAX_CELLS / 2u];
};

struct RegionsLds {
    RegionsHalves parent, count;
    uint64_t sad[REGIONS_MAX_PER_PICTURE];
    uint32_t x0[REGIONS_MAX_PER_PICTURE], y0[REGIONS_MAX_PER_PICTURE], x1[REGIONS_MAX_PER_PICTURE], y1[REGIONS_MAX_PER_PICTURE];
    uint32_t cells[REGIONS_MAX_PER_PICTURE], label[REGIONS_MAX_PER_PICTURE];
    unsigned long long vote[2][2][REGIONS_WAVES];        // [step parity][which ballot][wave]
};

struct RegionsLane {
    bool on, start, root, kept;
};

struct RegionsPackLds {
    uint32_t e[64], first[64], written[64];
};

struct RegionsPackLane {
    uint32_t e;
    bool skipped;
};

// A barrier of the workgroup between two phases (the checker runs a phase's threads to the end before the next phase begins)
H263_HD void regions_sync()
{
#if defined(__HIP_DEVICE_COMPILE__)
    __syncthreads();
#endif
}

H263_HD uint32_t regions_ld(const uint16_t *p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __atomic_load_n(p, __ATOMIC_RELAXED);
#else
    return *p;
#endif
}
H263_HD void regions_st(uint16_t *p, uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    __atomic_store_n(p, (uint16_t)v, __ATOMIC_RELAXED);
#else
    *p = (uint16_t)v;
#endif
}

H263_HD uint32_t regions_ld32(const uint32_t *p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __atomic_load_n(p, __ATOMIC_RELAXED);
#else
    return *p;
#endif
}

// parent[i] = min(parent[i], v), atomically; -> what it held
H263_HD uint32_t regions_min16(RegionsHalves &a, uint32_t i, uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t *const wp = &a.w[i >> 1];
    const uint32_t sh = (i & 1u) * 16u;
    uint32_t old = __atomic_load_n(wp, __ATOMIC_RELAXED);
    for (;;) {
        const uint32_t cur = (old >> sh) & 0xFFFFu;
        if (cur <= v) return cur;
        const uint32_t seen = atomicCAS(wp, old, (old & ~(0xFFFFu << sh)) | (v << sh));
        if (seen == old) return cur;
        old = seen;
    }
#else
    const uint32_t cur = a.h[i];
    if (v < cur) a.h[i] = (uint16_t)v;
    return cur;
#endif
}

// count[i] += 1 (no count passes 2^15: nothing carries into the other half)
H263_HD void regions_inc16(RegionsHalves &a, uint32_t i)
{
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(&a.w[i >> 1], 1u << ((i & 1u) * 16u));
#else
    a.h[i]++;
#endif
}

H263_HD void regions_add64(uint64_t *p, uint64_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v);
#else
    *p += v;
#endif
}
H263_HD void regions_min32(uint32_t *p, uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMin(p, v);
#else
    if (v < *p) *p = v;
#endif
}

// The root of changed cell x.  Parents only decrease and a cell that has a parent never becomes a root again, so the walk ends; on
// its way every cell it leaves is pointed at its grandparent (a store that may undo a concurrent hook of a cell that was no root
// any more: regions_union goes on from the parent it saw, so nothing is lost).
H263_HD uint32_t regions_find(RegionsLds &s, uint32_t x)
{
    for (;;) {
        const uint32_t p = regions_ld(&s.parent.h[x]);
        if (p == x) return x;
        const uint32_t g = regions_ld(&s.parent.h[p]);
        if (g != p) regions_st(&s.parent.h[x], g);
        x = g;
    }
}

// The root of changed cell x, nothing stored: for the phase behind the hooks, where the roots are final and a thread may store
// nothing but a cell's final root -- a grandparent read earlier and stored late would undo another thread's flattening.
H263_HD uint32_t regions_root(RegionsLds &s, uint32_t x)
{
    for (;;) {
        const uint32_t p = regions_ld(&s.parent.h[x]);
        if (p == x) return x;
        x = p;
    }
}

// a and b, changed cells, belong to one component
H263_HD void regions_union(RegionsLds &s, uint32_t a, uint32_t b)
{
    for (;;) {
        a = regions_find(s, a);
        b = regions_find(s, b);
        if (a == b) return;
        if (a < b) {
            const uint32_t t = a;
            a = b, b = t;
        }
        const uint32_t old = regions_min16(s.parent, a, b);          // a > b: hook a under b, if a is still a root
        if (old == a) return;
        a = old;                                                     // it was not: unite what it hung on with b
    }
}

// One thread's vote, collected per wave: the GPU's ballot, the checker's bit by bit (votes cleared in front)
H263_HD void regions_vote(unsigned long long *votes, int tid, bool v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const unsigned long long m = __builtin_amdgcn_ballot_w64(v);
    if ((tid & 63) == 0) votes[tid >> 6] = m;
#else
    if (v) votes[tid >> 6] |= 1ull << (tid & 63);
#endif
}
H263_HD void regions_votes_clear(RegionsLds &s, uint32_t parity)
{
#if !defined(__HIP_DEVICE_COMPILE__)
    for (uint32_t k = 0; k < REGIONS_WAVES; k++) s.vote[parity][0][k] = s.vote[parity][1][k] = 0;
#else
    (void)s, (void)parity;
#endif
}

H263_HD bool regions_judge(const RegionsArgs &a, const uint32_t *grid, uint32_t cy, uint32_t cx)
{
    const uint32_t c = 1u << a.cell_log2;
    const uint32_t cw = a.w - (cx << a.cell_log2) < c ? a.w - (cx << a.cell_log2) : c;
    const uint32_t ch = a.h - (cy << a.cell_log2) < c ? a.h - (cy << a.cell_log2) : c;
    return change_judge(grid[(size_t)cy * a.gw + cx], a.cell_log2, a.threshold, cw * ch);
}

// The workgroup of picture p.
template <class EachThread>
H263_HD void regions_picture(const RegionsArgs &a, RegionsLds &s, uint32_t p, EachThread each)
{
    h263mi_region_info *const info = a.info + p;
    if (a.summary && a.summary[p].changed_cells == 0) {
        each([&](int tid, RegionsLane &) {
            if (tid == 0) info->components = info->kept = 0;
        });
        return;
    }
    const uint32_t n = a.gw * a.gh, gw = a.gw;
    const uint32_t *const grid = a.cells + (size_t)p * n;
    auto on = [&](uint32_t j) { return regions_ld(&s.parent.h[j]) != REGIONS_NONE; };

    // 1. judge; flat row runs inside a wave's 64 cells
    for (uint32_t base = 0, step = 0; base < n; base += REGIONS_THREADS, step++) {
        regions_votes_clear(s, step & 1u);
        each([&](int tid, RegionsLane &t) {
            const uint32_t i = base + (uint32_t)tid;
            t.on = t.start = false;
            if (i < n) {
                const uint32_t cy = i / gw, cx = i - cy * gw;
                t.on = regions_judge(a, grid, cy, cx);
                t.start = t.on && ((tid & 63) == 0 || cx == 0 || !regions_judge(a, grid, cy, cx - 1u));
                s.count.h[i] = 0;
            }
            regions_vote(s.vote[step & 1u][0], tid, t.start);
        });
        regions_sync();
        each([&](int tid, RegionsLane &t) {
            const uint32_t i = base + (uint32_t)tid, lane = (uint32_t)tid & 63u;
            if (i < n) {
                const unsigned long long m = s.vote[step & 1u][0][tid >> 6] & (~0ull >> (63u - lane));   // the starts at or below
                s.parent.h[i] = (uint16_t)(t.on ? i - lane + (63u - (uint32_t)__builtin_clzll(m)) : REGIONS_NONE);
            }
        });
    }
    regions_sync();

    // 2. hook: runs across the 64s, and the row above
    for (uint32_t base = 0; base < n; base += REGIONS_THREADS) {
        each([&](int tid, RegionsLane &) {
            const uint32_t i = base + (uint32_t)tid;
            if (i >= n || !on(i)) return;
            const uint32_t cy = i / gw, cx = i - cy * gw;
            const bool left = cx > 0 && on(i - 1u);
            if ((tid & 63) == 0 && left) regions_union(s, i, i - 1u);
            if (cy == 0) return;
            const uint32_t up = i - gw;
            const bool up_left = cx > 0 && on(up - 1u);
            if (on(up)) {
                if (!(left && up_left)) regions_union(s, i, up);     // (else the cell on the left has united the two runs)
            } else if (a.connectivity == 8u) {
                const bool right = cx + 1u < gw && on(i + 1u);
                if (up_left && !left) regions_union(s, i, up - 1u);  // (else the cell on the left lies under it)
                if (!mutants::kRegionsDiagonal && cx + 1u < gw && on(up + 1u) && !right) regions_union(s, i, up + 1u);
            }
        });
    }
    regions_sync();

    // 3. flatten and count
    for (uint32_t base = 0; base < n; base += REGIONS_THREADS) {
        each([&](int tid, RegionsLane &) {
            const uint32_t i = base + (uint32_t)tid;
            if (i >= n || !on(i)) return;
            const uint32_t r = regions_root(s, i);
            for (uint32_t y = i; y != r;) {                          // (every store of this phase is the cell's final root)
                const uint32_t next = regions_ld(&s.parent.h[y]);
                regions_st(&s.parent.h[y], r);
                y = next;
            }
            regions_inc16(s.count, r);
        });
    }
    regions_sync();

    // 4. rank the roots in raster order; the first max_per kept ones take the slots
    uint32_t components = 0, kept = 0;
    for (uint32_t base = 0, step = 0; base < n; base += REGIONS_THREADS, step++) {
        unsigned long long(*const vote)[REGIONS_WAVES] = s.vote[step & 1u];
        regions_votes_clear(s, step & 1u);
        each([&](int tid, RegionsLane &t) {
            const uint32_t i = base + (uint32_t)tid;
            t.root = i < n && s.parent.h[i] == i;
            t.kept = t.root && s.count.h[i] >= a.min_cells;
            regions_vote(vote[0], tid, t.root);
            regions_vote(vote[1], tid, t.kept);
        });
        regions_sync();
        each([&](int tid, RegionsLane &t) {
            if (!t.root) return;
            const uint32_t i = base + (uint32_t)tid, wave = (uint32_t)tid >> 6;
            uint32_t slot = REGIONS_NONE;
            if (t.kept) {
                uint32_t rank = kept + (uint32_t)__builtin_popcountll(vote[1][wave] & ((1ull << (tid & 63)) - 1ull));
                for (uint32_t k = 0; k < wave; k++) rank += (uint32_t)__builtin_popcountll(vote[1][k]);
                if (rank < a.max_per) {
                    slot = rank;
                    s.sad[slot] = 0;
                    s.x0[slot] = s.y0[slot] = 0xFFFFFFFFu;
                    s.x1[slot] = s.y1[slot] = 0;
                    s.cells[slot] = s.count.h[i];
                    s.label[slot] = i;
                }
            }
            s.count.h[i] = (uint16_t)slot;
        });
        for (uint32_t k = 0; k < REGIONS_WAVES; k++) {
            components += (uint32_t)__builtin_popcountll(vote[0][k]);
            kept += (uint32_t)__builtin_popcountll(vote[1][k]);
        }
    }
    regions_sync();
    const uint32_t emitted = kept < a.max_per ? kept : a.max_per;

    // 5. the emitted components' sums and bounds
    if (emitted) {
        for (uint32_t base = 0; base < n; base += REGIONS_THREADS) {
            each([&](int tid, RegionsLane &) {
                const uint32_t i = base + (uint32_t)tid;
                if (i >= n) return;
                const uint32_t r = s.parent.h[i];
                if (r == REGIONS_NONE) return;
                const uint32_t slot = s.count.h[r];
                if (slot == REGIONS_NONE) return;
                const uint32_t cy = i / gw, cx = i - cy * gw;
                regions_add64(&s.sad[slot], grid[i]);
                // (a bound only ever moves outwards: a cell inside what it reads needs no atomic -- most cells of a large component)
                if (cx < regions_ld32(&s.x0[slot])) regions_min32(&s.x0[slot], cx);
                if (cy < regions_ld32(&s.y0[slot])) regions_min32(&s.y0[slot], cy);
                if (cx > regions_ld32(&s.x1[slot])) change_max32(&s.x1[slot], cx);
                if (cy > regions_ld32(&s.y1[slot])) change_max32(&s.y1[slot], cy);
            });
        }
        regions_sync();
    }

    // 6. the staged entries, the picture's counts
    each([&](int tid, RegionsLane &) {
        if (tid == 0) info->components = components, info->kept = kept;
        const uint32_t k = (uint32_t)tid;
        if (k >= emitted) return;
        const uint32_t cx0 = s.x0[k] > a.margin ? s.x0[k] - a.margin : 0u, cy0 = s.y0[k] > a.margin ? s.y0[k] - a.margin : 0u;
        const uint32_t cx1 = s.x1[k] + a.margin < gw ? s.x1[k] + a.margin : gw - 1u;
        const uint32_t cy1 = s.y1[k] + a.margin < a.gh ? s.y1[k] + a.margin : a.gh - 1u;
        const uint32_t x = cx0 << a.cell_log2, y = cy0 << a.cell_log2;
        uint32_t right = (cx1 + 1u) << a.cell_log2, bottom = (cy1 + 1u) << a.cell_log2;
        if (!mutants::kRegionsBoxClip) {
            right = right < a.w ? right : a.w;
            bottom = bottom < a.h ? bottom : a.h;
        }
        uint8_t *const e = a.work + ((size_t)p * a.max_per + k) * REGIONS_ENTRY;
        h263mi_roi roi;
        roi.picture = p;
        roi.x = (uint16_t)x, roi.y = (uint16_t)y, roi.w = (uint16_t)(right - x), roi.h = (uint16_t)(bottom - y);
        roi.reserved = 0;
        h263mi_region_stat st;
        st.sad = s.sad[k], st.cells = s.cells[k], st.label = s.label[k];
        *reinterpret_cast<h263mi_roi *>(e) = roi;
        *reinterpret_cast<h263mi_region_stat *>(e + sizeof(h263mi_roi)) = st;
    });
}

// The one wave of k_regions_pack.
template <class EachLane>
H263_HD void regions_pack(const RegionsPackArgs &f, RegionsPackLds &s, EachLane each)
{
    uint32_t total = 0;                                      // (at most 65535 * 256)
    for (uint32_t base = 0; base < f.n_pictures; base += 64u) {
        each([&](int lane, RegionsPackLane &t) {
            const uint32_t p = base + (uint32_t)lane;
            t.e = 0;
            t.skipped = p < f.n_pictures && f.summary && f.summary[p].changed_cells == 0;
            if (p < f.n_pictures && !t.skipped) t.e = f.info[p].kept < f.max_per ? f.info[p].kept : f.max_per;
            s.e[lane] = t.e;
        });
        wave_fence();
        each([&](int lane, RegionsPackLane &t) {
            const uint32_t p = base + (uint32_t)lane;
            uint32_t before = total;
            for (int k = 0; k < lane; k++) before += s.e[k];
            const uint32_t first = t.skipped ? 0u : (before < f.max_rois ? before : f.max_rois);
            const uint32_t written = t.e < f.max_rois - first ? t.e : f.max_rois - first;
            s.first[lane] = first, s.written[lane] = written;
            if (p < f.n_pictures) f.info[p].first = first, f.info[p].written = written;
        });
        wave_fence();
        for (uint32_t q = 0; q < 64u && base + q < f.n_pictures; q++) {
            total += s.e[q];
            const uint32_t written = s.written[q], first = s.first[q];
            if (!written) continue;
            const uint8_t *const src = f.work + (size_t)(base + q) * f.max_per * REGIONS_ENTRY;
            each([&](int lane, RegionsPackLane &) {
                for (uint32_t k = (uint32_t)lane; k < written; k += 64u) {
                    const uint8_t *const e = src + (size_t)k * REGIONS_ENTRY;
                    f.rois[first + k] = *reinterpret_cast<const h263mi_roi *>(e);
                    if (f.stats) f.stats[first + k] = *reinterpret_cast<const h263mi_region_stat *>(e + sizeof(h263mi_roi));
                }
            });
        }
        wave_fence();                                        // (the next step overwrites the hand-offs)
    }
    const uint32_t count = total < f.max_rois ? total : f.max_rois;
    each([&](int lane, RegionsPackLane &) {
        for (uint32_t j = count + (uint32_t)lane; j < f.max_rois; j += 64u) {
            h263mi_roi none;
            none.picture = 0xFFFFFFFFu;
            none.x = none.y = none.w = none.h = 0;
            none.reserved = 1;
            f.rois[j] = none;
            if (f.stats) {
                h263mi_region_stat zero;
                zero.sad = 0, zero.cells = zero.label = 0;
                f.stats[j] = zero;
            }
        }
        if (lane == 0) f.count[0] = count, f.count[1] = total;
    });
}

}  // namespace h263mi
