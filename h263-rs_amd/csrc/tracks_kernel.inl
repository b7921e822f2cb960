// tracks_kernel.inl -- k_tracks, k_tracks_pack: a device-resident table of tracks per picture, updated from a table of ROI boxes by
// greedy IoU matching, and the table of the tracks worth cropping (h263mi_tracks_on, h263mi_batch_tracks; ABI 7).
//
// The contract (include/h263mi.h): picture p's state is a h263mi_track_head and max_tracks h263mi_track slots.  One call per
// picture: a cut kills every live track; the valid entries of the picture's slice of d_rois, the first 256 of them, are the
// DETECTIONS; live tracks and detections are matched greedily by intersection over union, compared in integers; a matched track
// moves to its detection, an unmatched one ages and dies behind max_missed misses; unmatched detections are born into the free
// slots; a track born or matched is EMITTED by min_hits and emit_period.
//
// k_tracks: one workgroup of TRACKS_THREADS = 256 threads per picture.  Thread i is slot i and, in the matching, also detection i.
// The boxes, areas and partners of up to 256 tracks and 256 detections lie in LDS (sizeof(TracksLds), about 10 KiB):
//   0. load: thread i reads slot i and judges it (live: id != 0 and a valid box);
//   1. cut: the list, 256 entries a step, is compared with p; a hit raises a flag;
//   2. gather: the slice, 256 entries a step, is judged; a ballot's prefix gives a valid entry its place among the detections, so
//      table order is kept; the loop ends with the slice or the 256th detection;
//   3. match, in rounds of MUTUAL BEST: every unmatched track scans the unmatched detections for its best eligible pair, every
//      unmatched detection the unmatched tracks; a pair that chose each other is matched; rounds go on until one matches nothing.
//      A choice is kept from round to round while its partner is free -- the sets only shrink, so it is still the best.
//   4. update, deaths;  5. births: ballots of the free slots and of the unmatched detections, the k-th free slot takes the k-th
//      unmatched detection, so both orders are kept;  6. the emitted flag; every slot and the head are written back.
//
// Why mutual best is the greedy matching.  "Better" (more intersection over union, then the smaller slot, then the smaller
// detection) is a strict total order of the eligible pairs.  The greedy matching G(S) of a set S of pairs walks S from best to worst
// and takes a pair when its track and its detection are both free.  Let (i, j) in S be mutual best: no pair of S with track i or with
// detection j is better.  Then (a) greedy takes (i, j): every pair in front of it holds neither i nor j, so both are free when its
// turn comes; (b) greedy takes no other pair of i or of j, all of them come later; (c) what greedy decides about the pairs that
// hold neither i nor j does not depend on (i, j).  So G(S) = {(i, j)} + G(S without the pairs of i and of j), and the same for all
// mutual-best pairs of S at once, since they share no track and no detection.  A round therefore takes pairs of G only, and
// leaves a set whose greedy matching is the rest of G.  The best pair of a non-empty S is mutual best, so every round but the
// last takes at least one pair: at most min(tracks, detections) + 1 rounds, 257 for a chain in which track k prefers detection
// k - 1 and settles for k.
//
// k_tracks_pack: one wave.  k_tracks leaves a picture's emitted count in its info's `written`; the exclusive prefix of these, 64
// pictures a step, gives first and written; the emitted slots are copied straight from the state into the table in slot order (a
// ballot of the emitted flags, 64 slots a step), the rest of the table is written as invalid entries, the two count words last.
//
// Nothing wraps: a box lies inside W x H < 2^30, so an intersection and an area are below 2^30, a union below 2^31, inter * 1000
// and inter * union' below 2^61; a rank is at most 256; first + k is below n_rois <= 65535.
//
// Written in the H263_HD style of regions_kernel.inl, whose barrier and ballot helpers it uses: tests/sim_tracks/ runs
// tracks_picture and tracks_pack thread by thread under g++ (ASan / UBSan) over buffers of exactly their extents.  Everything
// outside `each` is uniform over the workgroup.
#pragma once

#include "regions_kernel.inl"

namespace h263mi {

constexpr uint32_t TRACKS_THREADS = 256u, TRACKS_WAVES = TRACKS_THREADS / 64u;
constexpr uint32_t TRACKS_MAX = 256u;                    // slots, and detections, of a picture
constexpr uint32_t TRACKS_MAX_ROIS = 65535u, TRACKS_MAX_OUT = 65535u, TRACKS_MAX_PICTURES = 65535u;
constexpr uint32_t TRACKS_NONE = 0xFFFFu;                // a partner: none yet; a choice: nothing eligible is left
constexpr uint32_t TRACKS_DEAD = 0xFFFEu;                // a track's partner: the slot holds no live track
constexpr uint32_t TRACKS_UNSCANNED = 0xFFFDu;           // a choice: not looked for yet
constexpr uint32_t TRACKS_BORN = 1u, TRACKS_MATCHED = 2u, TRACKS_EMITTED = 4u;
constexpr uint32_t TRACKS_NO_DET = 0xFFFFFFFFu;

static_assert(TRACKS_THREADS == TRACKS_MAX, "thread i is slot i and detection i");
static_assert(sizeof(h263mi_track) == 32 && sizeof(h263mi_track_head) == 32 && sizeof(h263mi_track_info) == 32 &&
              sizeof(h263mi_track_ref) == 16 && sizeof(h263mi_tracks) == 16, "the records are part of the ABI");

struct TracksArgs {
    const h263mi_roi *rois;                  // n_rois entries (nullptr with none)
    const h263mi_region_info *info_in;       // picture p's slice of rois
    uint8_t *state;                          // picture p's head and slots at + p * tracks_stride(max_tracks)
    const uint32_t *cut, *cut_count;         // both or neither
    h263mi_track_info *info;
    uint32_t n_rois, n_pictures, w, h;
    uint32_t max_tracks, iou_permille, max_missed, min_hits;
    uint32_t emit_period, pad;
};

struct TracksPackArgs {
    const uint8_t *state;
    h263mi_roi *rois;
    h263mi_track_ref *refs;                  // or nullptr
    h263mi_track_info *info;
    uint32_t *count;
    uint32_t n_pictures, max_tracks, max_out, pad;
};

H263_HD size_t tracks_stride(uint32_t max_tracks) { return sizeof(h263mi_track_head) + (size_t)max_tracks * sizeof(h263mi_track); }

struct TracksBox {
    uint16_t x, y, w, h;
};

// the ballots of a picture, one array of a word per wave each
enum : uint32_t {
    TRACKS_V_LIVE0,              // live at load
    TRACKS_V_DIED,               // died of misses
    TRACKS_V_FREE,               // a slot that a birth may take
    TRACKS_V_UNMATCHED,          // a detection without a track
    TRACKS_V_LIVE,               // live at the end
    TRACKS_V_STEP,               // + parity: a step of the gather, a round of the matching
    TRACKS_VOTES = TRACKS_V_STEP + 2u
};

struct TracksLds {
    TracksBox tbox[TRACKS_MAX], dbox[TRACKS_MAX];
    uint32_t tarea[TRACKS_MAX], darea[TRACKS_MAX];
    uint32_t didx[TRACKS_MAX];                           // a detection's index in rois
    uint16_t tp[TRACKS_MAX], dp[TRACKS_MAX];             // partners: a track's detection, a detection's track
    uint16_t tb[TRACKS_MAX], db[TRACKS_MAX];             // this round's choices
    uint16_t born[TRACKS_MAX];                           // the k-th unmatched detection
    unsigned long long vote[TRACKS_VOTES][TRACKS_WAVES];
    uint32_t cut;
};

struct TracksLane {
    uint32_t id, age, hits, missed, flags, det;
    TracksBox box;
    h263mi_roi q;
    uint32_t tb, db;                                     // the kept choices of track tid and of detection tid
    bool slot, live0, live, ok, free, unmatched;
};

struct TracksPackLds {
    uint32_t e[64], first[64], written[64];
    unsigned long long vote[2][1];
};

struct TracksPackLane {
    uint32_t e;
    bool emitted;
};

H263_HD void tracks_votes_clear(unsigned long long *votes, uint32_t waves)
{
#if !defined(__HIP_DEVICE_COMPILE__)
    for (uint32_t k = 0; k < waves; k++) votes[k] = 0;   // (the checker's votes are set bit by bit)
#else
    (void)votes, (void)waves;
#endif
}

H263_HD uint32_t tracks_count(const unsigned long long *votes)
{
    uint32_t n = 0;
    for (uint32_t k = 0; k < TRACKS_WAVES; k++) n += (uint32_t)__builtin_popcountll(votes[k]);
    return n;
}

// the votes of the threads below tid
H263_HD uint32_t tracks_prefix(const unsigned long long *votes, int tid)
{
    uint32_t n = (uint32_t)__builtin_popcountll(votes[tid >> 6] & ((1ull << (tid & 63)) - 1ull));
    for (int k = 0; k < (tid >> 6); k++) n += (uint32_t)__builtin_popcountll(votes[k]);
    return n;
}

H263_HD void tracks_raise(uint32_t *flag)
{
#if defined(__HIP_DEVICE_COMPILE__)
    __atomic_store_n(flag, 1u, __ATOMIC_RELAXED);
#else
    *flag = 1u;
#endif
}

H263_HD bool tracks_box_valid(uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint32_t W, uint32_t H)
{
    return w >= 1u && h >= 1u && x + w <= W && y + h <= H;
}

H263_HD uint32_t tracks_inter(const TracksBox &a, const TracksBox &b)
{
    const uint32_t x0 = a.x > b.x ? a.x : b.x, y0 = a.y > b.y ? a.y : b.y;
    const uint32_t ax1 = (uint32_t)a.x + a.w, bx1 = (uint32_t)b.x + b.w, ay1 = (uint32_t)a.y + a.h, by1 = (uint32_t)b.y + b.h;
    const uint32_t x1 = ax1 < bx1 ? ax1 : bx1, y1 = ay1 < by1 ? ay1 : by1;
    return x1 > x0 && y1 > y0 ? (x1 - x0) * (y1 - y0) : 0u;
}

H263_HD bool tracks_eligible(uint32_t inter, uint32_t uni, uint32_t permille)
{
    return inter >= 1u && (uint64_t)inter * 1000u >= (uint64_t)permille * uni;
}

// inter / uni > inter2 / uni2, exactly
H263_HD bool tracks_better(uint32_t inter, uint32_t uni, uint32_t inter2, uint32_t uni2)
{
    if (mutants::kTracksFloatIou) return (float)inter / (float)uni > (float)inter2 / (float)uni2;
    return (uint64_t)inter * uni2 > (uint64_t)inter2 * uni;
}

// n + k for k <= 256, going from 0xFFFFFFFF to 1
H263_HD uint32_t tracks_id(uint32_t n, uint32_t k)
{
    const uint64_t v = (uint64_t)n + k;
    return (uint32_t)(v > 0xFFFFFFFFull ? v - 0xFFFFFFFFull : v);
}

H263_HD uint32_t tracks_inc(uint32_t v) { return v == 0xFFFFFFFFu ? v : v + 1u; }

// The workgroup of picture p.
template <class EachThread>
H263_HD void tracks_picture(const TracksArgs &a, TracksLds &s, uint32_t p, EachThread each)
{
    uint8_t *const base = a.state + (size_t)p * tracks_stride(a.max_tracks);
    h263mi_track_head *const head = reinterpret_cast<h263mi_track_head *>(base);
    h263mi_track *const slots = reinterpret_cast<h263mi_track *>(base + sizeof(h263mi_track_head));
    const uint32_t next0 = head->next_id ? head->next_id : 1u, calls0 = head->calls;     // (thread 0 writes the head in the last phase)
    const h263mi_region_info in = a.info_in[p];
    for (uint32_t k = 0; k < TRACKS_VOTES; k++) tracks_votes_clear(s.vote[k], TRACKS_WAVES);

    // 0. load
    each([&](int tid, TracksLane &t) {
        t.id = t.age = t.hits = t.missed = t.flags = 0;
        t.det = TRACKS_NO_DET;
        t.box = TracksBox{0, 0, 0, 0};
        t.tb = t.db = TRACKS_UNSCANNED;
        t.slot = (uint32_t)tid < a.max_tracks;
        t.live0 = false;
        if (t.slot) {
            const h263mi_track r = slots[tid];
            if (r.id != 0 && tracks_box_valid(r.x, r.y, r.w, r.h, a.w, a.h)) {
                t.live0 = true;
                t.id = r.id, t.age = r.age, t.hits = r.hits, t.missed = r.missed;
                t.box = TracksBox{r.x, r.y, r.w, r.h};
            }
        }
        if (tid == 0) s.cut = 0;
        regions_vote(s.vote[TRACKS_V_LIVE0], tid, t.live0);
    });
    regions_sync();

    // 1. cut
    if (a.cut) {
        const uint32_t listed = a.cut_count[0] < a.n_pictures ? a.cut_count[0] : a.n_pictures;
        for (uint32_t b = 0; b < listed; b += TRACKS_THREADS)
            each([&](int tid, TracksLane &) {
                if (b + (uint32_t)tid < listed && a.cut[b + (uint32_t)tid] == p) tracks_raise(&s.cut);
            });
        regions_sync();
    }
    const bool cut = regions_ld32(&s.cut) != 0;
    uint32_t died = cut ? tracks_count(s.vote[TRACKS_V_LIVE0]) : 0u;

    // 2. gather the detections
    const uint32_t written = (uint64_t)in.first + in.written > a.n_rois ? 0u : in.written;
    uint32_t found = 0;
    for (uint32_t b = 0, step = 0; b < written && found < TRACKS_MAX; b += TRACKS_THREADS, step++) {
        unsigned long long *const vote = s.vote[TRACKS_V_STEP + (step & 1u)];
        tracks_votes_clear(vote, TRACKS_WAVES);
        each([&](int tid, TracksLane &t) {
            const uint32_t k = b + (uint32_t)tid;
            t.ok = false;
            if (k < written) {
                t.q = a.rois[in.first + k];
                t.ok = t.q.reserved == 0 && t.q.picture == p && tracks_box_valid(t.q.x, t.q.y, t.q.w, t.q.h, a.w, a.h);
            }
            regions_vote(vote, tid, t.ok);
        });
        regions_sync();
        each([&](int tid, TracksLane &t) {
            if (!t.ok) return;
            const uint32_t rank = found + tracks_prefix(vote, tid);
            if (rank >= TRACKS_MAX) return;
            s.dbox[rank] = TracksBox{t.q.x, t.q.y, t.q.w, t.q.h};
            s.darea[rank] = (uint32_t)t.q.w * t.q.h;
            s.didx[rank] = in.first + b + (uint32_t)tid;
            s.dp[rank] = (uint16_t)TRACKS_NONE;
        });
        found += tracks_count(vote);
    }
    const uint32_t D = found < TRACKS_MAX ? found : TRACKS_MAX;
    each([&](int tid, TracksLane &t) {
        t.live = t.live0 && !cut;
        s.tbox[tid] = t.box;
        s.tarea[tid] = (uint32_t)t.box.w * t.box.h;
        s.tp[tid] = (uint16_t)(t.live ? TRACKS_NONE : TRACKS_DEAD);
    });
    regions_sync();

    // 3. match: rounds of mutual best
    uint32_t matched = 0;
    for (uint32_t round = 0;; round++) {
        unsigned long long *const vote = s.vote[TRACKS_V_STEP + (round & 1u)];
        tracks_votes_clear(vote, TRACKS_WAVES);
        each([&](int tid, TracksLane &t) {
            const uint32_t me = (uint32_t)tid;
            uint32_t choice = TRACKS_NONE;
            if (t.live && s.tp[me] == TRACKS_NONE) {                 // track me, unmatched
                if (t.tb == TRACKS_UNSCANNED || (t.tb != TRACKS_NONE && s.dp[t.tb] != TRACKS_NONE)) {
                    uint32_t best = TRACKS_NONE, bi = 0, bu = 1;
                    for (uint32_t j = 0; j < D; j++) {
                        if (s.dp[j] != TRACKS_NONE) continue;
                        const uint32_t inter = tracks_inter(t.box, s.dbox[j]), uni = s.tarea[me] + s.darea[j] - inter;
                        if (!tracks_eligible(inter, uni, a.iou_permille)) continue;
                        if (best == TRACKS_NONE || tracks_better(inter, uni, bi, bu)) best = j, bi = inter, bu = uni;
                    }
                    t.tb = best;
                }
                choice = t.tb;
            }
            s.tb[me] = (uint16_t)choice;
            choice = TRACKS_NONE;
            if (me < D && s.dp[me] == TRACKS_NONE) {                 // detection me, unmatched
                if (t.db == TRACKS_UNSCANNED || (t.db != TRACKS_NONE && s.tp[t.db] != TRACKS_NONE)) {
                    uint32_t best = TRACKS_NONE, bi = 0, bu = 1;
                    for (uint32_t i = 0; i < a.max_tracks; i++) {
                        if (s.tp[i] != TRACKS_NONE) continue;
                        const uint32_t inter = tracks_inter(s.tbox[i], s.dbox[me]), uni = s.tarea[i] + s.darea[me] - inter;
                        if (!tracks_eligible(inter, uni, a.iou_permille)) continue;
                        if (best == TRACKS_NONE || tracks_better(inter, uni, bi, bu)) best = i, bi = inter, bu = uni;
                    }
                    t.db = best;
                }
                choice = t.db;
            }
            s.db[me] = (uint16_t)choice;
        });
        regions_sync();
        each([&](int tid, TracksLane &t) {
            const uint32_t me = (uint32_t)tid, j = s.tb[me];
            const bool take = j != TRACKS_NONE && (mutants::kTracksArgmax || s.db[j] == me);
            if (take) s.tp[me] = (uint16_t)j, s.dp[j] = (uint16_t)me;      // (no other thread reads or writes either in this phase)
            regions_vote(vote, tid, take);
        });
        regions_sync();
        const uint32_t n = tracks_count(vote);
        matched += n;
        if (!n || mutants::kTracksArgmax) break;
    }

    // 4. update, deaths; the ballots of the births
    each([&](int tid, TracksLane &t) {
        const uint32_t me = (uint32_t)tid;
        bool dies = false;
        if (t.live) {
            t.age = tracks_inc(t.age);
            const uint32_t j = s.tp[me];
            if (j != TRACKS_NONE) {
                t.box = s.dbox[j];
                t.hits = tracks_inc(t.hits);
                t.missed = 0;
                t.flags = TRACKS_MATCHED;
                t.det = s.didx[j];
            } else {
                t.missed++;
                dies = t.missed > a.max_missed;
            }
        }
        if (dies) t.live = false;
        t.free = t.slot && !(mutants::kTracksBirthBeforeDeath ? t.live0 : t.live);
        t.unmatched = me < D && s.dp[me] == TRACKS_NONE;
        regions_vote(s.vote[TRACKS_V_DIED], tid, dies);
        regions_vote(s.vote[TRACKS_V_FREE], tid, t.free);
        regions_vote(s.vote[TRACKS_V_UNMATCHED], tid, t.unmatched);
    });
    regions_sync();
    each([&](int tid, TracksLane &t) {
        if (t.unmatched) s.born[tracks_prefix(s.vote[TRACKS_V_UNMATCHED], tid)] = (uint16_t)tid;
    });
    regions_sync();
    died += tracks_count(s.vote[TRACKS_V_DIED]);
    const uint32_t unmatched = tracks_count(s.vote[TRACKS_V_UNMATCHED]), free_slots = tracks_count(s.vote[TRACKS_V_FREE]);
    const uint32_t born = unmatched < free_slots ? unmatched : free_slots;

    // 5. births; 6. the emitted flag; the slots
    unsigned long long *const emit_vote = s.vote[TRACKS_V_STEP];     // (the rounds are over, a barrier lies behind their last read)
    tracks_votes_clear(emit_vote, TRACKS_WAVES);
    each([&](int tid, TracksLane &t) {
        if (t.free) {
            const uint32_t r = tracks_prefix(s.vote[TRACKS_V_FREE], tid);
            if (r < born) {
                const uint32_t j = s.born[r];
                t.live = true;
                t.id = tracks_id(next0, r);
                t.box = s.dbox[j];
                t.age = t.hits = 1u;
                t.missed = 0;
                t.flags = TRACKS_BORN;
                t.det = s.didx[j];
            }
        }
        bool emitted = false;
        if (t.live && t.flags && t.hits >= a.min_hits)
            emitted = a.emit_period ? (t.hits - a.min_hits) % a.emit_period == 0 : t.hits == a.min_hits;
        if (emitted) t.flags |= TRACKS_EMITTED;
        regions_vote(s.vote[TRACKS_V_LIVE], tid, t.live);
        regions_vote(emit_vote, tid, emitted);
        if (t.slot) {
            h263mi_track r;
            r.id = t.live ? t.id : 0u;
            r.x = t.live ? t.box.x : 0, r.y = t.live ? t.box.y : 0, r.w = t.live ? t.box.w : 0, r.h = t.live ? t.box.h : 0;
            r.age = t.live ? t.age : 0u, r.hits = t.live ? t.hits : 0u;
            r.missed = (uint16_t)(t.live ? t.missed : 0u), r.flags = (uint16_t)(t.live ? t.flags : 0u);
            r.det = t.live ? t.det : 0u;
            r.reserved = 0;
            slots[tid] = r;
        }
    });
    regions_sync();
    each([&](int tid, TracksLane &) {
        if (tid != 0) return;
        h263mi_track_head hd;
        hd.next_id = tracks_id(next0, born);
        hd.live = tracks_count(s.vote[TRACKS_V_LIVE]);
        hd.calls = calls0 + 1u;
        for (int k = 0; k < 5; k++) hd.reserved[k] = 0;
        *head = hd;
        h263mi_track_info o;
        o.detections = D, o.ignored = in.written - D, o.matched = matched, o.born = born, o.died = died, o.dropped = unmatched - born;
        o.first = 0, o.written = tracks_count(emit_vote);           // (the emitted count: k_tracks_pack turns it into first and written)
        a.info[p] = o;
    });
}

// The one wave of k_tracks_pack.
template <class EachLane>
H263_HD void tracks_pack(const TracksPackArgs &f, TracksPackLds &s, EachLane each)
{
    uint32_t total = 0, step = 0;                            // (at most 65535 * 256)
    for (uint32_t base = 0; base < f.n_pictures; base += 64u) {
        each([&](int lane, TracksPackLane &t) {
            const uint32_t p = base + (uint32_t)lane;
            t.e = p < f.n_pictures ? f.info[p].written : 0u;
            s.e[lane] = t.e;
        });
        wave_fence();
        each([&](int lane, TracksPackLane &t) {
            const uint32_t p = base + (uint32_t)lane;
            uint32_t before = total;
            for (int k = 0; k < lane; k++) before += s.e[k];
            const uint32_t first = before < f.max_out ? before : f.max_out;
            const uint32_t written = t.e < f.max_out - first ? t.e : f.max_out - first;
            s.first[lane] = first, s.written[lane] = written;
            if (p < f.n_pictures) f.info[p].first = first, f.info[p].written = written;
        });
        wave_fence();
        for (uint32_t q = 0; q < 64u && base + q < f.n_pictures; q++) {
            total += s.e[q];
            const uint32_t written = s.written[q], first = s.first[q], p = base + q;
            const h263mi_track *const slots =
                reinterpret_cast<const h263mi_track *>(f.state + (size_t)p * tracks_stride(f.max_tracks) + sizeof(h263mi_track_head));
            for (uint32_t b = 0, done = 0; b < f.max_tracks && done < written; b += 64u, step++) {
                unsigned long long *const vote = s.vote[step & 1u];
                tracks_votes_clear(vote, 1u);
                each([&](int lane, TracksPackLane &t) {
                    const uint32_t i = b + (uint32_t)lane;
                    t.emitted = i < f.max_tracks && (slots[i].flags & TRACKS_EMITTED) != 0;
                    regions_vote(vote, lane, t.emitted);
                });
                wave_fence();
                const unsigned long long v = vote[0];
                each([&](int lane, TracksPackLane &t) {
                    if (!t.emitted) return;
                    const uint32_t r = done + (uint32_t)__builtin_popcountll(v & ((1ull << lane) - 1ull)), i = b + (uint32_t)lane;
                    if (r >= written) return;
                    const h263mi_track k = slots[i];
                    h263mi_roi roi;
                    roi.picture = p;
                    roi.x = k.x, roi.y = k.y, roi.w = k.w, roi.h = k.h;
                    roi.reserved = 0;
                    f.rois[first + r] = roi;
                    if (f.refs) {
                        h263mi_track_ref ref;
                        ref.id = k.id, ref.picture = p, ref.hits = k.hits;
                        ref.slot = (uint16_t)i, ref.flags = k.flags;
                        f.refs[first + r] = ref;
                    }
                });
                done += (uint32_t)__builtin_popcountll(v);
            }
        }
        wave_fence();                                        // (the next step overwrites the hand-offs)
    }
    const uint32_t count = total < f.max_out ? total : f.max_out;
    each([&](int lane, TracksPackLane &) {
        for (uint32_t j = count + (uint32_t)lane; j < f.max_out; j += 64u) {
            h263mi_roi none;
            none.picture = 0xFFFFFFFFu;
            none.x = none.y = none.w = none.h = 0;
            none.reserved = 1;
            f.rois[j] = none;
            if (f.refs) {
                h263mi_track_ref zero;
                zero.id = zero.picture = zero.hits = 0;
                zero.slot = zero.flags = 0;
                f.refs[j] = zero;
            }
        }
        if (lane == 0) f.count[0] = count, f.count[1] = total;
    });
}

}  // namespace h263mi
