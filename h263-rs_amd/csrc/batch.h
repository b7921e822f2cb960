// batch.h -- h263mi_batch: N independent streams (N x H263State, state.rs:16-50) on one GPU: the device-resident frame
// store, the per-stream reference bookkeeping of state.rs:464-483, the deferred post-processing of pipeline mode, launch
// timing, and the pinned staging slots of the entry points that take host data.
//   batch.cpp          frame store, submit / render / sync, timing, the entry points over DEVICE records
//   output_shape.h     the shapes a rendering writes in (RGBA and YUV layouts and resizes): placement rules, what the kernels
//   output_shape.cpp   are told, the device memory a shape holds, and the *_extent entry points
//   batch_staging.cpp  host records and bitstreams -> pinned staging -> one launch (h263mi_batch_submit_host*,
//                      h263mi_batch_decode_next_pictures*), and the checks of a caller's host arrays
//   mixed_set.cpp      streams of different picture sizes: one batch per size class
//   state.cpp          the H263State mirror: a batch of one stream fed with host records through batch_submit_host
//   pinned.h           pinned host + device buffer pairs and the upload rings built from them
#pragma once

#include <memory>
#include <vector>

#include "../host/bitstream.hpp"
#include "host_common.h"
#include "output_shape.h"
#include "pinned.h"
#include "worker_pool.h"

// Where the coefficients of one submit live, how far they may be read, and -- sparse records -- where the records are.
// Passed to submit() by value for the one launch it is for (rounds 2-5 parked these in "next submit" members of the batch,
// which an early return could leave behind for the submit after).
struct h263mi_coeff_source {
    const int16_t *coeffs = nullptr;             // dense transport: the pool
    const uint32_t *first_event = nullptr;       // sparse transport: block offsets ...
    const uint32_t *events = nullptr;            // ... and events (level << 16 | x + 8 * y)
    uint32_t n_events = 0;                       // words in `events`; 0 = unknown (trusted arrays only)
    const uint64_t *coeff_base = nullptr;        // per picture base (blocks), or nullptr: all 0
    uint64_t pool_blocks = 0;                    // blocks in the pool (dense) / entries of first_event minus one (events)
    bool checked = false;                        // the waves refuse to read beyond pool_blocks / n_events
    const uint32_t *group_index = nullptr;       // sparse RECORDS (ReconArgs::mb_group_index), with ...
    const uint64_t *mb_base = nullptr;           // ... each picture's first record
};

struct h263mi_batch {
    int device = 0;
    hipStream_t stream = nullptr;
    // H263MI_CFG_OVERLAP_POST: k_post runs on a second stream so that the post-processing of picture i overlaps
    // the reconstruction of picture i+1 (k_recon is VALU-heavy, k_post store-heavy).  Legal with two frame sets:
    // post(i) reads set i; recon(i+1) reads set i and overwrites the set of picture i-1, which post(i-1) must have
    // finished reading -- both dependencies are HIP events.
    hipStream_t post_stream = nullptr;
    hipEvent_t ev_recon_done = nullptr, ev_post_done[2] = {nullptr, nullptr};   // post events per frame set
    bool overlap_post = false;
    // H263MI_CFG_PIPELINE_POST: h263mi_batch_decode defers the post-processing of a picture to the launch that
    // reconstructs the NEXT one (k_frame: both read the same frame set, see decode_kernels.hip); `pending` is that deferred
    // half.  Flushed (as a plain k_post launch) by sync, render, submit, reset.
    bool pipeline_post = false;
    // H263MI_CFG_TRUSTED_ARRAYS: the caller vouches for the device arrays it hands to h263mi_batch_submit / _decode /
    // _decode_events; without it (the default, ABI 7) every such array is bounded -- by the counts the caller gives, else by the
    // allocation the pointer lies in -- and the waves read nothing beyond
    bool trusted_arrays = false;
    // The post-filter strength is a property of the PICTURE (its quantiser and its USE_DEBLOCKER flag: deblock.rs:5-8,
    // picture.rs:61-64, types.rs:94-96,216), so every stream of a call may have its own (ABI 7).
    struct Strengths {
        uint8_t uniform = 0;                   // every stream, unless ...
        std::vector<uint8_t> per_stream;       // ... this holds one value per stream (empty = uniform)
        uint8_t of(uint32_t i) const { return per_stream.empty() ? uniform : per_stream[i]; }
        bool same_for_all() const
        {
            for (uint8_t v : per_stream)
                if (v != per_stream[0]) return false;
            return true;
        }
    };
    // The shapes in force (output_shape.h): of the RGBA (h263mi_batch_set_rgba_layout, _set_rgba_resize, _set_tensor_output) and of the deblocked
    // planes (h263mi_batch_set_yuv_layout, _set_yuv_resize).  A rendering is told its shapes (render), these by default.
    typedef h263mi::OutLayout OutLayout;
    typedef h263mi::RgbaLayout RgbaLayout;
    typedef h263mi::YuvLayout YuvLayout;
    RgbaLayout layout;
    YuvLayout yuv;
    struct PendingPost {
        bool valid = false;
        YuvLayout yuv;                         // the plane layout in force when the rendering was requested
        Strengths strength;
        OutLayout out;                         // the layout in force when the rendering was requested
        RgbaLayout::Resize resize;             // ... or the resize, with the tensor it may end in (then `rgba` is its scratch)
        uint8_t *const *resize_dst = nullptr;  // DEVICE array: stream s's resized picture, nullptr = none
        const h263mi::PlaneDst *plane_dst = nullptr;   // yuv.resize: DEVICE array of the streams' planes (then `planes` is its scratch)
        bool plane_wide = false;               // ... which all allow word stores
        uint8_t *rgba = nullptr, *planes = nullptr;
        uint8_t *const *rgba_ptrs = nullptr;   // DEVICE array of per-stream output pointers (a batch inside a mixed-size set)
        std::vector<int8_t> set;               // per stream: frame set it reads, -1 = nothing to post-process
    } pending;
    // per-stream output pointers for the kernels (made on first use)
    h263mi::UploadRing<uint8_t *> ptr_ring;
    h263mi::UploadRing<h263mi::PlaneDst> plane_ring;       // ... and the plane pointers of a YUV resize
    uint32_t n = 0;
    h263mi::FrameLayout L{};
    uint8_t *frames[2] = {nullptr, nullptr};   // ping-pong frame sets, n * frame_bytes each
    // Every stream of the batch is its own H263State (state.rs:16-50): its own last picture, its own reference flag,
    // its own errors.  As long as all streams agree (the common case: they advance in lock step and nothing fails) the
    // kernels get one set of pointers; once they differ, a word per stream (dev_common.h: STREAM_*).
    struct StreamState {
        int8_t cur = -1;                       // frame set holding the stream's last picture, -1 = none
        bool has_ref = false;                  // state.rs:29-31 reference_picture.is_some()
        int8_t good_cur = -1;                  // ... as of the last successful sync (what an error falls back to)
        bool good_has_ref = false;
        uint32_t unsynced = 0;                 // pictures submitted since then
        bool active = true;                    // takes part in the next submit (h263mi_batch_set_active)
    };
    std::vector<StreamState> ss;
    h263mi::PinnedPair<uint32_t> status;       // one word per stream
    // per-stream words for the kernels (made in alloc())
    h263mi::UploadRing<uint32_t> word_ring;
    // (what sync() falls back to when the device reports an error -- state.rs:142, 464-487: an error leaves the state
    // unchanged -- is each stream's good_cur / good_has_ref, valid as long as at most one picture was submitted for the
    // stream since: the frame set it names is the one the ping-pong has not overwritten yet)
    unsigned frame_launches = 0;               // k_frame launches so far: odd ones walk the pictures backwards
    // host-record staging for h263mi_batch_submit_host: two slots (pinned host + device) used alternately, so
    // that packing picture i+1 overlaps the copy and the kernel of picture i
    struct HostStaging {
        h263mi::PinnedPair<h263mi::MbRecord> mbs;
        h263mi::PinnedPair<int16_t> coeffs;    // dense blocks, 64 each
        // ONE buffer for everything small that goes with a call, so that it crosses the link in one copy:
        // [base: 2n x u64 -- [0, n) coefficient base per stream, [n, 2n) record base (sparse records)]
        // [index: n x groups per picture x u32 -- sparse records, one word per group of 8 macroblocks]
        // [events: rebased block offsets, then the events -- sparse coefficient transport]
        h263mi::PinnedPair<uint32_t> words;
        uint64_t *h_base = nullptr, *d_base = nullptr;       // (into words)
        uint32_t *h_index = nullptr, *d_index = nullptr;
        uint32_t *h_events = nullptr, *d_events = nullptr;
        hipEvent_t done = nullptr;             // recorded after the kernel that reads the slot
        ~HostStaging()
        {
            if (done) (void)hipEventDestroy(done);
        }
    } host_stg[2];
    unsigned host_slot = 0;
    // h263mi_batch_decode_next_pictures: what each stream remembers of its last picture header (state.rs:143-167)
    // and the parse results of the current call (kept between calls so that their buffers are reused)
    std::vector<h263mi::bits::ParserContext> parser_ctx;
    std::vector<h263mi::bits::ParsedPicture> parsed;
    // Where the host side of this batch runs: the NUMA node of its device (worker_pool.h).  Looked up when the batch is made.
    h263mi::HostPlacement placement;
    std::unique_ptr<h263mi::WorkerPool> pool;  // host threads of the entry points that take host data
    long pool_spin_us = h263mi::WorkerPool::kSpinUsDefault;    // (HostThreadPlan::spin_us of the call that is being packed)
    h263mi::WorkerPool &workers(unsigned want)
    {
        if (!pool || pool->size() < want) pool.reset(new h263mi::WorkerPool(want - 1, &placement));
        return *pool;
    }
    // H263MI_TRACE_E2E=1: where the host time of h263mi_batch_decode_next_pictures goes (printed when the batch is
    // destroyed): [0] parser threads, [1] waiting for the staging slot, [2] packing into pinned staging, [3] enqueueing
    // copies and launches
    double host_ms[6] = {0, 0, 0, 0, 0, 0};     // ... [4] of [3]: the copies, [5] of [3]: submit (state words, launch)
    size_t frame_skew = 0;
    unsigned host_calls = 0;
    bool trace_host = getenv("H263MI_TRACE_E2E") != nullptr;
    bool trace_each = trace_host && getenv("H263MI_TRACE_E2E")[0] == '2';
    // timing
    bool timing = false;
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    struct TimedChain { size_t first; int kernel; uint32_t launches; };   // (index of the begin event, kernel id, launches)
    std::vector<TimedChain> ev_ranges;
    int chain_kernel = -1;
    hipStream_t chain_on = nullptr;            // the stream the chain's launches are queued on
    uint32_t chain_launches = 0;

    ~h263mi_batch();
    int alloc(uint32_t n_streams, uint32_t w, uint32_t h);

    // ---- views of the per-stream state
    bool any_picture() const;
    // every stream takes part and all agree on (cur, has_ref): the kernels need no per-stream words
    bool uniform() const;
    bool pending_uniform() const;
    // hand the kernels one element per stream (stream words, output pointers): the ring's next slot and its copy, queued on
    // `on`, the stream of the kernel that reads them
    template <typename T>
    int upload(h263mi::UploadRing<T> &ring, const T *host, const T **d_out, hipStream_t on)
    {
        RC_TRY(ring.make(n, placement));
        RC_TRY(time_close());                  // a copy is not part of any kernel's time
        return ring.push(host, d_out, on);
    }
    int forget_pictures();
    // one stream forgets its pictures (the seeking rule of state.rs:134-137 for a single H263State of the batch)
    int forget_stream(uint32_t i);
    void release_frames();

    // ---- staging (batch_staging.cpp)
    // the fixed-size part of a staging slot: the records of every stream, the event that says when the slot may be written again
    int ensure_record_staging(HostStaging &g2);
    // words in front of the events in HostStaging::h_words: the two base arrays and the sparse-record index
    size_t head_words() const { return 4 * (size_t)n + (size_t)n * h263mi::recon_tiles_x(L) * L.mbh; }
    int ensure_host_staging(HostStaging &g2, size_t n_blocks, size_t n_event_words = 0);

    // ---- launch timing (h263mi_batch_timing_begin / _end); kernel ids: 0 k_recon, 1 k_post, 2 k_frame
    hipStream_t stream_of(int kernel_id) const { return (kernel_id == 1 && overlap_post) ? post_stream : stream; }
    int time_close();
    // (kernel id 3: k_rgba_resize, queued on `on` behind the rendering it resizes; its time counts as post-processing.
    // id 4: k_plane_resize, likewise -- its time is post-processing time, and post_launches goes on counting renderings;
    // id 5: k_plane_filter, in the place of id 4 under a filtered YUV resize)
    int time_begin(int kernel_id, hipStream_t on = nullptr);

    // ---- the work
    // state.rs:432-483 for every stream of the batch that takes part.  types: one picture type per stream, or nullptr:
    // `picture_type` for all.  with_post: run the deferred post-processing (pending) in the same launch (pipeline mode).
    int submit(uint8_t picture_type, const h263mi::MbRecord *d_mbs, const h263mi_coeff_source &src, bool with_post = false,
               const uint8_t *types = nullptr);
    h263mi::PostArgs post_args(int set, uint8_t strength, uint8_t *d_rgba, uint8_t *d_planes) const;
    // k_post over `sets` (per stream: the frame set to read, -1 = skip the stream); rgba_ptrs: DEVICE array of per-stream
    // output pointers instead of d_rgba (or nullptr)
    // yuv (may be null; used when it is on and d_planes given): the planes go out in that layout through k_post_yuv, behind a
    // launch of their own for the RGBA if that is asked for too
    int launch_post_sets(const std::vector<int8_t> &sets, const Strengths &strength, uint8_t *d_rgba, uint8_t *d_planes, hipStream_t on,
                         uint8_t *const *rgba_ptrs = nullptr, OutLayout out = OutLayout(), const YuvLayout *yuv = nullptr);
    // the layout `lay` applied to d_rgba: false = the default layout (d_rgba as it is); true = `ptrs` holds n DEVICE pointers,
    // stream s's picture at d_rgba + its offset
    bool layout_ptrs(const RgbaLayout &lay, uint8_t *d_rgba, std::vector<uint8_t *> &ptrs) const;
    // the resize of `lay`: the DEVICE array of k_rgba_resize's destinations -- stream s at host_ptrs[s] (if given) or d_rgba +
    // its offset, nullptr where sets[s] < 0 -- uploaded on `on`
    int resize_dst(const RgbaLayout &lay, const std::vector<int8_t> &sets, uint8_t *d_rgba, uint8_t *const *host_ptrs, hipStream_t on,
                   uint8_t *const **d_out);
    // k_rgba_resize of `rz` -- or, where it ends in a tensor (rz.tensor), k_tensor_resize -- into `d_dst` (resize_dst), on `on`;
    // nothing when no stream has a set (sets[s] < 0 for all)
    int launch_resize(const RgbaLayout::Resize &rz, const std::vector<int8_t> &sets, uint8_t *const *d_dst, hipStream_t on);
    // a YUV resize `rz` of planes that go to d_planes: the DEVICE array of k_plane_resize's destinations -- stream s's planes at
    // d_planes + its offsets, null where sets[s] < 0 -- uploaded on `on`; *wide: word stores are possible
    int plane_resize_dst(const YuvLayout::Resize &rz, const std::vector<int8_t> &sets, uint8_t *d_planes, hipStream_t on,
                         const h263mi::PlaneDst **d_out, bool *wide);
    // k_plane_resize of `rz` -- or, under a filter (rz.filter), k_plane_filter -- into `d_dst` (plane_resize_dst), on `on`; nothing
    // when no stream has a set
    int launch_plane_resize(const YuvLayout::Resize &rz, const std::vector<int8_t> &sets, const h263mi::PlaneDst *d_dst, bool wide,
                            hipStream_t on);
    // pipeline mode: the post-processing of the pictures just submitted is deferred to the next launch.
    // host_ptrs (or nullptr): n DEVICE pointers, the RGBA buffer of each stream (nullptr = none for it) instead of d_rgba.
    int note_pending(const Strengths &strength, uint8_t *d_rgba, uint8_t *d_planes, uint8_t *const *host_ptrs = nullptr);
    // the deferred post-processing of pipeline mode, as a launch of its own
    int flush_pending();
    // only_active: the rendering half of a decode call -- streams that sat the call out (h263mi_batch_set_active, no data,
    // a picture that failed to parse) keep their part of the output buffers untouched, as the pipelined form (note_pending)
    // does; h263mi_batch_render_rgba renders every stream's last picture.  In the shapes `rgba_shape` and `yuv_shape` (nullptr: the
    // batch's own, `layout` and `yuv`).
    int render(const Strengths &strength, uint8_t *d_rgba, uint8_t *d_planes, bool only_active = false, uint8_t *const *host_ptrs = nullptr,
               const RgbaLayout *rgba_shape = nullptr, const YuvLayout *yuv_shape = nullptr);
    // stream_rc (may be null): per stream 0, H263MI_ERR_UNCODED_IFRAME_BLOCKS or H263MI_ERR_INVALID_ARGUMENT
    int sync(int *stream_rc = nullptr);
    int copy_yuv(uint32_t s, uint8_t *y, uint8_t *cb, uint8_t *cr);
    // ---- digests (h263mi_batch_digest_yuv, h263mi_batch_adler32_spans): the span table, the accumulators and the results of a
    // call, pinned and on the device (h263mi::digest_spans), and the table of the frame store's planes
    h263mi::PinnedPair<uint64_t> digest_words;
    std::vector<h263mi_digest_span> digest_planes;
    // the Adler-32 of Y, Cb, Cr of every stream's last picture, read in place (3 spans per stream, one launch pair); a stream
    // without a picture: digest 0, stream_rc H263MI_ERR_NO_PICTURE -- which is also what the call returns when stream_rc is null
    int digest_yuv(uint32_t seed, uint32_t *digests, int *stream_rc);
    // ---- change maps (h263mi_batch_change_last): cur is the luma of every stream's last picture, read in place; the streams'
    // CHANGE_* words (valid, frame set) travel through word_ring unless every stream has a picture in the same set.  Queues the
    // launches on `stream` and returns; a stream without a picture is left out as digest_yuv reports it
    int change_last(const h263mi_plane_set *prev, const h263mi_change *c, uint32_t *d_cells, uint64_t cells_bytes,
                    h263mi_change_summary *d_summary, uint32_t *d_selected, uint32_t *d_count, int *stream_rc);
    // ---- background model (h263mi_batch_background_last): cur as change_last's, the streams' words too; a stream without a
    // picture is left out in the same way
    int background_last(const h263mi_background *bg, void *d_state, uint64_t state_bytes, const uint32_t *d_cut, const uint32_t *d_cut_count,
                        const h263mi_plane_set *mask, uint32_t *d_cells, uint64_t cells_bytes, h263mi_change_summary *d_summary,
                        uint32_t *d_selected, uint32_t *d_count, int *stream_rc);
    // ---- histograms (h263mi_batch_hist_last): plane `plane` (0 Y, 1 Cb, 2 Cr) of every stream's last picture, read in place; the
    // streams' HIST_* words travel as change_last's do; a stream without a picture is left out in the same way
    int hist_last(uint32_t plane, const h263mi_hist *h, uint32_t *d_hist, uint64_t hist_bytes, uint32_t *d_prev_hist, uint64_t prev_bytes,
                  h263mi_hist_stats *d_stats, uint32_t *d_selected, uint32_t *d_count, int *stream_rc);
};

namespace h263mi {

// h263mi_adler32_spans_on on `stream` of the current device, staged through `buf` (grown when a call needs more).  The table is
// checked before any device call.
int digest_spans(PinnedPair<uint64_t> &buf, const HostPlacement &where, const uint8_t *d_base, uint64_t buffer_bytes,
                 const h263mi_digest_span *spans, uint32_t n_spans, uint32_t seed, uint32_t *digests, uint32_t n_digests,
                 hipStream_t stream);
// what the digest entry points report for a failure of the HIP runtime: H263MI_ERR_HIP, an allocation included
inline int digest_rc(int rc) { return rc == H263MI_ERR_OUT_OF_MEMORY ? H263MI_ERR_HIP : rc; }
// both halves of an Adler-32 start value are residues
inline bool digest_seed_valid(uint32_t seed) { return (seed & 0xffffu) < DIGEST_MOD && (seed >> 16) < DIGEST_MOD; }
int batch_create(uint32_t n_streams, uint32_t w, uint32_t h, const h263mi_backend_cfg *cfg, h263mi_batch **out);
// where the host side of device `dev`'s work belongs (worker_pool.h): the PCI addresses of the visible devices -> sysfs
HostPlacement placement_of_device(int dev);

// The `strength` / `strengths` pair of the ABI 7 entry points -> Strengths.  strengths != nullptr: one value per stream
// (0..12 each); else strength: 0..12 for every stream, or -- where the entry has parsed the headers (from_header_allowed) --
// H263MI_STRENGTH_FROM_HEADER: per_stream is sized and the entry fills it in per picture.  H263MI_ERR_INVALID_ARGUMENT for
// anything else.
int make_strengths(uint8_t strength, const uint8_t *strengths, uint32_t n, bool from_header_allowed, h263mi_batch::Strengths &out);

// DIRECT WORDS (round 5, h263mi_batch_decode_next_pictures only): the parser has written every stream's block offsets, events
// and group index straight into the staging slot -- stream i's block offsets at h_events + i * pitch_blocks, its events at
// h_events + n * pitch_blocks + i * pitch_events, the offsets counting from i * pitch_events -- so nothing is packed: the
// used head of every stream's part crosses the link in one 2-D copy per array.  The pitches are the worst case of the
// call's pictures (bits::event_words_bound), known from their lengths before a bit is parsed.
struct DirectWords {
    size_t pitch_blocks, pitch_events;
};

// The checks of a caller's host arrays (batch_staging.cpp); the device trusts what passes them.
// records: known types, quantisers 1..31, no bits beyond the six blocks, and the coded blocks of a record inside the n_blocks
bool records_valid(const h263mi_mb_record *mbs, size_t n_mbs, size_t n_blocks);
// block offsets that start at 0, never fall and end at n_events; at most 64 events per block, naming each position once (the
// device places them in no particular order).  No blocks: nothing to check.
bool events_valid(const uint32_t *first_event, size_t n_blocks, const uint32_t *events, size_t n_events);

// one picture per stream from per-stream host arrays; coefficients dense (`coeffs`) or as events (`first_event`,
// `events`, `n_events`) -- batch_staging.cpp.  validated: the arrays have passed the checks above already (a parser wrote
// them, or h263mi_submit_picture checked them), so they are not checked again
int batch_submit_host(h263mi_batch *b, uint8_t picture_type, const h263mi_mb_record *const *mbs, const uint32_t *n_mbs,
                      const int16_t *const *coeffs, const uint32_t *n_coeff_blocks, const uint32_t *const *first_event,
                      const uint32_t *const *events, const uint32_t *n_events, bool validated = false, uint32_t pack_threads = 0,
                      const uint8_t *types = nullptr, bool deferred_post = false, const uint32_t *const *group_index = nullptr,
                      const DirectWords *direct = nullptr);

// What the bitstream entries set before bits::parse_picture: events, no dense blocks, the frame store's size limit, sparse records
// or not, and nothing parsed into a caller's memory (an entry with a staging slot to parse into sets the *_ext fields after this).
inline void prepare_for_parse(bits::ParsedPicture &pic, bool sparse)
{
    pic.want_dense = false;
    pic.size_fits = &picture_size_fits;
    pic.sparse_records = sparse;
    pic.mbs_ext = nullptr;
    pic.events_ext = pic.first_event_ext = pic.group_index_ext = nullptr;
    pic.mbs_ext_cap = pic.events_ext_cap = pic.first_event_ext_cap = pic.group_index_ext_cap = pic.event_base = 0;
}
// The serial half of decode_next_picture (state.rs:143-427): parse(i) for the n streams on plan.threads host threads
// (StreamDeal), from the pool `workers` hands out when there are several.  timed (may be null): the batch whose
// H263MI_TRACE_E2E timing counts the phase (host_ms[0]).
void parse_streams(const HostThreadPlan &plan, const std::function<WorkerPool &(unsigned)> &workers, uint32_t n,
                   const std::function<void(uint32_t)> &parse, h263mi_batch *timed = nullptr);
// One launch of batch b from parsed pictures (batch_submit_host): slot s decodes *pics[s], nullptr = the slot sits the call out
// (the slots' active flags are set for the call and restored).  Then the rendering, deferred on a pipelined batch, into d_rgba /
// d_planes or rgba_ptrs (one DEVICE pointer per slot, nullptr = none), if there is any output.  from_header: st.per_stream
// (sized) is filled in from the headers.  The launch's and the rendering's rc come back apart: a picture whose launch is queued
// is decoded, whatever the rendering does.
struct SubmitResult { int rc, render_rc; };
SubmitResult submit_parsed(h263mi_batch *b, const bits::ParsedPicture *const *pics, uint32_t pack_threads, bool sparse_records,
                           const DirectWords *direct, h263mi_batch::Strengths st, bool from_header, uint8_t *d_rgba,
                           uint8_t *d_planes, uint8_t *const *rgba_ptrs = nullptr);

}  // namespace h263mi
