"""GPU tests of the plane histograms (h263mi_hist_on, h263mi_batch_hist, h263mi_batch_hist_last, h263mi_hist_last: k_hist,
k_hist_final, k_hist_select).  Every comparison is exact, against hist_ref: the histograms, the statistics, the list, the count,
prev after a roll, and the sentinels around every device buffer.  The cases are the ones the kernels are run at lane by lane on the
CPU (hist_cases.CASES), where every hazard of theirs is shown to occur."""
import numpy as np
import pytest
import torch  # before the library is loaded: torch brings its own HIP runtime, which the C-ABI library must share (as in bench.py)

import h263mi
import hist_cases as hc
import hist_ref as ref
import recgen

pytestmark = pytest.mark.gpu
SENTINEL = 0xC3
WORD = SENTINEL * 0x01010101
GUARD = 64                                                   # sentinel bytes in front of and behind every device buffer


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if h263mi.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the MI355X box")


@pytest.fixture(scope="module")
def stream():
    return torch.cuda.Stream(device=0)


def _guarded(data):
    """a device buffer of GUARD sentinels, the bytes of `data`, GUARD sentinels"""
    host = np.concatenate([np.full(GUARD, SENTINEL, np.uint8), np.ascontiguousarray(data).view(np.uint8).ravel(),
                           np.full(GUARD, SENTINEL, np.uint8)])
    d = h263mi.DeviceBuffer(host.size)
    d.upload(host)
    return d


def _inside(d, what):
    raw = d.download()
    assert (raw[:GUARD] == SENTINEL).all() and (raw[-GUARD:] == SENTINEL).all(), what + ": a guard was written"
    return raw[GUARD:-GUARD]


class Buffers:
    """the histograms, prev, the statistics, the list and the count of one call, each between sentinels; prev: (n, 256) or None
    (the buffer then holds sentinels and is not handed to the call)"""

    def __init__(self, n, prev):
        self.n, self.has_prev = n, prev is not None
        self.hist = _guarded(np.full(n * 1024, SENTINEL, np.uint8))
        self.prev = _guarded(prev if prev is not None else np.full(n * 1024, SENTINEL, np.uint8))
        self.stats = _guarded(np.full(n * 32, SENTINEL, np.uint8))
        self.list = _guarded(np.full(n * 4, SENTINEL, np.uint8))
        self.count = _guarded(np.full(4, SENTINEL, np.uint8))
        self.bytes = n * 1024

    def args(self, lst=True):
        """d_hist, hist_bytes, d_stats, d_prev_hist, prev_bytes, d_selected, d_count: the tail of the bindings' calls"""
        return (self.hist.at(GUARD), self.bytes, self.stats.at(GUARD), self.prev.at(GUARD) if self.has_prev else None,
                self.bytes if self.has_prev else 0, self.list.at(GUARD) if lst else None, self.count.at(GUARD) if lst else None)

    def read(self, what=""):
        """-> (hist, prev, stats, list words, count); the guards are checked"""
        return (_inside(self.hist, what).view(np.uint32).reshape(self.n, 256), _inside(self.prev, what).view(np.uint32).reshape(self.n, 256),
                _inside(self.stats, what).view(h263mi.HIST_STATS_DTYPE), _inside(self.list, what).view(np.uint32),
                int(_inside(self.count, what).view(np.uint32)[0]))

    def raw(self):
        return [d.download() for d in (self.hist, self.prev, self.stats, self.list, self.count)]

    def free(self):
        for d in (self.hist, self.prev, self.stats, self.list, self.count):
            d.free()


def _check(b, bufs, what, lst=True):
    """the buffers against the case's expectation; without prev or without a list their buffers still hold the sentinel"""
    hist, prev, stats, list_got, count = bufs.read(what)
    if not lst:
        assert count == WORD and (list_got == WORD).all(), what + ": no list was wanted"
    if not bufs.has_prev:
        assert (prev == WORD).all(), what + ": prev was not given"
    diff = hc.compare(b, hist, prev if bufs.has_prev else None, stats, list_got if lst else None, count if lst else None)
    assert diff is None, "%s: %s" % (what, diff)


def _set(b, d_planes):
    return h263mi.PlaneSet(d_planes.ptr.value + GUARD + b.off, b.buf.size - b.off, b.pitch, b.stride)


def _hist_of(b, roll=None):
    return h263mi.make_hist(b.lo, b.hi, b.cut, b.roll if roll is None else roll)


def _run(b, stream, d_planes, bufs, lst=True, roll=None):
    h263mi.hist(_set(b, d_planes), b.n, b.w, b.h, _hist_of(b, roll), *bufs.args(lst), stream=stream.cuda_stream)


GPU_CASES = [name for name in hc.CASES if not hc.CASES[name].get("words")]         # (the plain entry point has no per-picture words)


# ---------------------------------------------------------------------------------------------
# 1. the case table through h263mi_hist_on
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GPU_CASES)
def test_cases(stream, name):
    b = hc.build(name)
    d_planes = _guarded(b.buf)
    bufs = Buffers(b.n, b.prev)
    assert h263mi.hist_extent(b.n, b.w, b.h, _hist_of(b)) == bufs.bytes
    _run(b, stream, d_planes, bufs, lst=b.prev is not None)
    stream.synchronize()
    _check(b, bufs, name, lst=b.prev is not None)
    assert (_inside(d_planes, name) == b.buf).all(), "the set is read only"
    d_planes.free()
    bufs.free()


@pytest.mark.parametrize("name", ["size_1025x9", "cut_equal_and_above", "select_n130", "prev_ones", "decoded"])
def test_with_prev_but_without_a_list(stream, name):
    b = hc.build(name)
    assert b.prev is not None
    d_planes = _guarded(b.buf)
    bufs = Buffers(b.n, b.prev)
    _run(b, stream, d_planes, bufs, lst=False)
    stream.synchronize()
    _check(b, bufs, name, lst=False)
    d_planes.free()
    bufs.free()


def test_roll_then_a_second_call(stream):
    """the prev that a rolling call leaves is the first call's histograms: the same pictures again are at distance 0 and no cuts;
    other pictures, roll off, are at the distance of the two calls' histograms and leave prev alone"""
    first, other = hc.build("cut_first_call"), hc.build("pctl_exact")
    assert first.roll and (first.w, first.h, first.n) == (other.w, other.h, other.n)
    d_planes, d_other = _guarded(first.buf), _guarded(other.buf)
    bufs = Buffers(first.n, first.prev)
    _run(first, stream, d_planes, bufs)
    stream.synchronize()
    _check(first, bufs, "first call")
    hist1, prev1, stats1, _, count1 = bufs.read()
    assert count1 == 2 and (prev1 == hist1).all()
    _run(first, stream, d_planes, bufs)
    stream.synchronize()
    hist2, prev2, stats2, list2, count2 = bufs.read("second call")
    assert (hist2 == hist1).all() and (prev2 == hist1).all() and count2 == 0 and not stats2["distance"].any()
    assert (stats2["sum"] == stats1["sum"]).all() and list2[:2].tolist() == [0, 1]          # (the first call's entries: none written now)
    h263mi.hist(_set(other, d_other), other.n, other.w, other.h, _hist_of(other, roll=0), *bufs.args(), stream=stream.cuda_stream)
    stream.synchronize()
    hist3, prev3, stats3, _, _ = bufs.read("third call")
    want = [ref.distance(other.hist[p], first.hist[p]) for p in range(other.n)]
    assert stats3["distance"].tolist() == want and min(want) > 0 and (hist3 == other.hist).all()
    assert (prev3 == hist1).all()
    for d in (d_planes, d_other):
        d.free()
    bufs.free()


def test_the_call_is_ordered_behind_a_copy_queued_on_its_stream(stream):
    """the planes arrive behind 512 MiB of device-to-device copy on the same stream and the host waits for neither: a call that ran
    early, or on another stream, would count the flat decoy that the buffer held before"""
    b = hc.build("decoded")
    ballast = (torch.zeros(512 << 20, dtype=torch.uint8, device="cuda"), torch.empty(512 << 20, dtype=torch.uint8, device="cuda"))
    staged = torch.from_numpy(b.buf.copy()).cuda()
    d_planes = torch.full((b.buf.size,), 1, dtype=torch.uint8, device="cuda")
    bufs = Buffers(b.n, b.prev)
    pset = h263mi.PlaneSet(d_planes.data_ptr() + b.off, b.buf.size - b.off, b.pitch, b.stride)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        ballast[1].copy_(ballast[0], non_blocking=True)
        d_planes.copy_(staged, non_blocking=True)
    h263mi.hist(pset, b.n, b.w, b.h, _hist_of(b), *bufs.args(), stream=stream.cuda_stream)
    stream.synchronize()
    _check(b, bufs, "behind the copy")
    bufs.free()


def test_two_runs_give_identical_bytes(stream):
    b = hc.build("size_2049x17")
    runs = []
    for _ in range(2):
        d_planes = _guarded(b.buf)
        bufs = Buffers(b.n, b.prev)
        _run(b, stream, d_planes, bufs, lst=b.prev is not None)
        stream.synchronize()
        runs.append(bufs.raw())
        bufs.free()
        d_planes.free()
    assert all((x == y).all() for x, y in zip(*runs))


def test_no_prev_no_list_and_no_pictures(stream):
    b = hc.build("place_0_r16_padded16_w100")
    assert b.prev is not None
    d_planes = _guarded(b.buf)
    # no prev: distance 0, the buffer untouched
    bufs = Buffers(b.n, None)
    _run(b, stream, d_planes, bufs, lst=False)
    stream.synchronize()
    hist, prev, stats, list_got, count = bufs.read("no prev")
    assert (hist == hc.expected(b)[0]).all() and not stats["distance"].any() and (prev == WORD).all()
    assert [s[:2] + s[3:] for s in hc.stats_tuples(stats)] == [s[:2] + s[3:] for s in hc.expected(b)[1]]
    assert count == WORD and (list_got == WORD).all()
    bufs.free()
    # no pictures: nothing but the count, which becomes 0
    bufs = Buffers(b.n, b.prev)
    h263mi.hist(None, 0, b.w, b.h, _hist_of(b), None, 0, None, bufs.prev.at(GUARD), 0, bufs.list.at(GUARD), bufs.count.at(GUARD),
                stream=stream.cuda_stream)
    stream.synchronize()
    hist, prev, stats, list_got, count = bufs.read("no pictures")
    assert count == 0 and (list_got == WORD).all() and (hist == WORD).all() and (stats.view(np.uint8) == SENTINEL).all()
    assert (prev == b.prev).all()
    bufs.free()
    d_planes.free()


def test_a_failure_of_the_runtime_at_every_call_is_reported_and_the_same_call_then_succeeds(stream):
    """the injected return code of h263mi_debug_fail_nth_hip_call: nothing faults on the device.  Under roll: a failed call has
    not rolled anything"""
    b = hc.build("cut_first_call")
    assert b.roll == 1
    failures = 0
    for nth in range(1, 10):
        d_planes = _guarded(b.buf)
        bufs = Buffers(b.n, b.prev)
        h263mi.debug_fail_nth_hip_call(nth)
        try:
            _run(b, stream, d_planes, bufs)
            fired = h263mi.debug_fail_nth_hip_call(0) <= 0
            assert not fired, "the %d-th HIP call failed and the call reported success" % nth
            done = True
        except h263mi.H263Error as e:
            h263mi.debug_fail_nth_hip_call(0)
            assert e.code == h263mi.ERR_HIP, (nth, e.code)
            failures += 1
            done = False
            stream.synchronize()
            assert (bufs.read("after failure %d" % nth)[1] == b.prev).all()
            _run(b, stream, d_planes, bufs)
        stream.synchronize()
        _check(b, bufs, "nth = %d" % nth)
        bufs.free()
        d_planes.free()
        if done:
            break
    else:
        pytest.fail("the call never went through")
    assert failures == 2                                      # the clearing of the histograms, the launches


# ---------------------------------------------------------------------------------------------
# 2. the frame store in place: h263mi_batch_hist_last, h263mi_hist_last
# ---------------------------------------------------------------------------------------------
def _upload(pics):
    mbs = np.concatenate([m for m, _ in pics])
    co = np.concatenate([c for _, c in pics]).astype(np.int16)
    base = np.cumsum([0] + [c.shape[0] for _, c in pics[:-1]]).astype(np.uint64)
    bufs = []
    for arr in (mbs, co, base):
        d = h263mi.DeviceBuffer(max(arr.nbytes, 16))
        d.upload(arr)
        bufs.append(d)
    return bufs


@pytest.fixture(scope="module")
def three_pictures():
    """3 streams of 100 x 60: device records of I, P, P"""
    n, w, h = 3, 100, 60
    recs = [_upload([recgen.intra_picture(w, h, seed=7400 + s) for s in range(n)])]
    for f in (1, 2):
        recs.append(_upload([recgen.inter_picture(w, h, seed=7400 + 10 * f + s, mv_range=30, p_4v=0.2, p_coded=0.5, quant=8) for s in range(n)]))
    return n, w, h, recs


def _expect(planes, prev, valid, lo, hi, cut):
    """-> (hist, stats tuples, selected) of the (n, h, w) planes against prev (n, 256)"""
    hist = ref.histograms(planes)
    st = [ref.stats(hist[p], prev[p], lo, hi) if valid[p] else ref.ZERO_STATS for p in range(len(planes))]
    pixels = planes.shape[1] * planes.shape[2]
    return np.where(np.asarray(valid)[:, None], hist, 0), st, ref.select(st, cut, pixels, valid)


@pytest.mark.parametrize("mode", ["plain", "pipeline_post", "overlap_post"])
def test_batch_hist_last_follows_the_last_picture_across_both_frame_sets(three_pictures, mode):
    n, w, h, recs = three_pictures
    lo, hi, cut = 50, 950, 20
    desc = h263mi.make_hist(lo, hi, cut, roll=1)
    prev_host = np.random.default_rng(78).integers(0, 60, (n, 256)).astype(np.uint32)
    b = h263mi.Batch(n, w, h, 0, None, pipeline_post=mode == "pipeline_post", overlap_post=mode == "overlap_post")
    rgba = h263mi.DeviceBuffer(n * w * h * 4)
    valid = [True, False, True]
    # before any picture: every stream is invalid, all zero, prev untouched, nobody selected
    bufs = Buffers(n, prev_host)
    rcs = b.hist_last(0, desc, *bufs.args())
    b.sync()
    assert rcs == [h263mi.ERR_NO_PICTURE] * n
    hist, prev, stats, list_got, count = bufs.read("no pictures")
    assert not hist.any() and not stats.view(np.uint8).any() and count == 0 and (list_got == WORD).all() and (prev == prev_host).all()
    b.set_active(valid)                                      # stream 1 never gets a picture
    expect_prev = prev_host.copy()
    distances = []
    for f, ptype in enumerate((h263mi.PICTURE_I, h263mi.PICTURE_P, h263mi.PICTURE_P)):
        b.decode(ptype, recs[f][0].ptr, recs[f][1].ptr, recs[f][2].ptr, 0, 5, rgba.ptr, None)
        # no sync in front of it: ordered behind the decode
        rcs = b.hist_last(0, desc, *bufs.args())
        assert rcs == [0, h263mi.ERR_NO_PICTURE, 0]
        b.sync()
        luma = np.stack([b.copy_yuv(s)[0].reshape(h, w) if valid[s] else np.zeros((h, w), np.uint8) for s in range(n)])
        want_hist, want_stats, want_sel = _expect(luma, expect_prev, valid, lo, hi, cut)
        hist, prev, stats, list_got, count = bufs.read("%s, picture %d" % (mode, f))
        assert (hist == want_hist).all() and hc.stats_tuples(stats) == want_stats, (mode, f)
        assert count == len(want_sel) and list_got[:count].tolist() == want_sel, (mode, f)
        assert want_stats[0][2] > 0 and want_stats[1] == ref.ZERO_STATS
        distances.append(want_stats[0][2])
        for s in (0, 2):
            expect_prev[s] = want_hist[s]
        assert (prev == expect_prev).all(), "stream 1's prev intact, the others rolled"
    assert len(set(distances)) == 3
    # the chroma planes, against copy_yuv's
    for plane in (1, 2):
        cb = Buffers(n, None)
        assert b.hist_last(plane, h263mi.make_hist(lo, hi, 0), *cb.args(lst=False)) == [0, h263mi.ERR_NO_PICTURE, 0]
        b.sync()
        cw, ch = (w + 1) // 2, (h + 1) // 2
        chroma = np.stack([b.copy_yuv(s)[plane].reshape(ch, cw) if valid[s] else np.zeros((ch, cw), np.uint8) for s in range(n)])
        want_hist, want_stats, _ = _expect(chroma, [None] * n, valid, lo, hi, 0)
        hist, _, stats, _, _ = cb.read("plane %d" % plane)
        assert (hist == want_hist).all() and hc.stats_tuples(stats) == want_stats and hist[0].sum() == cw * ch
        cb.free()
    # without per-stream codes a stream without a picture is the call's code, after the rest was queued
    with pytest.raises(h263mi.H263Error) as e:
        b.hist_last(0, desc, *bufs.args(), stream_rc=None)
    assert e.value.code == h263mi.ERR_NO_PICTURE
    b.sync()
    hist, prev, stats, list_got, count = bufs.read("rolled")
    assert count == 0 and not stats["distance"].any() and (hist == want_hist_luma(b, valid, n, w, h)).all()
    # a plane above 2 is refused
    with pytest.raises(h263mi.H263Error) as e:
        b.hist_last(3, desc, *bufs.args())
    assert e.value.code == h263mi.ERR_INVALID_ARGUMENT
    bufs.free()
    b.close()
    rgba.free()


def want_hist_luma(b, valid, n, w, h):
    luma = np.stack([b.copy_yuv(s)[0].reshape(h, w) if valid[s] else np.zeros((h, w), np.uint8) for s in range(n)])
    return np.where(np.asarray(valid)[:, None], ref.histograms(luma), 0)


def test_state_hist_last():
    w, h = 100, 60
    lo, hi, cut = 100, 900, 10
    st = h263mi.H263State(h263mi.SORENSON_SPARK_BITSTREAM, device_id=0)
    desc = h263mi.make_hist(lo, hi, cut, roll=1)
    bufs = Buffers(1, np.zeros((1, 256), np.uint32))
    with pytest.raises(h263mi.H263Error) as e:
        st.hist_last(0, desc, *bufs.args())
    assert e.value.code == h263mi.ERR_NO_PICTURE
    assert (bufs.read()[0] == WORD).all()                     # nothing was queued
    expect_prev = np.zeros((1, 256), np.uint32)
    for f in range(2):
        if f == 0:
            mbs, co = recgen.intra_picture(w, h, seed=41)
            st.submit_picture(w, h, mbs, co, h263mi.PICTURE_I, temporal_reference=0, pquant=8)
        else:
            mbs, co = recgen.inter_picture(w, h, seed=42, mv_range=30, p_4v=0.2, p_coded=0.5, quant=8)
            st.submit_picture(w, h, mbs, co, h263mi.PICTURE_P, temporal_reference=1, pquant=8)
        st.hist_last(0, desc, *bufs.args())
        luma = st.get_last_picture().as_yuv()[0].reshape(1, h, w)      # (waits for the stream)
        want_hist, want_stats, want_sel = _expect(luma, expect_prev, [True], lo, hi, cut)
        hist, prev, stats, list_got, count = bufs.read("picture %d" % f)
        assert (hist == want_hist).all() and hc.stats_tuples(stats) == want_stats and list_got[:count].tolist() == want_sel
        assert (prev == want_hist).all() and want_stats[0][2] > 0
        if f == 0:
            assert want_stats[0][2] == w * h and want_sel == [0]          # a zeroed prev: distance P on the first call
        expect_prev = want_hist.astype(np.uint32)
    bufs.free()
    st.close()


# ---------------------------------------------------------------------------------------------
# 3. h263mi_batch_hist over a default d_deblocked buffer
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["plain", "pipeline_post"])
def test_batch_hist_over_a_deblocked_buffer(three_pictures, mode):
    n, w, h, recs = three_pictures
    lo, hi, cut = 10, 990, 5
    picture = w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)
    b = h263mi.Batch(n, w, h, 0, None, pipeline_post=mode == "pipeline_post")
    planes = h263mi.DeviceBuffer(n * picture)
    pset = h263mi.planes_default_set(planes.ptr.value, n, w, h)
    bufs = Buffers(n, np.zeros((n, 256), np.uint32))
    expect_prev = np.zeros((n, 256), np.uint32)
    for f, ptype in enumerate((h263mi.PICTURE_I, h263mi.PICTURE_P)):
        b.decode(ptype, recs[f][0].ptr, recs[f][1].ptr, recs[f][2].ptr, 0, 5, None, planes.ptr)
        # (no sync here: a pipelined batch has only deferred its rendering -- the call delivers it)
        b.hist(pset, h263mi.make_hist(lo, hi, cut, roll=1), *bufs.args())
        b.sync()
        luma = planes.download().reshape(n, picture)[:, :w * h].reshape(n, h, w)
        want_hist, want_stats, want_sel = _expect(luma, expect_prev, [True] * n, lo, hi, cut)
        hist, prev, stats, list_got, count = bufs.read("%s, picture %d" % (mode, f))
        assert (hist == want_hist).all() and hc.stats_tuples(stats) == want_stats, (mode, f)
        assert count == len(want_sel) and list_got[:count].tolist() == want_sel and (prev == want_hist).all()
        assert all(s[2] for s in want_stats)
        expect_prev = want_hist.astype(np.uint32)
    bufs.free()
    b.close()
    planes.free()
