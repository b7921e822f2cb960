"""GPU tests of the change maps (h263mi_change_map_on, h263mi_batch_change_map, h263mi_batch_change_last, h263mi_change_last:
k_change, k_change_select).  Every comparison is exact, against change_ref: cells, summaries, the list, the count, prev after a roll,
and the sentinels around every output.  The cases are the ones the kernel is run at lane by lane on the CPU
(change_cases.CASES), where every hazard of theirs is shown to occur."""
import numpy as np
import pytest
import torch  # before the library is loaded: torch brings its own HIP runtime, which the C-ABI library must share (as in bench.py)

import change_cases as cc
import change_ref as ref
import h263mi
import recgen

pytestmark = pytest.mark.gpu
SENTINEL = 0xC3
GUARD = 64                                                   # sentinel bytes in front of and behind every device buffer


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if h263mi.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the MI355X box")


@pytest.fixture(scope="module")
def stream():
    return torch.cuda.Stream(device=0)


def _guarded(data):
    """a device buffer of GUARD sentinels, the bytes of `data`, GUARD sentinels -> (buffer, what it holds now)"""
    host = np.concatenate([np.full(GUARD, SENTINEL, np.uint8), np.ascontiguousarray(data).view(np.uint8).ravel(),
                           np.full(GUARD, SENTINEL, np.uint8)])
    d = h263mi.DeviceBuffer(host.size)
    d.upload(host)
    return d, host


class Outputs:
    """the grids, the summaries, the list and the count of one call, each in sentinels"""

    def __init__(self, n, gw, gh):
        self.n, self.gw, self.gh = n, gw, gh
        self.cells, self.cells0 = _guarded(np.full(n * gw * gh * 4, SENTINEL, np.uint8))
        self.summary, self.summary0 = _guarded(np.full(n * 16, SENTINEL, np.uint8))
        self.list, self.list0 = _guarded(np.full(n * 4, SENTINEL, np.uint8))
        self.count, self.count0 = _guarded(np.full(4, SENTINEL, np.uint8))
        self.cells_bytes = n * gw * gh * 4

    def read(self):
        """-> (grids, summaries, list words, count); the guards are checked"""
        out = []
        for d, first in ((self.cells, self.cells0), (self.summary, self.summary0), (self.list, self.list0), (self.count, self.count0)):
            raw = d.download()
            assert (raw[:GUARD] == SENTINEL).all() and (raw[-GUARD:] == SENTINEL).all(), "a guard was written"
            out.append(raw[GUARD:-GUARD])
        return (out[0].view(np.uint32).reshape(self.n, self.gh, self.gw), out[1].view(h263mi.CHANGE_SUMMARY_DTYPE), out[2].view(np.uint32),
                int(out[3].view(np.uint32)[0]))

    def raw(self):
        return [d.download() for d in (self.cells, self.summary, self.list, self.count)]

    def free(self):
        for d in (self.cells, self.summary, self.list, self.count):
            d.free()


def _check_outputs(got, grid, summ, sel, valid, what, cells=True, lst=True):
    cells_got, summ_got, list_got, count = got
    word = SENTINEL * 0x01010101
    if cells:
        want = np.where(np.asarray(valid)[:, None, None], grid, word)
        bad = np.argwhere(cells_got != want)
        assert bad.size == 0, "%s: %d cells differ, first (p, cy, cx) = %s: %#x, want %#x" % (
            what, len(bad), bad[0], cells_got[tuple(bad[0])], want[tuple(bad[0])])
    else:
        assert (cells_got == word).all(), what + ": no grid was wanted"
    assert [tuple(int(v) for v in s) for s in summ_got] == summ, what
    if lst:
        assert count == len(sel) and list_got[:count].tolist() == sel, (what, count, list_got[:count].tolist(), sel)
        assert (list_got[count:] == word).all(), what + ": entries behind the count were written"
    else:
        assert count == word and (list_got == word).all(), what + ": no list was wanted"


def _sets(b, d_cur, d_prev):
    cur = h263mi.PlaneSet(d_cur.ptr.value + GUARD + b.cur_off, b.cur_buf.size - b.cur_off, b.cur_pitch, b.cur_stride)
    prev = h263mi.PlaneSet(d_prev.ptr.value + GUARD + b.prev_off, b.prev_buf.size - b.prev_off, b.prev_pitch, b.prev_stride)
    return cur, prev


def _change_of(b, roll=None):
    return h263mi.make_change(b.cl, b.thr, b.min_changed, b.roll if roll is None else roll)


def _prev_after(d_prev, host0, want, what):
    raw = d_prev.download()
    assert (raw[:GUARD] == SENTINEL).all() and (raw[-GUARD:] == SENTINEL).all(), what + ": a guard of prev was written"
    bad = np.flatnonzero(raw[GUARD:-GUARD] != want)
    assert bad.size == 0, "%s: prev differs at byte %d (%d bytes)" % (what, bad[0], bad.size)


GPU_CASES = [name for name in cc.CASES if not cc.CASES[name].get("words")]         # (the plain entry point has no per-picture words)


# ---------------------------------------------------------------------------------------------
# 1. the case table through h263mi_change_map_on
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GPU_CASES)
def test_cases(stream, name):
    b = cc.build(name)
    grid, summ, sel, after = cc.expected(b)
    d_cur, _ = _guarded(b.cur_buf)
    d_prev, prev0 = _guarded(b.prev_buf)
    out = Outputs(b.n, b.gw, b.gh)
    assert h263mi.change_extent(b.n, b.w, b.h, _change_of(b)) == (b.gw, b.gh, out.cells_bytes)
    cur, prev = _sets(b, d_cur, d_prev)
    h263mi.change_map(cur, prev, b.n, b.w, b.h, _change_of(b), out.cells.at(GUARD), out.cells_bytes, out.summary.at(GUARD),
                      out.list.at(GUARD), out.count.at(GUARD), stream=stream.cuda_stream)
    stream.synchronize()
    _check_outputs(out.read(), grid, summ, sel, b.valid, name)
    _prev_after(d_prev, prev0, after, name)
    assert (d_cur.download()[GUARD:-GUARD] == b.cur_buf).all(), "cur is read only"
    for d in (d_cur, d_prev):
        d.free()
    out.free()


@pytest.mark.parametrize("name", ["size_176x144_c16", "size_1025x9_c8", "corners_c32", "base_5_1"])
def test_roll_then_a_second_call_gives_all_zeros(stream, name):
    b = cc.build(name)
    grid, summ, sel, _ = cc.expected(b)
    d_cur, _ = _guarded(b.cur_buf)
    d_prev, prev0 = _guarded(b.prev_buf)
    cur, prev = _sets(b, d_cur, d_prev)
    rolled = b.prev_buf.copy()
    for p in range(b.n):
        cc._rows(rolled, b.prev_off, b.prev_pitch, b.prev_stride, p, b.w, b.h)[:] = b.cur_planes[p]
    for k in range(2):
        out = Outputs(b.n, b.gw, b.gh)
        h263mi.change_map(cur, prev, b.n, b.w, b.h, _change_of(b, roll=1), out.cells.at(GUARD), out.cells_bytes, out.summary.at(GUARD),
                          out.list.at(GUARD), out.count.at(GUARD), stream=stream.cuda_stream)
        stream.synchronize()
        if k == 0:
            _check_outputs(out.read(), grid, summ, sel, b.valid, name)
        else:
            zero = [(0, 0, 0)] * b.n
            _check_outputs(out.read(), np.zeros_like(grid), zero, ref.select(zero, b.min_changed), b.valid, name + ", second call")
        _prev_after(d_prev, prev0, rolled, name)              # prev equals cur in the rows, the padding is untouched
        out.free()
    for d in (d_cur, d_prev):
        d.free()


def test_the_call_is_ordered_behind_a_copy_queued_on_its_stream(stream):
    """cur arrives behind 512 MiB of device-to-device copy on the same stream and the host waits for neither: a call that ran
    early, or on another stream, would compare prev with the copy of prev that cur's buffer held before, and find nothing"""
    b = cc.build("size_176x144_c16")
    grid, summ, sel, _ = cc.expected(b)
    assert sel and all(s[0] for s in summ)
    ballast = (torch.zeros(512 << 20, dtype=torch.uint8, device="cuda"), torch.empty(512 << 20, dtype=torch.uint8, device="cuda"))
    staged = torch.from_numpy(b.cur_buf.copy()).cuda()
    decoy = b.cur_buf.copy()                                  # prev's pictures in cur's placement
    for p in range(b.n):
        cc._rows(decoy, b.cur_off, b.cur_pitch, b.cur_stride, p, b.w, b.h)[:] = b.prev_planes[p]
    d_cur = torch.from_numpy(decoy).cuda()
    d_prev = torch.from_numpy(b.prev_buf.copy()).cuda()
    out = Outputs(b.n, b.gw, b.gh)
    cur = h263mi.PlaneSet(d_cur.data_ptr() + b.cur_off, b.cur_buf.size - b.cur_off, b.cur_pitch, b.cur_stride)
    prev = h263mi.PlaneSet(d_prev.data_ptr() + b.prev_off, b.prev_buf.size - b.prev_off, b.prev_pitch, b.prev_stride)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        ballast[1].copy_(ballast[0], non_blocking=True)
        d_cur.copy_(staged, non_blocking=True)
    h263mi.change_map(cur, prev, b.n, b.w, b.h, _change_of(b, roll=0), out.cells.at(GUARD), out.cells_bytes, out.summary.at(GUARD),
                      out.list.at(GUARD), out.count.at(GUARD), stream=stream.cuda_stream)
    stream.synchronize()
    _check_outputs(out.read(), grid, summ, sel, b.valid, "behind the copy")
    out.free()


def test_two_runs_give_identical_bytes(stream):
    b = cc.build("size_2049x8_c8")
    runs = []
    for _ in range(2):
        d_cur, _g = _guarded(b.cur_buf)
        d_prev, _g = _guarded(b.prev_buf)
        cur, prev = _sets(b, d_cur, d_prev)
        out = Outputs(b.n, b.gw, b.gh)
        h263mi.change_map(cur, prev, b.n, b.w, b.h, _change_of(b), out.cells.at(GUARD), out.cells_bytes, out.summary.at(GUARD),
                          out.list.at(GUARD), out.count.at(GUARD), stream=stream.cuda_stream)
        stream.synchronize()
        runs.append(out.raw() + [d_prev.download()])
        out.free()
        d_cur.free()
        d_prev.free()
    assert all((x == y).all() for x, y in zip(*runs))


def test_no_grid_no_list_and_no_pictures(stream):
    b = cc.build("size_100x60_c16")
    grid, summ, sel, after = cc.expected(b)
    d_cur, _ = _guarded(b.cur_buf)
    d_prev, prev0 = _guarded(b.prev_buf)
    cur, prev = _sets(b, d_cur, d_prev)
    out = Outputs(b.n, b.gw, b.gh)
    h263mi.change_map(cur, prev, b.n, b.w, b.h, _change_of(b), None, 0, out.summary.at(GUARD), None, None, stream=stream.cuda_stream)
    stream.synchronize()
    _check_outputs(out.read(), grid, summ, sel, b.valid, "summaries alone", cells=False, lst=False)
    h263mi.change_map(cur, prev, b.n, b.w, b.h, _change_of(b), None, 0, out.summary.at(GUARD), out.list.at(GUARD), out.count.at(GUARD),
                      stream=stream.cuda_stream)
    stream.synchronize()
    _check_outputs(out.read(), grid, summ, sel, b.valid, "no grid", cells=False)
    out.free()
    # no pictures: nothing but the count, which becomes 0
    out = Outputs(b.n, b.gw, b.gh)
    h263mi.change_map(None, None, 0, b.w, b.h, _change_of(b), None, 0, None, out.list.at(GUARD), out.count.at(GUARD), stream=stream.cuda_stream)
    stream.synchronize()
    cells_got, summ_got, list_got, count = out.read()
    assert count == 0 and (list_got == SENTINEL * 0x01010101).all() and (summ_got.view(np.uint8) == SENTINEL).all()
    out.free()
    _prev_after(d_prev, prev0, after, "prev")
    for d in (d_cur, d_prev):
        d.free()


def test_a_failure_of_the_runtime_at_every_call_is_reported_and_the_same_call_then_succeeds(stream):
    """the injected return code of h263mi_debug_fail_nth_hip_call: nothing faults on the device.  Under roll: a failed call has
    not rolled anything"""
    b = cc.build("base_1_0")
    assert b.roll == 1
    grid, summ, sel, after = cc.expected(b)
    failures = 0
    for nth in range(1, 10):
        d_cur, _ = _guarded(b.cur_buf)
        d_prev, prev0 = _guarded(b.prev_buf)
        cur, prev = _sets(b, d_cur, d_prev)
        out = Outputs(b.n, b.gw, b.gh)
        call = lambda: h263mi.change_map(cur, prev, b.n, b.w, b.h, _change_of(b), out.cells.at(GUARD), out.cells_bytes, out.summary.at(GUARD),
                                         out.list.at(GUARD), out.count.at(GUARD), stream=stream.cuda_stream)
        h263mi.debug_fail_nth_hip_call(nth)
        try:
            call()
            fired = h263mi.debug_fail_nth_hip_call(0) <= 0
            assert not fired, "the %d-th HIP call failed and the call reported success" % nth
            done = True
        except h263mi.H263Error as e:
            h263mi.debug_fail_nth_hip_call(0)
            assert e.code == h263mi.ERR_HIP, (nth, e.code)
            failures += 1
            done = False
            stream.synchronize()
            _prev_after(d_prev, prev0, b.prev_buf, "after failure %d" % nth)
            call()
        stream.synchronize()
        _check_outputs(out.read(), grid, summ, sel, b.valid, "nth = %d" % nth)
        _prev_after(d_prev, prev0, after, "nth = %d" % nth)
        out.free()
        d_cur.free()
        d_prev.free()
        if done:
            break
    else:
        pytest.fail("the call never went through")
    assert failures == 2                                      # the clearing of the summaries, the launches


# ---------------------------------------------------------------------------------------------
# 2. the frame store in place: h263mi_batch_change_last, h263mi_change_last
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
    recs = [_upload([recgen.intra_picture(w, h, seed=7300 + s) for s in range(n)])]
    for f in (1, 2):
        recs.append(_upload([recgen.inter_picture(w, h, seed=7300 + 10 * f + s, mv_range=30, p_4v=0.2, p_coded=0.5, quant=8) for s in range(n)]))
    return n, w, h, recs


@pytest.mark.parametrize("mode", ["plain", "pipeline_post", "overlap_post"])
def test_batch_change_last_follows_the_last_picture_across_both_frame_sets(three_pictures, mode):
    n, w, h, recs = three_pictures
    cl, thr = 4, 300
    c = 1 << cl
    pitch, stride = w + 3, h * (w + 3) + 11                  # byte accesses for prev; cur is the frame store's aligned luma
    prev_bytes = (n - 1) * stride + (h - 1) * pitch + w
    rng = np.random.default_rng(77)
    prev_host = rng.integers(0, 256, prev_bytes, dtype=np.uint8)
    d_prev, prev0 = _guarded(prev_host)
    prev = h263mi.PlaneSet(d_prev.ptr.value + GUARD, prev_bytes, pitch, stride)
    change = h263mi.make_change(cl, thr, min_changed_cells=0, roll=1)
    gw, gh, cells_bytes = h263mi.change_extent(n, w, h, change)
    b = h263mi.Batch(n, w, h, 0, None, pipeline_post=mode == "pipeline_post", overlap_post=mode == "overlap_post")
    rgba = h263mi.DeviceBuffer(n * w * h * 4)
    valid = [True, False, True]
    # before any picture: every stream is invalid, nothing is touched, nobody is selected
    out = Outputs(n, gw, gh)
    rcs = b.change_last(prev, change, out.cells.at(GUARD), cells_bytes, out.summary.at(GUARD), out.list.at(GUARD), out.count.at(GUARD))
    b.sync()
    assert rcs == [h263mi.ERR_NO_PICTURE] * n
    _check_outputs(out.read(), np.zeros((n, gh, gw), np.int64), [(0, 0, 0)] * n, [], [False] * n, "no pictures")
    _prev_after(d_prev, prev0, prev_host, "no pictures")
    out.free()
    b.set_active(valid)                                      # stream 1 never gets a picture
    before = np.stack([cc._rows(prev_host, 0, pitch, stride, p, w, h) for p in range(n)]).copy()
    expect_prev = prev_host.copy()
    sums = []
    for f, ptype in enumerate((h263mi.PICTURE_I, h263mi.PICTURE_P, h263mi.PICTURE_P)):
        b.decode(ptype, recs[f][0].ptr, recs[f][1].ptr, recs[f][2].ptr, 0, 5, rgba.ptr, None)
        out = Outputs(n, gw, gh)
        # no sync in front of it: ordered behind the decode
        rcs = b.change_last(prev, change, out.cells.at(GUARD), cells_bytes, out.summary.at(GUARD), out.list.at(GUARD), out.count.at(GUARD))
        assert rcs == [0, h263mi.ERR_NO_PICTURE, 0]
        b.sync()
        luma = np.stack([b.copy_yuv(s)[0].reshape(h, w) if valid[s] else before[s] for s in range(n)])
        grid = ref.cells(luma, before, c)
        summ = ref.summaries(grid, w, h, c, thr, valid)
        _check_outputs(out.read(), grid, summ, [0, 2], valid, "%s, picture %d" % (mode, f))
        assert summ[0][0] and summ[2][0] and summ[1] == (0, 0, 0)
        sums.append(summ[0][0])
        for s in (0, 2):
            cc._rows(expect_prev, 0, pitch, stride, s, w, h)[:] = luma[s]
        _prev_after(d_prev, prev0, expect_prev, "%s, picture %d" % (mode, f))     # stream 1's prev and all padding intact
        before = luma
        out.free()
    assert len(set(sums)) == 3
    # without per-stream codes a stream without a picture is the call's code, after the rest was queued
    out = Outputs(n, gw, gh)
    with pytest.raises(h263mi.H263Error) as e:
        b.change_last(prev, change, out.cells.at(GUARD), cells_bytes, out.summary.at(GUARD), out.list.at(GUARD), out.count.at(GUARD),
                      stream_rc=None)
    assert e.value.code == h263mi.ERR_NO_PICTURE
    b.sync()
    _check_outputs(out.read(), np.zeros((n, gh, gw), np.int64), [(0, 0, 0)] * n, [0, 2], valid, "rolled: nothing changed")
    # under roll prev may not lie in the frame store, wherever that is: refused as an argument -- here by its NULL base
    with pytest.raises(h263mi.H263Error) as e:
        b.change_last(h263mi.PlaneSet(None, prev_bytes, pitch, stride), change, None, 0, out.summary.at(GUARD))
    assert e.value.code == h263mi.ERR_INVALID_ARGUMENT
    out.free()
    b.close()
    d_prev.free()
    rgba.free()


def test_state_change_last():
    w, h, cl = 100, 60, 3
    c = 1 << cl
    st = h263mi.H263State(h263mi.SORENSON_SPARK_BITSTREAM, device_id=0)
    change = h263mi.make_change(cl, 100, 1, roll=1)
    gw, gh, cells_bytes = h263mi.change_extent(1, w, h, change)
    prev_host = np.random.default_rng(5).integers(0, 256, w * h, dtype=np.uint8)
    d_prev, prev0 = _guarded(prev_host)
    prev = h263mi.PlaneSet(d_prev.ptr.value + GUARD, w * h, w, w * h)
    out = Outputs(1, gw, gh)
    args = (prev, change, out.cells.at(GUARD), cells_bytes, out.summary.at(GUARD), out.list.at(GUARD), out.count.at(GUARD))
    with pytest.raises(h263mi.H263Error) as e:
        st.change_last(*args)
    assert e.value.code == h263mi.ERR_NO_PICTURE
    before = prev_host.reshape(1, h, w)
    for f in range(2):
        if f == 0:
            mbs, co = recgen.intra_picture(w, h, seed=31)
            st.submit_picture(w, h, mbs, co, h263mi.PICTURE_I, temporal_reference=0, pquant=8)
        else:
            mbs, co = recgen.inter_picture(w, h, seed=32, mv_range=30, p_4v=0.2, p_coded=0.5, quant=8)
            st.submit_picture(w, h, mbs, co, h263mi.PICTURE_P, temporal_reference=1, pquant=8)
        st.change_last(*args)
        luma = st.get_last_picture().as_yuv()[0].reshape(1, h, w)      # (waits for the stream)
        grid = ref.cells(luma, before, c)
        summ = ref.summaries(grid, w, h, c, 100)
        _check_outputs(out.read(), grid, summ, ref.select(summ, 1), [True], "picture %d" % f)
        assert summ[0][0] > 0
        _prev_after(d_prev, prev0, luma.ravel(), "picture %d" % f)
        before = luma
        out.free()
        out = Outputs(1, gw, gh)
        args = (prev, change, out.cells.at(GUARD), cells_bytes, out.summary.at(GUARD), out.list.at(GUARD), out.count.at(GUARD))
    out.free()
    st.close()
    d_prev.free()


# ---------------------------------------------------------------------------------------------
# 3. h263mi_batch_change_map over two default d_deblocked buffers that the caller alternates between
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["plain", "pipeline_post"])
def test_batch_change_map_over_two_alternating_plane_buffers(three_pictures, mode):
    n, w, h, recs = three_pictures
    cl, thr = 5, 2000
    c = 1 << cl
    picture = w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)
    b = h263mi.Batch(n, w, h, 0, None, pipeline_post=mode == "pipeline_post")
    planes = [h263mi.DeviceBuffer(n * picture) for _ in range(2)]
    sets = [h263mi.planes_default_set(d.ptr.value, n, w, h) for d in planes]
    assert sets[0].bytes == n * picture and sets[0].pitch == w and sets[0].picture_stride == picture
    change = h263mi.make_change(cl, thr, 1, roll=0)
    gw, gh, cells_bytes = h263mi.change_extent(n, w, h, change)
    b.decode(h263mi.PICTURE_I, recs[0][0].ptr, recs[0][1].ptr, recs[0][2].ptr, 0, 5, None, planes[0].ptr)
    for f in (1, 2):
        k = f & 1
        b.decode(h263mi.PICTURE_P, recs[f][0].ptr, recs[f][1].ptr, recs[f][2].ptr, 0, 5, None, planes[k].ptr)
        out = Outputs(n, gw, gh)
        # (no sync here: a pipelined batch has only deferred its rendering -- the call delivers it)
        b.change_map(sets[k], sets[k ^ 1], change, out.cells.at(GUARD), cells_bytes, out.summary.at(GUARD), out.list.at(GUARD), out.count.at(GUARD))
        b.sync()
        luma = [planes[j].download().reshape(n, picture)[:, :w * h].reshape(n, h, w) for j in (k, k ^ 1)]
        grid = ref.cells(luma[0], luma[1], c)
        summ = ref.summaries(grid, w, h, c, thr)
        assert all(s[0] for s in summ)
        _check_outputs(out.read(), grid, summ, ref.select(summ, 1), [True] * n, "%s, picture %d" % (mode, f))
        out.free()
    b.close()
    for d in planes:
        d.free()
