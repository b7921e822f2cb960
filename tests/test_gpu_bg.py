"""GPU tests of the background model (h263mi_background_on, h263mi_batch_background, h263mi_batch_background_last,
h263mi_background_last: k_bg_begin, k_bg, k_change_select).  Every comparison is exact, against bg_ref: after EVERY call of a
sequence the whole state, the mask, the cells, the summaries, the list, the count, and the sentinels around every device buffer.
The cases are the ones the kernels are run at lane by lane on the CPU (bg_cases.CASES), where every hazard of theirs is shown to
occur.  The chain test queues, picture after picture, decode -> background_last -> regions -> tracks with no host read before the end,
on an object that stops: its track lives, and with change_last in the background model's place it dies."""
import numpy as np
import pytest
import torch  # before the library is loaded: torch brings its own HIP runtime, which the C-ABI library must share (as in bench.py)

import bg_cases as bc
import bg_ref as ref
import h263mi
import recgen
import regions_ref
import tracks_ref

pytestmark = pytest.mark.gpu
SENTINEL = 0xC3
WORD = SENTINEL * 0x01010101
GUARD = 64                                                   # sentinel bytes in front of and behind every device buffer (a multiple of 32)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if h263mi.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the MI355X box")


@pytest.fixture(scope="module")
def stream():
    return torch.cuda.Stream(device=0)


def _guarded(data):
    host = np.concatenate([np.full(GUARD, SENTINEL, np.uint8), np.ascontiguousarray(data).view(np.uint8).ravel(),
                           np.full(GUARD, SENTINEL, np.uint8)])
    d = h263mi.DeviceBuffer(host.size)
    d.upload(host)
    return d


def _inside(d, dtype=np.uint8):
    raw = d.download()
    assert (raw[:GUARD] == SENTINEL).all() and (raw[-GUARD:] == SENTINEL).all(), "a guard was written"
    return raw[GUARD:-GUARD].view(dtype)


def _sentinels(nbytes):
    return np.full(nbytes, SENTINEL, np.uint8)


def _background_of(prm):
    return h263mi.make_background(prm.cl, prm.learn, prm.fg_learn, prm.pix_thr, prm.warmup, prm.cell_thr, prm.min_changed)


class Outputs:
    """the grids, the summaries, the list and the count of one call, each in sentinels"""

    def __init__(self, n, gw, gh):
        self.n, self.gw, self.gh = n, gw, gh
        self.cells_bytes = n * gw * gh * 4
        self.cells, self.summary = _guarded(_sentinels(self.cells_bytes)), _guarded(_sentinels(n * 16))
        self.list, self.count = _guarded(_sentinels(n * 4)), _guarded(_sentinels(4))

    def args(self, cells=True, lst=True):
        return dict(d_cells=self.cells.at(GUARD) if cells else None, cells_bytes=self.cells_bytes if cells else 0, d_summary=self.summary.at(GUARD),
                    d_selected=self.list.at(GUARD) if lst else None, d_count=self.count.at(GUARD) if lst else None)

    def read(self):
        return (_inside(self.cells, np.uint32).reshape(self.n, self.gh, self.gw), _inside(self.summary, h263mi.CHANGE_SUMMARY_DTYPE),
                _inside(self.list, np.uint32), int(_inside(self.count, np.uint32)[0]))

    def raw(self):
        return [d.download() for d in (self.cells, self.summary, self.list, self.count)]

    def free(self):
        for d in (self.cells, self.summary, self.list, self.count):
            d.free()


def _check_outputs(got, cells, summ, sel, what, want_cells=True, lst=True):
    cells_got, summ_got, list_got, count = got
    if want_cells:
        bad = np.argwhere(cells_got != cells)
        assert bad.size == 0, "%s: %d cells differ, first (p, cy, cx) = %s: %#x, want %#x" % (
            what, len(bad), bad[0], cells_got[tuple(bad[0])], cells[tuple(bad[0])])
    else:
        assert (cells_got == WORD).all(), what + ": no grid was wanted"
    assert [tuple(int(v) for v in s) for s in summ_got] == summ, what
    if lst:
        assert count == len(sel) and list_got[:count].tolist() == sel, (what, count, list_got[:count].tolist(), sel)
        assert (list_got[count:] == WORD).all(), what + ": entries behind the count were written"
    else:
        assert count == WORD and (list_got == WORD).all(), what + ": no list was wanted"


def _same(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s differs at byte %d (%d bytes)" % (what, bad[0], bad.size)


class Sequence:
    """the device buffers of case b: the state and the mask live on through the calls, the outputs are sentinels before each"""

    def __init__(self, b, mask=True):
        self.b = b
        self.bg = _background_of(b.prm)
        self.gw, self.gh, self.cells_bytes, self.state_bytes = h263mi.background_extent(b.n, b.w, b.h, self.bg)
        assert (self.gw, self.gh, self.state_bytes) == (b.gw, b.gh, b.state0.size)
        self.state = _guarded(b.state0)
        self.mask = _guarded(b.mask0) if b.mask and mask else None
        self.bufs = []

    def call(self, q, run, **how):
        """one call: run(**arguments) queues it -> its Outputs"""
        b = self.b
        cur = _guarded(q.cur_buf)
        cut = _guarded(np.concatenate([q.cut, q.cut_extra])) if q.cut is not None else None      # (entries that the count names but no call may read)
        cut_count = _guarded(np.array([q.cut_count], np.uint32)) if q.cut is not None else None
        out = Outputs(b.n, b.gw, b.gh)
        mask = h263mi.PlaneSet(self.mask.ptr.value + GUARD + b.mask_off, b.mask0.size - b.mask_off, b.mask_pitch, b.mask_stride) if self.mask else None
        self.bufs += [d for d in (cur, cut, cut_count) if d]
        self.inputs = [(cur, q.cur_buf)] + ([(cut, np.concatenate([q.cut, q.cut_extra]))] if cut else [])
        run(cur=h263mi.PlaneSet(cur.ptr.value + GUARD + b.cur_off, q.cur_buf.size - b.cur_off, b.cur_pitch, b.cur_stride), background=self.bg,
            d_state=self.state.at(GUARD), state_bytes=self.state_bytes, mask=mask, d_cut=cut.at(GUARD) if cut else None,
            d_cut_count=cut_count.at(GUARD) if cut else None, **out.args(**how))
        return out

    def check(self, k, out, what, **how):
        want_state, want_mask, cells, summ, sel, _ = bc.expected(self.b)[k]
        _check_outputs(out.read(), cells, summ, sel, what, **{"want_cells": how.get("cells", True), "lst": how.get("lst", True)})
        _same(_inside(self.state), want_state, what + ": the state")
        if self.mask:
            _same(_inside(self.mask), want_mask, what + ": the mask")
        for d, host in self.inputs:
            assert _inside(d).tobytes() == host.tobytes(), what + ": the inputs are read only"

    def free(self):
        for d in self.bufs + [self.state] + ([self.mask] if self.mask else []):
            d.free()


GPU_CASES = [name for name in bc.CASES if not any(s["words"] for s in bc.CASES[name]["calls"] if isinstance(s, dict))]


# ---------------------------------------------------------------------------------------------
# 1. the case table through h263mi_background_on
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GPU_CASES)
def test_cases(stream, name):
    b = bc.build(name)
    s = Sequence(b)
    for k, q in enumerate(b.calls):
        out = s.call(q, lambda **a: h263mi.background_on(n_pictures=b.n, width=b.w, height=b.h, stream=stream.cuda_stream, **a))
        stream.synchronize()
        s.check(k, out, "%s, call %d" % (name, k))
        out.free()
    s.free()


@pytest.mark.parametrize("name", ["size_1025x9_c8", "warmup_3", "init_by_cut"])
def test_a_sequence_queued_without_a_host_read_between_its_calls(stream, name):
    """the calls of a sequence are ordered by the stream alone: what every one of them leaves is what the reference leaves"""
    b = bc.build(name)
    s = Sequence(b)
    outs = [s.call(q, lambda **a: h263mi.background_on(n_pictures=b.n, width=b.w, height=b.h, stream=stream.cuda_stream, **a)) for q in b.calls]
    stream.synchronize()
    want = bc.expected(b)
    for k, out in enumerate(outs):
        _check_outputs(out.read(), want[k][2], want[k][3], want[k][4], "%s, call %d" % (name, k))
        out.free()
    _same(_inside(s.state), want[-1][0], "the state")
    if s.mask:
        _same(_inside(s.mask), want[-1][1], "the mask")
    s.free()


def test_no_grid_no_list_no_mask_and_no_pictures(stream):
    b = bc.build("size_100x60_c32")
    assert b.mask
    for how, mask in ((dict(cells=False, lst=False), True), (dict(cells=False), False), (dict(lst=False), True)):
        s = Sequence(b, mask=mask)
        for k, q in enumerate(b.calls):
            out = s.call(q, lambda **a: h263mi.background_on(n_pictures=b.n, width=b.w, height=b.h, stream=stream.cuda_stream, **a), **how)
            stream.synchronize()
            s.check(k, out, "%r, call %d" % (how, k), **how)
            out.free()
        s.free()
    # no pictures: nothing but the count, which becomes 0
    out = Outputs(b.n, b.gw, b.gh)
    h263mi.background_on(None, 0, b.w, b.h, _background_of(b.prm), None, 0, None, 0, None, out.list.at(GUARD), out.count.at(GUARD),
                         stream=stream.cuda_stream)
    stream.synchronize()
    _, summ_got, list_got, count = out.read()
    assert count == 0 and (list_got == WORD).all() and (summ_got.view(np.uint8) == SENTINEL).all()
    out.free()


def test_a_failure_of_the_runtime_is_reported_and_the_same_call_then_succeeds(stream):
    """the injected return code of h263mi_debug_fail_nth_hip_call: nothing faults on the device.  A failed call has changed nothing"""
    b = bc.build("size_100x60_c16")
    failures = 0
    for nth in range(1, 6):
        s = Sequence(b)
        q = b.calls[0]
        try:                                                 # (the hook is set behind the uploads of the call's buffers)
            out = s.call(q, lambda **a: (h263mi.debug_fail_nth_hip_call(nth),
                                         h263mi.background_on(n_pictures=b.n, width=b.w, height=b.h, stream=stream.cuda_stream, **a)))
            assert h263mi.debug_fail_nth_hip_call(0) > 0, "the %d-th HIP call failed and the call reported success" % nth
            done = True
        except h263mi.H263Error as e:
            h263mi.debug_fail_nth_hip_call(0)
            assert e.code == h263mi.ERR_HIP, (nth, e.code)
            failures += 1
            done = False
            stream.synchronize()
            _same(_inside(s.state), b.state0, "the state after failure %d" % nth)
            out = s.call(q, lambda **a: h263mi.background_on(n_pictures=b.n, width=b.w, height=b.h, stream=stream.cuda_stream, **a))
        stream.synchronize()
        s.check(0, out, "nth = %d" % nth)
        out.free()
        s.free()
        if done:
            break
    else:
        pytest.fail("the call never went through")
    assert failures == 1                                      # the launches


# ---------------------------------------------------------------------------------------------
# 2. the frame store in place: h263mi_batch_background_last, h263mi_background_last
# ---------------------------------------------------------------------------------------------
def _upload(pics):
    mbs = np.concatenate([m for m, _ in pics])
    co = np.concatenate([c for _, c in pics]).astype(np.int16)
    base = np.cumsum([0] + [c.shape[0] for _, c in pics[:-1]]).astype(np.uint64)
    bufs = []
    for arr in (mbs, co, base):
        d = h263mi.DeviceBuffer(max(arr.nbytes, 128))              # (a pool without a coded block still has room for one)
        d.upload(arr)
        bufs.append(d)
    return bufs


def test_batch_background_last_over_streams_of_which_one_has_no_picture():
    """three 176 x 144 streams, four pictures; stream 1 never gets one; stream 2 sits out the third decode, so that in the last
    call the streams' pictures lie in different frame sets; the cut list is the one a histogram call has just written"""
    n, w, h, pictures = 3, 176, 144, 4
    recs = [_upload([recgen.intra_picture(w, h, seed=8100 + s) for s in range(n)])]
    for f in range(1, pictures):
        pics = [recgen.inter_picture(w, h, seed=8100 + 10 * f + s, mv_range=30, p_4v=0.2, p_coded=0.5, quant=8) for s in range(n)]
        if f == 3:
            pics[0] = _block_picture(w, h, None, 0)          # stream 0's last picture is flat grey: a scene cut
        recs.append(_upload(pics))
    prm = ref.Params(cl=4, learn=2, fg_learn=5, pix_thr=12, warmup=0, cell_thr=20, min_changed=0)
    bg = _background_of(prm)
    gw, gh, cells_bytes, state_bytes = h263mi.background_extent(n, w, h, bg)
    hist = h263mi.make_hist(10, 990, cut_permille=400, roll=1)
    hist_bytes = h263mi.hist_extent(n, w, h, hist)
    d_hist, d_prev, d_stats = (h263mi.DeviceBuffer(hist_bytes), h263mi.DeviceBuffer(hist_bytes), h263mi.DeviceBuffer(n * 32))
    d_prev.upload(np.zeros(hist_bytes, np.uint8))
    state = _guarded(np.zeros(state_bytes, np.uint8))
    mask_host = np.random.default_rng(3).integers(0, 256, n * w * h, dtype=np.uint8)
    mask = _guarded(mask_host)
    mask_set = h263mi.PlaneSet(mask.ptr.value + GUARD, n * w * h, w, w * h)
    b = h263mi.Batch(n, w, h, 0, None)
    rgba = h263mi.DeviceBuffer(n * w * h * 4)
    # before any picture: every stream is invalid, nothing is touched, nobody is selected
    out = Outputs(n, gw, gh)
    rcs = b.background_last(bg, state.at(GUARD), state_bytes, mask=mask_set, **out.args())
    b.sync()
    assert rcs == [h263mi.ERR_NO_PICTURE] * n
    _check_outputs(out.read(), np.full((n, gh, gw), WORD, np.uint32), [(0, 0, 0)] * n, [], "no pictures")
    assert not _inside(state).any() and (_inside(mask) == mask_host).all()
    out.free()
    want_state, want_mask = np.zeros(state_bytes, np.uint8), mask_host.copy()
    luma = np.zeros((n, h, w), np.uint8)
    active = [[True, False, True], [True, False, True], [True, False, False], [True, False, True]]
    valid = [True, False, True]
    modes = []
    for f in range(pictures):
        b.set_active(active[f])
        b.decode(h263mi.PICTURE_I if f == 0 else h263mi.PICTURE_P, recs[f][0].ptr, recs[f][1].ptr, recs[f][2].ptr, 0, 5, rgba.ptr, None)
        cuts, cut_count = _guarded(_sentinels(n * 4)), _guarded(_sentinels(4))
        out = Outputs(n, gw, gh)
        # no sync between them: the histogram's list is read by the background call on the device
        assert b.hist_last(0, hist, d_hist.ptr, hist_bytes, d_stats.ptr, d_prev.ptr, hist_bytes, cuts.at(GUARD), cut_count.at(GUARD)) == \
            [0, h263mi.ERR_NO_PICTURE, 0]
        rcs = b.background_last(bg, state.at(GUARD), state_bytes, mask=mask_set, d_cut=cuts.at(GUARD), d_cut_count=cut_count.at(GUARD), **out.args())
        assert rcs == [0, h263mi.ERR_NO_PICTURE, 0]
        b.sync()
        for s in (0, 2):
            luma[s] = b.copy_yuv(s)[0].reshape(h, w)
        count = int(_inside(cut_count, np.uint32)[0])
        cut = _inside(cuts, np.uint32)[:count].copy()
        if f == 0:
            assert cut.tolist() == [0, 2]                    # (a zeroed prev: every first picture is a cut)
        fg, grid, summ, sel = ref.call(want_state, luma, prm, valid, cut, count)
        for s in (0, 2):
            want_mask.reshape(n, h, w)[s] = np.where(fg[s], 255, 0)
        what = "picture %d" % f
        _check_outputs(out.read(), np.where(np.asarray(valid)[:, None, None], grid, WORD), summ, sel, what)
        _same(_inside(state), want_state, what + ": the state")
        _same(_inside(mask), want_mask, what + ": the mask")
        assert summ[1] == (0, 0, 0) and sel == [0, 2]
        modes.append([int(ref.head_of(want_state, s, w, h)[1]) for s in range(n)])
        for d in (cuts, cut_count):
            d.free()
        out.free()
    # initialised by their age, then learning; the histogram's cut of stream 0's last picture initialises it anew
    assert modes == [[ref.VALID | ref.INIT, 0, ref.VALID | ref.INIT], [ref.VALID, 0, ref.VALID], [ref.VALID, 0, ref.VALID],
                     [ref.VALID | ref.INIT, 0, ref.VALID]]
    assert not ref.words_of(want_state, 1, w, h).any()       # the stream without a picture: an empty state still
    # without per-stream codes a stream without a picture is the call's code, after the rest was queued
    out = Outputs(n, gw, gh)
    with pytest.raises(h263mi.H263Error) as e:
        b.background_last(bg, state.at(GUARD), state_bytes, **out.args(), stream_rc=None)
    assert e.value.code == h263mi.ERR_NO_PICTURE
    b.sync()
    fg, grid, summ, sel = ref.call(want_state, luma, prm, valid)
    _check_outputs(out.read(), np.where(np.asarray(valid)[:, None, None], grid, WORD), summ, sel, "once more")
    _same(_inside(state), want_state, "once more: the state")
    # an output may not lie in the frame store, wherever that is: refused as an argument -- here by the state's alignment
    with pytest.raises(h263mi.H263Error) as e:
        b.background_last(bg, state.at(GUARD + 8), state_bytes, **out.args())
    assert e.value.code == h263mi.ERR_INVALID_ARGUMENT
    out.free()
    b.close()
    for d in (d_hist, d_prev, d_stats, state, mask, rgba, *[x for rec in recs for x in rec]):
        d.free()


def test_state_background_last():
    w, h = 100, 60
    prm = ref.Params(cl=3, learn=3, fg_learn=ref.KEEP, pix_thr=10, warmup=0, cell_thr=4, min_changed=1)
    bg = _background_of(prm)
    st = h263mi.H263State(h263mi.SORENSON_SPARK_BITSTREAM, device_id=0)
    gw, gh, cells_bytes, state_bytes = h263mi.background_extent(1, w, h, bg)
    state = _guarded(np.zeros(state_bytes, np.uint8))
    out = Outputs(1, gw, gh)
    with pytest.raises(h263mi.H263Error) as e:
        st.background_last(bg, state.at(GUARD), state_bytes, **out.args())
    assert e.value.code == h263mi.ERR_NO_PICTURE
    assert (out.read()[1].view(np.uint8) == SENTINEL).all()  # nothing was queued
    want_state = np.zeros(state_bytes, np.uint8)
    for f in range(3):
        if f == 0:
            mbs, co = recgen.intra_picture(w, h, seed=51)
            st.submit_picture(w, h, mbs, co, h263mi.PICTURE_I, temporal_reference=0, pquant=8)
        else:
            mbs, co = recgen.inter_picture(w, h, seed=51 + f, mv_range=30, p_4v=0.2, p_coded=0.5, quant=8)
            st.submit_picture(w, h, mbs, co, h263mi.PICTURE_P, temporal_reference=f, pquant=8)
        st.background_last(bg, state.at(GUARD), state_bytes, **out.args())
        luma = st.get_last_picture().as_yuv()[0].reshape(1, h, w)      # (waits for the stream)
        fg, grid, summ, sel = ref.call(want_state, luma, prm)
        _check_outputs(out.read(), grid, summ, sel, "picture %d" % f)
        _same(_inside(state), want_state, "picture %d: the state" % f)
        assert (summ[0][0] > 0) == (f > 0)
        out.free()
        out = Outputs(1, gw, gh)
    out.free()
    st.close()
    state.free()


# ---------------------------------------------------------------------------------------------
# 3. the chain on an object that stops: decode -> background_last -> regions -> tracks
# ---------------------------------------------------------------------------------------------
def _block_picture(w, h, bx, by):
    """an intra picture of flat blocks (no coefficient but the DC): grey, but for the luma block (by, bx), which is bright; bx None:
    no block"""
    mbw, mbh = recgen.mb_dims(w, h)
    mbs = np.zeros(mbw * mbh, recgen.MB_RECORD_DTYPE)
    mbs["mb_type"] = recgen.INTRA
    mbs["quant"] = 8
    mbs["intradc"] = 60
    if bx is not None:
        mbs[(by // 2) * mbw + bx // 2]["intradc"][(by % 2) * 2 + bx % 2] = 200
    return mbs, np.zeros((0, 64), np.int16)


STOPPED = [None, 2, 3, 4, 4, 4, 4, 4, 4, 4]                  # the block's column: it enters, moves for three pictures, stands still for six


def _run_chain(first_link):
    """first_link: "background" or "change".  -> (lumas, per picture (rois, region info, table, track info, count), states' bytes at
    the end, cells and summaries of every picture)"""
    n, w, h, cl, max_rois, max_out = 2, 176, 144, 3, 8, 4
    rows = [4, 11]
    recs = [_upload([_block_picture(w, h, bx, rows[s]) for s in range(n)]) for bx in STOPPED]
    b = h263mi.Batch(n, w, h, 0, None)
    rgba = h263mi.DeviceBuffer(n * w * h * 4)
    prm = ref.Params(cl=cl, learn=4, fg_learn=ref.KEEP, pix_thr=24, warmup=0, cell_thr=16, min_changed=1)
    bg = _background_of(prm)
    change = h263mi.make_change(cl, 16 * 24, min_changed_cells=1, roll=1)
    regions = h263mi.make_regions(cl, 16 if first_link == "background" else 16 * 24, connectivity=8, margin_cells=0, min_cells=1, max_per_picture=4)
    tracks = h263mi.make_tracks(max_tracks=7, iou_permille=300, max_missed=2, min_hits=2, emit_period=0)
    gw, gh, cells_bytes, work_bytes = h263mi.regions_extent(n, w, h, regions)
    _, _, _, bg_bytes = h263mi.background_extent(n, w, h, bg)
    tracks_bytes = h263mi.tracks_extent(n, w, h, tracks)
    bg_state, tr_state, work = _guarded(np.zeros(bg_bytes, np.uint8)), _guarded(np.zeros(tracks_bytes, np.uint8)), _guarded(_sentinels(work_bytes))
    d_prev = h263mi.DeviceBuffer(n * w * h)
    d_prev.upload(np.full(n * w * h, 60, np.uint8))
    prev = h263mi.PlaneSet(d_prev.ptr.value, n * w * h, w, w * h)
    per = []
    for rec in recs:                                         # the chain: four calls a picture, no host read before the end
        d = dict(cells=_guarded(_sentinels(cells_bytes)), summary=_guarded(_sentinels(n * 16)), rois=_guarded(_sentinels(max_rois * 16)),
                 rinfo=_guarded(_sentinels(n * 16)), rcount=_guarded(_sentinels(8)), table=_guarded(_sentinels(max_out * 16)),
                 tinfo=_guarded(_sentinels(n * 32)), count=_guarded(_sentinels(8)))
        b.decode(h263mi.PICTURE_I, rec[0].ptr, rec[1].ptr, rec[2].ptr, 0, 5, rgba.ptr, None)
        if first_link == "background":
            assert b.background_last(bg, bg_state.at(GUARD), bg_bytes, d["cells"].at(GUARD), cells_bytes, d["summary"].at(GUARD)) == [0, 0]
        else:
            assert b.change_last(prev, change, d["cells"].at(GUARD), cells_bytes, d["summary"].at(GUARD)) == [0, 0]
        b.regions(d["cells"].at(GUARD), cells_bytes, regions, work.at(GUARD), work_bytes, d["rois"].at(GUARD), max_rois, d["rinfo"].at(GUARD),
                  d["rcount"].at(GUARD), d_summary=d["summary"].at(GUARD))
        b.tracks(d["rois"].at(GUARD), max_rois, d["rinfo"].at(GUARD), tracks, tr_state.at(GUARD), tracks_bytes, d["table"].at(GUARD), max_out,
                 d["tinfo"].at(GUARD), d["count"].at(GUARD))
        per.append(d)
    b.sync()
    got = [dict(cells=_inside(d["cells"], np.uint32).reshape(n, gh, gw), summary=_inside(d["summary"], h263mi.CHANGE_SUMMARY_DTYPE),
                rois=_inside(d["rois"], tracks_ref.ROI), rinfo=_inside(d["rinfo"], tracks_ref.INFO_IN), table=_inside(d["table"], tracks_ref.ROI),
                tinfo=_inside(d["tinfo"], tracks_ref.INFO), count=_inside(d["count"], np.uint32)) for d in per]
    end = dict(bg=_inside(bg_state).copy(), tracks=_inside(tr_state).copy())
    # the pictures themselves: the same records through a second batch, read back one by one
    b2 = h263mi.Batch(n, w, h, 0, None)
    lumas = []
    for rec in recs:
        b2.decode(h263mi.PICTURE_I, rec[0].ptr, rec[1].ptr, rec[2].ptr, 0, 5, rgba.ptr, None)
        b2.sync()
        lumas.append(np.stack([b2.copy_yuv(s)[0].reshape(h, w) for s in range(n)]))
    b2.close()
    b.close()
    for d in per:
        for buf in d.values():
            buf.free()
    for buf in (bg_state, tr_state, work, d_prev, rgba, *[x for rec in recs for x in rec]):
        buf.free()
    return dict(n=n, w=w, h=h, cl=cl, prm=prm, max_rois=max_rois, max_out=max_out, rows=rows), lumas, got, end


def _live(tracks_state, n, max_tracks=7):
    stride = 32 + 32 * max_tracks
    return [int(tracks_state[p * stride:p * stride + 32].view(tracks_ref.HEAD)[0]["live"]) for p in range(n)]


def test_the_chain_keeps_the_track_of_an_object_that_stops():
    g, lumas, got, end = _run_chain("background")
    n, w, h, prm = g["n"], g["w"], g["h"], g["prm"]
    c = 1 << g["cl"]
    assert lumas[0].min() == lumas[0].max() and lumas[4].max() - lumas[4].min() > 100 and (lumas[4] == lumas[9]).all()
    bg_state = ref.empty_state(n, w, h)
    tr_state = np.zeros(n * (32 + 32 * 7), np.uint8)
    tprm = tracks_ref.Params(7, 300, 2, 2, 0)
    for k, (luma, d) in enumerate(zip(lumas, got)):
        # the reference's chain: bg_ref's cells into the regions reference, its table into the tracks reference
        fg, grid, summ, sel = ref.call(bg_state, luma, prm)
        assert (d["cells"] == grid).all() and [tuple(int(v) for v in s) for s in d["summary"]] == summ, k
        rois, _, info, counts = regions_ref.table(grid, w, h, c, prm.cell_thr, 8, 0, 1, 4, g["max_rois"], [s[1] for s in summ])
        assert [tuple(int(v) for v in r) for r in d["rois"]] == [tuple(r) for r in rois], k
        assert [tuple(int(v) for v in r) for r in d["rinfo"]] == [tuple(i) for i in info], k
        want = tracks_ref.call(tr_state, tprm, w, h, n, d["rois"], d["rinfo"], None, None, g["max_out"])
        assert d["table"].tobytes() == want[1].tobytes() and d["tinfo"].tobytes() == want[3].tobytes() and d["count"].tolist() == want[4].tolist(), k
        tr_state = want[0]
        if k >= 3:                                           # the block stands at column 4: one box of one cell per stream
            assert [tuple(int(v) for v in r) for r in d["rois"][:2]] == [(s, 32, 8 * g["rows"][s], 8, 8, 0) for s in range(n)], k
            assert d["tinfo"]["matched"].tolist() == ([0, 0] if k == 3 else [1, 1])
    _same(end["bg"], bg_state, "the background states")
    _same(end["tracks"], tr_state, "the track states")
    assert _live(end["tracks"], n) == [1, 1]                 # alive at the end, after six still pictures
    slots = end["tracks"][32:32 + 32 * 7].view(tracks_ref.TRACK)
    assert [(int(t["hits"]), int(t["missed"])) for t in slots if t["id"]] == [(7, 0)]


def test_the_chain_with_a_change_map_in_front_loses_the_object_that_stops():
    g, lumas, got, end = _run_chain("change")
    n = g["n"]
    assert [d["tinfo"]["detections"].tolist() for d in got[1:4]] == [[1, 1]] * 3          # while it moves it is seen
    assert all(d["tinfo"]["detections"].tolist() == [0, 0] for d in got[4:])               # a still picture changes nothing
    assert sum(int(d["tinfo"]["died"].sum()) for d in got) > 0 and _live(end["tracks"], n) == [0, 0]


# ---------------------------------------------------------------------------------------------
# 4. determinism
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["size_176x144_c8", "many_items_2"])
def test_two_runs_from_an_empty_state_give_identical_bytes(stream, name):
    b = bc.build(name)
    assert not b.state0.any()
    runs = []
    for _ in range(2):
        s = Sequence(b)
        raw = []
        for q in b.calls:
            out = s.call(q, lambda **a: h263mi.background_on(n_pictures=b.n, width=b.w, height=b.h, stream=stream.cuda_stream, **a))
            stream.synchronize()
            raw += out.raw() + [s.state.download()] + ([s.mask.download()] if s.mask else [])
            out.free()
        s.free()
        runs.append(raw)
    assert len(runs[0]) == len(runs[1]) and all((x == y).all() for x, y in zip(*runs))
