"""GPU tests of the region tracks (h263mi_tracks_on, h263mi_batch_tracks: k_tracks, k_tracks_pack).  Every comparison is exact,
against tracks_ref (sequential Python): after EVERY call of a sequence the whole state, the table with its invalid tail, the refs, the
info, both count words, and the sentinels around every buffer.  The cases are the ones the kernels are run at thread by thread on
the CPU (tracks_cases.CASES), where every hazard of theirs is shown to occur.  The chain test queues, picture after picture, decode
-> change_last -> regions -> tracks -> roi_tensor with no host read before the end and compares with the same chain computed on the
CPU."""
import numpy as np
import pytest
import torch  # before the library is loaded: torch brings its own HIP runtime, which the C-ABI library must share (as in bench.py)

import h263mi
import recgen
import roi_ref
import tensor_out_ref as tref
import tracks_cases as tc
import tracks_ref as ref

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
    host = np.concatenate([np.full(GUARD, SENTINEL, np.uint8), np.ascontiguousarray(data).view(np.uint8).ravel(),
                           np.full(GUARD, SENTINEL, np.uint8)])
    d = h263mi.DeviceBuffer(host.size)
    d.upload(host)
    return d


def _inside(d, dtype):
    raw = d.download()
    assert (raw[:GUARD] == SENTINEL).all() and (raw[-GUARD:] == SENTINEL).all(), "a guard was written"
    return raw[GUARD:-GUARD].view(dtype)


def _sentinels(nbytes):
    return np.full(nbytes, SENTINEL, np.uint8)


class Sequence:
    """the device buffers of case k: the state lives on through the calls, the outputs are sentinels before each"""

    def __init__(self, k):
        self.k = k
        p = k.prm
        self.tracks = h263mi.make_tracks(p.max_tracks, p.iou_permille, p.max_missed, p.min_hits, p.emit_period)
        self.state_bytes = h263mi.tracks_extent(k.n, k.w, k.h, self.tracks)
        assert self.state_bytes == k.state_bytes
        self.state = _guarded(k.state0) if k.n else None
        self.bufs = []

    def call(self, c, run):
        """one call: run(**arguments) queues it; -> (state, rois, refs or None, info, count) behind it, the guards checked"""
        k = self.k
        rois = _guarded(c.rois) if c.rois.size else None
        info_in = _guarded(c.info_in) if k.n else None
        cut = _guarded(c.cut) if c.cut is not None else None
        cut_count = _guarded(np.array([c.cut_count], np.uint32)) if c.cut is not None else None
        out, info, count = _guarded(_sentinels(k.max_out * 16)), _guarded(_sentinels(k.n * 32)) if k.n else None, _guarded(_sentinels(8))
        refs = _guarded(_sentinels(k.max_out * 16)) if k.refs else None
        at = lambda d: d.at(GUARD) if d else None
        run(d_rois=at(rois), n_rois=int(c.rois.size), d_info_in=at(info_in), tracks=self.tracks, d_state=at(self.state),
            state_bytes=self.state_bytes, d_out_rois=at(out), max_out=k.max_out, d_info=at(info), d_count=at(count), d_out_refs=at(refs),
            d_cut=at(cut), d_cut_count=at(cut_count))
        self.bufs += [d for d in (rois, info_in, cut, cut_count, out, info, count, refs) if d]
        return lambda: (_inside(self.state, np.uint8) if self.state else np.zeros(0, np.uint8), _inside(out, ref.ROI),
                        _inside(refs, ref.REF) if refs else None, _inside(info, ref.INFO) if info else np.zeros(0, ref.INFO),
                        _inside(count, np.uint32)), (rois, c.rois), (info_in, c.info_in)

    def free(self):
        for d in self.bufs + ([self.state] if self.state else []):
            d.free()


# ---------------------------------------------------------------------------------------------
# 1. the case table through h263mi_tracks_on
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(tc.CASES))
def test_cases(stream, name):
    k = tc.build(name)
    s = Sequence(k)
    for c, want in zip(k.calls, tc.expected(name)):
        read, *inputs = s.call(c, lambda **a: h263mi.tracks(n_pictures=k.n, width=k.w, height=k.h, stream=stream.cuda_stream, **a))
        stream.synchronize()
        assert tc.compare(want, *read()) is None
        for d, host in inputs:
            assert d is None or _inside(d, np.uint8).tobytes() == host.tobytes(), "the inputs are read only"
    s.free()


def test_the_chain_case_through_the_batch_call():
    k = tc.build("chain256")
    b = h263mi.Batch(k.n, k.w, k.h, 0, None)
    s = Sequence(k)
    for c, want in zip(k.calls, tc.expected("chain256")):
        read, *_ = s.call(c, lambda **a: b.tracks(**a))
        b.sync()
        assert tc.compare(want, *read()) is None
    with pytest.raises(h263mi.H263Error) as e:                  # the batch's streams decide the extent: these bytes are too few
        s.call(k.calls[0], lambda **a: b.tracks(**dict(a, state_bytes=s.state_bytes - 1)))
    assert e.value.code == h263mi.ERR_INVALID_ARGUMENT
    s.free()
    b.close()


def test_a_sequence_queued_without_a_host_read_between_its_calls(stream):
    """the calls of a sequence are ordered by the stream alone: what the last one leaves is what the reference leaves"""
    k = tc.build("emit_h3_p4")
    s = Sequence(k)
    reads = [s.call(c, lambda **a: h263mi.tracks(n_pictures=k.n, width=k.w, height=k.h, stream=stream.cuda_stream, **a))[0] for c in k.calls]
    stream.synchronize()
    want = tc.expected("emit_h3_p4")
    for c, (r, w) in enumerate(zip(reads, want)):
        got = r()
        assert tc.compare(w, got[0] if c == len(want) - 1 else None, *got[1:]) is None, c
    s.free()


# ---------------------------------------------------------------------------------------------
# 2. the whole device-side chain
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


def _bright_block_picture(w, h, bx, by):
    """an intra picture of flat blocks (no coefficient but the DC): grey, but for the luma block (by, bx), which is bright"""
    mbw, mbh = recgen.mb_dims(w, h)
    mbs = np.zeros(mbw * mbh, recgen.MB_RECORD_DTYPE)
    mbs["mb_type"] = recgen.INTRA
    mbs["quant"] = 8
    mbs["intradc"] = 60
    mbs[(by // 2) * mbw + bx // 2]["intradc"][(by % 2) * 2 + bx % 2] = 200
    return mbs, np.zeros((0, 64), np.int16)


def test_the_chain_decode_change_regions_tracks_roi_tensor():
    n, w, h, cl, pictures, max_rois, max_out, ow, oh = 2, 176, 144, 3, 6, 8, 4, 8, 8
    rows = [4, 11]                                               # the block row of the bright block in stream 0 and 1
    recs = [_upload([_bright_block_picture(w, h, 2 + k, rows[s]) for s in range(n)]) for k in range(pictures)]
    b = h263mi.Batch(n, w, h, 0, None)
    d_prev = h263mi.DeviceBuffer(n * w * h)
    d_prev.upload(np.zeros(n * w * h, np.uint8))
    prev = h263mi.PlaneSet(d_prev.ptr.value, n * w * h, w, w * h)
    change = h263mi.make_change(cl, 0, min_changed_cells=1, roll=1)
    regions = h263mi.make_regions(cl, 0, connectivity=8, margin_cells=0, min_cells=1, max_per_picture=4)
    tracks = h263mi.make_tracks(max_tracks=7, iou_permille=300, max_missed=2, min_hits=2, emit_period=0)
    prm = ref.Params(7, 300, 2, 2, 0)
    gw, gh, cells_bytes, work_bytes = h263mi.regions_extent(n, w, h, regions)
    state_bytes = h263mi.tracks_extent(n, w, h, tracks)
    scale, bias = tref.IMAGENET
    t = h263mi.make_tensor_out(ow, oh, tref.F32, scale, bias)
    out_bytes = h263mi.tensor_extent(max_out, t)
    cells, summary, work = _guarded(_sentinels(cells_bytes)), _guarded(_sentinels(n * 16)), _guarded(_sentinels(work_bytes))
    state = _guarded(np.zeros(state_bytes, np.uint8))
    per = []                                                     # every picture's own outputs: nothing is read before the end
    for k in range(pictures):
        per.append(dict(rgba=h263mi.DeviceBuffer(n * w * h * 4), rois=_guarded(_sentinels(max_rois * 16)), rinfo=_guarded(_sentinels(n * 16)),
                        rcount=_guarded(_sentinels(8)), table=_guarded(_sentinels(max_out * 16)), refs=_guarded(_sentinels(max_out * 16)),
                        tinfo=_guarded(_sentinels(n * 32)), count=_guarded(_sentinels(8)), out=_guarded(_sentinels(out_bytes)),
                        status=_guarded(_sentinels(max_out * 4))))
    # the chain: five calls a picture, six pictures, no host read
    for k, (rec, d) in enumerate(zip(recs, per)):
        b.decode(h263mi.PICTURE_I, rec[0].ptr, rec[1].ptr, rec[2].ptr, 0, 5, d["rgba"].ptr, None)
        assert b.change_last(prev, change, cells.at(GUARD), cells_bytes, summary.at(GUARD)) == [0, 0]
        b.regions(cells.at(GUARD), cells_bytes, regions, work.at(GUARD), work_bytes, d["rois"].at(GUARD), max_rois, d["rinfo"].at(GUARD),
                  d["rcount"].at(GUARD), d_summary=summary.at(GUARD))
        b.tracks(d["rois"].at(GUARD), max_rois, d["rinfo"].at(GUARD), tracks, state.at(GUARD), state_bytes, d["table"].at(GUARD), max_out,
                 d["tinfo"].at(GUARD), d["count"].at(GUARD), d_out_refs=d["refs"].at(GUARD))
        b.roi_tensor(d["rgba"].ptr, n * w * h * 4, d["table"].at(GUARD), max_out, t, d["out"].at(GUARD), out_bytes, d["status"].at(GUARD))
    b.sync()
    # the reference tracker over the tables that regions wrote
    st = np.zeros(state_bytes, np.uint8)
    emitted = []                                                 # (picture of the sequence, ref)
    ids = []
    for k, d in enumerate(per):
        rois, rinfo = _inside(d["rois"], ref.ROI), _inside(d["rinfo"], ref.INFO_IN)
        if k == 0:
            assert rinfo["written"].tolist() == [1, 1] and [tuple(r)[1:5] for r in rois[:2]] == [(0, 0, w, h)] * 2      # all is new
        else:
            # the block left the cell at 8 * (1 + k) and entered the next: a box of two cells
            assert [tuple(int(v) for v in r) for r in rois[:2]] == [(s, 8 * (1 + k), 8 * rows[s], 16, 8, 0) for s in range(n)]
        want = ref.call(st, prm, w, h, n, rois, rinfo, None, None, max_out)
        last = k == pictures - 1
        got = (_inside(state, np.uint8) if last else None, _inside(d["table"], ref.ROI), _inside(d["refs"], ref.REF),
               _inside(d["tinfo"], ref.INFO), _inside(d["count"], np.uint32))
        assert tc.compare(want, *got) is None, k
        st = want[0]
        written = int(want[4][0])
        emitted += [(k, tuple(int(v) for v in r)) for r in want[2][:written]]
        slots = st.reshape(n, prm.stride())[:, 32:].view(ref.TRACK).reshape(n, prm.max_tracks)
        ids.append([{int(s["id"]) for s in slots[p] if s["flags"] & (ref.BORN | ref.MATCHED)} for p in range(n)])
        # the tensors: the emitted boxes cut out of this picture's RGBA, every other slot untouched
        full = d["rgba"].download().reshape(n, h, w, 4)
        table = [tuple(int(v) for v in r) for r in want[1]]
        crops = [roi_ref.crop([full[s] for s in range(n)], r, ow, oh) if roi_ref.valid(r, n, w, h) else None for r in table]
        canvas = np.full(out_bytes // 4, SENTINEL * 0x01010101, np.uint32)
        want_out, want_status = roi_ref.expected(canvas, crops, table, n, w, h, tref.F32, scale, bias, False, 0, 3 * oh * ow, oh * ow, ow)
        assert list(want_status) == [0] * written + [1] * (max_out - written)
        assert _inside(d["status"], np.uint32).tolist() == list(want_status)
        assert (_inside(d["out"], np.uint32) == want_out).all(), k
        if not written:
            assert (_inside(d["out"], np.uint8) == SENTINEL).all()
    # one id per stream persists over the pictures in which the block moves, and is emitted exactly once: when it is confirmed
    assert ids[0] == [{1}, {1}] and all(i == [{2}, {2}] for i in ids[1:])
    assert [(k, r[0], r[1], r[2]) for k, r in emitted] == [(2, 2, 0, 2), (2, 2, 1, 2)]
    boxes = _inside(per[2]["table"], ref.ROI)
    assert [tuple(int(v) for v in r) for r in boxes[:2]] == [(s, 24, 8 * rows[s], 16, 8, 0) for s in range(n)]
    for d in per:
        for buf in d.values():
            buf.free()
    for buf in (cells, summary, work, state, d_prev, *[x for rec in recs for x in rec]):
        buf.free()
    b.close()
