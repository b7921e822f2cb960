"""GPU tests of the motion regions (h263mi_regions_on, h263mi_batch_regions: k_regions, k_regions_pack).  Every comparison is exact,
against regions_ref (a flood fill): the whole table with its invalid tail, the stats, the info, both count words, and the sentinels
around every buffer.  The cases are the ones the kernels are run at thread by thread on the CPU (regions_cases.CASES), where every
hazard of theirs is shown to occur.  The chain test queues decode -> change_last -> regions -> roi_tensor with no host read in
between and compares with the same chain computed on the CPU."""
import numpy as np
import pytest
import torch  # before the library is loaded: torch brings its own HIP runtime, which the C-ABI library must share (as in bench.py)

import change_ref
import h263mi
import recgen
import regions_cases as rc
import regions_ref
import roi_ref
import tensor_out_ref as tref

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


class Call:
    """the device buffers of one call for case k, the outputs in sentinels"""

    def __init__(self, k):
        self.k = k
        self.regions = h263mi.make_regions(k.cl, k.thr, k.conn, k.margin, k.min_cells, k.max_per)
        gw, gh, self.cells_bytes, self.work_bytes = h263mi.regions_extent(k.n, k.w, k.h, self.regions)
        assert (gw, gh, self.cells_bytes, self.work_bytes) == (k.gw, k.gh, k.n * k.gw * k.gh * 4, k.n * k.max_per * 32)
        self.cells = _guarded(k.grids)
        self.summary = _guarded(np.array(k.summaries(), dtype=rc.SUMMARY)) if k.summary is not None else None
        self.work = _guarded(np.full(self.work_bytes, SENTINEL, np.uint8))
        self.rois = _guarded(np.full(k.max_rois * 16, SENTINEL, np.uint8))
        self.stats = _guarded(np.full(k.max_rois * 16, SENTINEL, np.uint8)) if k.stats else None
        self.info = _guarded(np.full(k.n * 16, SENTINEL, np.uint8))
        self.count = _guarded(np.full(8, SENTINEL, np.uint8))

    def args(self):
        k = self.k
        return dict(d_cells=self.cells.at(GUARD), cells_bytes=self.cells_bytes, regions=self.regions, d_work=self.work.at(GUARD),
                    work_bytes=self.work_bytes, d_rois=self.rois.at(GUARD), max_rois=k.max_rois, d_info=self.info.at(GUARD),
                    d_count=self.count.at(GUARD), d_stats=self.stats.at(GUARD) if self.stats else None,
                    d_summary=self.summary.at(GUARD) if self.summary else None)

    def run(self, stream):
        k = self.k
        h263mi.regions(n_pictures=k.n, width=k.w, height=k.h, stream=stream.cuda_stream, **self.args())

    def read(self):
        """-> (rois, stats or None, info, count); the guards are checked, and the inputs are what they were"""
        k = self.k
        assert _inside(self.cells, np.uint32).tobytes() == k.grids.tobytes(), "the grids are read only"
        _inside(self.work, np.uint8)
        if self.summary:
            assert _inside(self.summary, rc.SUMMARY).tolist() == k.summaries(), "the summaries are read only"
        return (_inside(self.rois, rc.ROI), _inside(self.stats, rc.STAT) if self.stats else None, _inside(self.info, rc.INFO),
                _inside(self.count, np.uint32))

    def raw(self):
        return [d.download().tobytes() for d in (self.rois, self.stats, self.info, self.count, self.work) if d]

    def free(self):
        for d in (self.cells, self.summary, self.work, self.rois, self.stats, self.info, self.count):
            if d:
                d.free()


# ---------------------------------------------------------------------------------------------
# 1. the case table through h263mi_regions_on
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rc.CASES))
def test_cases(stream, name):
    k = rc.build(name)
    call = Call(k)
    call.run(stream)
    stream.synchronize()
    assert rc.compare(k, *call.read()) is None
    call.free()


def test_the_serpentine_at_the_cap_twice_gives_identical_bytes(stream):
    k = rc.build("serpentine_cap")
    runs = []
    for _ in range(2):
        call = Call(k)
        call.run(stream)
        stream.synchronize()
        assert rc.compare(k, *call.read()) is None
        runs.append(call.raw())
        call.free()
    assert runs[0] == runs[1]


def test_no_pictures_still_fills_the_table(stream):
    k = rc.Case(40, 24, 3, np.zeros((0, 3, 5), np.uint32), max_rois=5)
    k.want = k.expected()
    assert k.want[0] == [regions_ref.INVALID_ROI] * 5 and k.want[3] == (0, 0)
    call = Call(k)
    a = call.args()
    a.update(d_cells=None, d_work=None, d_info=None)            # nothing of them is needed without pictures
    h263mi.regions(n_pictures=0, width=k.w, height=k.h, stream=stream.cuda_stream, **a)
    stream.synchronize()
    assert rc.compare(k, *call.read()) is None
    call.free()


def test_a_call_reuses_a_table_that_held_more(stream):
    """no stale box survives: the same buffers take a case with many boxes, then one with few"""
    many = rc.build("max_per_at_kept")
    few = rc.of_mask(rc.THREE, 3, conn=4, min_cells=4, max_per=4)
    few.want = few.expected()
    assert (many.max_rois, many.max_per, many.gw, many.gh) == (few.max_rois, few.max_per, few.gw, few.gh)
    assert many.want[3][0] == 4 and few.want[3][0] == 1
    call = Call(many)
    call.run(stream)
    call.k = few
    call.regions = h263mi.make_regions(few.cl, few.thr, few.conn, few.margin, few.min_cells, few.max_per)
    call.run(stream)                                             # (ordered behind the first on the stream)
    stream.synchronize()
    assert rc.compare(few, *call.read()) is None
    call.free()


# ---------------------------------------------------------------------------------------------
# 2. the batch form, and the whole device-side chain
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


def test_batch_regions_on_a_two_stream_batch():
    k = rc.Case(176, 144, 4, np.stack([rc.sads(rc.blobs(9, 11, 0.3, 1), 176, 144, 16, 1), rc.sads(rc.blobs(9, 11, 0.5, 2), 176, 144, 16, 2)]),
                conn=4, margin=1, min_cells=2, max_per=5, max_rois=7)
    k.want = k.expected()
    assert k.want[3][0] == 7 and k.want[3][1] > 7
    b = h263mi.Batch(2, k.w, k.h, 0, None)
    call = Call(k)
    b.regions(**call.args())
    b.sync()
    assert rc.compare(k, *call.read()) is None
    with pytest.raises(h263mi.H263Error) as e:                  # the batch's size decides the grid: these bytes are too few
        b.regions(**dict(call.args(), cells_bytes=call.cells_bytes - 1))
    assert e.value.code == h263mi.ERR_INVALID_ARGUMENT
    call.free()
    b.close()


def _moving_p_picture(w, h, moved):
    """a P picture that copies the reference except for the macroblocks `moved`: {(mby, mbx): (dx, dy) in half pels}"""
    mbw, mbh = recgen.mb_dims(w, h)
    mbs = np.zeros(mbw * mbh, recgen.MB_RECORD_DTYPE)
    mbs["quant"] = 8
    for (mby, mbx), mv in moved.items():
        mbs[mby * mbw + mbx]["mv"] = np.tile(np.array(mv), (4, 1))
    return mbs, np.zeros((0, 64), np.int16)


MOVED = [{(2, 3): (8, 2), (2, 4): (8, 2), (3, 4): (-6, 4), (7, 9): (4, 4)},
         {(0, 0): (6, 0), (5, 5): (2, 8), (6, 6): (2, 8), (8, 10): (-4, -4), (8, 9): (-4, -4)}]


def test_the_chain_decode_change_regions_roi_tensor():
    n, w, h, cl, max_rois, ow, oh = 3, 176, 144, 4, 8, 16, 16
    c = 1 << cl
    active = [True, True, False]                                 # stream 2 never gets a picture
    rec_i = _upload([recgen.intra_picture(w, h, seed=9100 + s) for s in range(n)])
    rec_p = _upload([_moving_p_picture(w, h, MOVED[s] if s < 2 else {}) for s in range(n)])
    b = h263mi.Batch(n, w, h, 0, None)
    b.set_active(active)
    rgba = h263mi.DeviceBuffer(n * w * h * 4)
    rgba.upload(np.full(rgba.nbytes, SENTINEL, np.uint8))
    d_prev = h263mi.DeviceBuffer(n * w * h)
    d_prev.upload(np.zeros(n * w * h, np.uint8))
    prev = h263mi.PlaneSet(d_prev.ptr.value, n * w * h, w, w * h)
    change = h263mi.make_change(cl, 0, min_changed_cells=1, roll=1)
    regions = h263mi.make_regions(cl, 0, connectivity=8, margin_cells=1, min_cells=1, max_per_picture=4)
    gw, gh, cells_bytes, work_bytes = h263mi.regions_extent(n, w, h, regions)
    assert (gw, gh) == (11, 9) and h263mi.change_extent(n, w, h, change)[:3] == (gw, gh, cells_bytes)
    scale, bias = tref.IMAGENET
    t = h263mi.make_tensor_out(ow, oh, tref.F32, scale, bias)
    out_bytes = h263mi.tensor_extent(max_rois, t)
    assert out_bytes == max_rois * 3 * oh * ow * 4
    cells = _guarded(np.full(cells_bytes, SENTINEL, np.uint8))
    summary = _guarded(np.full(n * 16, SENTINEL, np.uint8))
    work = _guarded(np.full(work_bytes, SENTINEL, np.uint8))
    rois = _guarded(np.full(max_rois * 16, SENTINEL, np.uint8))
    stats = _guarded(np.full(max_rois * 16, SENTINEL, np.uint8))
    info = _guarded(np.full(n * 16, SENTINEL, np.uint8))
    count = _guarded(np.full(8, SENTINEL, np.uint8))
    out = _guarded(np.full(out_bytes, SENTINEL, np.uint8))
    status = _guarded(np.full(max_rois * 4, SENTINEL, np.uint8))
    # the set-up: the I pictures, rolled into prev
    b.decode(h263mi.PICTURE_I, rec_i[0].ptr, rec_i[1].ptr, rec_i[2].ptr, 0, 5, rgba.ptr, None)
    b.change_last(prev, change, cells.at(GUARD), cells_bytes, summary.at(GUARD))
    b.sync()
    luma_i = [b.copy_yuv(s)[0].reshape(h, w) if active[s] else np.zeros((h, w), np.uint8) for s in range(n)]
    # the chain: four calls, no host read between them
    b.decode(h263mi.PICTURE_P, rec_p[0].ptr, rec_p[1].ptr, rec_p[2].ptr, 0, 5, rgba.ptr, None)
    rcs = b.change_last(prev, change, cells.at(GUARD), cells_bytes, summary.at(GUARD))
    b.regions(cells.at(GUARD), cells_bytes, regions, work.at(GUARD), work_bytes, rois.at(GUARD), max_rois, info.at(GUARD), count.at(GUARD),
              d_stats=stats.at(GUARD), d_summary=summary.at(GUARD))
    b.roi_tensor(rgba.ptr, rgba.nbytes, rois.at(GUARD), max_rois, t, out.at(GUARD), out_bytes, status.at(GUARD))
    b.sync()
    assert rcs == [0, 0, h263mi.ERR_NO_PICTURE]
    # the same chain on the CPU, from the decoded planes and the rendered RGBA
    luma_p = [b.copy_yuv(s)[0].reshape(h, w) if active[s] else luma_i[s] for s in range(n)]
    grid = change_ref.cells(np.stack(luma_p), np.stack(luma_i), c)
    summ = change_ref.summaries(grid, w, h, c, 0, active)
    assert [tuple(int(v) for v in s) for s in _inside(summary, rc.SUMMARY)] == summ
    assert summ[0][1] >= 3 and summ[1][1] >= 3 and summ[2] == (0, 0, 0)
    got_cells = _inside(cells, np.uint32).reshape(n, gh, gw)
    assert (got_cells[:2] == grid[:2]).all() and (got_cells[2] == SENTINEL * 0x01010101).all()   # stream 2's cells were never written
    k = rc.Case(w, h, cl, got_cells, thr=0, conn=8, margin=1, min_cells=1, max_per=4, max_rois=max_rois, summary=[s[1] for s in summ])
    k.want = k.expected()
    want_rois, _, want_info, (written, wanted) = k.want
    assert 2 <= written == wanted < max_rois and want_info[2] == (0, 0, 0, 0) and all(r[0] in (0, 1) for r in want_rois[:written])
    assert {r[0] for r in want_rois[:written]} == {0, 1}
    assert rc.compare(k, _inside(rois, rc.ROI), _inside(stats, rc.STAT), _inside(info, rc.INFO), _inside(count, np.uint32)) is None
    full = rgba.download().reshape(n, h, w, 4)
    pics = [full[s] for s in range(n)]
    assert (full[2] == SENTINEL).all()
    table = [r[:5] + (r[5],) for r in want_rois]
    crops = [roi_ref.crop(pics, r, ow, oh) if roi_ref.valid(r, n, w, h) else None for r in table]
    canvas = np.full(out_bytes // 4, SENTINEL * 0x01010101, np.uint32)
    want, want_status = roi_ref.expected(canvas, crops, table, n, w, h, tref.F32, scale, bias, False, 0, 3 * oh * ow, oh * ow, ow)
    assert list(want_status) == [0] * written + [1] * (max_rois - written)
    assert _inside(status, np.uint32).tolist() == list(want_status)
    assert (_inside(out, np.uint32) == want).all()
    for d in (cells, summary, work, rois, stats, info, count, out, status, rgba, d_prev, *rec_i, *rec_p):
        d.free()
    b.close()
