"""GPU tests of the deblocked-plane output layout (h263mi_yuv_layout: I420 or NV12, pitches, per-stream placement): every
plane against the oracle's deblock() (strength 0: the planes as decoded), placed by the numpy restatement
(tests/yuv_layout_ref.py), byte for byte, and the sentinel everywhere outside the planes' rectangles."""
import numpy as np
import pytest

import h263mi
import recgen
import yuv_layout_ref as ref
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
SIZES = [(1, 1), (5, 4), (7, 9), (176, 144), (352, 288), (1920, 1080)]
W, H = 1920, 1080
SENTINEL = 0xC3
FORMATS = [h263mi.YUV_I420, h263mi.YUV_NV12]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if h263mi.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the MI355X box")


def deblocked(planes, w, strength):
    cw = (w + 1) // 2
    return tuple(planes) if strength == 0 else tuple(orc.deblock(p, pw, strength) for p, pw in zip(planes, (w, cw, cw)))


def padded(v):
    return ((v + 255) // 256) * 256 + 256


def check_canvas(got, want_pics, w, h, fmt, pitch_y, pitch_c, offs, what, skip=()):
    n = len(want_pics)
    exp = ref.place(np.full(got.size, SENTINEL, np.uint8), want_pics, w, h, fmt, pitch_y, pitch_c, *offs, skip=skip)
    bad = np.flatnonzero(got != exp)
    inside = ref.rect_mask(got.size, n, w, h, fmt, pitch_y, pitch_c, *offs)
    assert bad.size == 0, "%s: %d bytes differ (%d of them outside the planes), first at byte %s" % (
        what, bad.size, int((~inside[bad]).sum()), bad[:8])


# ---------------------------------------------------------------------------------------------
# one state: h263mi_render_yuv
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SIZES)
def test_state_render_yuv(w, h):
    st = h263mi.H263State(h263mi.SORENSON_SPARK_BITSTREAM, device_id=0)
    b1 = h263mi.Batch(1, w, h, 0, None)
    mbs, co = recgen.intra_picture(w, h, seed=w + 3 * h)
    st.submit_picture(w, h, mbs, co, h263mi.PICTURE_I, temporal_reference=0, pquant=8)
    b1.submit_host(h263mi.PICTURE_I, [mbs], [co])
    rc, planes = orc.decode_picture(w, h, mbs, co, None)
    assert rc == 0
    mbs, co = recgen.inter_picture(w, h, seed=w + 5 * h, mv_range=40, p_4v=0.2, p_intra=0.1)
    st.submit_picture(w, h, mbs, co, h263mi.PICTURE_P, temporal_reference=1, pquant=10)
    b1.submit_host(h263mi.PICTURE_P, [mbs], [co])
    rc, planes = orc.decode_picture(w, h, mbs, co, planes)
    assert rc == 0
    cw, ch = ref.chroma_size(w, h)
    today = h263mi.DeviceBuffer(w * h + 2 * cw * ch)
    for strength in (0, 5, 12):
        want = deblocked(planes, w, strength)
        for fmt in FORMATS:
            ry, rc_ = ref.row_bytes(w, fmt)
            # tight: exactly the extent's bytes, every one of them a sample
            got = st.render_yuv(strength, fmt)
            assert got.size == w * h + 2 * cw * ch
            exp = np.concatenate([p.ravel() for p in ref.planes_of(want, w, h, fmt)])
            assert (got == exp).all(), (strength, fmt, np.flatnonzero(got != exp)[:8])
            # padded: the bytes between rows stay untouched
            py, pc = padded(ry), padded(rc_)
            offs = ref.default_offsets(1, w, h, fmt, py, pc)
            out = np.full(h263mi.yuv_layout_extent(1, w, h, fmt, py, pc), SENTINEL, np.uint8)
            assert out.size == ref.picture_bytes(w, h, fmt, py, pc)
            st.render_yuv_into(strength, out, fmt, py, pc)
            check_canvas(out, [want], w, h, fmt, py, pc, offs, "state %dx%d strength %d format %d" % (w, h, strength, fmt))
        # tight I420 is what a 1-stream batch writes to d_deblocked without any layout
        today.upload(np.full(today.nbytes, SENTINEL, np.uint8))
        b1.render_rgba(strength, None, today.ptr)
        b1.sync()
        assert (st.render_yuv(strength, h263mi.YUV_I420) == today.download()).all(), strength
    # the strength the picture's own header asks for (USE_DEBLOCKER is not set here: none)
    assert (st.render_yuv(h263mi.STRENGTH_FROM_HEADER) == st.render_yuv(0)).all()
    # placement inside the caller's buffer: Cr in front of Cb in front of Y, gaps between them (every plane starts on a row
    # of its own grid, the tight pitches cw and w, so that no row crosses a pitch boundary)
    fmt = h263mi.YUV_I420
    ocr = [2 * cw]
    ocb = [ocr[0] + cw * (ch + 3)]
    oy = [-(-(ocb[0] + cw * ch + 5) // w) * w]
    out = np.full(oy[0] + w * h + 7, SENTINEL, np.uint8)
    st.render_yuv_into(5, out, fmt, offsets_y=oy, offsets_cb=ocb, offsets_cr=ocr)
    check_canvas(out, [deblocked(planes, w, 5)], w, h, fmt, w, cw, (oy, ocb, ocr), "state %dx%d placed" % (w, h))
    b1.close()
    st.close()


# ---------------------------------------------------------------------------------------------
# small batches: immediate rendering, d_rgba and d_deblocked together under an NV12 layout
# ---------------------------------------------------------------------------------------------
def _small_streams(n, w, h, seed):
    return [recgen.intra_picture(w, h, seed=seed + s) for s in range(n)]


def _upload_records(pics, w, h):
    """dense device records of one picture per stream -> (d_mbs, d_coeffs, d_base) and the oracle's planes"""
    mbs = np.concatenate([m for m, _ in pics])
    co = np.concatenate([c for _, c in pics]).astype(np.int16)
    base = np.cumsum([0] + [c.shape[0] for _, c in pics[:-1]]).astype(np.uint64)
    bufs = []
    for arr in (mbs, co, base):
        d = h263mi.DeviceBuffer(max(arr.nbytes, 16))
        d.upload(arr)
        bufs.append(d)
    planes = []
    for m, c in pics:
        rc, p = orc.decode_picture(w, h, m, c, None)
        assert rc == 0
        planes.append(p)
    return bufs, planes


def _sentinel_buffer(nbytes):
    d = h263mi.DeviceBuffer(nbytes)
    d.upload(np.full(nbytes, SENTINEL, np.uint8))
    return d


@pytest.mark.parametrize("w,h", [(5, 4), (7, 9), (176, 144), (352, 288)])
def test_batch_rgba_and_nv12_planes_in_one_call(w, h):
    """a non-pipelined batch; tight NV12 rows of an odd width take the narrow stores, the padded ones the wide ones"""
    n, strength, fmt = 3, 7, h263mi.YUV_NV12
    recs, planes = _upload_records(_small_streams(n, w, h, 400 + w), w, h)
    want = [deblocked(p, w, strength) for p in planes]
    # the RGBA of the same call on a batch without any YUV layout
    plain = h263mi.Batch(n, w, h, 0, None)
    rgba_plain = _sentinel_buffer(n * w * h * 4)
    plain.decode(h263mi.PICTURE_I, recs[0].ptr, recs[1].ptr, recs[2].ptr, 0, strength, rgba_plain.ptr, None)
    plain.sync()
    plain.close()
    ry, rc_ = ref.row_bytes(w, fmt)
    for py, pc in ((0, 0), (padded(ry), padded(rc_))):
        b = h263mi.Batch(n, w, h, 0, None)
        b.set_yuv_layout(fmt, py, pc)
        nbytes = h263mi.yuv_layout_extent(n, w, h, fmt, py, pc)
        assert nbytes == n * ref.picture_bytes(w, h, fmt, py, pc)
        rgba, yuv = _sentinel_buffer(n * w * h * 4), _sentinel_buffer(nbytes)
        b.decode(h263mi.PICTURE_I, recs[0].ptr, recs[1].ptr, recs[2].ptr, 0, strength, rgba.ptr, yuv.ptr)
        b.sync()
        offs = ref.default_offsets(n, w, h, fmt, py, pc)
        check_canvas(yuv.download(), want, w, h, fmt, py or ry, pc or rc_, offs, "%dx%d pitches %d %d" % (w, h, py, pc))
        assert (rgba.download() == rgba_plain.download()).all()
        # streams with nothing to render are not written
        b.set_active([True, False, True])
        yuv2 = _sentinel_buffer(nbytes)
        b.decode(h263mi.PICTURE_I, recs[0].ptr, recs[1].ptr, recs[2].ptr, 0, strength, None, yuv2.ptr)
        b.sync()
        check_canvas(yuv2.download(), want, w, h, fmt, py or ry, pc or rc_, offs, "inactive stream", skip=(1,))
        b.close()


def test_pipelined_planes_follow_the_layout_of_their_request():
    n, w, h = 4, 176, 144
    cw, ch = ref.chroma_size(w, h)
    b = h263mi.Batch(n, w, h, 0, None, pipeline_post=True)
    recs1, planes1 = _upload_records(_small_streams(n, w, h, 100), w, h)
    recs2, planes2 = _upload_records(_small_streams(n, w, h, 200), w, h)
    recs3, planes3 = _upload_records(_small_streams(n, w, h, 300), w, h)
    # call 1: NV12, a 2 x 2 mosaic on one grid; call 2: I420 at padded pitches, RGBA beside it; call 3: no layout at all
    p1 = 2 * w + 80
    oy1 = [(s // 2) * (h + ch + 1) * p1 + (s % 2) * (w + 64) + 8 for s in range(n)]
    oc1 = [o + h * p1 for o in oy1]
    py2, pc2 = 256, 128
    c1 = _sentinel_buffer(h263mi.yuv_layout_extent(n, w, h, h263mi.YUV_NV12, p1, p1, oy1, oc1))
    c2 = _sentinel_buffer(h263mi.yuv_layout_extent(n, w, h, h263mi.YUV_I420, py2, pc2))
    c3 = _sentinel_buffer(n * (w * h + 2 * cw * ch))
    rgba2 = _sentinel_buffer(n * w * h * 4)
    b.set_yuv_layout(h263mi.YUV_NV12, p1, p1, oy1, oc1)
    b.decode(h263mi.PICTURE_I, recs1[0].ptr, recs1[1].ptr, recs1[2].ptr, 0, 7, None, c1.ptr)         # deferred
    b.set_yuv_layout(h263mi.YUV_I420, py2, pc2)
    b.decode(h263mi.PICTURE_I, recs2[0].ptr, recs2[1].ptr, recs2[2].ptr, 0, 3, rgba2.ptr, c2.ptr)    # k_frame renders call 1
    b.set_yuv_layout(default=True)
    b.decode(h263mi.PICTURE_I, recs3[0].ptr, recs3[1].ptr, recs3[2].ptr, 0, 5, None, c3.ptr)         # ... and call 2
    b.sync()                                                                                        # k_post renders call 3
    check_canvas(c1.download(), [deblocked(p, w, 7) for p in planes1], w, h, ref.NV12, p1, p1, (oy1, oc1, None), "call 1")
    want2 = [deblocked(p, w, 3) for p in planes2]
    check_canvas(c2.download(), want2, w, h, ref.I420, py2, pc2, ref.default_offsets(n, w, h, ref.I420, py2, pc2), "call 2")
    assert (rgba2.download() == np.concatenate([orc.yuv420_to_rgba(*p, w) for p in want2])).all()
    want3 = np.concatenate([np.concatenate(deblocked(p, w, 5)) for p in planes3])
    assert (c3.download() == want3).all()
    b.close()


def test_a_plane_buffer_one_byte_short_is_refused_before_anything_is_queued():
    n, w, h = 4, 176, 144
    b = h263mi.Batch(n, w, h, 0, None)
    recs, planes = _upload_records(_small_streams(n, w, h, 500), w, h)
    fmt, py, pc = h263mi.YUV_NV12, 256, 256
    b.set_yuv_layout(fmt, py, pc)
    nbytes = h263mi.yuv_layout_extent(n, w, h, fmt, py, pc)
    small = h263mi.DeviceBuffer(nbytes - 1)
    with pytest.raises(h263mi.H263Error) as e:
        b.decode(h263mi.PICTURE_I, recs[0].ptr, recs[1].ptr, recs[2].ptr, 0, 5, None, small.ptr)
    assert e.value.code == h263mi.ERR_INVALID_ARGUMENT
    assert not any(b.stream_has_picture(s) for s in range(n))    # no stream advanced
    ok = _sentinel_buffer(nbytes)
    b.decode(h263mi.PICTURE_I, recs[0].ptr, recs[1].ptr, recs[2].ptr, 0, 5, None, ok.ptr)
    b.sync()
    check_canvas(ok.download(), [deblocked(p, w, 5) for p in planes], w, h, fmt, py, pc,
                 ref.default_offsets(n, w, h, fmt, py, pc), "after the refusal")
    with pytest.raises(h263mi.H263Error) as e:
        b.render_rgba(5, None, small.ptr)
    assert e.value.code == h263mi.ERR_INVALID_ARGUMENT
    # a refused layout leaves the one in force as it was
    with pytest.raises(h263mi.H263Error):
        b.set_yuv_layout(fmt, 100, 256)
    ok2 = _sentinel_buffer(nbytes)
    b.render_rgba(5, None, ok2.ptr)
    b.sync()
    assert (ok2.download() == ok.download()).all()
    b.close()


# ---------------------------------------------------------------------------------------------
# the bench path: 64 x 1080p, events, H263MI_CFG_PIPELINE_POST (k_frame), one strength per stream, planes only
# ---------------------------------------------------------------------------------------------
N_BENCH, FIRST_STREAM, GOP = 64, 5, 4
STRENGTHS = np.array([s % 13 for s in range(N_BENCH)], np.uint8)


@pytest.fixture(scope="module")
def bench_reference():
    """[frame][stream] -> the stream's deblocked planes"""
    out = [[None] * N_BENCH for _ in range(GOP)]
    for s in range(N_BENCH):
        planes = None
        for f in range(GOP):
            kind = h263mi.SYNTH_I_MIXED if f == 0 else h263mi.SYNTH_P
            mbs, co = h263mi.synth_picture_host(kind, W, H, FIRST_STREAM + s, f)
            rc, planes = orc.decode_picture(W, H, mbs, co, planes)
            assert rc == 0
            out[f][s] = deblocked(planes, W, int(STRENGTHS[s]))
    return out


def _bench_path(want, fmt, pitch_y, pitch_c, offs, set_offsets):
    import bench
    n, gop = N_BENCH, GOP
    wl = bench.Workload(h263mi, n, gop, FIRST_STREAM, 0, None, events=True)
    b = h263mi.Batch(n, W, H, 0, None, pipeline_post=True)
    oy, ocb, ocr = offs
    if set_offsets:
        nbytes = h263mi.yuv_layout_extent(n, W, H, fmt, pitch_y, pitch_c, oy, ocb, ocr)
        b.set_yuv_layout(fmt, pitch_y, pitch_c, oy, ocb, ocr)
    else:
        nbytes = h263mi.yuv_layout_extent(n, W, H, fmt, pitch_y, pitch_c)
        b.set_yuv_layout(fmt, pitch_y, pitch_c)
    assert nbytes == ref.span_end(n, W, H, fmt, pitch_y, pitch_c, *offs) if set_offsets else nbytes == n * ref.picture_bytes(W, H, fmt, pitch_y, pitch_c)
    canvases = []
    b.timing_reserve(4 * gop)
    b.timing_begin()
    for f in range(gop):
        c = _sentinel_buffer(nbytes)
        canvases.append(c)
        fr = wl.frames[f]
        if fr.get("first") is not None:
            b.decode_events(fr["ptype"], fr["mbs"].ptr, fr["first"].ptr, fr["ev"].ptr, fr["base"].ptr, 0, 0, None, c.ptr,
                            strengths=STRENGTHS)
        else:
            b.decode(fr["ptype"], fr["mbs"].ptr, fr["co"].ptr, fr["base"].ptr, 0, 0, None, c.ptr, strengths=STRENGTHS)
    b.sync()
    kt = b.timing_end()
    assert kt.frame_launches == gop - 1 and kt.post_launches == 1 and kt.recon_launches == 1
    for f in range(gop):
        check_canvas(canvases[f].download(), want[f], W, H, fmt, pitch_y, pitch_c, offs, "frame %d" % f)
        canvases[f].free()
    b.close()


def test_bench_path_nv12_mosaic_k_frame(bench_reference):
    """bench.py's Workload(events=True) on Batch(64, 1920, 1080, pipeline_post): I + 3 P, every stream its own strength, no
    RGBA; each frame index into one canvas, 8 x 8 tiles of a 1920 x 1080 luma plane with its 1920 x 540 CbCr plane below it.
    The k_frame launches alternate their direction: both are walked.  All 64 tiles of every frame are compared."""
    pitch = 8 * W
    oy = [(s // 8) * (H + H // 2) * pitch + (s % 8) * W for s in range(N_BENCH)]
    oc = [o + H * pitch for o in oy]
    assert h263mi.yuv_layout_extent(N_BENCH, W, H, h263mi.YUV_NV12, pitch, pitch, oy, oc) == 8 * 1620 * pitch
    _bench_path(bench_reference, h263mi.YUV_NV12, pitch, pitch, (oy, oc, None), True)


def test_bench_path_i420_padded_default_placement_k_frame(bench_reference):
    """the same as I420 at padded pitches (2048 / 1024), pictures back to back"""
    py, pc = 2048, 1024
    _bench_path(bench_reference, h263mi.YUV_I420, py, pc, ref.default_offsets(N_BENCH, W, H, ref.I420, py, pc), False)
