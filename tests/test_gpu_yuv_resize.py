"""GPU tests of the deblocked planes resized to any W' x H' (h263mi_yuv_resize, k_plane_resize): every plane against the oracle's
deblock() (strength 0: the planes as decoded) put through the numpy restatement (tests/yuv_resize_ref.py) and placed by
tests/yuv_layout_ref.py, byte for byte, and the sentinel everywhere outside the planes' rectangles."""
import numpy as np
import pytest

import h263mi
import recgen
import rgba_resize_ref
import yuv_layout_ref as lay
import yuv_resize_ref as ref
from oracle import oracle as orc
from test_gpu_yuv_layout import SENTINEL, _sentinel_buffer, _small_streams, _upload_records, check_canvas, deblocked, padded

pytestmark = pytest.mark.gpu
FORMATS = [h263mi.YUV_I420, h263mi.YUV_NV12]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if h263mi.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the MI355X box")


def resized(planes, w, h, strength, ow, oh):
    return ref.resize_planes(deblocked(planes, w, strength), w, h, ow, oh)


# ---------------------------------------------------------------------------------------------
# one state: h263mi_render_yuv_resize into host memory
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(1, 1), (5, 4), (7, 9), (176, 144), (352, 288)])
def test_state_render_yuv_resize(w, h):
    st = h263mi.H263State(h263mi.SORENSON_SPARK_BITSTREAM, device_id=0)
    mbs, co = recgen.intra_picture(w, h, seed=w + 3 * h)
    st.submit_picture(w, h, mbs, co, h263mi.PICTURE_I, temporal_reference=0, pquant=8)
    rc, planes = orc.decode_picture(w, h, mbs, co, None)
    assert rc == 0
    mbs, co = recgen.inter_picture(w, h, seed=w + 5 * h, mv_range=40, p_4v=0.2, p_intra=0.1)
    st.submit_picture(w, h, mbs, co, h263mi.PICTURE_P, temporal_reference=1, pquant=10)
    rc, planes = orc.decode_picture(w, h, mbs, co, planes)
    assert rc == 0
    for strength in (0, 5, 12):
        for ow, oh in ((1, 1), (w + 3, h + 5), (max(1, w * 5 // 9), max(1, h * 3 // 7))):
            want = resized(planes, w, h, strength, ow, oh)
            for fmt in FORMATS:
                what = "state %dx%d -> %dx%d strength %d format %d" % (w, h, ow, oh, strength, fmt)
                ry, rc_ = lay.row_bytes(ow, fmt)
                # tight: exactly the extent's bytes, every one of them a sample
                got = st.render_yuv_resize(strength, ow, oh, fmt)
                exp = np.concatenate([p.ravel() for p in lay.planes_of(want, ow, oh, fmt)])
                assert got.size == exp.size and (got == exp).all(), (what, np.flatnonzero(got != exp)[:8])
                # padded: the bytes between rows stay untouched
                py, pc = padded(ry), padded(rc_)
                out = np.full(h263mi.yuv_resize_extent(1, ow, oh, fmt, py, pc), SENTINEL, np.uint8)
                assert out.size == lay.picture_bytes(ow, oh, fmt, py, pc)
                st.render_yuv_resize_into(strength, out, ow, oh, fmt, py, pc)
                check_canvas(out, [want], ow, oh, fmt, py, pc, lay.default_offsets(1, ow, oh, fmt, py, pc), what)
        # W' = w, H' = h is render_yuv of the same placement
        for fmt in FORMATS:
            ry, rc_ = lay.row_bytes(w, fmt)
            assert (st.render_yuv_resize(strength, w, h, fmt) == st.render_yuv(strength, fmt)).all()
            py, pc = padded(ry), padded(rc_)
            a = np.full(h263mi.yuv_layout_extent(1, w, h, fmt, py, pc), SENTINEL, np.uint8)
            b = a.copy()
            st.render_yuv_resize_into(strength, a, w, h, fmt, py, pc)
            st.render_yuv_into(strength, b, fmt, py, pc)
            assert (a == b).all()
    # the strength the picture's own header asks for (USE_DEBLOCKER is not set here: none)
    assert (st.render_yuv_resize(h263mi.STRENGTH_FROM_HEADER, 3, 2) == st.render_yuv_resize(0, 3, 2)).all()
    # placement inside the caller's buffer: Cr in front of Cb in front of Y, gaps between them, tight pitches
    ow, oh = w + 3, h + 5
    cow, coh = lay.chroma_size(ow, oh)
    ocr = [2 * cow]
    ocb = [ocr[0] + cow * (coh + 3)]
    oy = [-(-(ocb[0] + cow * coh + 5) // ow) * ow]
    out = np.full(oy[0] + ow * oh + 7, SENTINEL, np.uint8)
    st.render_yuv_resize_into(5, out, ow, oh, h263mi.YUV_I420, offsets_y=oy, offsets_cb=ocb, offsets_cr=ocr)
    check_canvas(out, [resized(planes, w, h, 5, ow, oh)], ow, oh, lay.I420, ow, cow, (oy, ocb, ocr), "state %dx%d placed" % (w, h))
    with pytest.raises(h263mi.H263Error):
        st.render_yuv_resize(0, 0, 4)
    st.close()


# ---------------------------------------------------------------------------------------------
# a small batch, immediate: resized NV12 planes and resized RGBA in one call
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("padded_pitch", [False, True])
def test_batch_resized_nv12_planes_and_resized_rgba_in_one_call(padded_pitch):
    n, w, h, strength, fmt = 3, 176, 144, 7, h263mi.YUV_NV12
    ow, oh, rw, rh = 100, 37, 50, 30
    recs, planes = _upload_records(_small_streams(n, w, h, 700), w, h)
    want = [resized(p, w, h, strength, ow, oh) for p in planes]
    # the RGBA of the same call on a batch without any YUV shape
    plain = h263mi.Batch(n, w, h, 0, None)
    plain.set_rgba_resize(rw, rh)
    rgba_plain = _sentinel_buffer(h263mi.rgba_resize_extent(n, rw, rh))
    plain.decode(h263mi.PICTURE_I, recs[0].ptr, recs[1].ptr, recs[2].ptr, 0, strength, rgba_plain.ptr, None)
    plain.sync()
    plain.close()
    full = [orc.yuv420_to_rgba(*deblocked(p, w, strength), w) for p in planes]
    assert (rgba_plain.download() == np.concatenate([rgba_resize_ref.resize(f, w, h, rw, rh).ravel() for f in full])).all()
    ry, rc_ = lay.row_bytes(ow, fmt)
    py, pc = (padded(ry), padded(rc_)) if padded_pitch else (0, 0)
    b = h263mi.Batch(n, w, h, 0, None)
    b.set_yuv_resize(ow, oh, fmt, py, pc)
    b.set_rgba_resize(rw, rh)
    nbytes = h263mi.yuv_resize_extent(n, ow, oh, fmt, py, pc)
    assert nbytes == n * lay.picture_bytes(ow, oh, fmt, py, pc)
    rgba, yuv = _sentinel_buffer(rgba_plain.nbytes), _sentinel_buffer(nbytes)
    b.decode(h263mi.PICTURE_I, recs[0].ptr, recs[1].ptr, recs[2].ptr, 0, strength, rgba.ptr, yuv.ptr)
    b.sync()
    offs = lay.default_offsets(n, ow, oh, fmt, py, pc)
    check_canvas(yuv.download(), want, ow, oh, fmt, py or ry, pc or rc_, offs, "pitches %d %d" % (py, pc))
    assert (rgba.download() == rgba_plain.download()).all()
    # streams with nothing to render are not written
    b.set_active([True, False, True])
    yuv2 = _sentinel_buffer(nbytes)
    b.decode(h263mi.PICTURE_I, recs[0].ptr, recs[1].ptr, recs[2].ptr, 0, strength, None, yuv2.ptr)
    b.sync()
    check_canvas(yuv2.download(), want, ow, oh, fmt, py or ry, pc or rc_, offs, "inactive stream", skip=(1,))
    b.close()


# ---------------------------------------------------------------------------------------------
# a deferred rendering keeps the YUV shape of its request
# ---------------------------------------------------------------------------------------------
def test_pipelined_planes_follow_the_resize_of_their_request():
    n, w, h = 4, 176, 144
    cw, ch = lay.chroma_size(w, h)
    ow, oh = 100, 37
    coh = (oh + 1) // 2
    b = h263mi.Batch(n, w, h, 0, None, pipeline_post=True)
    recs1, planes1 = _upload_records(_small_streams(n, w, h, 100), w, h)
    recs2, planes2 = _upload_records(_small_streams(n, w, h, 200), w, h)
    recs3, planes3 = _upload_records(_small_streams(n, w, h, 300), w, h)
    # call 1: resized to 100 x 37 NV12, a 2 x 2 mosaic on one grid; call 2: full-size I420 at padded pitches; call 3: no shape
    p1 = 2 * ow + 56
    oy1 = [(s // 2) * (oh + coh + 1) * p1 + (s % 2) * (ow + 28) + 8 for s in range(n)]
    oc1 = [o + oh * p1 for o in oy1]
    py2, pc2 = 256, 128
    c1 = _sentinel_buffer(h263mi.yuv_resize_extent(n, ow, oh, h263mi.YUV_NV12, p1, p1, oy1, oc1))
    c2 = _sentinel_buffer(h263mi.yuv_layout_extent(n, w, h, h263mi.YUV_I420, py2, pc2))
    c3 = _sentinel_buffer(n * (w * h + 2 * cw * ch))
    b.set_yuv_resize(ow, oh, h263mi.YUV_NV12, p1, p1, oy1, oc1)
    b.decode(h263mi.PICTURE_I, recs1[0].ptr, recs1[1].ptr, recs1[2].ptr, 0, 7, None, c1.ptr)         # deferred
    b.set_yuv_layout(h263mi.YUV_I420, py2, pc2)
    b.decode(h263mi.PICTURE_I, recs2[0].ptr, recs2[1].ptr, recs2[2].ptr, 0, 3, None, c2.ptr)         # k_frame renders call 1
    b.set_yuv_layout(default=True)
    b.decode(h263mi.PICTURE_I, recs3[0].ptr, recs3[1].ptr, recs3[2].ptr, 0, 5, None, c3.ptr)         # ... and call 2
    b.set_yuv_resize(3, 2)                                                                          # (not what call 3 asked for)
    b.sync()                                                                                        # k_post renders call 3
    check_canvas(c1.download(), [resized(p, w, h, 7, ow, oh) for p in planes1], ow, oh, lay.NV12, p1, p1, (oy1, oc1, None), "call 1")
    check_canvas(c2.download(), [deblocked(p, w, 3) for p in planes2], w, h, lay.I420, py2, pc2,
                 lay.default_offsets(n, w, h, lay.I420, py2, pc2), "call 2")
    want3 = np.concatenate([np.concatenate(deblocked(p, w, 5)) for p in planes3])
    assert (c3.download() == want3).all()
    b.close()


# ---------------------------------------------------------------------------------------------
# refusals queue nothing; a layout and a resize replace each other
# ---------------------------------------------------------------------------------------------
def test_refusals_and_the_one_yuv_shape_in_force():
    n, w, h = 4, 176, 144
    ow, oh, fmt, py, pc = 100, 37, h263mi.YUV_NV12, 128, 128
    b = h263mi.Batch(n, w, h, 0, None)
    recs, planes = _upload_records(_small_streams(n, w, h, 500), w, h)
    b.set_yuv_resize(ow, oh, fmt, py, pc)
    nbytes = h263mi.yuv_resize_extent(n, ow, oh, fmt, py, pc)
    small = h263mi.DeviceBuffer(nbytes - 1)                          # one byte short: refused before anything is queued
    with pytest.raises(h263mi.H263Error) as e:
        b.decode(h263mi.PICTURE_I, recs[0].ptr, recs[1].ptr, recs[2].ptr, 0, 5, None, small.ptr)
    assert e.value.code == h263mi.ERR_INVALID_ARGUMENT
    assert not any(b.stream_has_picture(s) for s in range(n))       # no stream advanced
    ok = _sentinel_buffer(nbytes)
    b.decode(h263mi.PICTURE_I, recs[0].ptr, recs[1].ptr, recs[2].ptr, 0, 5, None, ok.ptr)
    b.sync()
    want = [resized(p, w, h, 5, ow, oh) for p in planes]
    offs = lay.default_offsets(n, ow, oh, fmt, py, pc)
    check_canvas(ok.download(), want, ow, oh, fmt, py, pc, offs, "after the refusal")
    with pytest.raises(h263mi.H263Error) as e:
        b.render_rgba(5, None, small.ptr)
    assert e.value.code == h263mi.ERR_INVALID_ARGUMENT
    # a refused resize leaves the shape in force as it was
    for bad in (dict(out_width=0, out_height=10), dict(out_width=ow, out_height=oh, format=fmt, pitch_y=99, pitch_c=128),
                dict(out_width=ow, out_height=oh, format=fmt, offsets_y=[0] * n)):
        with pytest.raises(h263mi.H263Error) as e:
            b.set_yuv_resize(**bad)
        assert e.value.code == h263mi.ERR_INVALID_ARGUMENT
    ok2 = _sentinel_buffer(nbytes)
    b.render_rgba(5, None, ok2.ptr)
    b.sync()
    assert (ok2.download() == ok.download()).all()
    # a layout replaces the resize ...
    b.set_yuv_layout(h263mi.YUV_I420, 256, 128)
    c = _sentinel_buffer(h263mi.yuv_layout_extent(n, w, h, h263mi.YUV_I420, 256, 128))
    b.render_rgba(5, None, c.ptr)
    b.sync()
    check_canvas(c.download(), [deblocked(p, w, 5) for p in planes], w, h, lay.I420, 256, 128,
                 lay.default_offsets(n, w, h, lay.I420, 256, 128), "layout after resize")
    # ... a resize the layout ...
    b.set_yuv_resize(ow, oh, fmt, py, pc)
    ok3 = _sentinel_buffer(nbytes)
    b.render_rgba(5, None, ok3.ptr)
    b.sync()
    assert (ok3.download() == ok.download()).all()
    # ... W' = w, H' = h is the full-size layout byte for byte ...
    b.set_yuv_resize(w, h, h263mi.YUV_I420, 256, 128)
    c2 = _sentinel_buffer(c.nbytes)
    b.render_rgba(5, None, c2.ptr)
    b.sync()
    assert (c2.download() == c.download()).all()
    # ... and NULL restores the default
    b.set_yuv_resize(default=True)
    cw, ch = lay.chroma_size(w, h)
    c3 = _sentinel_buffer(n * (w * h + 2 * cw * ch))
    b.render_rgba(5, None, c3.ptr)
    b.sync()
    assert (c3.download() == np.concatenate([np.concatenate(deblocked(p, w, 5)) for p in planes])).all()
    b.close()


# ---------------------------------------------------------------------------------------------
# 1080p, pipelined: a ladder rung in NV12 and an odd size in I420
# ---------------------------------------------------------------------------------------------
W, H, N1080 = 1920, 1080, 4


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
def streams_1080p():
    """-> ([frame] device records, [frame][stream] deblocked planes (strength 5)): an I then a P picture per stream"""
    recs, want = [], []
    planes = [None] * N1080
    for f in range(2):
        kind = h263mi.SYNTH_I_MIXED if f == 0 else h263mi.SYNTH_P
        pics = [h263mi.synth_picture_host(kind, W, H, 9 + s, f) for s in range(N1080)]
        for s, (m, c) in enumerate(pics):
            rc, planes[s] = orc.decode_picture(W, H, m, c, planes[s])
            assert rc == 0
        recs.append(_upload(pics))
        want.append([deblocked(p, W, 5) for p in planes])
    return recs, want


def _two_calls(b, recs, canvases):
    b.timing_reserve(8)
    b.timing_begin()
    for f, ptype in enumerate((h263mi.PICTURE_I, h263mi.PICTURE_P)):
        b.decode(ptype, recs[f][0].ptr, recs[f][1].ptr, recs[f][2].ptr, 0, 5, None, canvases[f].ptr)
    b.sync()
    return b.timing_end()


@pytest.mark.parametrize("ow,oh,fmt", [(640, 360, h263mi.YUV_NV12), (853, 481, h263mi.YUV_I420)])
def test_1080p_pipelined_rung(streams_1080p, ow, oh, fmt):
    recs, want = streams_1080p
    cw, ch = lay.chroma_size(W, H)
    plain = h263mi.Batch(N1080, W, H, 0, None, pipeline_post=True)
    kt0 = _two_calls(plain, recs, [h263mi.DeviceBuffer(N1080 * (W * H + 2 * cw * ch)) for _ in range(2)])
    plain.close()
    b = h263mi.Batch(N1080, W, H, 0, None, pipeline_post=True)
    b.set_yuv_resize(ow, oh, fmt)
    nbytes = h263mi.yuv_resize_extent(N1080, ow, oh, fmt)
    canvases = [_sentinel_buffer(nbytes + 64) for _ in range(2)]
    kt = _two_calls(b, recs, canvases)
    b.close()
    # the resize launches are post-processing time of the same renderings: no launch count moves
    assert (kt.frame_launches, kt.recon_launches, kt.post_launches) == (kt0.frame_launches, kt0.recon_launches, kt0.post_launches)
    assert (kt.frame_launches, kt.recon_launches, kt.post_launches) == (1, 1, 1)
    ry, rc_ = lay.row_bytes(ow, fmt)
    offs = lay.default_offsets(N1080, ow, oh, fmt)
    for f in range(2):
        check_canvas(canvases[f].download(), [ref.resize_planes(p, W, H, ow, oh) for p in want[f]], ow, oh, fmt, ry, rc_, offs,
                     "frame %d" % f)


# ---------------------------------------------------------------------------------------------
# a failure injected at every HIP call of one decode under a resize
# ---------------------------------------------------------------------------------------------
def test_a_failure_at_any_hip_call_of_a_resized_decode_leaves_a_consistent_state():
    n, w, h, strength, fmt = 3, 176, 144, 5, h263mi.YUV_NV12
    ow, oh, py, pc = 100, 37, 128, 128
    pics0 = _small_streams(n, w, h, 900)
    recs0, planes0 = _upload_records(pics0, w, h)
    pics1 = [recgen.inter_picture(w, h, seed=950 + s, mv_range=30, p_4v=0.2, p_coded=0.5, quant=8) for s in range(n)]
    recs1 = _upload(pics1)
    planes1 = []
    for (m, c), p0 in zip(pics1, planes0):
        rc, p = orc.decode_picture(w, h, m, c, p0)
        assert rc == 0
        planes1.append(p)
    nbytes = h263mi.yuv_resize_extent(n, ow, oh, fmt, py, pc)
    offs = lay.default_offsets(n, ow, oh, fmt, py, pc)
    states = {"old": planes0, "new": planes1}
    seen, failures = set(), 0
    for nth in range(1, 100):
        b = h263mi.Batch(n, w, h, 0, None)
        b.set_yuv_resize(ow, oh, fmt, py, pc)
        b.decode(h263mi.PICTURE_I, recs0[0].ptr, recs0[1].ptr, recs0[2].ptr, 0, strength, None, None)
        b.sync()
        out = _sentinel_buffer(nbytes)
        h263mi.debug_fail_nth_hip_call(nth)
        try:
            b.decode(h263mi.PICTURE_P, recs1[0].ptr, recs1[1].ptr, recs1[2].ptr, 0, strength, None, out.ptr)
            fired = h263mi.debug_fail_nth_hip_call(0) <= 0
            assert not fired, "the %d-th HIP call failed and the decode reported success" % nth
            done = True
        except h263mi.H263Error as e:
            assert e.code == h263mi.ERR_OUT_OF_MEMORY, (nth, e.code)
            h263mi.debug_fail_nth_hip_call(0)
            failures += 1
            done = False
        b.sync()
        # every stream as it was (a failure in front of the reconstruction launch), or every stream advanced
        got = [b.copy_yuv(s) for s in range(n)]
        which = [k for k, pl in states.items() if all((np.concatenate(g) == np.concatenate(p)).all() for g, p in zip(got, pl))]
        assert len(which) == 1, "failure at HIP call %d: the streams are neither all old nor all new" % nth
        assert which[0] == "new" if done else True
        seen.add(which[0])
        # ... and the batch still renders that state under its resize
        again = _sentinel_buffer(nbytes)
        b.render_rgba(strength, None, again.ptr)
        b.sync()
        check_canvas(again.download(), [resized(p, w, h, strength, ow, oh) for p in states[which[0]]], ow, oh, fmt, py, pc, offs,
                     "after a failure at HIP call %d" % nth)
        if done:
            check_canvas(out.download(), [resized(p, w, h, strength, ow, oh) for p in planes1], ow, oh, fmt, py, pc, offs, "the decode")
        b.close()
        if done:
            break
    else:
        pytest.fail("the decode never went through")
    assert failures >= 3 and seen == {"old", "new"}
