"""GPU tests of the RGBA output layout (h263mi_rgba_layout: 1/1, 1/2, 1/4 box averages, a row pitch, per-stream placement),
every picture against the oracle's full-size RGBA put through the numpy restatement (tests/rgba_layout_ref.py)."""
import numpy as np
import pytest

import h263mi
import recgen
import rgba_layout_ref as ref
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
SIZES = [(1, 1), (5, 4), (7, 9), (176, 144), (352, 288), (1920, 1080)]
W, H = 1920, 1080
SENTINEL = 0xC3


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if h263mi.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the MI355X box")


def full_rgba(planes, w, strength):
    cw = (w + 1) // 2
    if strength:
        planes = tuple(orc.deblock(p, pw, strength) for p, pw in zip(planes, (w, cw, cw)))
    return orc.yuv420_to_rgba(*planes, w)


def check_canvas(got, want_pics, w, h, scale, pitch, offsets, what):
    exp = ref.place(np.full(got.size, SENTINEL, np.uint8), want_pics, pitch, offsets)
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, "%s: %d bytes differ, first at byte %s" % (what, bad.size, bad[:8])


# ---------------------------------------------------------------------------------------------
# one state: h263mi_render_rgba_layout
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SIZES)
def test_state_render_layout(w, h):
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
        full = full_rgba(planes, w, strength)
        # scale 1/1 at the tight pitch is h263mi_render_rgba, byte for byte
        assert (st.render_rgba_layout(strength) == st.render_rgba(strength)).all()
        for scale in (0, 1, 2):
            ow, oh = ref.out_size(w, h, scale)
            want = ref.box_average(full, w, h, scale)
            assert (st.render_rgba_layout(strength, scale) == want.ravel()).all(), (strength, scale)
            pitch = ((4 * ow + 255) // 256) * 256 + 256                  # padded: the bytes between rows stay untouched
            out = np.full(oh * pitch, SENTINEL, np.uint8)
            st.render_rgba_layout_into(strength, out, scale, pitch)
            check_canvas(out, [want], w, h, scale, pitch, [0], "state %dx%d strength %d scale %d" % (w, h, strength, scale))
    st.close()


# ---------------------------------------------------------------------------------------------
# the bench path: 64 x 1080p, events, H263MI_CFG_PIPELINE_POST (k_frame), one strength per stream, 1/4 into a 4K mosaic
# ---------------------------------------------------------------------------------------------
def _streams_reference(n, first_stream, gop, strengths, scale):
    """[frame][stream] -> the stream's picture at the layout's scale"""
    out = [[None] * n for _ in range(gop)]
    for s in range(n):
        planes = None
        for f in range(gop):
            kind = h263mi.SYNTH_I_MIXED if f == 0 else h263mi.SYNTH_P
            mbs, co = h263mi.synth_picture_host(kind, W, H, first_stream + s, f)
            rc, planes = orc.decode_picture(W, H, mbs, co, planes)
            assert rc == 0
            out[f][s] = ref.box_average(full_rgba(planes, W, strengths[s]), W, H, scale)
    return out


def _mosaic(n, scale, cols):
    ow, oh = ref.out_size(W, H, scale)
    pitch = cols * ow * 4
    return pitch, [(s // cols) * oh * pitch + (s % cols) * ow * 4 for s in range(n)]


def test_bench_path_quarter_scale_4k_mosaic_k_frame():
    """bench.py's Workload(events=True) on Batch(64, 1920, 1080, pipeline_post): I + 3 P, every stream its own strength,
    each frame index into one 3840 x 2160 canvas (8 x 8 tiles of 480 x 270).  The k_frame launches alternate their
    direction: both are walked.  All 64 tiles of every frame are compared."""
    import bench
    n, first_stream, gop, scale = 64, 5, 4, 2
    strengths = np.array([s % 13 for s in range(n)], np.uint8)
    wl = bench.Workload(h263mi, n, gop, first_stream, 0, None, events=True)
    b = h263mi.Batch(n, W, H, 0, None, pipeline_post=True)
    pitch, offs = _mosaic(n, scale, 8)
    assert h263mi.rgba_layout_extent(n, W, H, scale, pitch, offs) == (480, 270, 3840 * 2160 * 4)
    b.set_rgba_layout(scale, pitch, offs)
    canvases = []
    b.timing_reserve(4 * gop)
    b.timing_begin()
    for f in range(gop):
        c = h263mi.DeviceBuffer(3840 * 2160 * 4)
        c.upload(np.full(c.nbytes, SENTINEL, np.uint8))
        canvases.append(c)
        fr = wl.frames[f]
        if fr.get("first") is not None:
            b.decode_events(fr["ptype"], fr["mbs"].ptr, fr["first"].ptr, fr["ev"].ptr, fr["base"].ptr, 0, 0, c.ptr, None,
                            strengths=strengths)
        else:
            b.decode(fr["ptype"], fr["mbs"].ptr, fr["co"].ptr, fr["base"].ptr, 0, 0, c.ptr, None, strengths=strengths)
    b.sync()
    kt = b.timing_end()
    assert kt.frame_launches == gop - 1 and kt.post_launches == 1 and kt.recon_launches == 1
    want = _streams_reference(n, first_stream, gop, strengths, scale)
    for f in range(gop):
        check_canvas(canvases[f].download(), want[f], W, H, scale, pitch, offs, "frame %d" % f)
    b.close()


def test_half_scale_immediate_k_post_render_ps():
    """the same at 1/2 through the immediate path: decode without output, then h263mi_batch_render_rgba_ps (k_post) into
    a 8 x 8 mosaic of 960 x 540 tiles with a padded pitch"""
    import bench
    n, first_stream, gop, scale = 64, 11, 2, 1
    strengths = np.array([(3 * s) % 13 for s in range(n)], np.uint8)
    wl = bench.Workload(h263mi, n, gop, first_stream, 0, None, events=True)
    b = h263mi.Batch(n, W, H, 0, None)
    ow, oh = ref.out_size(W, H, scale)
    pitch = 8 * ow * 4 + 256
    offs = [(s // 8) * oh * pitch + (s % 8) * ow * 4 for s in range(n)]
    _, _, nbytes = h263mi.rgba_layout_extent(n, W, H, scale, pitch, offs)
    b.set_rgba_layout(scale, pitch, offs)
    want = _streams_reference(n, first_stream, gop, strengths, scale)
    for f in range(gop):
        fr = wl.frames[f]
        if fr.get("first") is not None:
            b.decode_events(fr["ptype"], fr["mbs"].ptr, fr["first"].ptr, fr["ev"].ptr, fr["base"].ptr, 0, 0, None, None)
        else:
            b.decode(fr["ptype"], fr["mbs"].ptr, fr["co"].ptr, fr["base"].ptr, 0, 0, None, None)
        c = h263mi.DeviceBuffer(nbytes)
        c.upload(np.full(nbytes, SENTINEL, np.uint8))
        b.render_rgba(0, c.ptr, None, strengths=strengths)
        b.sync()
        check_canvas(c.download(), want[f], W, H, scale, pitch, offs, "frame %d" % f)
    b.close()


# ---------------------------------------------------------------------------------------------
# a deferred rendering keeps the layout of the call that requested it; refusals queue nothing
# ---------------------------------------------------------------------------------------------
def _small_streams(n, w, h, seed):
    pics = []
    for s in range(n):
        mbs, co = recgen.intra_picture(w, h, seed=seed + s)
        pics.append((mbs, co))
    return pics


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


def test_pipelined_output_follows_the_layout_of_its_request():
    n, w, h = 4, 176, 144
    b = h263mi.Batch(n, w, h, 0, None, pipeline_post=True)
    recs1, planes1 = _upload_records(_small_streams(n, w, h, 100), w, h)
    recs2, planes2 = _upload_records(_small_streams(n, w, h, 200), w, h)
    # call 1: 1/4, 2 x 2 mosaic; call 2: 1/2, one column with a padded pitch
    p1, o1 = 2 * 44 * 4, [(s // 2) * 36 * 2 * 44 * 4 + (s % 2) * 44 * 4 for s in range(n)]
    p2 = 88 * 4 + 64
    o2 = [s * 72 * p2 for s in range(n)]
    c1 = h263mi.DeviceBuffer(h263mi.rgba_layout_extent(n, w, h, 2, p1, o1)[2])
    c2 = h263mi.DeviceBuffer(h263mi.rgba_layout_extent(n, w, h, 1, p2, o2)[2])
    for c in (c1, c2):
        c.upload(np.full(c.nbytes, SENTINEL, np.uint8))
    b.set_rgba_layout(2, p1, o1)
    b.decode(h263mi.PICTURE_I, recs1[0].ptr, recs1[1].ptr, recs1[2].ptr, 0, 7, c1.ptr, None)      # deferred
    b.set_rgba_layout(1, p2, o2)
    b.decode(h263mi.PICTURE_I, recs2[0].ptr, recs2[1].ptr, recs2[2].ptr, 0, 3, c2.ptr, None)      # k_frame renders call 1
    b.set_rgba_layout(default=True)
    b.sync()                                                                                      # k_post renders call 2
    check_canvas(c1.download(), [ref.box_average(full_rgba(p, w, 7), w, h, 2) for p in planes1], w, h, 2, p1, o1, "call 1")
    check_canvas(c2.download(), [ref.box_average(full_rgba(p, w, 3), w, h, 1) for p in planes2], w, h, 1, p2, o2, "call 2")
    b.close()


def test_refused_layouts_and_canvases_queue_nothing():
    n, w, h = 4, 176, 144
    b = h263mi.Batch(n, w, h, 0, None)
    with pytest.raises(h263mi.H263Error) as e:
        b.set_rgba_layout(1, 88 * 4 * 2, [0, 88 * 4 - 4, 2 * 72 * 88 * 8, 2 * 72 * 88 * 8 + 88 * 4])   # 0 and 1 overlap
    assert e.value.code == h263mi.ERR_INVALID_ARGUMENT
    recs, planes = _upload_records(_small_streams(n, w, h, 300), w, h)
    pitch, offs = 2 * 44 * 4, [(s // 2) * 36 * 2 * 44 * 4 + (s % 2) * 44 * 4 for s in range(n)]
    b.set_rgba_layout(2, pitch, offs)
    nbytes = h263mi.rgba_layout_extent(n, w, h, 2, pitch, offs)[2]
    small = h263mi.DeviceBuffer(nbytes - 1)                       # one byte too small: refused before anything is queued
    with pytest.raises(h263mi.H263Error) as e:
        b.decode(h263mi.PICTURE_I, recs[0].ptr, recs[1].ptr, recs[2].ptr, 0, 5, small.ptr, None)
    assert e.value.code == h263mi.ERR_INVALID_ARGUMENT
    assert not any(b.stream_has_picture(s) for s in range(n))    # no stream advanced
    ok = h263mi.DeviceBuffer(nbytes)
    ok.upload(np.full(nbytes, SENTINEL, np.uint8))
    b.decode(h263mi.PICTURE_I, recs[0].ptr, recs[1].ptr, recs[2].ptr, 0, 5, ok.ptr, None)
    b.sync()
    check_canvas(ok.download(), [ref.box_average(full_rgba(p, w, 5), w, h, 2) for p in planes], w, h, 2, pitch, offs, "after")
    with pytest.raises(h263mi.H263Error):
        b.render_rgba(5, small.ptr, None)
    b.close()
