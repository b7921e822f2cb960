"""GPU tests of the RGBA output resized to any W' x H' (h263mi_rgba_resize, k_rgba_resize), every picture against the oracle's
full-size RGBA put through the numpy restatement (tests/rgba_resize_ref.py)."""
import numpy as np
import pytest

import h263mi
import recgen
import rgba_layout_ref
import rgba_resize_ref as ref
from oracle import oracle as orc
from test_gpu_rgba_layout import _small_streams, _upload_records, full_rgba

pytestmark = pytest.mark.gpu
W, H = 1920, 1080
SENTINEL = 0xC3


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if h263mi.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the MI355X box")


def check_canvas(got, want_pics, pitch, offsets, what):
    exp = rgba_layout_ref.place(np.full(got.size, SENTINEL, np.uint8), want_pics, pitch, offsets)
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, "%s: %d bytes differ, first at byte %s" % (what, bad.size, bad[:8])


# ---------------------------------------------------------------------------------------------
# one state: h263mi_render_rgba_resize into host memory at a pitch
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(1, 1), (7, 9), (176, 144), (1920, 1080)])
def test_state_render_resize(w, h):
    st = h263mi.H263State(h263mi.SORENSON_SPARK_BITSTREAM, device_id=0)
    mbs, co = recgen.intra_picture(w, h, seed=w + 3 * h)
    st.submit_picture(w, h, mbs, co, h263mi.PICTURE_I, temporal_reference=0, pquant=8)
    rc, planes = orc.decode_picture(w, h, mbs, co, None)
    assert rc == 0
    for strength in (0, 7):
        full = full_rgba(planes, w, strength)
        for ow, oh in ((1, 1), (3, 4), (w, h), (w + 5, h + 2), (640, 360), (max(1, w // 2), max(1, h // 2))):
            want = ref.resize(full, w, h, ow, oh)
            assert (st.render_rgba_resize(strength, ow, oh) == want.ravel()).all(), (strength, ow, oh)
            pitch = ((4 * ow + 255) // 256) * 256 + 256
            out = np.full(oh * pitch, SENTINEL, np.uint8)
            st.render_rgba_resize_into(strength, out, ow, oh, pitch)
            check_canvas(out, [want], pitch, [0], "state %dx%d -> %dx%d strength %d" % (w, h, ow, oh, strength))
    with pytest.raises(h263mi.H263Error):
        st.render_rgba_resize(0, 0, 4)
    st.close()


# ---------------------------------------------------------------------------------------------
# the bench path: 64 x 1080p, events, H263MI_CFG_PIPELINE_POST (k_frame), one strength per stream
# ---------------------------------------------------------------------------------------------
def _streams_full(n, first_stream, gop, strengths):
    """[frame][stream] -> the stream's full-size RGBA"""
    out = [[None] * n for _ in range(gop)]
    for s in range(n):
        planes = None
        for f in range(gop):
            kind = h263mi.SYNTH_I_MIXED if f == 0 else h263mi.SYNTH_P
            mbs, co = h263mi.synth_picture_host(kind, W, H, first_stream + s, f)
            rc, planes = orc.decode_picture(W, H, mbs, co, planes)
            assert rc == 0
            out[f][s] = full_rgba(planes, W, strengths[s])
    return out


@pytest.fixture(scope="module")
def bench_streams():
    import bench
    n, first_stream, gop = 64, 5, 4
    strengths = np.array([s % 13 for s in range(n)], np.uint8)
    wl = bench.Workload(h263mi, n, gop, first_stream, 0, None, events=True)
    return wl, strengths, _streams_full(n, first_stream, gop, strengths)


def _decode(b, fr, out, strengths):
    """one frame index of bench.py's Workload (events where it has them)"""
    if fr.get("first") is not None:
        b.decode_events(fr["ptype"], fr["mbs"].ptr, fr["first"].ptr, fr["ev"].ptr, fr["base"].ptr, 0, 0, out, None, strengths=strengths)
    else:
        b.decode(fr["ptype"], fr["mbs"].ptr, fr["co"].ptr, fr["base"].ptr, 0, 0, out, None, strengths=strengths)


def _run_bench_path(wl, strengths, ow, oh, pitch, offs, nbytes, gop=4):
    b = h263mi.Batch(64, W, H, 0, None, pipeline_post=True)
    b.set_rgba_resize(ow, oh, pitch, offs)
    canvases = []
    for f in range(gop):
        c = h263mi.DeviceBuffer(nbytes)
        c.upload(np.full(nbytes, SENTINEL, np.uint8))
        canvases.append(c)
        _decode(b, wl.frames[f], c.ptr, strengths)
    b.sync()
    got = [c.download() for c in canvases]
    b.close()
    return got


def test_bench_path_640x360_tiles_in_an_8x8_canvas(bench_streams):
    """Batch(64, 1920, 1080, pipeline_post) with 64 strengths, events transport, I + 3 P: every frame index into one
    5120 x 2880 canvas of 640 x 360 tiles at a pitch of 20 480 bytes (k_frame into the scratch, then k_rgba_resize)"""
    wl, strengths, full = bench_streams
    ow, oh, pitch = 640, 360, 20480
    offs = [(s // 8) * oh * pitch + (s % 8) * ow * 4 for s in range(64)]
    nbytes = h263mi.rgba_resize_extent(64, ow, oh, pitch, offs)
    assert nbytes == 5120 * 2880 * 4
    got = _run_bench_path(wl, strengths, ow, oh, pitch, offs, nbytes)
    for f in range(4):
        check_canvas(got[f], [ref.resize(p, W, H, ow, oh) for p in full[f]], pitch, offs, "frame %d" % f)


def test_bench_path_480x270_is_routed_and_equals_quarter_layout(bench_streams):
    """480 x 270 is 1/4 of 1080p: the resize goes through the fused layout kernels and is byte for byte scale_log2 = 2"""
    wl, strengths, full = bench_streams
    pitch = 3840 * 4
    offs = [(s // 8) * 270 * pitch + (s % 8) * 480 * 4 for s in range(64)]
    nbytes = 3840 * 2160 * 4
    got = _run_bench_path(wl, strengths, 480, 270, pitch, offs, nbytes)
    for f in range(4):
        check_canvas(got[f], [rgba_layout_ref.box_average(p, W, H, 2) for p in full[f]], pitch, offs, "frame %d" % f)


def test_immediate_k_post_render_ps():
    """decode without output, then h263mi_batch_render_rgba_ps (k_post into the scratch, then k_rgba_resize): 600 x 340 tiles,
    4 x 4 in a canvas with a padded pitch"""
    import bench
    n, first_stream, gop = 16, 11, 2
    strengths = np.array([(3 * s) % 13 for s in range(n)], np.uint8)
    wl = bench.Workload(h263mi, n, gop, first_stream, 0, None, events=True)
    b = h263mi.Batch(n, W, H, 0, None)
    ow, oh = 600, 340
    pitch = 4 * ow * 4 + 256
    offs = [(s // 4) * oh * pitch + (s % 4) * ow * 4 for s in range(n)]
    nbytes = h263mi.rgba_resize_extent(n, ow, oh, pitch, offs)
    b.set_rgba_resize(ow, oh, pitch, offs)
    planes = [None] * n
    for f in range(gop):
        _decode(b, wl.frames[f], None, None)
        c = h263mi.DeviceBuffer(nbytes)
        c.upload(np.full(nbytes, SENTINEL, np.uint8))
        b.render_rgba(0, c.ptr, None, strengths=strengths)
        b.sync()
        want = []
        for s in range(n):
            kind = h263mi.SYNTH_I_MIXED if f == 0 else h263mi.SYNTH_P
            mbs, co = h263mi.synth_picture_host(kind, W, H, first_stream + s, f)
            rc, planes[s] = orc.decode_picture(W, H, mbs, co, planes[s])
            assert rc == 0
            want.append(ref.resize(full_rgba(planes[s], W, strengths[s]), W, H, ow, oh))
        check_canvas(c.download(), want, pitch, offs, "frame %d" % f)
    b.close()


# ---------------------------------------------------------------------------------------------
# a deferred rendering keeps the shape of its request; refusals queue nothing
# ---------------------------------------------------------------------------------------------
def test_pipelined_output_keeps_the_shape_of_its_request():
    n, w, h = 4, 176, 144
    b = h263mi.Batch(n, w, h, 0, None, pipeline_post=True)
    recs = [_upload_records(_small_streams(n, w, h, 100 * k), w, h) for k in (1, 2, 3, 4)]
    # call 1: resize 50 x 30 in a 2 x 2 canvas; call 2: layout 1/2; call 3: resize 200 x 170 tight; call 4: default
    p1, o1 = 2 * 50 * 4, [(s // 2) * 30 * 2 * 50 * 4 + (s % 2) * 50 * 4 for s in range(n)]
    c1 = h263mi.DeviceBuffer(h263mi.rgba_resize_extent(n, 50, 30, p1, o1))
    c2 = h263mi.DeviceBuffer(h263mi.rgba_layout_extent(n, w, h, 1)[2])
    c3 = h263mi.DeviceBuffer(h263mi.rgba_resize_extent(n, 200, 170))
    c4 = h263mi.DeviceBuffer(n * w * h * 4)
    for c in (c1, c2, c3, c4):
        c.upload(np.full(c.nbytes, SENTINEL, np.uint8))
    b.set_rgba_resize(50, 30, p1, o1)
    b.decode(h263mi.PICTURE_I, recs[0][0][0].ptr, recs[0][0][1].ptr, recs[0][0][2].ptr, 0, 7, c1.ptr, None)   # deferred
    b.set_rgba_layout(1)
    b.decode(h263mi.PICTURE_I, recs[1][0][0].ptr, recs[1][0][1].ptr, recs[1][0][2].ptr, 0, 3, c2.ptr, None)   # renders 1
    b.set_rgba_resize(200, 170)
    b.decode(h263mi.PICTURE_I, recs[2][0][0].ptr, recs[2][0][1].ptr, recs[2][0][2].ptr, 0, 5, c3.ptr, None)   # renders 2
    b.set_rgba_resize(default=True)
    b.decode(h263mi.PICTURE_I, recs[3][0][0].ptr, recs[3][0][1].ptr, recs[3][0][2].ptr, 0, 9, c4.ptr, None)   # renders 3
    b.set_rgba_layout(2)
    b.sync()                                                                                                   # renders 4
    f = lambda k, s: full_rgba(recs[k][1][s], w, (7, 3, 5, 9)[k])
    check_canvas(c1.download(), [ref.resize(f(0, s), w, h, 50, 30) for s in range(n)], p1, o1, "call 1")
    check_canvas(c2.download(), [rgba_layout_ref.box_average(f(1, s), w, h, 1) for s in range(n)], 88 * 4,
                 rgba_layout_ref.default_offsets(n, w, h, 1), "call 2")
    check_canvas(c3.download(), [ref.resize(f(2, s), w, h, 200, 170) for s in range(n)], 800,
                 [s * 170 * 800 for s in range(n)], "call 3")
    check_canvas(c4.download(), [f(3, s).reshape(h, w, 4) for s in range(n)], w * 4, [s * h * w * 4 for s in range(n)], "call 4")
    b.close()


def test_refused_resizes_and_canvases_queue_nothing():
    n, w, h = 4, 176, 144
    b = h263mi.Batch(n, w, h, 0, None)
    for bad in (dict(out_width=0, out_height=10), dict(out_width=40, out_height=30, row_pitch=100),
                dict(out_width=40, out_height=30, row_pitch=320, offsets=[0, 156, 30 * 320, 30 * 320 + 160])):
        with pytest.raises(h263mi.H263Error) as e:
            b.set_rgba_resize(**bad)
        assert e.value.code == h263mi.ERR_INVALID_ARGUMENT
    recs, planes = _upload_records(_small_streams(n, w, h, 300), w, h)
    pitch, offs = 2 * 40 * 4, [(s // 2) * 30 * 2 * 40 * 4 + (s % 2) * 40 * 4 for s in range(n)]
    b.set_rgba_resize(40, 30, pitch, offs)
    nbytes = h263mi.rgba_resize_extent(n, 40, 30, pitch, offs)
    small = h263mi.DeviceBuffer(nbytes - 1)                       # one byte too small: refused before anything is queued
    small.upload(np.full(nbytes - 1, SENTINEL, np.uint8))
    with pytest.raises(h263mi.H263Error) as e:
        b.decode(h263mi.PICTURE_I, recs[0].ptr, recs[1].ptr, recs[2].ptr, 0, 5, small.ptr, None)
    assert e.value.code == h263mi.ERR_INVALID_ARGUMENT
    assert not any(b.stream_has_picture(s) for s in range(n))    # no stream advanced
    assert (small.download() == SENTINEL).all()
    ok = h263mi.DeviceBuffer(nbytes)
    ok.upload(np.full(nbytes, SENTINEL, np.uint8))
    b.decode(h263mi.PICTURE_I, recs[0].ptr, recs[1].ptr, recs[2].ptr, 0, 5, ok.ptr, None)
    b.sync()
    check_canvas(ok.download(), [ref.resize(full_rgba(p, w, 5), w, h, 40, 30) for p in planes], pitch, offs, "after")
    with pytest.raises(h263mi.H263Error):
        b.render_rgba(5, small.ptr, None)
    assert (small.download() == SENTINEL).all()
    b.close()


# ---------------------------------------------------------------------------------------------
# a mixed-size set: every stream as 320 x 180 at its own buffer
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", [True, False])
def test_mixed_set_wall_of_320x180_tiles(pipeline):
    import sorenson_enc as enc
    from test_bitstream_e2e import make_codable
    q, strength = 6, 5
    sizes = [(176, 144), (320, 240), (352, 288), (1920, 1080), (176, 144)]
    n = len(sizes)
    ow, oh, pitch = 320, 180, 320 * 4 + 64
    need = (oh - 1) * pitch + 4 * ow
    m = h263mi.MixedBatch(n, pipeline_post=pipeline)
    m.set_rgba_resize(ow, oh, pitch)
    refs = [None] * n
    for f in range(2):
        datas, wants = [], []
        for s, (w, h) in enumerate(sizes):
            intra = f == 0
            if intra:
                mbs, co = recgen.intra_picture(w, h, seed=1000 * f + s, max_level=60)
                mbs = make_codable(mbs, q, s, 0)
            else:
                mbs, co = recgen.inter_picture(w, h, seed=1000 * f + s, mv_range=32, p_4v=0.2, p_intra=0.05, p_coded=0.4, quant=q,
                                               max_level=60)
                mbs = make_codable(mbs, q, s + f, 1)
            datas.append(enc.encode_picture(w, h, 0 if intra else 1, q, mbs, co, temporal_reference=f))
            rc, refs[s] = orc.decode_picture(w, h, mbs, co, None if intra else refs[s])
            assert rc == 0
            wants.append(ref.resize(full_rgba(refs[s], w, strength), w, h, ow, oh))
        # stream 4's buffer is one byte short in call 1: refused for that stream only
        bufs = [h263mi.DeviceBuffer(need - 1 if (f == 1 and s == 4) else need + 32) for s in range(n)]
        for c in bufs:
            c.upload(np.full(c.nbytes, SENTINEL, np.uint8))
        used, rcs, _ = m.decode_next_pictures(datas, n_threads=2, strength=strength, rgba=bufs)
        assert not any(m.sync())
        for s in range(n):
            if f == 1 and s == 4:
                assert rcs[s] == h263mi.ERR_INVALID_ARGUMENT
                assert (bufs[s].download() == SENTINEL).all()
                continue
            assert rcs[s] == 0, (f, s, rcs[s])
            check_canvas(bufs[s].download(), [wants[s]], pitch, [0], "call %d stream %d %s" % (f, s, sizes[s]))
    assert m.frame_store_bytes() > 0
    m.close()
