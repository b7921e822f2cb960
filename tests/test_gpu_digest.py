"""GPU tests of the on-device Adler-32 digests (k_digest, k_digest_final): every digest against zlib.adler32 -- chained row by
row over the uploaded or downloaded buffer for span tables, over the planes that copy_yuv delivers for the *_digest_yuv calls.
Exact: no tolerance anywhere."""
import zlib

import numpy as np
import pytest

import digest_ref as ref
import h263mi
import recgen
from test_gpu_yuv_layout import _sentinel_buffer, _small_streams, _upload_records

pytestmark = pytest.mark.gpu
CASES = ref.cases(h263mi.DIGEST_PIECE)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if h263mi.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the MI355X box")


def zlib_of_planes(planes, seed=1):
    v = seed
    for p in planes:
        v = zlib.adler32(np.ascontiguousarray(p).tobytes(), v)
    return v


def spans_of(case):
    return [h263mi.DigestSpan(*sp, 0) for sp in case.spans]


# ---------------------------------------------------------------------------------------------
# the case table through h263mi_adler32_spans_on, on an uploaded buffer
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,data", [(c, d) for c in CASES for d in c.data], ids=["%s-%s" % (c.name, d) for c in CASES for d in c.data])
def test_case_table(case, data):
    dev = h263mi.DeviceBuffer(max(case.nbytes, 1))
    results = []
    for garbage in (1, 2):
        buf = case.buffer(data, garbage)
        if case.nbytes:
            dev.upload(buf)
        got = [h263mi.adler32_spans(dev.ptr, case.nbytes, spans_of(case), seed, case.n_digests) for seed in ref.SEEDS]
        for seed, digests in zip(ref.SEEDS, got):
            assert digests == ref.zlib_of_spans(buf, case.spans, seed, case.n_digests), (case.name, data, garbage, hex(seed))
        results.append(got)
    assert results[0] == results[1]                          # the bytes between the rows never enter
    if case.name == "abc-cba" and data == "random":
        assert all(d[0] != d[1] for d in results[0])
    if case.name == "ff-long-row":
        assert case.nbytes == (16 << 20) + 5 and results[0][0] == [1636759246]
    dev.free()


def test_one_byte_between_rows_does_not_count_one_inside_a_row_does():
    case = next(c for c in CASES if c.name == "unaligned-1021x5")
    off, pitch, row_bytes, rows, _ = case.spans[0]
    buf = case.buffer("random", 1)
    dev = h263mi.DeviceBuffer(case.nbytes)
    dev.upload(buf)
    before = h263mi.adler32_spans(dev.ptr, case.nbytes, spans_of(case))
    assert before == ref.zlib_of_spans(buf, case.spans, 1, 1)
    gap = off + 2 * pitch + row_bytes + 3                   # between rows 2 and 3
    dev.upload(np.array([buf[gap] ^ 0x55], np.uint8), gap)
    assert h263mi.adler32_spans(dev.ptr, case.nbytes, spans_of(case)) == before
    inside = off + 2 * pitch + row_bytes - 1                # the last byte of row 2
    buf[inside] ^= 0x55
    dev.upload(buf[inside:inside + 1], inside)
    after = h263mi.adler32_spans(dev.ptr, case.nbytes, spans_of(case))
    assert after != before and after == ref.zlib_of_spans(buf, case.spans, 1, 1)
    dev.free()


# ---------------------------------------------------------------------------------------------
# one state: the digest follows the frame set that holds the last picture
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(1, 1), (5, 4), (100, 60), (176, 144)])
def test_state_digest_yuv(w, h):
    st = h263mi.H263State(h263mi.SORENSON_SPARK_BITSTREAM, device_id=0)
    with pytest.raises(h263mi.H263Error) as e:
        st.digest_yuv()
    assert e.value.code == h263mi.ERR_NO_PICTURE
    mbs, co = recgen.intra_picture(w, h, seed=w + 3 * h)
    st.submit_picture(w, h, mbs, co, h263mi.PICTURE_I, temporal_reference=0, pquant=8)
    seen = []
    for seed in ref.SEEDS:
        assert st.digest_yuv(seed) == zlib_of_planes(st.get_last_picture().as_yuv(), seed)
    seen.append(st.digest_yuv())
    for k in (1, 2):
        mbs, co = recgen.inter_picture(w, h, seed=w + 5 * h + k, mv_range=40, p_4v=0.2, p_intra=0.1)
        st.submit_picture(w, h, mbs, co, h263mi.PICTURE_P, temporal_reference=k, pquant=10)
        got = st.digest_yuv()                                # (in front of the download: ordered behind the decode by itself)
        assert got == zlib_of_planes(st.get_last_picture().as_yuv())
        seen.append(got)
    assert st.digest_yuv(0) == zlib_of_planes(st.get_last_picture().as_yuv(), 0)
    if w > 1:
        assert len(set(seen)) == 3                           # three pictures, three digests: `cur` is followed
    with pytest.raises(h263mi.H263Error) as e:
        st.digest_yuv(65521)
    assert e.value.code == h263mi.ERR_INVALID_ARGUMENT
    st.close()


# ---------------------------------------------------------------------------------------------
# a small batch: a stream without a picture, no sync needed, pipelined and overlapped batches
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["plain", "pipeline_post", "overlap_post"])
def test_batch_digest_yuv(mode):
    n, w, h = 3, 100, 60
    b = h263mi.Batch(n, w, h, 0, None, pipeline_post=mode == "pipeline_post", overlap_post=mode == "overlap_post")
    digests, rcs = b.digest_yuv()
    assert digests == [0] * n and rcs == [h263mi.ERR_NO_PICTURE] * n
    recs, _ = _upload_records(_small_streams(n, w, h, 900), w, h)
    rgba = _sentinel_buffer(n * w * h * 4)
    b.set_active([True, False, True])                        # stream 1 never gets a picture
    b.decode(h263mi.PICTURE_I, recs[0].ptr, recs[1].ptr, recs[2].ptr, 0, 5, rgba.ptr, None)
    early, rcs = b.digest_yuv()                              # no sync in front of it
    assert rcs == [0, h263mi.ERR_NO_PICTURE, 0] and early[1] == 0
    with pytest.raises(h263mi.H263Error) as e:
        b.digest_yuv(stream_rc=None)
    assert e.value.code == h263mi.ERR_NO_PICTURE
    b.sync()
    late, rcs = b.digest_yuv()
    assert late == early and rcs == [0, h263mi.ERR_NO_PICTURE, 0]
    for s in (0, 2):
        assert early[s] == zlib_of_planes(b.copy_yuv(s)), (mode, s)
        assert b.digest_yuv(0xFFF0FFF0)[0][s] == zlib_of_planes(b.copy_yuv(s), 0xFFF0FFF0)
    assert early[0] != early[2]
    with pytest.raises(h263mi.H263Error) as e:
        b.digest_yuv(seed=65521 << 16)
    assert e.value.code == h263mi.ERR_INVALID_ARGUMENT
    # every stream has one now: the call without per-stream codes goes through
    b.set_active(None)
    b.decode(h263mi.PICTURE_I, recs[0].ptr, recs[1].ptr, recs[2].ptr, 0, 5, rgba.ptr, None)
    all_three = b.digest_yuv(stream_rc=None)
    assert all_three == [zlib_of_planes(b.copy_yuv(s)) for s in range(n)]
    b.close()


def test_mixed_set_digest_yuv():
    from test_gpu_round5 import _MixedChains
    n = 5
    ch = _MixedChains(n, pipeline=False)
    qcif, small = (176, 144), (100, 60)
    ch.call({s: ("I", qcif if s % 2 == 0 else small) for s in range(n - 1)})      # the last stream never gets a picture
    ch.call({s: ("P", ch.size[s]) for s in range(n - 1)})
    digests, rcs = ch.m.digest_yuv()
    assert rcs == [0] * (n - 1) + [h263mi.ERR_NO_PICTURE] and digests[-1] == 0
    for s in range(n - 1):
        assert digests[s] == zlib_of_planes(ch.m.copy_yuv(s)), s
    assert h263mi.MixedSet is h263mi.MixedBatch
    with pytest.raises(h263mi.H263Error) as e:
        ch.m.digest_yuv(stream_rc=None)
    assert e.value.code == h263mi.ERR_NO_PICTURE
    ch.m.close()


# ---------------------------------------------------------------------------------------------
# output buffers of a pipelined batch through h263mi_batch_adler32_spans, no explicit sync
# ---------------------------------------------------------------------------------------------
def _digest_output(b, buf, nbytes, spans, n):
    """the digests of the call, and zlib's over the buffer downloaded behind it"""
    got = b.adler32_spans(buf.ptr, nbytes, spans)
    host = buf.download()
    want = ref.zlib_of_spans(host, [(sp.offset, sp.pitch, sp.row_bytes, sp.rows, sp.digest) for sp in spans], 1, n)
    # (the rows were rendered: they do not hold the sentinel any more)
    blank = ref.zlib_of_spans(np.full(nbytes, 0xC3, np.uint8), [(sp.offset, sp.pitch, sp.row_bytes, sp.rows, sp.digest) for sp in spans], 1, n)
    assert all(w_ != b_ for w_, b_ in zip(want, blank))
    return got, want


def test_output_buffers_of_a_pipelined_batch():
    n, w, h, strength = 4, 176, 144, 5
    recs, _ = _upload_records(_small_streams(n, w, h, 950), w, h)
    # d_rgba under a layout: half size, a row pitch, a 2 x 2 mosaic
    b = h263mi.Batch(n, w, h, 0, None, pipeline_post=True)
    ow, oh = w // 2, h // 2
    pitch = 2 * 4 * ow + 64
    offsets = [(s // 2) * oh * pitch + (s % 2) * (4 * ow + 32) for s in range(n)]
    _, _, nbytes = h263mi.rgba_layout_extent(n, w, h, 1, pitch, offsets)
    b.set_rgba_layout(1, pitch, offsets)
    rgba = _sentinel_buffer(nbytes)
    b.decode(h263mi.PICTURE_I, recs[0].ptr, recs[1].ptr, recs[2].ptr, 0, strength, rgba.ptr, None)
    got, want = _digest_output(b, rgba, nbytes, h263mi.spans_of_rgba(n, ow, oh, pitch, offsets), n)
    assert got == want
    b.close()
    # d_deblocked as NV12 with pitches
    b = h263mi.Batch(n, w, h, 0, None, pipeline_post=True)
    py, pc = 256, 192
    nbytes = h263mi.yuv_layout_extent(n, w, h, h263mi.YUV_NV12, py, pc)
    b.set_yuv_layout(h263mi.YUV_NV12, py, pc)
    planes = _sentinel_buffer(nbytes)
    b.decode(h263mi.PICTURE_I, recs[0].ptr, recs[1].ptr, recs[2].ptr, 0, strength, None, planes.ptr)
    got, want = _digest_output(b, planes, nbytes, h263mi.spans_of_yuv(n, w, h, h263mi.YUV_NV12, py, pc), n)
    assert got == want
    b.close()
    # resized I420, tight
    b = h263mi.Batch(n, w, h, 0, None, pipeline_post=True)
    rw, rh = 100, 37
    nbytes = h263mi.yuv_resize_extent(n, rw, rh, h263mi.YUV_I420)
    b.set_yuv_resize(rw, rh, h263mi.YUV_I420)
    planes = _sentinel_buffer(nbytes)
    b.decode(h263mi.PICTURE_I, recs[0].ptr, recs[1].ptr, recs[2].ptr, 0, strength, None, planes.ptr)
    got, want = _digest_output(b, planes, nbytes, h263mi.spans_of_yuv(n, rw, rh, h263mi.YUV_I420), n)
    assert got == want
    # ... which is the default shape of a rw x rh picture
    assert got == b.adler32_spans(planes.ptr, nbytes, h263mi.spans_of_planes_default(n, rw, rh))
    b.close()


# ---------------------------------------------------------------------------------------------
# a failure of the HIP runtime at every call of digest_yuv (the injected return code: nothing faults on the device)
# ---------------------------------------------------------------------------------------------
def test_hip_failure_at_every_call_of_digest_yuv():
    n, w, h = 3, 100, 60
    recs, _ = _upload_records(_small_streams(n, w, h, 970), w, h)
    failures = 0
    for nth in range(1, 40):
        b = h263mi.Batch(n, w, h, 0, None)                    # a new batch: its first digest call makes the staging too
        b.decode(h263mi.PICTURE_I, recs[0].ptr, recs[1].ptr, recs[2].ptr, 0, 0, None, None)
        b.sync()
        planes = [b.copy_yuv(s) for s in range(n)]
        want = [zlib_of_planes(p) for p in planes]
        h263mi.debug_fail_nth_hip_call(nth)
        try:
            got, rcs = b.digest_yuv()
            fired = h263mi.debug_fail_nth_hip_call(0) <= 0
            assert not fired, "the %d-th HIP call failed and digest_yuv reported success" % nth
            assert got == want
            b.close()
            break
        except h263mi.H263Error as e:
            h263mi.debug_fail_nth_hip_call(0)
            assert e.code == h263mi.ERR_HIP, (nth, e.code)
            failures += 1
        # the same call then succeeds, and the pictures are as they were
        got, rcs = b.digest_yuv()
        assert got == want and rcs == [0] * n, nth
        for s in range(n):
            assert all((a == p).all() for a, p in zip(b.copy_yuv(s), planes[s]))
        b.close()
    else:
        pytest.fail("digest_yuv never went through")
    assert failures >= 5                                      # two allocations, two copies, the launches, the wait


# ---------------------------------------------------------------------------------------------
# the headline geometry: 64 x 1080p, one I and two P pictures, every stream compared
# ---------------------------------------------------------------------------------------------
def test_64_streams_of_1080p_in_one_call():
    import bench
    n, gop, w, h = 64, 3, 1920, 1080
    wl = bench.Workload(h263mi, n, gop, 5, 0, None, events=True)
    b = h263mi.Batch(n, w, h, 0, None, pipeline_post=True)
    for f in range(gop):
        fr = wl.frames[f]
        if fr.get("first") is not None:
            b.decode_events(fr["ptype"], fr["mbs"].ptr, fr["first"].ptr, fr["ev"].ptr, fr["base"].ptr, 0, 0, None, None)
        else:
            b.decode(fr["ptype"], fr["mbs"].ptr, fr["co"].ptr, fr["base"].ptr, 0, 0, None, None)
    first, rcs = b.digest_yuv()
    assert rcs == [0] * n
    second = b.digest_yuv(stream_rc=None)
    want = [zlib_of_planes(b.copy_yuv(s)) for s in range(n)]
    assert first == want
    assert second == first
    assert len(set(first)) == n                              # 64 streams, 64 pictures
    b.close()
