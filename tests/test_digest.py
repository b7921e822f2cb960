"""CPU side of the on-device Adler-32 digests (h263mi_adler32_spans_on, h263mi_*_digest_yuv): the chunked formula the kernel
implements against zlib.adler32 (a numpy model, digest_ref.py), every refusal of the span table from the built library -- all of
them are decided on the host before any device call --, and the pure-Python span builders against the *_layout_extent functions."""
import ctypes as C
import os
import zlib

import numpy as np
import pytest

import digest_ref as ref
import h263mi

NO_GPU = not os.path.exists("/dev/kfd")
PIECES = (1, 3, 16, 4096, h263mi.DIGEST_PIECE, 1 << 20)
NEIGHBOUR = 65520 << 16 | 65520


@pytest.mark.parametrize("piece", PIECES)
def test_fixed_answers(piece):
    for seed in ref.SEEDS:
        assert ref.adler32_chunked(b"", seed, piece) == seed
    assert ref.adler32_chunked(b"a", 1, piece) == 0x00620062
    assert ref.adler32_chunked(b"abc", 1, piece) == 0x024D0127
    assert ref.adler32_chunked(b"Wikipedia", 1, piece) == 0x11E60398


@pytest.mark.parametrize("case", ref.cases(h263mi.DIGEST_PIECE), ids=lambda c: c.name)
def test_model_equals_zlib_on_the_case_table(case):
    for data in case.data:
        buf = case.buffer(data, 1)
        for k in range(case.n_digests):
            string = b"".join(buf[off + r * pitch:off + r * pitch + rb].tobytes()
                              for off, pitch, rb, rows, d in case.spans if d == k for r in range(rows))
            for seed in ref.SEEDS + (NEIGHBOUR,):
                want = zlib.adler32(string, seed)
                assert want == ref.zlib_of_spans(buf, case.spans, seed, case.n_digests)[k]
                for piece in PIECES:
                    if piece < 4096 and len(string) > 10000:
                        continue
                    assert ref.adler32_chunked(string, seed, piece) == want, (case.name, data, hex(seed), piece)


def _call(spans, n_spans=None, buffer_bytes=1 << 20, base=0x1000, seed=1, n_digests=1, out=True, batch=False):
    arr, n = h263mi._span_array(spans)
    digests = (C.c_uint32 * max(n_digests, 1))()
    return h263mi.lib().h263mi_adler32_spans_on(None, base, buffer_bytes, arr, n if n_spans is None else n_spans, seed,
                                               digests if out else None, n_digests)


def test_every_refusal_is_made_on_the_host():
    """each of these returns ERR_INVALID_ARGUMENT without a device (the base pointer is never read)"""
    S = h263mi.DigestSpan
    bad = h263mi.ERR_INVALID_ARGUMENT
    ok_span = S(0, 16, 16, 2, 0, 0)
    assert _call([ok_span], out=False) == bad                                   # digests NULL
    assert _call([ok_span], n_digests=0) == bad                                 # no digests
    assert _call([], n_spans=1) == bad                                          # spans NULL, n_spans > 0
    assert _call([S(0, 0, 0, 0, 0, 0)] * 65537) == bad                          # more than 65536 spans
    assert _call([S(0, 16, 16, 2, 0, 1)]) == bad                                # reserved word
    assert _call([S(0, 16, 16, 2, 1, 0)]) == bad                                # digest index >= n_digests
    assert _call([S(0, 16, 16, 2, 1, 0), S(0, 16, 16, 2, 0, 0)], n_digests=2) == bad      # index falls
    assert _call([S(0, 15, 16, 2, 0, 0)]) == bad                                # rows > 1, pitch < row_bytes
    assert _call([S(0, 0, 0, 2, 0, 0), S(0, 15, 16, 2, 0, 0)]) == bad           # ... also behind an empty span
    assert _call([S(1, 16, 16, 2, 0, 0)], buffer_bytes=32) == bad               # one byte behind the buffer
    assert _call([S(0, 17, 16, 2, 0, 0)], buffer_bytes=32) == bad
    assert _call([S(2 ** 64 - 8, 16, 16, 1, 0, 0)], buffer_bytes=2 ** 64 - 1) == bad      # offset + row wraps
    assert _call([S(0, 2 ** 63, 1, 3, 0, 0)], buffer_bytes=2 ** 64 - 1) == bad            # (rows - 1) * pitch wraps
    assert _call([S(16, 2 ** 64 - 16, 16, 2, 0, 0)], buffer_bytes=2 ** 64 - 1) == bad      # offset + ... wraps
    assert _call([ok_span], base=None) == bad                                   # d_base NULL, a span with bytes
    assert _call([S(0, 65536, 65536, 65536, 0, 0)], buffer_bytes=2 ** 33) == bad           # one digest of 2^32 bytes
    assert _call([S(0, 65536, 65536, 32768, 0, 0)] * 2, buffer_bytes=2 ** 33) == bad       # ... out of two spans
    assert _call([ok_span], seed=65521) == bad                                  # a half of the seed >= 65521
    assert _call([ok_span], seed=65521 << 16) == bad
    assert _call([ok_span], seed=0xFFFFFFFF) == bad
    L = h263mi.lib()
    out = (C.c_uint32 * 1)()
    assert L.h263mi_batch_adler32_spans(None, None, 0, None, 0, 1, out, 1) == bad          # no batch
    assert L.h263mi_digest_yuv(None, 1, out) == bad
    assert L.h263mi_batch_digest_yuv(None, 1, out, None) == bad
    assert L.h263mi_mixed_digest_yuv(None, 1, out, None) == bad


def test_well_formed_calls_get_as_far_as_the_device():
    """what passes the checks needs a device: ERR_NO_DEVICE where there is none.  The spans here name no byte (a NULL base is
    allowed then), so with a device the call is complete: every digest is the seed."""
    S = h263mi.DigestSpan
    for spans, nd in (([], 1), ([S(5, 0, 0, 7, 1, 0), S(0, 3, 9, 0, 2, 0)], 4)):
        arr, n = h263mi._span_array(spans)
        out = (C.c_uint32 * nd)()
        rc = h263mi.lib().h263mi_adler32_spans_on(None, None, 0, arr, n, NEIGHBOUR, out, nd)
        if NO_GPU:
            assert rc == h263mi.ERR_NO_DEVICE
        else:
            assert rc == h263mi.OK and list(out) == [NEIGHBOUR] * nd
    if NO_GPU:
        # spans with bytes, two 2^31-byte halves of one digest's limit, the largest seed: nothing left to refuse
        assert _call([S(0, 65536, 65536, 32768, 0, 0), S(0, 65536, 65535, 32768, 0, 0)], buffer_bytes=2 ** 33,
                     seed=NEIGHBOUR) == h263mi.ERR_NO_DEVICE
        with pytest.raises(h263mi.H263Error) as e:
            h263mi.adler32_spans(0x1000, 64, [(0, 16, 16, 2, 0)])
        assert e.value.code == h263mi.ERR_NO_DEVICE


def _last_byte(spans):
    return max(sp.offset + (sp.rows - 1) * sp.pitch + sp.row_bytes for sp in spans) - 1


def _strings(spans, n):
    """per digest: the (offset, length) of every row, in order"""
    out = [[] for _ in range(n)]
    for sp in spans:
        out[sp.digest] += [(sp.offset + r * sp.pitch, sp.row_bytes) for r in range(sp.rows)]
    return out


@pytest.mark.parametrize("w,h", [(1, 1), (5, 4), (100, 60), (176, 144), (1920, 1080)])
def test_span_builders_agree_with_the_layout_extents(w, h):
    n = 3
    cw, ch = (w + 1) // 2, (h + 1) // 2
    # RGBA: full size and the scaled layouts, tight and pitched
    for scale in (0, 1, 2):
        for pad in (0, 36):
            ow, oh = -(-w // (1 << scale)), -(-h // (1 << scale))
            pitch = 4 * ow + pad if pad else 0
            got_w, got_h, extent = h263mi.rgba_layout_extent(n, w, h, scale, pitch)
            assert (got_w, got_h) == (ow, oh)
            spans = h263mi.spans_of_rgba(n, ow, oh, pitch)
            assert [sp.digest for sp in spans] == list(range(n))
            assert _last_byte(spans) == extent - 1
            assert all(sp.row_bytes == 4 * ow and sp.rows == oh for sp in spans)
    assert _last_byte(h263mi.spans_of_rgba(n, 7, 3, 32)) == h263mi.rgba_resize_extent(n, 7, 3, 32) - 1
    # planes: I420 and NV12, tight and pitched; Y rows, then Cb rows, then Cr rows (NV12: the interleaved rows)
    for fmt, row_c, planes in ((h263mi.YUV_I420, cw, 3), (h263mi.YUV_NV12, 2 * cw, 2)):
        for py, pc in ((0, 0), (w + 13, row_c + 5)):
            extent = h263mi.yuv_layout_extent(n, w, h, fmt, py, pc)
            spans = h263mi.spans_of_yuv(n, w, h, fmt, py, pc)
            assert len(spans) == planes * n and [sp.digest for sp in spans] == sorted(sp.digest for sp in spans)
            # (h263mi_yuv_layout_extent counts whole pictures of P bytes back to back: behind the last chroma row it
            # includes the rest of that row's pitch, which no span names)
            assert _last_byte(spans) == extent - 1 - ((pc - row_c) if pc else 0)
            for s, rows in enumerate(_strings(spans, n)):
                assert sum(length for _, length in rows) == w * h + 2 * cw * ch
                assert [length for _, length in rows] == [w] * h + [row_c] * (ch * (planes - 1))
                assert all(a < b for (a, _), (b, _) in zip(rows, rows[1:]))
    # explicit offsets are taken as they are
    oy, ocb, ocr = [1000, 0], [5000, 4000], [7000, 6000]
    spans = h263mi.spans_of_yuv(2, w, h, h263mi.YUV_I420, 0, 0, oy, ocb, ocr)
    assert [sp.offset for sp in spans] == [1000, 5000, 7000, 0, 4000, 6000]
    assert [sp.offset for sp in h263mi.spans_of_rgba(2, w, h, 0, [64, 0])] == [64, 0]
    # the default planes of d_deblocked: tightly packed I420 per stream
    spans = h263mi.spans_of_planes_default(n, w, h)
    assert _last_byte(spans) == h263mi.yuv_layout_extent(n, w, h, default=True) - 1
    assert [(sp.offset, sp.pitch, sp.row_bytes, sp.rows) for sp in spans[:3]] == [(0, w, w, h), (w * h, cw, cw, ch),
                                                                                (w * h + cw * ch, cw, cw, ch)]
