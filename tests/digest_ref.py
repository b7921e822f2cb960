"""Reference side of the digest tests (TEST INFRASTRUCTURE): a numpy model of the chunked Adler-32 formula that
h263-rs_amd/csrc/digest_kernel.inl implements, the expected value of a span table from zlib.adler32 chained row by row, and the
case table that the CPU checker (test_sim_digest.py) and the GPU (test_gpu_digest.py) both run.

The formula (include/h263mi.h): with N the string's length, a0 = seed & 0xffff, b0 = seed >> 16, M = 65521,
    A = (a0 + sum d_i) mod M,   B = (b0 + N * a0 + sum (N - i) * d_i) mod M,   digest = B << 16 | A,
and a piece of length L with T bytes behind it adds a_c = sum d_j to A and b_c + a_c * T, b_c = sum (L - j) * d_j, to B."""
import zlib

import numpy as np

M = 65521
SEEDS = (1, 0, 0xFFF0FFF0)


def adler32_chunked(data, seed=1, piece=4096):
    """the formula, piece by piece, every piece on its own (exact: Python integers)"""
    d = np.frombuffer(bytes(data), np.uint8).astype(np.uint64)
    n = int(d.size)
    a0, b0 = seed & 0xffff, seed >> 16
    a_sum, b_sum = 0, 0
    for p0 in range(0, n, piece):
        c = d[p0:p0 + piece]
        length = int(c.size)
        a_c = int(c.sum())
        b_c = int((c * np.arange(length, 0, -1, dtype=np.uint64)).sum())      # < 255 * piece^2 / 2: piece <= 2^26 stays below 2^64
        a_sum += a_c
        b_sum += b_c + a_c * (n - p0 - length)
    return ((b0 + n * a0 + b_sum) % M) << 16 | (a0 + a_sum) % M


def zlib_of_spans(buf, spans, seed, n_digests):
    """expected digests: zlib.adler32 chained row by row.  spans: (offset, pitch, row_bytes, rows, digest)"""
    out = [seed] * n_digests
    mv = memoryview(buf)
    for off, pitch, row_bytes, rows, k in spans:
        if not row_bytes:
            continue
        v = out[k]
        for r in range(rows):
            v = zlib.adler32(mv[off + r * pitch:off + r * pitch + row_bytes], v)
        out[k] = v
    return out


def extent_of(spans):
    """bytes a buffer must hold for the spans: exactly up to the last byte any of them names"""
    return max([off + (rows - 1) * pitch + row_bytes for off, pitch, row_bytes, rows, _ in spans if rows and row_bytes], default=0)


class Case:
    def __init__(self, name, spans, n_digests=None, data=("random", "ff")):
        self.name, self.spans = name, [tuple(int(v) for v in sp) for sp in spans]
        self.n_digests = n_digests if n_digests is not None else max([sp[4] for sp in self.spans], default=0) + 1
        self.data = data
        self.nbytes = extent_of(self.spans)

    def row_mask(self):
        mask = np.zeros(self.nbytes, bool)
        for off, pitch, row_bytes, rows, _ in self.spans:
            if not row_bytes or not rows:
                continue
            if pitch == row_bytes or rows == 1:
                mask[off:off + (rows - 1) * pitch + row_bytes] = True
            else:
                for r in range(rows):
                    mask[off + r * pitch:off + r * pitch + row_bytes] = True
        return mask

    def buffer(self, data, garbage_seed):
        """the rows hold `data` ("random": a fixed pseudo-random string by position, "ff": all 0xFF), every byte between them
        garbage that depends on garbage_seed"""
        buf = np.random.default_rng(1000 + garbage_seed).integers(0, 256, self.nbytes, dtype=np.uint8)
        mask = self.row_mask()
        if data == "ff":
            buf[mask] = 0xFF
        else:
            buf[mask] = np.random.default_rng(7).integers(0, 256, self.nbytes, dtype=np.uint8)[mask]
        return buf


def frame_store_spans(w, h, digest=0, base=0):
    """the three spans the library builds for one stream's picture in a pitched frame store (pitches beyond the widths)"""
    cw, ch = (w + 1) // 2, (h + 1) // 2
    pitch_c = (cw + 63) // 64 * 64 + 64
    pitch_y = 2 * pitch_c
    rows_y, rows_c = (h + 15) // 16 * 16, (h + 15) // 16 * 8
    off_cb = base + rows_y * pitch_y
    off_cr = off_cb + rows_c * pitch_c
    return [(base, pitch_y, w, h, digest), (off_cb, pitch_c, cw, ch, digest), (off_cr, pitch_c, cw, ch, digest)]


def cases(piece, big=(16 << 20) + 5):
    """the case table of the issue; piece: the kernel's piece length; big: the long single row (the checker may shrink it)"""
    out = [Case("row-%d" % n, [(0, n, n, 1, 0)]) for n in (0, 1, 15, 16, 17)]
    out.append(Case("unaligned-1021x5", [(3, 1031, 1021, 5, 0)]))
    out.append(Case("rows-of-1", [(0, 7, 1, 300, 0)]))
    out += [Case("piece%+d" % (n - piece) if n <= piece + 1 else "two-pieces+1", [(0, n, n, 1, 0)])
            for n in (piece - 1, piece, piece + 1, 2 * piece + 1)]
    out += [Case("ff-%d" % n, [(0, n, n, 1, 0)], data=("ff",)) for n in (5552, 5553, 65521 + 1)]
    out.append(Case("ff-long-row", [(0, big, big, 1, 0)], data=("ff",)))
    out.append(Case("ff-4099x4093", [(0, 4096, 4093, 4099, 0)], data=("ff",)))
    # three spans A, B, C and the same three as C, B, A: the weights follow the logical position, not the address
    a, b, c = (5, 40, 33, 7), (301, 17, 17, 3), (400, 2000, 1999, 2)
    out.append(Case("abc-cba", [a + (0,), b + (0,), c + (0,), c + (1,), b + (1,), a + (1,)]))
    # 5 digests with 0, 3, 0, 1 and 70 spans: empty digests in the middle, the waves' search through the table
    spans = [(11, 100, 90, 4, 1), (0, 0, 0, 0, 1), (500, 64, 64, 3, 1), (9, 5000, 4500, 1, 3)]
    spans += [(13 * k, 301, 1 + (37 * k) % 300, 1 + k % 4, 4) for k in range(70)]
    out.append(Case("five-digests", spans, n_digests=5))
    out += [Case("frame-%dx%d" % (w, h), frame_store_spans(w, h)) for w, h in ((5, 4), (100, 60), (176, 144))]
    return out
