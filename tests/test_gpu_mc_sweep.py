"""Motion compensation swept over every vector phase, border and width -- on the MI355X.

The designed tables of tests/mc_cases.py (the CPU twin of this file, test_sim_mc_sweep.py, holds the oracle, the numpy
restatement and the kernel phases on the CPU to the same cases and asserts that no case class is missing) through the
C ABI, all three planes compared byte for byte with the C oracle.  The reconstruction code is compiled separately into
two kernels, so every table goes through
  H263State                      -- k_recon
  Batch(8, pipeline_post=True)   -- k_frame with 8 bands per picture
  Batch(16, pipeline_post=True)  -- k_frame with 4 bands
with different cases in the streams of a batch (streams share a size: the cases are grouped by picture size) and the
launch direction alternating (an extra key-frame call in front of every other batch of cases flips it).

Every case is decoded over a freshly installed reference: the key frame of mc_cases.reference_records, which the
oracle decodes too.  A decoder takes a reference in no other way, so table (f) -- every pair of two-tap sums -- runs
over its construction blown up to flat 8x8 blocks (mc_cases.f_blocks_reference): the same 261 121 pairs, at the corners
where four blocks meet."""
import numpy as np
import pytest

import h263mi
import mc_cases as mc
from oracle import oracle as orc
from simlib import pad_records

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if h263mi.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the MI355X box")


TABLES = {
    "a[1-40]": lambda: mc.table_a(tuple(range(1, 41))),
    "a[41-80]": lambda: mc.table_a(tuple(range(41, 81))),
    "a[128]": lambda: mc.table_a((128,)),
    "a[1920]": lambda: mc.table_a((1920,)),
    "b": mc.table_b,
    "c": mc.table_c,
    "d": mc.table_d,
    "e": mc.table_e,
    "e_wrap": mc.table_e_wrap,
}
MISSING = {
    "a[1-40]": lambda cov: cov.missing_a(tuple(range(1, 41))),
    "a[41-80]": lambda cov: cov.missing_a(tuple(range(41, 81))),
    "a[128]": lambda cov: cov.missing_a((128,)),
    "a[1920]": lambda cov: cov.missing_a((1920,)),
    "b": lambda cov: cov.missing_b(),
    "c": lambda cov: cov.missing_c(),
    "d": lambda cov: cov.missing_d(),
    "e": lambda cov: cov.missing_e(),
    "e_wrap": lambda cov: cov.missing_e_wrap(),
}
PATHS = ("state", "batch8", "batch16")
_REFS = {}
_CASES = {}                                                     # the last table's [(picture, expected planes)]


def reference(w, h):
    """(records, coefficients, the oracle's planes) of the key frame every case of that size is predicted from"""
    if (w, h) not in _REFS:
        mbs, co = mc.reference_records(w, h)
        rc, planes = orc.decode_picture(w, h, mbs, co, None)
        assert rc == 0
        _REFS[(w, h)] = (mbs, co, planes)
    return _REFS[(w, h)]


def cases(table):
    """[(picture, the oracle's planes)] of a table, kept for the table's three paths"""
    if table not in _CASES:
        _CASES.clear()
        out = []
        cov = mc.Coverage()
        for pic in TABLES[table]():
            rc, want = orc.decode_picture(pic["w"], pic["h"], pic["mbs"], pic["coeffs"], reference(pic["w"], pic["h"])[2])
            assert rc == 0
            cov.add(pic)
            out.append((pic, want))
        assert MISSING[table](cov) == []
        _CASES[table] = out
    return _CASES[table]


def groups_by_size(items):
    """runs of consecutive cases of one picture size"""
    run = []
    for it in items:
        if run and (run[0][0]["w"], run[0][0]["h"]) != (it[0]["w"], it[0]["h"]):
            yield run
            run = []
        run.append(it)
    if run:
        yield run


def check(pic, got, want, path):
    diff = mc.first_difference(pic, got, want)
    assert diff is None, "%s: %s" % (path, diff)


def run_state(items):
    st = h263mi.H263State()
    for pic, want in items:
        mbs, co, _ = reference(pic["w"], pic["h"])
        st.submit_picture(pic["w"], pic["h"], mbs, co, h263mi.PICTURE_I)
        st.submit_picture(pic["w"], pic["h"], pic["mbs"], pic["coeffs"], h263mi.PICTURE_P, temporal_reference=1)
        check(pic, st.get_last_picture().as_yuv(), want, "H263State (k_recon)")
    st.close()


class _Uploads:
    """the device arrays of one Batch.decode call: n streams' records, one coefficient pool, the streams' bases"""

    def __init__(self, n, mbs_per_picture, max_blocks):
        self.n, self.mpp = n, mbs_per_picture
        self.d_mbs = h263mi.DeviceBuffer(n * mbs_per_picture * 32)
        self.d_co = h263mi.DeviceBuffer(max(1, max_blocks) * 128)
        self.d_base = h263mi.DeviceBuffer(n * 8)
        self.blocks = 1

    def fill(self, pictures, w, h):
        """pictures: n (records, coefficients)"""
        mbs = np.concatenate([pad_records(m, w, h) for m, _ in pictures])
        self.d_mbs.upload(mbs)
        if all(c is pictures[0][1] for _, c in pictures):       # the same picture in every stream: one copy, every base 0
            base, at = [0] * len(pictures), len(pictures[0][1])
            if at:
                self.d_co.upload(np.ascontiguousarray(pictures[0][1], np.int16))
        else:
            base, at = [], 0
            for _, c in pictures:
                base.append(at)
                at += len(c)
            if at:
                self.d_co.upload(np.concatenate([np.ascontiguousarray(c, np.int16).reshape(-1, 64) for _, c in pictures if len(c)]))
        self.d_base.upload(np.array(base, np.uint64))
        self.blocks = max(at, 1)

    def decode(self, b, picture_type, d_rgba):
        b.decode(picture_type, self.d_mbs.ptr, self.d_co.ptr, self.d_base.ptr, self.blocks, 0, d_rgba.ptr)

    def free(self):
        for d in (self.d_mbs, self.d_co, self.d_base):
            d.free()


def run_batch(items, n):
    """every case in a stream of a frame-pipelined batch: the key frame in every stream, then n cases at once"""
    calls = 0
    for run in groups_by_size(items):
        w, h = run[0][0]["w"], run[0][0]["h"]
        b = h263mi.Batch(n, w, h, pipeline_post=True)
        d_rgba = h263mi.DeviceBuffer(n * w * h * 4)
        ref_mbs, ref_co, _ = reference(w, h)
        key = _Uploads(n, b.mbs_per_picture, n * len(ref_co))
        key.fill([(ref_mbs, ref_co)] * n, w, h)
        cur = _Uploads(n, b.mbs_per_picture, n * max(len(p["coeffs"]) for p, _ in run))
        for at in range(0, len(run), n):
            part = run[at:at + n]
            part = part + [run[0]] * (n - len(part))             # (idle streams repeat the first case)
            cur.fill([(p["mbs"], p["coeffs"]) for p, _ in part], w, h)
            for _ in range(1 + (calls & 1)):                     # (one more launch in front of every other set: the direction flips)
                key.decode(b, h263mi.PICTURE_I, d_rgba)
            cur.decode(b, h263mi.PICTURE_P, d_rgba)              # k_frame: this picture's reconstruction + the key frame's post half
            calls += 1
            assert all(rc == 0 for rc in b.sync_streams())
            for s, (pic, want) in enumerate(part):
                check(pic, b.copy_yuv(s), want, "Batch(%d, pipeline_post) stream %d (k_frame, %d bands)" % (n, s, 8 if n < 16 else 4))
        b.sync()
        b.close()
        for d in (key, cur):
            d.free()
        d_rgba.free()


@pytest.mark.parametrize("table,path", [(t, p) for t in TABLES for p in PATHS])
def test_mc_table(table, path):
    items = cases(table)
    if path == "state":
        run_state(items)
    else:
        run_batch(items, 8 if path == "batch8" else 16)


# ---------------------------------------------------------------------------------------------------------------
# (f): every pair of two-tap sums, over the flat-block reference
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table_f():
    w, h, intra, push, co = mc.f_blocks_reference()
    rc, ref = orc.decode_picture(w, h, intra, mc.NO_COEFFS, None)
    assert rc == 0
    rc, ref = orc.decode_picture(w, h, push, co, ref)
    assert rc == 0
    # the coverage the table exists for, recomputed from the reference the decoders will hold
    assert mc.pair_coverage(ref[0].reshape(h, w)).sum() == 511 * 511
    hs, vs = mc.sum_coverage(ref[0].reshape(h, w))
    assert hs.all() and vs.all()
    items = []
    for pic in mc.table_f(w):
        rc, want = orc.decode_picture(w, h, pic["mbs"], pic["coeffs"], ref)
        assert rc == 0
        items.append((pic, want))
    return w, h, intra, push, co, ref, items


def test_mc_table_f_state(table_f):
    w, h, intra, push, co, ref, items = table_f
    st = h263mi.H263State()
    for pic, want in items:
        st.submit_picture(w, h, intra, mc.NO_COEFFS, h263mi.PICTURE_I)
        st.submit_picture(w, h, push, co, h263mi.PICTURE_P, temporal_reference=1)
        check(pic, st.get_last_picture().as_yuv(), ref, "H263State (k_recon), the reference itself")
        st.submit_picture(w, h, pic["mbs"], pic["coeffs"], h263mi.PICTURE_P, temporal_reference=2)
        check(pic, st.get_last_picture().as_yuv(), want, "H263State (k_recon)")
    st.close()


@pytest.mark.parametrize("n", [3, 16])
def test_mc_table_f_batch(table_f, n):
    """the three pictures of (f) in the streams of a batch (stream s takes picture s % 3); with n = 3 the RGBA of the
    (+1/2, +1/2) picture is checked too (strength 0), so the pipelined post half has seen it"""
    w, h, intra, push, co, ref, items = table_f
    b = h263mi.Batch(n, w, h, pipeline_post=True)
    d_rgba = [h263mi.DeviceBuffer(n * w * h * 4) for _ in range(2)]
    up = _Uploads(n, b.mbs_per_picture, n * len(co))
    up.fill([(intra, mc.NO_COEFFS)] * n, w, h)
    up.decode(b, h263mi.PICTURE_I, d_rgba[0])
    assert all(rc == 0 for rc in b.sync_streams())
    up.fill([(push, co)] * n, w, h)
    up.decode(b, h263mi.PICTURE_P, d_rgba[0])
    assert all(rc == 0 for rc in b.sync_streams())
    up.fill([(items[s % 3][0]["mbs"], mc.NO_COEFFS) for s in range(n)], w, h)
    up.decode(b, h263mi.PICTURE_P, d_rgba[1])
    assert all(rc == 0 for rc in b.sync_streams())
    for s in range(n):
        pic, want = items[s % 3]
        check(pic, b.copy_yuv(s), want, "Batch(%d, pipeline_post) stream %d (k_frame)" % (n, s))
    b.sync()                                                    # the last picture's post half
    if n == 3:
        got = d_rgba[1].download(w * h * 4, 0)
        assert (got == orc.yuv420_to_rgba(*items[0][1], w)).all(), "RGBA of the (+1/2, +1/2) picture"
    b.close()
    up.free()
    for d in d_rgba:
        d.free()
