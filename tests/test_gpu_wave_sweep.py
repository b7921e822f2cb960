"""The bookkeeping of the reconstruction waves -- record forms, fill, wave kinds, group words -- on the MI355X.

The designed tables of tests/wave_cases.py (the CPU twin of this file, test_sim_wave_sweep.py, holds the oracle and the kernel
phases on the CPU to the same cases, holds the checker's per-wave report against the anatomy and asserts that no declared
case is missing) through the C ABI, all three planes compared byte for byte with the C oracle.  The reconstruction code is
compiled separately into two kernels, so tables (a)-(c) go through
  H263State                      -- k_recon
  Batch(8, pipeline_post=True)   -- k_frame with 8 bands per picture
  Batch(16, pipeline_post=True)  -- k_frame with 4 bands
with different cases in the streams of a batch (streams share a size), and each path takes its pictures three ways: dense
coefficient blocks (submit_picture / Batch.decode), events (submit_picture_events / Batch.decode_events) and host records
(Batch.submit_host; an H263State takes host records in both of its entries).  Table (d) -- every group word -- is legal
content only and goes through the bitstream entry, Batch.decode_next_pictures_ex, immediate and pipelined, and once per
record-transport setting in a child process.

Every P picture is decoded over a freshly installed key frame (wave_cases.reference_records), which the oracle decodes too;
the expected planes are computed once per table and shared by its paths.  Every status word must be 0."""
import os
import subprocess
import sys

import numpy as np
import pytest

import h263mi
import wave_cases as wc
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if h263mi.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the MI355X box")


TABLES = {
    "a": wc.table_a_p,
    "a-I": wc.table_a_i,
    "a-dc": wc.table_a_dc,
    "b": wc.table_b,
    "c": wc.table_c,
}
MISSING = {
    "a": lambda cov: cov.missing_a((wc.PICTURE_P,)),
    "a-I": lambda cov: cov.missing_a((wc.PICTURE_I,)),
    "a-dc": lambda cov: cov.missing_a_dc(),
    "b": lambda cov: cov.missing_b(),
    "c": lambda cov: cov.missing_c(),
}
PATHS = ("state", "batch8", "batch16")
TRANSPORTS = ("dense", "events", "host")
_REFS = {}
_CASES = {}                                                     # the last table's [(picture, expected planes)]


def reference(w, h):
    """(records, coefficients, the oracle's planes) of the key frame every P picture of that size is predicted from"""
    if (w, h) not in _REFS:
        mbs, co = wc.reference_records(w, h)
        rc, planes = orc.decode_picture(w, h, mbs, co, None)
        assert rc == 0
        _REFS[(w, h)] = (mbs, co, planes)
    return _REFS[(w, h)]


def expected(pic):
    ref = reference(pic["w"], pic["h"])[2] if pic["picture_type"] != wc.PICTURE_I else None
    rc, want = orc.decode_picture(pic["w"], pic["h"], pic["mbs"], pic["coeffs"], ref)
    assert rc == 0
    return want


def cases(table):
    """[(picture, the oracle's planes)] of a table, kept for the table's paths and transports"""
    if table not in _CASES:
        _CASES.clear()
        cov = wc.Coverage()
        out = []
        for pic in TABLES[table]():
            cov.add(pic)
            out.append((pic, expected(pic)))
        assert MISSING[table](cov) == []
        _CASES[table] = out
    return _CASES[table]


def groups_by_size(items):
    """the cases of one picture size and type together, in the order the sizes first appear"""
    by = {}
    for it in items:
        by.setdefault((it[0]["w"], it[0]["h"], it[0]["picture_type"]), []).append(it)
    return list(by.values())


def check(pic, got, want, path):
    diff = wc.first_difference(pic, got, want)
    assert diff is None, "%s: %s" % (path, diff)


def intra_blocks(mbs, n_blocks):
    """mask of the pool blocks that belong to intra macroblocks (their element 0 is not a TCOEF)"""
    out = np.zeros(n_blocks, bool)
    for r in mbs:
        if int(r["mb_type"]) in wc.INTRA_TYPES:
            k = int(r["coeff_index"])
            out[k:k + wc.popcount(r["cbp"])] = True
    return out


def events_of(mbs, co):
    co = np.ascontiguousarray(co, np.int16).reshape(-1, 64)
    return h263mi.events_from_dense(co, intra_blocks(mbs, len(co)))


def run_state(items, transport):
    st = h263mi.H263State()

    def submit(w, h, mbs, co, picture_type, tr):
        if transport == "events":
            first, ev = events_of(mbs, co)
            st.submit_picture_events(w, h, mbs, first, ev, picture_type, temporal_reference=tr)
        else:
            st.submit_picture(w, h, mbs, co, picture_type, temporal_reference=tr)

    for pic, want in items:
        w, h = pic["w"], pic["h"]
        if pic["picture_type"] != wc.PICTURE_I:
            mbs, co, _ = reference(w, h)
            submit(w, h, mbs, co, h263mi.PICTURE_I, 0)
        submit(w, h, pic["mbs"], pic["coeffs"], pic["picture_type"], 1)
        check(pic, st.get_last_picture().as_yuv(), want, "H263State (k_recon), %s" % transport)
    st.close()


class Uploads:
    """the arrays of one Batch call: n streams' records, one coefficient pool (dense and as events), the streams' bases"""

    def __init__(self, n, mbs_per_picture, max_blocks, max_events):
        self.n = n
        self.d_mbs = h263mi.DeviceBuffer(n * mbs_per_picture * 32)
        self.d_co = h263mi.DeviceBuffer(max(1, max_blocks) * 128)
        self.d_first = h263mi.DeviceBuffer((max_blocks + 1) * 4 + 16)
        self.d_ev = h263mi.DeviceBuffer(max_events * 4 + 64)
        self.d_base = h263mi.DeviceBuffer(n * 8)
        self.blocks = 1

    def fill(self, pictures, w, h):
        """pictures: n (records, coefficients)"""
        from simlib import pad_records
        self.host = [(np.ascontiguousarray(m), np.ascontiguousarray(c, np.int16).reshape(-1, 64)) for m, c in pictures]
        padded = [pad_records(m, w, h) for m, _ in self.host]
        self.d_mbs.upload(np.concatenate(padded))
        base, at = [], 0
        for _, c in self.host:
            base.append(at)
            at += len(c)
        pool = np.concatenate([c for _, c in self.host]) if at else np.zeros((0, 64), np.int16)
        if at:
            self.d_co.upload(pool)
        intra = np.concatenate([intra_blocks(m, len(c)) for m, c in self.host]) if at else np.zeros(0, bool)
        first, ev = h263mi.events_from_dense(pool, intra)
        self.d_first.upload(first)
        if len(ev):
            self.d_ev.upload(ev)
        self.d_base.upload(np.array(base, np.uint64))
        self.blocks, self.n_events = max(at, 1), len(ev)

    def decode(self, b, picture_type, d_rgba, transport):
        if transport == "dense":
            b.decode(picture_type, self.d_mbs.ptr, self.d_co.ptr, self.d_base.ptr, self.blocks, 0, d_rgba.ptr)
        elif transport == "events":
            b.decode_events(picture_type, self.d_mbs.ptr, self.d_first.ptr, self.d_ev.ptr, self.d_base.ptr, 0, 0, d_rgba.ptr)
        else:
            b.submit_host(picture_type, [m for m, _ in self.host], [c for _, c in self.host])

    def free(self):
        for d in (self.d_mbs, self.d_co, self.d_first, self.d_ev, self.d_base):
            d.free()


def decode_batch(run, n, transport, what="Batch"):
    """the cases of one size in the streams of a frame-pipelined batch, n at a time: the key frame in every stream (P
    pictures), then n cases at once.  Returns the planes per case"""
    w, h, ptype = run[0][0]["w"], run[0][0]["h"], run[0][0]["picture_type"]
    b = h263mi.Batch(n, w, h, pipeline_post=True)
    d_rgba = h263mi.DeviceBuffer(n * w * h * 4)
    ref_mbs, ref_co, _ = reference(w, h)
    key = Uploads(n, b.mbs_per_picture, n * len(ref_co), n * 4 * len(ref_co))
    key.fill([(ref_mbs, ref_co)] * n, w, h)
    most = max(len(p["coeffs"]) for p, _ in run)
    most_ev = max(int(np.count_nonzero(p["coeffs"])) for p, _ in run)
    cur = Uploads(n, b.mbs_per_picture, n * most, n * most_ev)
    out = []
    for at in range(0, len(run), n):
        part = run[at:at + n]
        part = part + [run[0]] * (n - len(part))                 # (idle streams repeat the first case)
        cur.fill([(p["mbs"], p["coeffs"]) for p, _ in part], w, h)
        if ptype != wc.PICTURE_I:
            for _ in range(1 + ((at // n) & 1)):                 # (one more launch in front of every other set: the direction flips)
                key.decode(b, h263mi.PICTURE_I, d_rgba, "dense")
        cur.decode(b, ptype, d_rgba, transport)                  # k_frame: this picture's reconstruction + the one before's post half
        rcs = b.sync_streams()
        assert all(rc == 0 for rc in rcs), (what, rcs)
        out += [b.copy_yuv(s) for s in range(min(n, len(run) - at))]
    b.sync()
    b.close()
    for d in (key, cur):
        d.free()
    d_rgba.free()
    return out


def run_batch(items, n, transport):
    for run in groups_by_size(items):
        got = decode_batch(run, n, transport)
        for k, ((pic, want), planes) in enumerate(zip(run, got)):
            check(pic, planes, want, "Batch(%d, pipeline_post) stream %d (k_frame, %d bands), %s" % (n, k % n, 8 if n < 16 else 4, transport))


@pytest.mark.parametrize("table,path,transport", [(t, p, tr) for t in TABLES for p in PATHS for tr in TRANSPORTS
                                                  if not (p == "state" and tr == "host")])
def test_wave_table(table, path, transport):
    items = cases(table)
    if path == "state":
        run_state(items, transport)
    else:
        run_batch(items, 8 if path == "batch8" else 16, transport)


# ---------------------------------------------------------------------------------------------------------------
# (d): every group word, through the bitstream entry
# ---------------------------------------------------------------------------------------------------------------
_D = {}


def d_cases(n):
    """(key frame bytes, the oracle's key frame, [(picture, bytes, expected planes)]) of table (d)'s width for n"""
    import sorenson_enc as enc
    if n not in _D:
        w, h = wc.d_size(n)
        mbs, co = wc.d_reference_records(n)
        key = enc.encode_picture(w, h, 0, wc.D_PQUANT, mbs, co, temporal_reference=0)
        rc, ref = orc.decode_picture(w, h, mbs, co, None)
        assert rc == 0
        cov = wc.Coverage()
        pics = []
        for pic in wc.table_d((n,)):
            cov.add(pic)
            data = enc.encode_picture(w, h, 1, wc.D_PQUANT, pic["mbs"], pic["coeffs"], temporal_reference=1)
            rc, want = orc.decode_picture(w, h, pic["mbs"], pic["coeffs"], ref)
            assert rc == 0
            pics.append((pic, data, want))
        assert cov.missing_d((n,)) == []
        _D[n] = (key, ref, pics)
    return _D[n]


def run_d(n, pipelined):
    """the four pictures of one width in the four streams of a batch: the key frame in every stream, then the P pictures"""
    key, ref, pics = d_cases(n)
    w, h = wc.d_size(n)
    b = h263mi.Batch(len(pics), w, h, pipeline_post=pipelined)
    d_rgba = h263mi.DeviceBuffer(len(pics) * w * h * 4)
    for datas in ([key] * len(pics), [data for _, data, _ in pics]):
        used, rcs = b.decode_next_pictures_ex(datas, n_threads=2, strength=0, d_rgba=d_rgba.ptr)
        assert not any(rcs), rcs
    assert all(rc == 0 for rc in b.sync_streams())
    b.sync()
    for s, (pic, _, want) in enumerate(pics):
        check(pic, b.copy_yuv(s), want, "Batch.decode_next_pictures_ex (%s), n = %d, stream %d" % ("pipelined" if pipelined else "immediate", n, s))
    b.close()
    d_rgba.free()


@pytest.mark.parametrize("pipelined", [False, True], ids=["immediate", "pipelined"])
@pytest.mark.parametrize("n", range(1, 8))
def test_group_words_through_the_bitstream_entry(n, pipelined):
    run_d(n, pipelined)


@pytest.mark.parametrize("sparse,direct", [("1", "1"), ("1", "0"), ("0", "1")],
                         ids=["sparse_records_direct_words", "sparse_records_packed_words", "dense_records"])
def test_group_words_in_every_record_transport_setting(sparse, direct):
    """table (d) once per setting of H263MI_SPARSE_RECORDS / H263MI_DIRECT_WORDS (read when the library is loaded: a fresh
    interpreter, as tests/test_gpu_round5.py::test_sparse_and_dense_record_transport_decode_alike starts one)"""
    root = os.path.dirname(HERE)
    code = ("import sys\n"
            "sys.path[:0] = [%r, %r, %r]\n"
            "import test_gpu_wave_sweep as t\n"
            "for n in range(1, 8):\n"
            "    t.run_d(n, True)\n"
            "print('group-words-ok')\n" % (root, os.path.join(root, "h263-rs_amd"), HERE))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, H263MI_SPARSE_RECORDS=sparse, H263MI_DIRECT_WORDS=direct),
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "group-words-ok" in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])
