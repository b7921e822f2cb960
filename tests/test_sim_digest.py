"""k_digest and k_digest_final (h263-rs_amd/csrc/digest_kernel.inl) run lane by lane on the CPU under AddressSanitizer + UBSan
(tests/sim_digest/sim_digest.cpp) over a buffer of exactly buffer_bytes, against zlib.adler32 chained row by row (digest_ref.py).
Every case of the table runs twice with different garbage between the rows: the digests must be equal, and equal to zlib's.
The long single row has its full size here, 16 MiB + 5 bytes (it is not shrunk)."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import digest_ref as ref
import h263mi

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ref.cases(h263mi.DIGEST_PIECE)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    # built into a temporary directory: a read-only checkout passes too
    out = str(tmp_path_factory.mktemp("sim_digest") / "sim_digest")
    subprocess.check_call(["g++", "-O1", "-g", "-fno-strict-aliasing", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                           "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", out,
                           os.path.join(HERE, "sim_digest", "sim_digest.cpp")])
    return out


def _env():
    return dict(os.environ, ASAN_OPTIONS="detect_leaks=0")


def _run(driver, tmp, case, buf, seeds=ref.SEEDS):
    """buf: the buffer's bytes, or None: all 0xFF, made by the checker.  -> per seed: the digests, or None (refused)"""
    inp, outp = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<Q4I", case.nbytes, len(case.spans), case.n_digests, len(seeds), 1 if buf is None else 0))
        f.write(struct.pack("<%dI" % len(seeds), *seeds))
        for off, pitch, row_bytes, rows, k in case.spans:
            f.write(struct.pack("<QQIIII", off, pitch, row_bytes, rows, k, 0))
        if buf is not None:
            f.write(buf.tobytes())
    r = subprocess.run([driver, inp, outp], capture_output=True, text=True, env=_env(), timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    words = np.fromfile(outp, np.uint32).reshape(len(seeds), 1 + case.n_digests)
    return [None if row[0] else [int(v) for v in row[1:]] for row in words]


def test_piece_length_is_the_one_the_tests_are_built_around(driver):
    r = subprocess.run([driver, "--piece"], capture_output=True, text=True, env=_env(), timeout=60)
    assert r.returncode == 0 and int(r.stdout) == h263mi.DIGEST_PIECE


@pytest.mark.parametrize("case,data", [(c, d) for c in CASES for d in c.data], ids=["%s-%s" % (c.name, d) for c in CASES for d in c.data])
def test_digest_lane_by_lane(driver, tmp_path, case, data):
    results = []
    for garbage in (1, 2):
        buf = case.buffer(data, garbage)
        got = _run(driver, str(tmp_path), case, buf)
        for seed, digests in zip(ref.SEEDS, got):
            assert digests == ref.zlib_of_spans(buf, case.spans, seed, case.n_digests), (case.name, data, garbage, hex(seed))
        results.append(got)
    assert results[0] == results[1]
    if case.name == "abc-cba" and data == "random":      # (all 0xFF: the two orders are one string)
        assert all(d[0] != d[1] for d in results[0])
    if case.name == "ff-long-row":
        assert case.nbytes == (16 << 20) + 5 and results[0][0] == [1636759246]
        assert zlib.adler32(b"\xff" * ((16 << 20) + 5)) == 1636759246


def test_buffer_made_by_the_checker_equals_an_uploaded_one(driver, tmp_path):
    case = next(c for c in CASES if c.name == "ff-5553")
    assert _run(driver, str(tmp_path), case, None) == _run(driver, str(tmp_path), case, case.buffer("ff", 1))


def test_checker_refuses_what_the_library_refuses(driver, tmp_path):
    """digest_table is the library's own check: a row that ends one byte behind the buffer, and a seed half of 65521"""
    case = ref.Case("behind", [(0, 16, 16, 2, 0)])
    case.nbytes -= 1
    assert _run(driver, str(tmp_path), case, np.zeros(case.nbytes, np.uint8), seeds=(1,)) == [None]
    case = ref.Case("seed", [(0, 16, 16, 2, 0)])
    got = _run(driver, str(tmp_path), case, np.zeros(case.nbytes, np.uint8), seeds=(65521, 65520 << 16 | 65520))
    assert got[0] is None and got[1] == [zlib.adler32(bytes(32), 65520 << 16 | 65520)]
