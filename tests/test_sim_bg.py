"""k_bg_begin, k_bg and the selection behind them (bg_begin, bg_wave: h263-rs_amd/csrc/background_kernel.inl; change_select) run lane
by lane on the CPU under AddressSanitizer + UBSan (tests/sim_bg/sim_bg.cpp: a stand-alone program, run as a child process), against
the numpy reference (bg_ref), exactly.  cur, the mask and the cut list are heap buffers of exactly the bytes a call may touch, the
state, the grids, the summaries and the list of exactly their extents: ASan sees any access outside, and inside them every byte that
must not change keeps its value.  A case is a sequence of calls on one state (bg_cases.CASES): the state a call leaves is the next
call's, and everything is compared after every call.  That each hazard occurs among the cases is asserted on the reference's side.
The two mutants of mutants.h must fail the cases named for them and pass cases that their arithmetic does not reach."""
import os
import struct
import subprocess

import numpy as np
import pytest

import bg_cases as bc

HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL = bc.SENTINEL
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
SUMMARY = np.dtype([("sad", np.uint64), ("changed_cells", np.uint32), ("max_cell_sad", np.uint32)])


def build_driver(out, *defines):
    subprocess.check_call(["g++", "-O1", "-g", "-fno-strict-aliasing", "-std=c++17", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *["-D" + d for d in defines], "-o", out,
                           os.path.join(HERE, "sim_bg", "sim_bg.cpp")])
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    # built into a temporary directory: a read-only checkout passes too
    return build_driver(str(tmp_path_factory.mktemp("sim_bg") / "sim_bg"))


@pytest.fixture(scope="module")
def mutant_drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("sim_bg_mutants")
    return {m: build_driver(str(d / m.lower()), m) for m in bc.MUTANT_CASES}


def run_call(driver, tmp, b, q, state, mask, want_cells=True, want_list=True, want_mask=True, items_per_wave=0):
    """one call -> (state after, mask after or None, grids or None, summaries, list words or None, count or None)"""
    inp, outp = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    want_mask = want_mask and b.mask
    cut = q.cut[:min(q.cut_count, b.n)] if q.cut is not None else None           # exactly the entries a call may read
    flags = ((1 if want_cells else 0) | (2 if want_list else 0) | (4 if q.words else 0) | (8 if cut is not None else 0) |
             (16 if want_mask else 0) | items_per_wave << 8)
    prm = b.prm
    with open(inp, "wb") as f:
        f.write(struct.pack("<16I", b.w, b.h, b.n, b.cl, prm.learn, prm.fg_learn, prm.pix_thr, prm.warmup, prm.cell_thr, prm.min_changed, flags,
                            q.cut_count, len(cut) if cut is not None else 0, 0, 0, 0))
        m = (b.mask_off, b.mask_pitch, b.mask_stride, mask.size) if want_mask else (0, 0, 0, 0)
        f.write(struct.pack("<9Q", b.cur_off, b.cur_pitch, b.cur_stride, q.cur_buf.size, b.set1, *m))
        if q.words:
            f.write(np.asarray(q.words, np.uint32).tobytes())
        if cut is not None:
            f.write(cut.tobytes())
        f.write(state.tobytes())
        f.write(q.cur_buf.tobytes())
        if want_mask:
            f.write(mask.tobytes())
    r = subprocess.run([driver, inp, outp], capture_output=True, text=True, env=ENV, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = np.fromfile(outp, np.uint8)
    at = [0]

    def take(nbytes, dtype):
        out = raw[at[0]:at[0] + nbytes].view(dtype)
        at[0] += nbytes
        return out
    state = take(state.size, np.uint8)
    mask = take(mask.size, np.uint8) if want_mask else None
    cells = take(b.n * b.gw * b.gh * 4, np.uint32).reshape(b.n, b.gh, b.gw) if want_cells else None
    summ = take(b.n * 16, SUMMARY)
    lst = take(b.n * 4, np.uint32) if want_list else None
    count = int(take(4, np.uint32)[0]) if want_list else None
    assert at[0] == raw.size
    return state, mask, cells, summ, lst, count


def compare(b, k, got, mutant=None):
    """None, or what differs from the reference after call k"""
    state, mask, cells, summ, lst, count = got
    want_state, want_mask, want_cells, want_summ, want_sel, _ = bc.expected(b)[k]
    if not (state == want_state).all():
        at = int(np.nonzero(state != want_state)[0][0])
        return "call %d: the state differs at byte %d (picture %d, byte %d of it)" % (k, at, at // b.stride, at % b.stride)
    if mask is not None and not (mask == want_mask).all():
        return "call %d: the mask differs at byte %d" % (k, int(np.nonzero(mask != want_mask)[0][0]))
    if cells is not None and not (cells == want_cells).all():
        p, cy, cx = [int(v[0]) for v in np.nonzero(cells != want_cells)]
        return "call %d: cell (%d, %d, %d): %#x, want %#x" % (k, p, cy, cx, cells[p, cy, cx], want_cells[p, cy, cx])
    if [tuple(int(v) for v in s) for s in summ] != want_summ:
        return "call %d: summaries %r, want %r" % (k, summ.tolist(), want_summ)
    if lst is not None:
        if count != len(want_sel) or lst[:count].tolist() != want_sel:
            return "call %d: list %r (%r), want %r" % (k, lst[:min(count, b.n)].tolist(), count, want_sel)
        if not (lst[count:] == SENTINEL).all():
            return "call %d: entries behind the count were written" % k
    return None


def run_case(driver, tmp, b, **how):
    """the case's calls, each on the state (and the mask) that the one before left -> None, or the first difference"""
    state, mask = b.state0, b.mask0 if b.mask else None
    for k, q in enumerate(b.calls):
        got = run_call(driver, tmp, b, q, state, mask, **how)
        bad = compare(b, k, got)
        if bad:
            return bad
        state = got[0]
        if got[1] is not None:
            mask = got[1]
    return None


def test_every_hazard_occurs_among_the_cases():
    bc.check_hazards()


@pytest.mark.parametrize("name", list(bc.CASES))
def test_cases_lane_by_lane(driver, tmp_path, name):
    assert run_case(driver, str(tmp_path), bc.build(name)) is None


@pytest.mark.parametrize("items_per_wave", [2, 3, 16])
@pytest.mark.parametrize("name", ["size_2049x8_c8", "size_1025x9_c8", "size_176x144_c8", "size_33x65_c8", "segment_c32", "segment_2049",
                                  "words_invalid_and_sets", "init_by_cut", "height_c8+1"])
def test_a_wave_that_takes_several_items(driver, tmp_path, name, items_per_wave):
    """the launcher gives a wave several items only in launches of thousands (many_items_*): here every small shape gets them"""
    b = bc.build(name)
    assert b.gh * -(-b.w // bc.SEG) > 1
    assert run_case(driver, str(tmp_path), b, items_per_wave=items_per_wave) is None


@pytest.mark.parametrize("absent", ["cells", "list", "mask", "all"])
@pytest.mark.parametrize("name", ["size_1025x9_c8", "size_100x60_c32", "words_invalid_and_sets", "warmup_3", "fg_shift_differs"])
def test_with_each_optional_output_absent(driver, tmp_path, name, absent):
    b = bc.build(name)
    assert b.mask
    how = dict(want_cells=absent not in ("cells", "all"), want_list=absent not in ("list", "all"), want_mask=absent not in ("mask", "all"))
    assert run_case(driver, str(tmp_path), b, **how) is None


@pytest.mark.parametrize("mutant", list(bc.MUTANT_CASES))
def test_a_mutant_fails_its_named_cases_and_passes_the_rest(mutant_drivers, tmp_path, mutant):
    for name in bc.MUTANT_CASES[mutant]:
        assert run_case(mutant_drivers[mutant], str(tmp_path), bc.build(name)) is not None, name
    # the rest: what the mutated arithmetic does not reach (bg_cases.affected, the reference with the same mutation)
    rest = [name for name in bc.CASES if not bc.affected(bc.build(name), mutant)]
    assert len(rest) >= 8
    for name in rest:
        assert run_case(mutant_drivers[mutant], str(tmp_path), bc.build(name)) is None, name
