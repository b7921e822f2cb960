"""The host path of a filtered YUV resize (h263mi_batch_set_yuv_resize_filtered), traced against the stub runtime of tests/tsan
(no GPU) under AddressSanitizer + UBSan: tests/plane_filter_trace/trace_plane_filter.cpp is a stand-alone program that records
which kernels the calls launch, on which stream, from and to which memory and with which tables; the stub gains the one launcher it
lacks in stub_with_plane_filter.cpp.  The sections are compared with one another and with the definition: the tap tables are
recomputed here from filter_ref.taps in the layout of filter_taps.h: filter_table."""
import os
import re
import subprocess

import numpy as np
import pytest

import filter_ref as flt

HERE = os.path.dirname(os.path.abspath(__file__))
P = os.path.join(HERE, "..", "h263-rs_amd")
W, H, OW, OH = 48, 32, 20, 12
HOST = ["csrc/worker_pool.cpp", "csrc/batch.cpp", "csrc/output_shape.cpp", "csrc/batch_staging.cpp", "csrc/mixed_set.cpp", "csrc/state.cpp",
        "csrc/device_util.cpp", "host/bitstream.cpp"]


@pytest.fixture(scope="module")
def sections(tmp_path_factory):
    """{section title: [lines]} of one run of the driver, built into a temporary directory"""
    tmp = tmp_path_factory.mktemp("plane_filter_trace")
    exe, out = str(tmp / "trace_plane_filter"), str(tmp / "trace.txt")
    src = [os.path.join(HERE, "plane_filter_trace", n) for n in ("trace_plane_filter.cpp", "stub_with_plane_filter.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-pthread", "-fno-strict-aliasing", "-Wall", "-Wno-unused-function",
                           "-Wno-unknown-pragmas", "-I" + os.path.join(HERE, "tsan", "hip_stub"), "-o", exe] + src +
                          [os.path.join(P, s) for s in HOST])
    env = dict(os.environ, H263MI_NUMA="0")
    env.pop("LOCAL_WORLD_SIZE", None)
    r = subprocess.run([exe, out], env=env, capture_output=True, text=True, timeout=300)
    assert "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stderr[-2000:]
    got, title = {}, None
    with open(out) as f:
        for line in f.read().splitlines():
            if line.startswith("== "):
                title = line[3:]
                got[title] = []
            else:
                got[title].append(line)
    return got


def _launches(lines):
    """the launches of a section without what differs from one call to the next by construction: event numbers, and where in its
    ring an uploaded array lies"""
    out = []
    for line in lines:
        if line.startswith(("record ", "wait ")):
            continue
        out.append(re.sub(r"=@lib:(\d+)\+\d+\[", r"=@lib:\1[", line))
    return out


def _fields(line):
    return dict(kv.split("=", 1) for kv in line.split(" ")[2:] if "=" in kv)


def _table_words(kind, sw, sh, dw, dh):
    """filter_taps.h: filter_table -- dw (first, count) pairs, dh pairs, dw * ksx weights, dh * ksy weights"""
    spans, coeffs = [], []
    for n_in, n_out in ((sw, dw), (sh, dh)):
        if n_in == n_out:
            first, count, co = np.arange(n_out), np.ones(n_out, np.int64), np.full((n_out, 1), 1 << 22, np.int64)
        else:
            _, first, count, co = flt.taps(kind, n_in, n_out)
        spans.append(np.stack([first, count], axis=1).ravel().astype(np.uint32))
        coeffs.append(co.ravel().astype(np.int32).view(np.uint32))
    return np.concatenate(spans + coeffs)


def _fnv(words):
    h = 0xcbf29ce484222325
    for b in words.astype("<u4").tobytes():
        h = ((h ^ b) * 0x100000001b3) & 0xffffffffffffffff
    return h


@pytest.mark.parametrize("name,kind", [("bicubic", flt.BICUBIC), ("bilinear", flt.BILINEAR)])
def test_a_rendering_queues_the_planes_and_then_k_plane_filter_on_the_same_stream(sections, name, kind):
    lines = _launches(sections["shape | " + name])
    kinds = [l.split(" ")[0] for l in lines]
    assert kinds == ["recon", "post", "plane_filter", "post", "plane_filter"], kinds
    cw, ch, cow, coh = (W + 1) // 2, (H + 1) // 2, (OW + 1) // 2, (OH + 1) // 2
    words = np.concatenate([_table_words(kind, W, H, OW, OH), _table_words(kind, cw, ch, cow, coh)])
    for post, pf in ((lines[1], lines[2]), (lines[3], lines[4])):
        assert post.split(" ")[1] == pf.split(" ")[1] == "main"
        fp, ff = _fields(post), _fields(pf)
        # the full-size planes go into the scratch by the default kernels; k_plane_filter reads them from there
        assert fp["planes"] == ff["src"] == "lib:%d+0" % (3 * (W * H + 2 * cw * ch))
        # the four tables, made as the definition says, in one block that holds nothing else
        assert ff["tables"] == "lib:%d+0#%d:%016x" % (4 * words.size, words.size, _fnv(words)) and ff["axes_in_order"] == "1"
        assert (ff["ksx_y"], ff["ksy_y"], ff["ksx_c"], ff["ksy_c"]) == tuple(
            str(flt.taps(kind, a, b)[0]) for a, b in ((W, OW), (H, OH), (cw, cow), (ch, coh)))
        assert (ff["ow"], ff["oh"], ff["cow"], ff["coh"], ff["pitch_y"], ff["pitch_c"]) == ("20", "12", "10", "6", "20", "10")
        assert "nv12" not in ff and "wide" not in ff      # (tight I420 of 20 x 12 at out + 20480: byte stores)
    # the first rendering writes RGBA too, the second the planes alone
    assert "rgba" in _fields(lines[1]) and "rgba" not in _fields(lines[3])


def test_area_and_null_queue_exactly_what_the_unfiltered_setter_queues(sections):
    want = sections["shape | unfiltered"]
    assert [l.split(" ")[0] for l in _launches(want)] == ["recon", "post", "plane_resize", "post", "plane_resize"]
    assert sections["shape | area"] == want and sections["shape | null"] == want
    assert sections["shape | bicubic, then unfiltered"] == want
    assert sections["shape | layout, then bicubic"] == sections["shape | bicubic"]


def test_full_size_under_a_filter_queues_the_layout_path(sections):
    want = sections["shape | layout"]
    assert [l.split(" ")[0] for l in want] == ["recon", "post", "post_yuv", "post_yuv"]
    assert sections["shape | full size bicubic"] == want


def test_the_tables_are_made_once(sections):
    """(the driver itself counts the allocations: two at the setter, none at a later rendering)"""
    lines = [l for l in sections["filtered | tables made once"] if l.startswith("plane_filter ")]
    assert len(lines) == 5 and len({_fields(l)["tables"] for l in lines}) == 1 and len({_fields(l)["src"] for l in lines}) == 1


def test_a_refused_filter_leaves_the_launches_of_the_shape_in_force_unchanged(sections):
    before, after = _launches(sections["refusals | before"]), _launches(sections["refusals | after"])
    assert [l.split(" ")[0] for l in before] == ["post", "plane_filter"] and before == after
    f = _fields(before[1])
    assert (f["nv12"], f["wide"], f["pitch_y"], f["pitch_c"], f["ksx_y"]) == ("1", "1", "32", "32", str(flt.taps(flt.BILINEAR, W, OW)[0]))


def test_a_pending_rendering_keeps_the_filter_the_scratch_and_the_tables_of_its_request(sections):
    lines = _launches(sections["pipeline | shape switched while a filtered rendering is pending"])
    assert [l.split(" ")[0] for l in lines] == ["recon", "frame", "plane_filter", "frame", "plane_resize", "post", "plane_filter"]
    assert all(l.split(" ")[1] == "main" for l in lines)
    tables = _fields(_launches(sections["shape | bicubic"])[2])["tables"]
    assert _fields(lines[2])["tables"] == _fields(lines[6])["tables"] == tables
    assert (_fields(lines[4])["ow"], _fields(lines[4])["oh"]) == ("10", "6")
