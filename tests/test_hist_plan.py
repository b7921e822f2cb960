"""The launch plan of k_hist (hist_plan, beside HistArgs in h263-rs_amd/csrc/hist_kernel.inl) on the CPU under AddressSanitizer +
UBSan (tests/hist_plan/hist_plan.cpp): the waves of a picture, the work items a wave takes and the split of a call into launches
of whole pictures at the shapes where the arithmetic can go wrong, and every refusal -- one accepted argument set, then that set
with one field pushed over its limit.  launch_hist (analysis_kernels.hip) is the plan and a loop of launches; the host refuses bad
arguments earlier, so nothing else reaches these checks.

Every expected value is a literal worked out by hand: a work item is a band of 8 rows times a segment of 1024 columns, items =
ceil(H / 8) * ceil(W / 1024) a picture, items_per_wave = clamp(n * items / 2048, 1, 16), waves = ceil(items / items_per_wave),
pictures a launch = floor(2^24 / waves)."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

CASES = []      # (id, the case's line, the expected line)


def case(line, want):
    CASES.append((line.replace(" ", "-") or "accepted", line, want))


# the accepted set itself: 64 pictures of 1920 x 1080 -- 135 bands x 2 segments = 270 items a picture, 17 280 in all, 8 a wave,
# 34 waves a picture, floor(2^24 / 34) = 493 447 pictures a launch: one launch
case("", "ok 8 34 493447 0")
case("n=1", "ok 1 270 62137 0")                        # a small launch: an item a wave
case("n=65", "ok 8 34 493447 0")
case("n=65535", "ok 16 17 986895 0")                   # 16 a wave at the most
case("items_per_wave=3", "ok 3 90 186413 0")           # (the checker's override)
# widths at 135 bands: one segment up to 1024 columns (8 640 items, 4 a wave), two from 1025 on, three from 2049 on (405 items a
# picture, 25 920 in all, 12 a wave, ceil(405 / 12) = 34)
for w in (1, 15, 16, 17, 63, 1023, 1024):
    case("w=%d segs=1" % w, "ok 4 34 493447 0")
case("w=1025", "ok 8 34 493447 0")
case("w=2049 segs=3", "ok 12 34 493447 0")
# heights at two segments: one band up to 8 rows, two at 9, three at 17
for h, bands, pictures in ((1, 1, 8388608), (2, 1, 8388608), (8, 1, 8388608), (9, 2, 4194304), (17, 3, 2796202)):
    case("h=%d bands=%d" % (h, bands), "ok 1 %d %d 0" % (2 * bands, pictures))
# 16384 x 65535: 8192 bands x 16 segments = 131 072 items a picture, 16 a wave, 8 192 waves a picture, 2^24 / 8192 = 2 048
# pictures a launch: 10 000 pictures go out as four launches of 2 048 and one of 1 808
BIG = "w=16384 h=65535 segs=16 bands=8192"
case(BIG + " n=10000", "ok 16 8192 2048 0,2048,4096,6144,8192")
case(BIG + " n=2048", "ok 16 8192 2048 0")
case(BIG + " n=2049", "ok 16 8192 2048 0,2048")
case("w=32768 h=32767 segs=32 bands=4096", "ok 16 8192 2048 0")              # w * h = 2^30 - 2^15
case("w=65535 h=1 segs=64 bands=1", "ok 2 32 524288 0")                       # 64 items a picture, 4 096 in all
case("align=4", "ok 8 34 493447 0")
case("align=1", "ok 8 34 493447 0")
# the refusals, each the accepted set with one field over its limit
for over in ("n=65536", "w=0 segs=0", "h=0 bands=0", "w=65536 segs=64", "h=65536 bands=8192", "w=32768 h=32768 segs=32 bands=4096", "null=src",
             "null=hist", "align=0", "align=2", "align=8", "align=32", "segs=1", "segs=3", "bands=134", "bands=136"):
    case(over, "refused")


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    # built into a temporary directory: a read-only checkout passes too
    tmp = tmp_path_factory.mktemp("hist_plan")
    exe, inp, outp = str(tmp / "hist_plan"), str(tmp / "cases.txt"), str(tmp / "out.txt")
    subprocess.check_call(["g++", "-O1", "-g", "-fno-strict-aliasing", "-std=c++17", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(HERE, "hist_plan", "hist_plan.cpp")])
    with open(inp, "w") as f:
        f.write("".join(line + "\n" for _, line, _ in CASES))
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"), timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(outp) as f:
        got = f.read().splitlines()
    assert len(got) == len(CASES)
    return got


def test_case_ids_are_unique():
    assert len({i for i, _, _ in CASES}) == len(CASES)


@pytest.mark.parametrize("k", range(len(CASES)), ids=[i for i, _, _ in CASES])
def test_plan(results, k):
    assert results[k] == CASES[k][2], CASES[k][1]
