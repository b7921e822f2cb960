"""The launch plans of the banded kernels and of k_change (resize_plan ... roi_plan, change_plan: beside their Args in
h263-rs_amd/csrc/*.inl) on the CPU under AddressSanitizer + UBSan (tests/launch_plan/launch_plan.cpp): bands, chunk, segs_y and
the grid at the shapes where the arithmetic can go wrong, and every refusal -- one accepted argument set, then that set with one
field pushed over its limit.  The launchers of output_kernels.hip and analysis_kernels.hip are the plan and one launch; the host refuses bad arguments earlier, so
nothing else reaches these checks.

Every expected value is a literal worked out by hand from bands = ceil(rows / 4) (RESIZE_ROWS, FILTER_ROWS, PLANE_ROWS and
PFILTER_ROWS are all 4), chunk = ceil(bands / 8), grid x = 8 * chunk, y = pictures or regions, z = ceil(width / 64) -- for the
plane kernels segs_y = ceil(W' / 256) luma segments and ceil(cW' / 256) chroma segments behind them."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

# output rows -> bands, chunk, grid x
HEIGHTS = {1: (1, 1, 8), 4: (1, 1, 8), 5: (2, 1, 8), 32: (8, 1, 8), 33: (9, 2, 16)}
# output columns -> grid z of the kernels that take 64 columns a wave
WIDTHS = {1: 1, 64: 1, 65: 2}
# luma and chroma columns -> segs_y, grid z of the plane kernels (PLANE_OUT = 256 columns a wave); 511 and 513 are odd widths
# whose chroma width rounds up, to the last column of a segment and into the next one
PLANE_WIDTHS = {(1, 1): (1, 2), (64, 32): (1, 2), (65, 33): (1, 2), (256, 128): (1, 2), (257, 129): (2, 3), (511, 256): (2, 3),
                (513, 257): (3, 5)}

CASES = []      # (id, the case's line, the expected line)


def case(line, want):
    CASES.append((line.replace(" ", "-"), line, want))


# the accepted sets themselves: 100 x 50 outputs (13 bands, 2 to an XCD, 2 segments), 3 pictures, 5 regions
case("resize", "ok 13 2 0 16 3 2")
case("tensor", "ok 13 2 0 16 3 2")
case("roi", "ok 13 2 0 16 5 2")
# (the launch covers the 100 x 50 output, not the 90 x 45 rectangle, which would be 12 bands)
for plan in ("framed", "framed_tensor", "filter", "filter_tensor"):
    case(plan, "ok 13 2 0 16 3 2")
    case(plan + " ch=33 dy=0 dh=1", "ok 9 2 0 16 3 2")
    case(plan + " cw=65 dx=0 dw=64", "ok 13 2 0 16 3 2")
case("plane_resize", "ok 13 2 1 16 3 2")
case("plane_filter", "ok 13 2 1 16 3 2")

for rows, (bands, chunk, x) in HEIGHTS.items():
    for plan, y in (("resize", 3), ("tensor", 3), ("roi", 5)):
        case("%s oh=%d" % (plan, rows), "ok %d %d 0 %d %d 2" % (bands, chunk, x, y))
    for plan in ("framed", "framed_tensor", "filter", "filter_tensor"):
        case("%s ch=%d dy=0 dh=%d" % (plan, rows, rows), "ok %d %d 0 %d 3 2" % (bands, chunk, x))
    case("plane_resize oh=%d coh=%d" % (rows, (rows + 1) // 2), "ok %d %d 1 %d 3 2" % (bands, chunk, x))
    case("plane_filter oh=%d coh=%d" % (rows, (rows + 1) // 2), "ok %d %d 1 %d 3 2" % (bands, chunk, x))

for cols, z in WIDTHS.items():
    for plan, y in (("resize", 3), ("tensor", 3), ("roi", 5)):
        case("%s ow=%d" % (plan, cols), "ok 13 2 0 16 %d %d" % (y, z))
    for plan in ("framed", "framed_tensor", "filter", "filter_tensor"):
        case("%s cw=%d dx=0 dw=%d" % (plan, cols, cols), "ok 13 2 0 16 3 %d" % z)

for (ow, cow), (segs_y, z) in PLANE_WIDTHS.items():
    case("plane_resize ow=%d cow=%d" % (ow, cow), "ok 13 2 %d 16 3 %d" % (segs_y, z))
    case("plane_filter ow=%d cow=%d" % (ow, cow), "ok 13 2 %d 16 3 %d" % (segs_y, z))

# the refusals, each the accepted set with one field over its limit -- and the last value inside it
case("resize n=65536", "ok 13 2 0 16 65536 2")          # k_rgba_resize's launcher never counted its pictures: the host does
for plan in ("tensor", "framed", "framed_tensor", "filter", "filter_tensor", "plane_resize", "plane_filter"):
    case(plan + " n=65535", "ok 13 2 %d 16 65535 2" % (1 if plan.startswith("plane") else 0))
    case(plan + " n=65536", "refused")
case("roi n_rois=65535", "ok 13 2 0 16 65535 2")
case("roi n_rois=65536", "refused")
for plan in ("tensor", "framed_tensor", "filter_tensor", "roi"):
    case(plan + " dtype=0", "ok 13 2 0 16 %d 2" % (5 if plan == "roi" else 3))
    case(plan + " dtype=3", "refused")
for plan in ("framed", "framed_tensor", "filter", "filter_tensor"):
    # the rectangle one pixel outside the output, in x and in y; keep is 0 or 1; nothing is empty
    for over in ("dx=11", "dy=6", "dw=91", "dh=46", "dx=101 dw=1", "dy=51 dh=1", "keep=2", "dw=0", "dh=0", "cw=0", "ch=0"):
        case("%s %s" % (plan, over), "refused")
    case(plan + " keep=0", "ok 13 2 0 16 3 2")
for plan in ("filter", "filter_tensor"):
    for over in ("null=src", "null=dst", "null=x.span", "null=x.coeff", "null=y.span", "null=y.coeff", "x.ksize=0", "y.ksize=0",
                 "w=0", "h=0"):
        case("%s %s" % (plan, over), "refused")
for over in ("null=src", "null=dst", "w=0 cw=0", "h=0 ch=0", "ow=0 cow=0", "oh=0 coh=0", "cw=160", "cw=162", "ch=120", "ch=122",
             "cow=49", "cow=51", "coh=24", "coh=26"):
    case("plane_filter " + over, "refused")
for axis in ("xy", "yy", "xc", "yc"):
    for over in ("%s.ksize=0", "null=%s.span", "null=%s.coeff"):
        case("plane_filter " + over % axis, "refused")
for over in ("ow=0", "oh=0", "ow=65536", "oh=65536", "w=0", "h=0", "w=65536", "h=65536", "w=32768 h=32768", "n=0", "null=src",
             "null=rois", "null=dst"):
    case("roi " + over, "refused")
case("roi ow=65535", "ok 13 2 0 16 5 1024")
case("roi oh=65535", "ok 16384 2048 0 16384 5 2")
case("roi w=32768 h=32767", "ok 13 2 0 16 5 2")         # w * h = 2^30 - 2^15

# k_change: 1920 x 1080 in cells of 16 is 120 x 68 cells and 2 segments of 1024 columns, 136 items a picture; 64 pictures are
# 8 704 items, 4 a wave (items / 2048), 34 waves a picture, floor(2^24 / 34) = 493 447 pictures a launch: one launch
case("change", "ok 4 34 493447 0")
case("change n=1", "ok 1 136 123361 0")                 # a small launch: an item a wave
case("change items_per_wave=3", "ok 3 46 364722 0")     # (the checker's override)
# 16384 x 32768 in cells of 8: 4096 cell rows x 16 segments = 65 536 items a picture, 16 a wave at most, 4 096 waves a picture,
# 2^24 / 4096 = 4 096 pictures a launch: 10 000 pictures go out as 4 096 + 4 096 + 1 808
case("change w=16384 h=32768 cell_log2=3 gw=2048 gh=4096 segs=16 n=10000", "ok 16 4096 4096 0,4096,8192")
case("change w=16384 h=32768 cell_log2=3 gw=2048 gh=4096 segs=16 n=4096", "ok 16 4096 4096 0")
case("change w=16384 h=32768 cell_log2=3 gw=2048 gh=4096 segs=16 n=4097", "ok 16 4096 4096 0,4096")
case("change n=65535", "ok 16 9 1864135 0")
case("change w=32768 h=32767 cell_log2=6 gw=512 gh=512 segs=32", "ok 16 1024 16384 0")
case("change cell_log2=3 gw=240 gh=135", "ok 8 34 493447 0")
case("change cell_log2=6 gw=30 gh=17", "ok 1 34 493447 0")
for over in ("n=65536", "cell_log2=2 gw=480 gh=270", "cell_log2=7 gw=15 gh=9", "w=0", "h=0", "w=65536 gw=4096 segs=64",
             "h=65536 gh=4096", "w=32768 h=32768 cell_log2=6 gw=512 gh=512 segs=32", "null=cur", "null=prev", "null=summary",
             "gw=119", "gw=121", "gh=67", "gh=69", "segs=1", "segs=3"):
    case("change " + over, "refused")


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    # built into a temporary directory: a read-only checkout passes too
    tmp = tmp_path_factory.mktemp("launch_plan")
    exe, inp, outp = str(tmp / "launch_plan"), str(tmp / "cases.txt"), str(tmp / "out.txt")
    subprocess.check_call(["g++", "-O1", "-g", "-fno-strict-aliasing", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                           "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(HERE, "launch_plan", "launch_plan.cpp")])
    with open(inp, "w") as f:
        f.write("".join(line + "\n" for _, line, _ in CASES))
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"),
                       timeout=300)
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
