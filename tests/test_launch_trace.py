"""The launch trace of the host path (tests/tsan/trace_driver.cpp): which kernels every batch kind, output shape, stream
activity and strength form launches, on which stream, from and to which memory, with which arguments and behind which events --
recorded by the stub runtime of tests/tsan (no GPU), under AddressSanitizer + UBSan.  tests/golden/launch_trace.txt was recorded
from the host sources as they were before the output shapes moved out of batch.cpp; host code that is restructured without a
change of behaviour reproduces it byte for byte.  To trace another checkout's sources with this driver and stub:
    make -C tests/tsan -B P=<that checkout>/h263-rs_amd trace_driver && tests/tsan/trace_driver <file>"""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
TSAN = os.path.join(HERE, "tsan")
GOLDEN = os.path.join(HERE, "golden", "launch_trace.txt")


def test_launch_trace_is_the_recorded_one(tmp_path):
    subprocess.check_call(["make", "-C", TSAN, "-s", "trace_driver"])
    out = tmp_path / "launch_trace.txt"
    env = dict(os.environ, H263MI_NUMA="0")
    env.pop("LOCAL_WORLD_SIZE", None)
    r = subprocess.run([os.path.join(TSAN, "trace_driver"), str(out)], env=env, capture_output=True, text=True, timeout=300)
    assert "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stderr[-2000:]
    got = out.read_bytes()
    with open(GOLDEN, "rb") as f:
        want = f.read()
    if got != want:
        g, w = got.decode().splitlines(), want.decode().splitlines()
        first = next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
        section = next((l for l in reversed(w[:first + 1]) if l.startswith("== ")), "")
        raise AssertionError("the launch trace differs from tests/golden/launch_trace.txt at line %d (%s):\n  recorded: %s\n  now:      %s"
                             % (first + 1, section, w[first] if first < len(w) else "<end>", g[first] if first < len(g) else "<end>"))
    # the golden is a fixture like the others: no larger than the largest of them
    largest = max(os.path.getsize(os.path.join(HERE, "golden", n)) for n in os.listdir(os.path.join(HERE, "golden")) if n != "launch_trace.txt")
    assert len(want) <= largest
