"""The arithmetic of the reconstruction rounds in every form it is compiled in, on the MI355X.

The designed tables of tests/idct_form_cases.py -- blocks on which a fused or re-associated IDCT changes a pixel, placed in the
first and the later general rounds, dense rounds, wide rounds, all-intra waves, truncated and widened sums, beside every
special class -- through the three paths of test_gpu_wave_sweep.py (its helpers are used as they are):
  H263State                      -- k_recon
  Batch(8, pipeline_post=True)   -- k_frame with 8 bands per picture
  Batch(16, pipeline_post=True)  -- k_frame with 4 bands
each with dense coefficient blocks, events and host records.  All three planes are compared byte for byte with the C oracle,
every fixture block additionally with clamp(base + the fixture's soft-float residual), and every status word must be 0.

The CPU twin, test_sim_idct_forms.py, holds the checker's per-round report against the declaration of every case (so each case
takes the form it is meant for) and asserts that nothing of the case space is missing.  P pictures are decoded over a flat key
frame of 128."""
import pytest

import h263mi
import idct_form_cases as fc
import test_gpu_wave_sweep as gpu
import wave_cases as wc
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
_CASES = {}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if h263mi.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the MI355X box")


def check_fixture_blocks(pic, planes, what):
    views = wc.plane_views(pic, planes)
    for k, x, y, e, mby, r, slot in pic["placed"]:
        assert (views[k][y:y + 8, x:x + 8] == fc.expected_block(e, pic["base"])).all(), \
            "%s: table (%s) %s, wave %d round %d (%s) slot %d: fixture block %s is not clamp(%d + the soft-float residual)" % (
                what, pic["table"], pic["tag"], mby, r, pic["decl"][mby]["rounds"][r]["form"], slot, e["id"], pic["base"])


def cases(name):
    """[(picture, the oracle's planes)] of a table, computed once and shared by its paths and transports"""
    if name not in _CASES:
        cov = fc.Coverage()
        out = []
        for pic in fc.table(name):
            cov.add(pic)
            rc, want = orc.decode_picture(pic["w"], pic["h"], pic["mbs"], pic["coeffs"], fc.flat_reference()[2] if pic["base"] else None)
            assert rc == 0
            check_fixture_blocks(pic, want, "the C oracle")
            out.append((pic, want))
        assert cov.missing((name,)) == []
        _CASES[name] = out
    return _CASES[name]


@pytest.fixture
def wave_sweep_paths(monkeypatch):
    """test_gpu_wave_sweep's runners, decoding P pictures over the flat key frame and holding every fixture block to its
    soft-float residual as well"""
    compare = gpu.check

    def check(pic, got, want, path):
        compare(pic, got, want, path)
        check_fixture_blocks(pic, got, path)

    monkeypatch.setattr(gpu, "reference", fc.flat_reference)
    monkeypatch.setattr(gpu, "check", check)
    return gpu


@pytest.mark.parametrize("table,path,transport", [(t, p, tr) for t in fc.TABLES for p in gpu.PATHS for tr in gpu.TRANSPORTS
                                                  if not (p == "state" and tr == "host")])
def test_form_table(table, path, transport, wave_sweep_paths):
    items = cases(table)
    if path == "state":
        wave_sweep_paths.run_state(items, transport)
    else:
        wave_sweep_paths.run_batch(items, 8 if path == "batch8" else 16, transport)
