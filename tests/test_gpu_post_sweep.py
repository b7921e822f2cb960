"""The deblocking post-filter swept over every quartet class, tile kind and output path -- on the MI355X.

The designed tables of tests/post_cases.py (whose coverage conditions tests/test_sim_post_sweep.py asserts without a GPU),
byte for byte against the C oracle (planes) and the oracle -> orc.yuv420_to_rgba (RGBA):
  table (a)  the whole quartet lattice in floor / truncation x horizontal / vertical edge x low / high half, strengths 1..12,
             through h263mi.deblock: the DEVICE branches of the packed arithmetic, which the CPU checker never compiles
  table (b)  every tile kind through every output path: Batch.render_rgba RGBA only (interior instantiations of k_post) and
             RGBA + planes (general form); the pipelined batch (the post waves of k_frame: RGBA only, planes only, both; dense
             records and events); set_rgba_layout scale 0 at a padded pitch; set_yuv_layout I420 and NV12, wide (pitches and
             offsets multiples of 4) and odd (byte stores), immediate and through k_frame_yuv; H263State.render_rgba / render_yuv
The averaged outputs (layout scales 1 and 2, rgba_resize, yuv_resize) run the same pictures against their own references; an
average can swallow +-1, so they carry no coverage accounting."""
import numpy as np
import pytest

import h263mi
import post_cases as pc
import rgba_layout_ref
import rgba_resize_ref
import yuv_layout_ref
import yuv_resize_ref
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
SENTINEL = 0xC3
SIZE_IDS = ["%dx%d" % s for s in pc.SIZES_B]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if h263mi.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the MI355X box")


# ---------------------------------------------------------------------------------------------------------------
# table (a)
# ---------------------------------------------------------------------------------------------------------------
CONFIG_IDS = ["%s-%s" % ("hv"[d], "floor" if f else "trunc") for d, f in pc.A_CONFIGS]
_PLANES_A = {}


def planes_a(config):
    """the planes of one configuration (they do not depend on the strength: built once)"""
    if config not in _PLANES_A:
        _PLANES_A[config] = list(pc.table_a(*pc.A_CONFIGS[config]))
    return _PLANES_A[config]


@pytest.mark.parametrize("config", range(len(pc.A_CONFIGS)), ids=CONFIG_IDS)
@pytest.mark.parametrize("strength", range(1, 13))
def test_table_a_every_lattice_point_in_every_semantics_direction_and_half(strength, config):
    """one configuration (direction x division) at one strength: 32 or 43 planes of 8191 edges, both halves of every packed
    quartet run through the whole lattice (the coverage itself: test_sim_post_sweep.py)"""
    for pic in planes_a(config):
        want = orc.deblock(pic["plane"], pic["w"], strength)
        got = h263mi.deblock(pic["plane"], pic["w"], strength)
        if not (got == want).all():
            pytest.fail(pc.first_difference(pic["name"], "h263mi.deblock, strength %d" % strength, pic["w"], pic["h"], got, want,
                                            pic["plane"], strength))


# ---------------------------------------------------------------------------------------------------------------
# table (b)
# ---------------------------------------------------------------------------------------------------------------
class Case:
    """one size of table (b): records, device copies of them, and everything the oracle says"""

    def __init__(self, pic):
        self.name, self.w, self.h = pic["name"], pic["w"], pic["h"]
        self.cw, self.ch = (self.w + 1) // 2, (self.h + 1) // 2
        self.streams, self.strengths = pic["streams"], np.array(pic["strengths"], np.uint8)
        self.n = len(self.streams)
        self.source, self.filtered, self.rgba = [], [], []
        for (mbs, co), s in zip(self.streams, pic["strengths"]):
            rc, planes = orc.decode_picture(self.w, self.h, mbs, co, None)
            assert rc == 0
            filt = planes if s == 0 else tuple(orc.deblock(p, pw, s) for p, pw in zip(planes, (self.w, self.cw, self.cw)))
            self.source.append(planes)
            self.filtered.append(filt)
            self.rgba.append(orc.yuv420_to_rgba(*filt, self.w))
        self.plane_bytes = self.w * self.h + 2 * self.cw * self.ch
        self._dev = None

    def device_records(self):
        """(d_mbs, d_coeffs, d_base, d_first, d_events): dense records with dense coefficients and with events"""
        if self._dev is None:
            mbs = np.concatenate([m for m, _ in self.streams])
            co = np.concatenate([c for _, c in self.streams]).astype(np.int16)
            base = np.cumsum([0] + [c.shape[0] for _, c in self.streams[:-1]]).astype(np.uint64)
            first, ev = h263mi.events_from_dense(co, np.ones(len(co), bool))          # (every block is intra)
            ev = np.concatenate([ev, np.zeros(4, np.uint32)])
            self._dev = []
            for arr in (mbs, co, base, first, ev):
                d = h263mi.DeviceBuffer(max(arr.nbytes, 16))
                d.upload(arr)
                self._dev.append(d)
        return self._dev

    def batch(self, **kw):
        return h263mi.Batch(self.n, self.w, self.h, 0, None, **kw)

    def decode(self, b, rgba, planes, events=False):
        d = self.device_records()
        if events:
            b.decode_events(h263mi.PICTURE_I, d[0].ptr, d[3].ptr, d[4].ptr, d[2].ptr, 0, 0, rgba, planes, strengths=self.strengths)
        else:
            b.decode(h263mi.PICTURE_I, d[0].ptr, d[1].ptr, d[2].ptr, 0, 0, rgba, planes, strengths=self.strengths)

    # -- comparisons ---------------------------------------------------------------------------------------
    def check_rgba(self, got, path):
        got = got.reshape(self.n, -1)
        for s in range(self.n):
            diff = pc.rgba_difference("%s stream %d strength %d" % (self.name, s, self.strengths[s]), path, self.w, self.h, got[s],
                                      self.rgba[s], self.source[s], int(self.strengths[s]))
            assert diff is None, diff

    def check_planes(self, got, path):
        got = got.reshape(self.n, -1)
        wh, cc = self.w * self.h, self.cw * self.ch
        for s in range(self.n):
            planes = (got[s, :wh], got[s, wh:wh + cc], got[s, wh + cc:])
            diff = pc.first_difference("%s stream %d strength %d" % (self.name, s, self.strengths[s]), path, self.w, self.h, planes,
                                       self.filtered[s], self.source[s], int(self.strengths[s]))
            assert diff is None, diff

    def check_yuv_canvas(self, got, fmt, py, pc_, offs, path, pictures=None, w=None, h=None):
        """a placed YUV canvas: on a mismatch, the planes are cut out of it and named like tight ones"""
        w, h = w or self.w, h or self.h
        pictures = self.filtered if pictures is None else pictures
        exp = yuv_layout_ref.place(np.full(got.size, SENTINEL, np.uint8), pictures, w, h, fmt, py, pc_, *offs)
        if (got == exp).all():
            return
        if pictures is self.filtered:
            cw, ch = self.cw, self.ch
            for s in range(self.n):
                y = np.stack([got[offs[0][s] + r * py: offs[0][s] + r * py + w] for r in range(h)]).ravel()
                if fmt == h263mi.YUV_NV12:
                    c = np.stack([got[offs[1][s] + r * pc_: offs[1][s] + r * pc_ + 2 * cw] for r in range(ch)])
                    cb, cr = c[:, 0::2].ravel(), c[:, 1::2].ravel()
                else:
                    cb = np.stack([got[offs[1][s] + r * pc_: offs[1][s] + r * pc_ + cw] for r in range(ch)]).ravel()
                    cr = np.stack([got[offs[2][s] + r * pc_: offs[2][s] + r * pc_ + cw] for r in range(ch)]).ravel()
                diff = pc.first_difference("%s stream %d strength %d" % (self.name, s, self.strengths[s]), path, w, h, (y, cb, cr),
                                           self.filtered[s], self.source[s], int(self.strengths[s]))
                assert diff is None, diff
        bad = np.flatnonzero(got != exp)
        pytest.fail("%s, %s: %d bytes differ outside the planes' samples or in an averaged output, first at byte %s" % (
            self.name, path, bad.size, bad[:8]))

    def check_rgba_canvas(self, got, pictures, pitch, offs, path):
        exp = rgba_layout_ref.place(np.full(got.size, SENTINEL, np.uint8), pictures, pitch, offs)
        bad = np.flatnonzero(got != exp)
        assert bad.size == 0, "%s, %s: %d bytes differ, first at byte %s" % (self.name, path, bad.size, bad[:8])


_CASES = {}


@pytest.fixture(params=range(len(pc.SIZES_B)), ids=SIZE_IDS)
def case(request):
    if not _CASES:
        for k, pic in enumerate(pc.table_b()):
            _CASES[k] = Case(pic)
    return _CASES[request.param]


def sentinel(nbytes):
    d = h263mi.DeviceBuffer(nbytes)
    d.upload(np.full(nbytes, SENTINEL, np.uint8))
    return d


def test_table_b_immediate_rgba_only_and_rgba_with_planes(case):
    c = case
    b = c.batch()
    b.submit_host(h263mi.PICTURE_I, [m for m, _ in c.streams], [co for _, co in c.streams])
    rgba, planes = sentinel(c.n * c.w * c.h * 4), sentinel(c.n * c.plane_bytes)
    b.render_rgba(0, rgba.ptr, None, strengths=c.strengths)
    b.sync()
    c.check_rgba(rgba.download(), "Batch.render_rgba, RGBA only (interior instantiations)")
    rgba.upload(np.full(rgba.nbytes, SENTINEL, np.uint8))
    b.render_rgba(0, rgba.ptr, planes.ptr, strengths=c.strengths)
    b.sync()
    c.check_planes(planes.download(), "Batch.render_rgba, RGBA + planes (general form), the planes")
    c.check_rgba(rgba.download(), "Batch.render_rgba, RGBA + planes (general form), the RGBA")
    planes.upload(np.full(planes.nbytes, SENTINEL, np.uint8))
    b.render_rgba(0, None, planes.ptr, strengths=c.strengths)
    b.sync()
    c.check_planes(planes.download(), "Batch.render_rgba, planes only")
    b.close()


@pytest.mark.parametrize("events", [False, True], ids=["dense", "events"])
def test_table_b_pipelined_post_waves_of_k_frame(case, events):
    """three calls on a pipelined batch: the post waves of the second call's k_frame render the first call's request, those of
    the third the second's, and k_post at sync() the third's -- RGBA only, planes only, both"""
    c = case
    b = c.batch(pipeline_post=True)
    r1, p2, r3, p3 = sentinel(c.n * c.w * c.h * 4), sentinel(c.n * c.plane_bytes), sentinel(c.n * c.w * c.h * 4), sentinel(c.n * c.plane_bytes)
    c.decode(b, r1.ptr, None, events)
    c.decode(b, None, p2.ptr, events)
    c.decode(b, r3.ptr, p3.ptr, events)
    b.sync()
    c.check_rgba(r1.download(), "pipelined batch, k_frame post waves, RGBA only")
    c.check_planes(p2.download(), "pipelined batch, k_frame post waves, planes only")
    c.check_rgba(r3.download(), "pipelined batch, k_post at sync, the RGBA")
    c.check_planes(p3.download(), "pipelined batch, k_post at sync, the planes")
    b.close()


@pytest.mark.parametrize("pipelined", [False, True], ids=["immediate", "k_frame_layout"])
def test_table_b_rgba_layout_scale_0_at_a_padded_pitch(case, pipelined):
    c = case
    pitch = 4 * c.w + 64
    offs = rgba_layout_ref.default_offsets(c.n, c.w, c.h, 0, pitch)
    nbytes = h263mi.rgba_layout_extent(c.n, c.w, c.h, 0, pitch)[2]
    b = c.batch(pipeline_post=pipelined)
    b.set_rgba_layout(0, pitch)
    canvas = sentinel(nbytes)
    c.decode(b, canvas.ptr, None)
    if pipelined:
        other = sentinel(nbytes)
        c.decode(b, other.ptr, None)
    b.sync()
    got = canvas.download()
    # the rows of each picture, cut out of the canvas, are the tight RGBA
    rows = np.stack([got[offs[s] + r * pitch: offs[s] + r * pitch + 4 * c.w] for s in range(c.n) for r in range(c.h)])
    c.check_rgba(rows.ravel(), "set_rgba_layout scale 0, pitch %d, %s" % (pitch, "k_frame" if pipelined else "k_post"))
    c.check_rgba_canvas(got, [r.reshape(c.h, c.w, 4) for r in c.rgba], pitch, offs, "set_rgba_layout scale 0: outside the pictures")
    b.close()


@pytest.mark.parametrize("pipelined", [False, True], ids=["immediate", "k_frame_yuv"])
@pytest.mark.parametrize("wide", [True, False], ids=["wide", "odd-pitch"])
@pytest.mark.parametrize("fmt", [h263mi.YUV_I420, h263mi.YUV_NV12], ids=["I420", "NV12"])
def test_table_b_yuv_layout(case, fmt, wide, pipelined):
    c = case
    ry, rc_ = yuv_layout_ref.row_bytes(c.w, fmt)
    py, pc_ = ((ry + 3) // 4 * 4 + 64, (rc_ + 3) // 4 * 4 + 32) if wide else (ry + 61, rc_ + 33)     # (odd: byte stores)
    assert (py % 4 == 0 and pc_ % 4 == 0) == wide
    offs = yuv_layout_ref.default_offsets(c.n, c.w, c.h, fmt, py, pc_)
    nbytes = h263mi.yuv_layout_extent(c.n, c.w, c.h, fmt, py, pc_)
    b = c.batch(pipeline_post=pipelined)
    b.set_yuv_layout(fmt, py, pc_)
    canvas = sentinel(nbytes)
    c.decode(b, None, canvas.ptr)
    if pipelined:
        other = sentinel(nbytes)
        c.decode(b, None, other.ptr)
    b.sync()
    c.check_yuv_canvas(canvas.download(), fmt, py, pc_, offs, "set_yuv_layout %s pitches %d / %d, %s" % (
        "NV12" if fmt == h263mi.YUV_NV12 else "I420", py, pc_, "k_frame_yuv" if pipelined else "k_post_yuv"))
    b.close()


def test_table_b_one_state(case):
    c = case
    st = h263mi.H263State()
    for s, (mbs, co) in enumerate(c.streams):
        strength = int(c.strengths[s])
        name = "%s stream %d strength %d" % (c.name, s, strength)
        st.submit_picture(c.w, c.h, mbs, co, h263mi.PICTURE_I)
        diff = pc.rgba_difference(name, "H263State.render_rgba", c.w, c.h, st.render_rgba(strength), c.rgba[s], c.source[s], strength)
        assert diff is None, diff
        got = st.render_yuv(strength, h263mi.YUV_I420)
        wh, cc = c.w * c.h, c.cw * c.ch
        diff = pc.first_difference(name, "H263State.render_yuv I420", c.w, c.h, (got[:wh], got[wh:wh + cc], got[wh + cc:]),
                                   c.filtered[s], c.source[s], strength)
        assert diff is None, diff
        if s % 5 == 0:
            got = st.render_yuv(strength, h263mi.YUV_NV12)
            exp = np.concatenate([p.ravel() for p in yuv_layout_ref.planes_of(c.filtered[s], c.w, c.h, h263mi.YUV_NV12)])
            assert (got == exp).all(), name + ", H263State.render_yuv NV12"
    st.close()


def test_table_b_averaged_outputs_against_their_references(case):
    """layout scales 1 and 2, rgba_resize and yuv_resize of the same pictures (immediate): no coverage accounting here"""
    c = case
    b = c.batch()
    b.submit_host(h263mi.PICTURE_I, [m for m, _ in c.streams], [co for _, co in c.streams])
    for scale in (1, 2):
        ow, oh, nbytes = h263mi.rgba_layout_extent(c.n, c.w, c.h, scale)
        b.set_rgba_layout(scale)
        canvas = sentinel(nbytes)
        b.render_rgba(0, canvas.ptr, None, strengths=c.strengths)
        b.sync()
        c.check_rgba_canvas(canvas.download(), [rgba_layout_ref.box_average(r, c.w, c.h, scale) for r in c.rgba], 4 * ow,
                            rgba_layout_ref.default_offsets(c.n, c.w, c.h, scale), "set_rgba_layout scale %d" % scale)
    b.set_rgba_layout(default=True)
    ow, oh = c.w * 5 // 7, c.h * 3 // 5
    b.set_rgba_resize(ow, oh)
    canvas = sentinel(h263mi.rgba_resize_extent(c.n, ow, oh))
    b.render_rgba(0, canvas.ptr, None, strengths=c.strengths)
    b.sync()
    c.check_rgba_canvas(canvas.download(), [rgba_resize_ref.resize(r, c.w, c.h, ow, oh) for r in c.rgba], 4 * ow,
                        [s * oh * 4 * ow for s in range(c.n)], "set_rgba_resize %dx%d" % (ow, oh))
    b.set_rgba_resize(default=True)
    for fmt in (h263mi.YUV_I420, h263mi.YUV_NV12):
        b.set_yuv_resize(ow, oh, fmt)
        ry, rc_ = yuv_layout_ref.row_bytes(ow, fmt)
        canvas = sentinel(h263mi.yuv_resize_extent(c.n, ow, oh, fmt))
        b.render_rgba(0, None, canvas.ptr, strengths=c.strengths)
        b.sync()
        want = [yuv_resize_ref.resize_planes(p, c.w, c.h, ow, oh) for p in c.filtered]
        c.check_yuv_canvas(canvas.download(), fmt, ry, rc_, yuv_layout_ref.default_offsets(c.n, ow, oh, fmt), "set_yuv_resize %dx%d" % (ow, oh),
                           pictures=want, w=ow, h=oh)
    b.close()
