"""GPU tests of the normalised planar float tensor output (h263mi_tensor_out, k_tensor_resize).  Every comparison is of bit
patterns, against the oracle's planes -> full-size RGBA (test_gpu_rgba_layout.full_rgba) -> rgba_resize_ref.resize ->
tensor_out_ref.  Small pictures only: the kernel's own hazards (more than 64 output columns, an odd W' tail, a source wider
than one 256-column chunk, H' not a multiple of 4, odd element alignment) all occur at CIF and below."""
import numpy as np
import pytest
import torch  # before the library is loaded: torch brings its own HIP runtime, which the C-ABI library must share (as in bench.py)

import h263mi
import recgen
import rgba_resize_ref
import tensor_out_ref as ref
from oracle import oracle as orc
from test_gpu_rgba_layout import _small_streams, _upload_records, full_rgba

pytestmark = pytest.mark.gpu
SENTINEL = 0xC3
DTYPES = [ref.F32, ref.F16, ref.BF16]
IDS = ["f32", "f16", "bf16"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if h263mi.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the MI355X box")


def _sentinel(dtype):
    return np.array([SENTINEL] * 4, np.uint8).view(ref.BITS_DTYPE[dtype])[0]


def _canvas(nbytes):
    c = h263mi.DeviceBuffer(nbytes)
    c.upload(np.full(nbytes, SENTINEL, np.uint8))
    return c


def _want(n_elem, dtype, small_pics, tensor, base=0, stride_n=0, skip=()):
    """the canvas of n_elem elements that the tensor `tensor` of these W' x H' RGBA pictures comes to (None: not written)"""
    want = np.full(n_elem, _sentinel(dtype), ref.BITS_DTYPE[dtype])
    scale, bias = list(tensor.scale), list(tensor.bias)
    for s, pic in enumerate(small_pics):
        if pic is None or s in skip:
            continue
        ref.place(want, ref.planes(pic, dtype, scale, bias, bool(tensor.bgr)), base + s * stride_n, tensor.stride_c, tensor.stride_h)
    return want


def _same(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d elements differ, first at %s: %#x, want %#x" % (what, bad.size, bad[:8], got[bad[0]], want[bad[0]])


def _upload(pics):
    mbs = np.concatenate([m for m, _ in pics])
    co = np.concatenate([c for _, c in pics]).astype(np.int16)
    base = np.cumsum([0] + [c.shape[0] for _, c in pics[:-1]]).astype(np.uint64)
    bufs = []
    for arr in (mbs, co, base):
        d = h263mi.DeviceBuffer(max(arr.nbytes, 16))
        d.upload(arr)
        bufs.append(d)
    return bufs


# ---------------------------------------------------------------------------------------------
# 1. one state: every one of the 256 inputs through every conversion
# ---------------------------------------------------------------------------------------------
STATE_SIZES = [(1, 1), (65, 5), (224, 224), (352, 288), (357, 290)]


@pytest.fixture(scope="module")
def cif_state():
    w, h = 352, 288
    mbs, co = recgen.intra_picture(w, h, seed=2)
    rc, planes = orc.decode_picture(w, h, mbs, co, None)
    assert rc == 0
    small = {}
    for strength in (0, 7):
        full = full_rgba(planes, w, strength)
        for ow, oh in STATE_SIZES:
            small[(strength, ow, oh)] = rgba_resize_ref.resize(full, w, h, ow, oh)
    st = h263mi.H263State(h263mi.SORENSON_SPARK_BITSTREAM, device_id=0)
    st.submit_picture(w, h, mbs, co, h263mi.PICTURE_I, temporal_reference=0, pquant=8)
    yield st, small
    st.close()


def test_reference_picture_holds_all_256_values(cif_state):
    """without this the conversion test below is vacuous: every u of 0..255 in R, G and B at both sizes"""
    _, small = cif_state
    for ow, oh in ((352, 288), (224, 224)):
        for c in range(3):
            assert np.unique(small[(0, ow, oh)][:, :, c]).size == 256, (ow, oh, c)


@pytest.mark.parametrize("params", ["imagenet", "edges"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_state_render_tensor_all_inputs(cif_state, dtype, params):
    st, small = cif_state
    for ow, oh in ((352, 288), (224, 224)):
        for c in range(3):
            assert np.unique(small[(0, ow, oh)][:, :, c]).size == 256, (ow, oh, c)
    scale, bias = ref.IMAGENET if params == "imagenet" else ref.EDGES
    for strength in (0, 7):
        for k, (ow, oh) in enumerate(STATE_SIZES):
            t = h263mi.make_tensor_out(ow, oh, dtype, scale, bias, bgr=bool(k & 1))
            want = ref.planes(small[(strength, ow, oh)], dtype, scale, bias, bool(k & 1))
            got = st.render_tensor(strength, t).view(ref.BITS_DTYPE[dtype])
            _same(got.ravel(), want.ravel(), "state -> %dx%d strength %d" % (ow, oh, strength))
            # padded strides, the base one element into the host buffer: nothing outside the rectangles is touched
            t = h263mi.make_tensor_out(ow, oh, dtype, scale, bias, bgr=bool(k & 1), stride_h=ow + 3, stride_c=oh * (ow + 3) + 5)
            n_elem = 1 + h263mi.tensor_extent(1, t) // ref.ELT[dtype] + 7
            out = np.full(n_elem, _sentinel(dtype), ref.BITS_DTYPE[dtype])
            st.render_tensor_into(strength, t, out[1:])
            _same(out, _want(n_elem, dtype, [small[(strength, ow, oh)]], t, base=1), "state padded -> %dx%d" % (ow, oh))
    # the header's strength: this picture's header does not ask for the filter
    t = h263mi.make_tensor_out(65, 5, dtype, scale, bias)
    got = st.render_tensor(h263mi.STRENGTH_FROM_HEADER, t).view(ref.BITS_DTYPE[dtype])
    _same(got.ravel(), ref.planes(small[(0, 65, 5)], dtype, scale, bias).ravel(), "strength from header")
    with pytest.raises(h263mi.H263Error) as e:
        st.render_tensor(13, t)
    assert e.value.code == h263mi.ERR_INVALID_ARGUMENT


# ---------------------------------------------------------------------------------------------
# 2. a batch, immediate rendering: BGR, padded strides, an odd element base, one stream inactive
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def qcif_streams():
    """4 streams of 176 x 144, I then P: device records and the oracle's planes of both pictures"""
    n, w, h = 4, 176, 144
    pics0 = _small_streams(n, w, h, 4100)
    recs0, planes0 = _upload_records(pics0, w, h)
    pics1 = [recgen.inter_picture(w, h, seed=4150 + s, mv_range=30, p_4v=0.2, p_coded=0.5, quant=8) for s in range(n)]
    recs1 = _upload(pics1)
    planes1 = []
    for (m, c), p0 in zip(pics1, planes0):
        rc, p = orc.decode_picture(w, h, m, c, p0)
        assert rc == 0
        planes1.append(p)
    return n, w, h, (recs0, recs1), (planes0, planes1)


def _small(planes, w, h, strengths, ow, oh):
    return [rgba_resize_ref.resize(full_rgba(p, w, s), w, h, ow, oh) for p, s in zip(planes, strengths)]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_batch_immediate_bgr_padded_odd_base_one_stream_inactive(qcif_streams, dtype):
    n, w, h, recs, planes = qcif_streams
    ow, oh = 65, 5
    stride_h = ow + 3
    stride_c = oh * stride_h + 5
    stride_n = 3 * stride_c + 7
    elt = ref.ELT[dtype]
    strengths = np.array([0, 5, 7, 12], np.uint8)
    t = h263mi.make_tensor_out(ow, oh, dtype, *ref.IMAGENET, bgr=True, stride_n=stride_n, stride_c=stride_c, stride_h=stride_h)
    nbytes = h263mi.tensor_extent(n, t)
    assert nbytes == elt * (3 * stride_n + 2 * stride_c + (oh - 1) * stride_h + ow)
    b = h263mi.Batch(n, w, h, 0, None)
    b.set_tensor_output(t)
    n_elem = 1 + nbytes // elt + 5
    for f, ptype in enumerate((h263mi.PICTURE_I, h263mi.PICTURE_P)):
        if f == 1:
            b.set_active([1, 1, 0, 1])
        c = _canvas(n_elem * elt)
        b.decode(ptype, recs[f][0].ptr, recs[f][1].ptr, recs[f][2].ptr, 0, 0, c.at(elt), None, strengths=strengths)
        b.sync()
        got = c.download().view(ref.BITS_DTYPE[dtype])
        want = _want(n_elem, dtype, _small(planes[f], w, h, strengths, ow, oh), t, base=1, stride_n=stride_n, skip=(2,) if f else ())
        _same(got, want, "call %d" % f)
    # every stream's last picture: stream 2 still has its I picture
    b.set_active(None)
    c = _canvas(n_elem * elt)
    b.render_rgba(0, c.at(elt), None, strengths=strengths)
    b.sync()
    last = [planes[1][0], planes[1][1], planes[0][2], planes[1][3]]
    _same(c.download().view(ref.BITS_DTYPE[dtype]), _want(n_elem, dtype, _small(last, w, h, strengths, ow, oh), t, base=1, stride_n=stride_n),
          "render")
    b.close()


# ---------------------------------------------------------------------------------------------
# 3. a deferred rendering keeps the whole description of its request
# ---------------------------------------------------------------------------------------------
def test_pipelined_output_keeps_the_tensor_of_its_request():
    n, w, h = 4, 176, 144
    b = h263mi.Batch(n, w, h, 0, None, pipeline_post=True)
    recs = [_upload_records(_small_streams(n, w, h, 4200 + 100 * k), w, h) for k in range(4)]
    # call 1: tensor A (f16, RGB, 50 x 30, padded); call 2: RGBA resize 40 x 30; call 3: tensor B (f32, BGR, other scale,
    # 181 x 146); call 4: default
    ta = h263mi.make_tensor_out(50, 30, ref.F16, *ref.IMAGENET, stride_h=53, stride_c=30 * 53 + 1)
    tb = h263mi.make_tensor_out(181, 146, ref.F32, [1 / 127.5] * 3, [-1.0] * 3, bgr=True)
    c1 = _canvas(h263mi.tensor_extent(n, ta))
    c2 = _canvas(h263mi.rgba_resize_extent(n, 40, 30))
    c3 = _canvas(h263mi.tensor_extent(n, tb))
    c4 = _canvas(n * w * h * 4)
    dec = lambda k, strength, c: b.decode(h263mi.PICTURE_I, recs[k][0][0].ptr, recs[k][0][1].ptr, recs[k][0][2].ptr, 0, strength, c.ptr, None)
    b.set_tensor_output(ta)
    dec(0, 7, c1)                                                     # deferred
    ta.scale[0] = 99.0                                                # (the description was copied)
    b.set_rgba_resize(40, 30)
    dec(1, 3, c2)                                                     # renders 1
    b.set_tensor_output(tb)
    dec(2, 5, c3)                                                     # renders 2
    b.set_tensor_output(None)
    dec(3, 9, c4)                                                     # renders 3
    b.set_tensor_output(ta)
    b.sync()                                                          # renders 4
    ta.scale[0] = ref.IMAGENET[0][0]
    small = lambda k, ow, oh: _small(recs[k][1], w, h, [(7, 3, 5, 9)[k]] * n, ow, oh)
    _same(c1.download().view(np.uint16), _want(c1.nbytes // 2, ref.F16, small(0, 50, 30), ta, stride_n=3 * ta.stride_c), "call 1")
    want2 = np.concatenate([p.ravel() for p in small(1, 40, 30)])
    _same(c2.download(), want2, "call 2")
    _same(c3.download().view(np.uint32), _want(c3.nbytes // 4, ref.F32, small(2, 181, 146), tb, stride_n=3 * 146 * 181), "call 3")
    want4 = np.concatenate([full_rgba(p, w, 9).ravel() for p in recs[3][1]])
    _same(c4.download(), want4, "call 4")
    b.close()


# ---------------------------------------------------------------------------------------------
# 4. refusals queue nothing; an injected failure leaves state and shape as they were
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [ref.F32, ref.BF16], ids=["f32", "bf16"])
def test_refusals_queue_nothing(qcif_streams, dtype):
    n, w, h, recs, planes = qcif_streams
    elt = ref.ELT[dtype]
    b = h263mi.Batch(n, w, h, 0, None)
    good = h263mi.make_tensor_out(40, 30, dtype, *ref.IMAGENET)
    b.set_tensor_output(good)
    # refused setters leave the shape in force untouched
    inf = h263mi.make_tensor_out(40, 30, dtype, [1.0, float("inf"), 1.0], [0.0] * 3)
    narrow = h263mi.make_tensor_out(40, 30, dtype, *ref.IMAGENET, stride_h=39)
    for bad in (inf, narrow):
        with pytest.raises(h263mi.H263Error) as e:
            b.set_tensor_output(bad)
        assert e.value.code == h263mi.ERR_INVALID_ARGUMENT
    nbytes = h263mi.tensor_extent(n, good)
    dec = lambda ptr: b.decode(h263mi.PICTURE_I, recs[0][0].ptr, recs[0][1].ptr, recs[0][2].ptr, 0, 5, ptr, None)
    short = _canvas(nbytes - 1)                                       # one byte short on a checked batch
    with pytest.raises(h263mi.H263Error) as e:
        dec(short.ptr)
    assert e.value.code == h263mi.ERR_INVALID_ARGUMENT
    roomy = _canvas(nbytes + 8)
    with pytest.raises(h263mi.H263Error) as e:                        # not a multiple of the element size
        dec(roomy.at(elt // 2))
    assert e.value.code == h263mi.ERR_INVALID_ARGUMENT
    with pytest.raises(h263mi.H263Error) as e:
        b.render_rgba(5, roomy.at(1), None)
    assert e.value.code in (h263mi.ERR_INVALID_ARGUMENT, h263mi.ERR_NO_PICTURE)
    assert not any(b.stream_has_picture(s) for s in range(n))        # no stream advanced
    b.sync()
    assert (short.download() == SENTINEL).all() and (roomy.download() == SENTINEL).all()
    # the following correct call succeeds, in the shape that was in force all along
    ok = _canvas(nbytes)
    dec(ok.ptr)
    b.sync()
    _same(ok.download().view(ref.BITS_DTYPE[dtype]), _want(nbytes // elt, dtype, _small(planes[0], w, h, [5] * n, 40, 30), good,
                                                             stride_n=3 * 30 * 40), "after the refusals")
    with pytest.raises(h263mi.H263Error) as e:
        b.render_rgba(5, short.ptr, None)
    assert e.value.code == h263mi.ERR_INVALID_ARGUMENT
    assert (short.download() == SENTINEL).all()
    b.close()


def test_a_failure_at_any_hip_call_of_set_then_decode_leaves_state_and_shape(qcif_streams):
    """h263mi_debug_fail_nth_hip_call swept over one set-tensor-then-decode: the hook skips the n-th HIP call and reports an
    allocation failure, it faults nothing.  The streams are all as they were or all advanced, and the shape in force is the one
    before the setter (when the setter failed) or the new one."""
    n, w, h, recs, planes = qcif_streams
    strength = 5
    ta = h263mi.make_tensor_out(40, 30, ref.F16, *ref.IMAGENET)
    tb = h263mi.make_tensor_out(65, 5, ref.BF16, [1 / 127.5] * 3, [-1.0] * 3, bgr=True, stride_h=67)
    shapes = {"a": (ta, ref.F16, 40, 30), "b": (tb, ref.BF16, 65, 5)}
    states = {"old": planes[0], "new": planes[1]}

    def rendered(b, shape, state):
        t, dtype, ow, oh = shapes[shape]
        nbytes = h263mi.tensor_extent(n, t)
        c = _canvas(nbytes)
        b.render_rgba(strength, c.ptr, None)
        b.sync()
        sh = t.stride_h or ow
        want = _want(nbytes // 2, dtype, _small(states[state], w, h, [strength] * n, ow, oh), t, stride_n=3 * oh * sh)
        return c.download().view(np.uint16), want

    seen, failures = set(), 0
    for nth in range(1, 100):
        b = h263mi.Batch(n, w, h, 0, None)
        b.set_tensor_output(ta)
        b.decode(h263mi.PICTURE_I, recs[0][0].ptr, recs[0][1].ptr, recs[0][2].ptr, 0, strength, None, None)
        b.sync()
        out = _canvas(h263mi.tensor_extent(n, tb))
        h263mi.debug_fail_nth_hip_call(nth)
        shape, done = "a", False
        try:
            b.set_tensor_output(tb)
            shape = "b"
            b.decode(h263mi.PICTURE_P, recs[1][0].ptr, recs[1][1].ptr, recs[1][2].ptr, 0, strength, out.ptr, None)
            fired = h263mi.debug_fail_nth_hip_call(0) <= 0
            assert not fired, "the %d-th HIP call failed and the calls reported success" % nth
            done = True
        except h263mi.H263Error as e:
            assert e.code == h263mi.ERR_OUT_OF_MEMORY, (nth, e.code)
            h263mi.debug_fail_nth_hip_call(0)
            failures += 1
        b.sync()
        got = [b.copy_yuv(s) for s in range(n)]
        which = [k for k, pl in states.items() if all((np.concatenate(g) == np.concatenate(p)).all() for g, p in zip(got, pl))]
        assert len(which) == 1, "failure at HIP call %d: the streams are neither all old nor all new" % nth
        assert which[0] == "new" if done else True
        assert which[0] == "old" if shape == "a" else True           # (a failed setter: the decode was never called)
        seen.add((shape, which[0]))
        _same(*rendered(b, shape, which[0]), "the shape in force after a failure at HIP call %d" % nth)
        if done:
            t, dtype, ow, oh = shapes["b"]
            _same(out.download().view(np.uint16),
                  _want(out.nbytes // 2, dtype, _small(planes[1], w, h, [strength] * n, ow, oh), t, stride_n=3 * oh * 67), "the decode")
        b.close()
        if done:
            break
    else:
        pytest.fail("the calls never went through")
    assert failures >= 3 and {("a", "old"), ("b", "new")} <= seen


# ---------------------------------------------------------------------------------------------
# 5. a mixed-size set: streams of four sizes land in ONE contiguous [4, 3, 64, 96] tensor
# ---------------------------------------------------------------------------------------------
class _Part:
    """a part of a device buffer, as MixedBatch.decode_next_pictures takes it"""

    def __init__(self, buf, offset, nbytes):
        self.ptr, self.nbytes = buf.at(offset), nbytes


@pytest.mark.parametrize("pipeline", [True, False], ids=["pipelined", "immediate"])
@pytest.mark.parametrize("dtype", [ref.F32, ref.BF16], ids=["f32", "bf16"])
def test_mixed_set_into_one_tensor(pipeline, dtype):
    import sorenson_enc as enc
    from test_bitstream_e2e import make_codable
    q, strength = 6, 5
    sizes = [(176, 144), (352, 288), (320, 240), (176, 144)]
    n, ow, oh, elt = len(sizes), 96, 64, ref.ELT[dtype]
    t = h263mi.make_tensor_out(ow, oh, dtype, *ref.IMAGENET)
    one = h263mi.tensor_extent(1, t)
    assert one == 3 * oh * ow * elt
    m = h263mi.MixedBatch(n, pipeline_post=pipeline)
    with pytest.raises(h263mi.H263Error):                             # stride_n must be 0: the caller places the streams
        m.set_tensor_output(h263mi.make_tensor_out(ow, oh, dtype, stride_n=3 * oh * ow))
    m.set_tensor_output(t)
    buf = _canvas(n * one)
    refs = [None] * n
    held = None
    for f in range(2):
        datas, wants = [], []
        for s, (w, h) in enumerate(sizes):
            intra = f == 0
            if intra:
                mbs, co = recgen.intra_picture(w, h, seed=5000 + s, max_level=60)
                mbs = make_codable(mbs, q, s, 0)
            else:
                mbs, co = recgen.inter_picture(w, h, seed=5100 + s, mv_range=32, p_4v=0.2, p_intra=0.05, p_coded=0.4, quant=q,
                                               max_level=60)
                mbs = make_codable(mbs, q, s + f, 1)
            datas.append(enc.encode_picture(w, h, 0 if intra else 1, q, mbs, co, temporal_reference=f))
            if f == 1 and s == 2:
                wants.append(held[s])                                 # refused below: its part keeps the previous contents
                continue
            rc, refs[s] = orc.decode_picture(w, h, mbs, co, None if intra else refs[s])
            assert rc == 0
            wants.append(rgba_resize_ref.resize(full_rgba(refs[s], w, strength), w, h, ow, oh))
        # stream 2's capacity is one byte short in call 2: refused for that stream alone
        parts = [_Part(buf, s * one, one - 1 if (f == 1 and s == 2) else one) for s in range(n)]
        used, rcs, _ = m.decode_next_pictures(datas, n_threads=2, strength=strength, rgba=parts)
        assert not any(m.sync())
        assert list(rcs) == ([0, 0, h263mi.ERR_INVALID_ARGUMENT, 0] if f else [0] * n)
        _same(buf.download().view(ref.BITS_DTYPE[dtype]), _want(n * one // elt, dtype, wants, t, stride_n=3 * oh * ow), "call %d" % f)
        held = wants
    # the classes' scratches count: 2 slots of 176 x 144, one of 352 x 288, one of 320 x 240, and each class's span tables
    with_tensor = m.frame_store_bytes()
    m.set_tensor_output(None)
    scratch = 4 * (2 * 176 * 144 + 352 * 288 + 320 * 240) + 3 * (ow + oh) * 16
    assert with_tensor - m.frame_store_bytes() == scratch
    m.set_tensor_output(t)
    assert m.frame_store_bytes() == with_tensor
    m.close()


# ---------------------------------------------------------------------------------------------
# 6. straight into a torch tensor
# ---------------------------------------------------------------------------------------------
def test_into_a_torch_tensor(qcif_streams):
    if not torch.cuda.is_available():
        pytest.skip("torch sees no device while the library does")
    n, w, h, recs, planes = qcif_streams
    ow, oh = 96, 64
    x = torch.empty((n, 3, oh, ow), dtype=torch.bfloat16, device="cuda")
    x.view(torch.int16).fill_(-0x3C3D)                                # 0xC3C3
    torch.cuda.synchronize()
    t = h263mi.make_tensor_out(ow, oh, ref.BF16, *ref.IMAGENET)
    assert h263mi.tensor_extent(n, t) == x.numel() * x.element_size()
    b = h263mi.Batch(n, w, h, 0, None)
    b.set_tensor_output(t)
    b.decode(h263mi.PICTURE_I, recs[0][0].ptr, recs[0][1].ptr, recs[0][2].ptr, 0, 5, x.data_ptr(), None)
    b.sync()
    got = x.cpu().view(torch.int16).numpy().view(np.uint16)
    want = np.stack([ref.planes(p, ref.BF16, *ref.IMAGENET) for p in _small(planes[0], w, h, [5] * n, ow, oh)])
    assert got.shape == want.shape == (n, 3, oh, ow)
    _same(got.ravel(), want.ravel(), "torch tensor")
    # what the model reads are the same numbers torch's own conversion gives
    assert torch.equal(x.cpu().float(), torch.from_numpy((want.astype(np.uint32) << 16).view(np.float32)))
    b.close()
