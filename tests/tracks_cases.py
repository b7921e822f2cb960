"""The cases of the region tracks (h263mi_tracks_on), shared by the reference's own tests, the CPU checker's tests and the GPU tests.
A case is a SEQUENCE of calls over one state: the parameters, the picture size (geometry only: no pixel is read), the first state
(zeros, or bytes given) and per call the table of boxes, its per-picture infos and the cut list.  check_hazards() asserts, on the
reference's side, that each hazard the cases are there for occurs.  TEST INFRASTRUCTURE."""
import functools
import itertools

import numpy as np

import tracks_ref as ref


class Call:
    def __init__(self, rois, info_in, cut=None, cut_count=None):
        self.rois = np.array(rois, ref.ROI).reshape(-1)
        self.info_in = np.array(info_in, ref.INFO_IN).reshape(-1)
        self.cut = None if cut is None else np.array(cut, np.uint32).reshape(-1)
        self.cut_count = cut_count


class Case:
    def __init__(self, prm, w, h, n, calls, max_out=None, state0=None, refs=True):
        self.prm, self.w, self.h, self.n, self.calls, self.refs = prm, w, h, n, calls, refs
        self.max_out = max_out if max_out is not None else max(1, min(65535, n * prm.max_tracks))
        self.state_bytes = n * prm.stride()
        self.state0 = np.zeros(self.state_bytes, np.uint8) if state0 is None else np.array(state0, np.uint8)
        assert self.state0.size == self.state_bytes and all(c.info_in.size == n for c in calls)

    def expected(self, matcher=ref.match_sorted, debug=None):
        """-> per call (state, out_rois, out_refs, info, count)"""
        out, state = [], self.state0
        for c in self.calls:
            dbg = None if debug is None else []
            r = ref.call(state, self.prm, self.w, self.h, self.n, c.rois, c.info_in, c.cut, c.cut_count, self.max_out, matcher, dbg)
            if debug is not None:
                debug.append(dbg)
            out.append(r)
            state = r[0]
        return out


def table(n, per_picture, pad=2, lead=0):
    """per picture a list of boxes (x, y, w, h) or whole entries (picture, x, y, w, h, reserved) -> the table as regions lays it out
    (the slices back to back, `pad` invalid entries behind them, `lead` in front) and the infos"""
    rois, info = [ref.INVALID_ROI] * lead, []
    for p in range(n):
        boxes = per_picture[p] if p < len(per_picture) else []
        info.append((len(boxes), len(boxes), len(rois), len(boxes)))
        rois += [b if len(b) == 6 else (p,) + tuple(b) + (0,) for b in boxes]
    return Call(rois + [ref.INVALID_ROI] * pad, info)


def sequence(n, steps, **kw):
    return [table(n, s, **kw) for s in steps]


P = ref.Params

# ---------------------------------------------------------------------------------------------------------------------------
CHAIN_W, CHAIN_H = 12840, 1000


def chain_boxes():
    """S_0 = T_0, S_1 = D_0, S_2 = T_1, ...: boxes 40 wide, 25 apart, so only neighbours overlap (15 columns); heights 1000 - m, so
    the IoU of S_m and S_m+1, 15 h' / (65 h' + 40) with h' = 999 - m, falls strictly along the chain: track k prefers detection
    k - 1 and settles for k"""
    s = [(25 * m, 0, 40, 1000 - m) for m in range(512)]
    return s[0::2], s[1::2]


def grid_boxes(count, cols, size=10, pitch=20, x0=0, y0=0):
    return [(x0 + (k % cols) * pitch, y0 + (k // cols) * pitch, size, size) for k in range(count)]


def case_ties():
    return Case(P(7, 100, 2, 1, 0), 64, 48, 2, sequence(2, [
        [[(10, 10, 10, 10)], [(5, 10, 10, 10), (15, 10, 10, 10)]],
        [[(5, 10, 10, 10), (15, 10, 10, 10)], [(10, 10, 10, 10)]]]))


FLOAT_TRACK, FLOAT_INSIDE, FLOAT_AROUND = (100, 100, 8133, 6966), (100, 100, 8095, 6957), (90, 90, 8163, 6982)
EQUAL_TRACK, EQUAL_SMALL, EQUAL_LARGE = (0, 0, 5000, 5000), (0, 0, 4096, 4098), (0, 0, 4097, 4097)


def case_float_order():
    """picture 0: the detection inside the track has the larger IoU, float32 division gives it the smaller quotient; picture 1: two
    detections inside the track whose areas, 16785408 and 16785409, are one float32"""
    return Case(P(7, 500, 2, 1, 0), 16384, 16384, 2, sequence(2, [
        [[FLOAT_TRACK], [EQUAL_TRACK]],
        [[FLOAT_AROUND, FLOAT_INSIDE], [EQUAL_SMALL, EQUAL_LARGE]]]))


def case_threshold():
    """permille 500: 100 / 200 is on the threshold, 99 / 200 one pixel below"""
    return Case(P(7, 500, 2, 1, 0), 64, 48, 2, sequence(2, [
        [[(0, 0, 20, 10)], [(0, 0, 20, 10)]],
        [[(0, 0, 10, 10)], [(0, 0, 11, 9)]]]))


def case_permille0():
    """permille 0: one pixel of overlap matches, boxes that touch do not"""
    return Case(P(7, 0, 2, 1, 0), 64, 48, 2, sequence(2, [
        [[(10, 10, 10, 10)], [(10, 10, 10, 10)]],
        [[(19, 19, 10, 10)], [(20, 10, 10, 10)]]]))


def case_greedy_not_argmax():
    return Case(P(7, 100, 2, 1, 0), 64, 48, 1, sequence(1, [
        [[(0, 0, 10, 10), (4, 0, 10, 10)]],
        [[(1, 0, 10, 10), (8, 0, 10, 10)]]]))


def case_chain256():
    t, d = chain_boxes()
    return Case(P(256, 100, 2, 2, 0), CHAIN_W, CHAIN_H, 1, sequence(1, [[t], [d]]))


def case_greedy_not_optimal():
    return Case(P(7, 50, 2, 1, 0), 256, 48, 1, sequence(1, [
        [[(100, 0, 100, 10), (120, 0, 100, 10)]],
        [[(105, 0, 100, 10), (15, 0, 100, 10)]]]))


def case_full_256():
    """all 256 slots live; 200 detections match, 56 further ones find no slot"""
    first = grid_boxes(256, 16)
    second = [(x + 1, y, w, h) for x, y, w, h in first[:200]] + grid_boxes(56, 16, x0=400)
    return Case(P(256, 300, 2, 2, 1), 1024, 512, 1, sequence(1, [[first], [second], [second]]))


def case_deaths_and_births():
    """max_missed 0: tracks 0, 2, 4 die, the four births take the slots 0, 2, 4, 5"""
    first = grid_boxes(5, 5)
    second = [first[1], first[3]] + grid_boxes(4, 4, y0=30)
    return Case(P(7, 300, 0, 1, 0), 128, 48, 1, sequence(1, [[first], [second], [second[:3]]]))


def case_max_missed_2():
    """three calls without a detection: missed 1, 2, then death; the same box is a new track afterwards"""
    b = [[(8, 8, 16, 16)]]
    return Case(P(7, 300, 2, 1, 1), 64, 48, 1, sequence(1, [b, [[]], [[]], b, [[]], [[]], [[]], b]))


def case_emit(min_hits, period):
    """an object that moves two pixels a call over 14 calls and is not seen in the 7th and 8th; a flicker in the 4th call"""
    steps = []
    for k in range(14):
        boxes = [] if k in (6, 7) else [(4 + 2 * k, 6, 20, 20)]
        if k == 3:
            boxes.append((50, 30, 6, 6))
        steps.append([boxes, boxes[:1]])
    return Case(P(7, 300, 2, min_hits, period), 64, 48, 2, sequence(2, steps))


def case_max_tracks_1():
    return Case(P(1, 300, 0, 1, 1), 64, 48, 2, sequence(2, [
        [[(0, 0, 10, 10), (30, 0, 10, 10)], []],
        [[(31, 0, 10, 10), (1, 0, 10, 10)], [(5, 5, 5, 5)]],
        [[(31, 0, 10, 10)], [(5, 5, 5, 5)]]]))


def case_cuts():
    """the list 7, 2, 2, 9, 1 with a count of 9: min(9, 4) = 4 entries are read, so picture 2 is cut (twice) and picture 1 is not;
    then no list, a count of 0, and a list that cuts all"""
    boxes = [[(8 * p, 4, 12, 12), (8 * p, 24, 12, 12)] for p in range(4)]
    calls = sequence(4, [boxes, boxes, boxes, boxes, boxes])
    calls[1].cut, calls[1].cut_count = np.array([7, 2, 2, 9, 1], np.uint32), 9
    calls[3].cut, calls[3].cut_count = np.array([0, 1, 2, 3], np.uint32), 0
    calls[4].cut, calls[4].cut_count = np.array([3, 0, 1, 2], np.uint32), 4
    return Case(P(7, 300, 2, 2, 0), 64, 48, 4, calls)


def case_garbage_state():
    """random bytes as the first state; by hand a live slot, a slot with w == 0, one with x + w > W, a live slot whose missed is
    65535, a next_id of 0"""
    prm = P(7, 300, 2, 1, 1)
    rng = np.random.default_rng(5)
    state = rng.integers(0, 256, 2 * prm.stride(), dtype=np.uint8)
    s = state.reshape(2, prm.stride())
    slots = s[0, 32:].view(ref.TRACK)
    slots[1] = (77, 10, 10, 12, 12, 5, 4, 1, 0xFFFF, 123, 0xDEAD)            # live
    slots[2] = (78, 10, 10, 0, 12, 5, 4, 1, 0, 0, 0)                         # w == 0
    slots[3] = (79, 60, 10, 5, 12, 5, 4, 1, 0, 0, 0)                         # x + w = 65 > 64
    slots[4] = (80, 30, 30, 8, 8, 0xFFFFFFFF, 0xFFFFFFFF, 65535, 0, 0, 0)    # live, dies of its 65536th miss
    slots[5] = (81, 40, 4, 8, 8, 0xFFFFFFFF, 0xFFFFFFFF, 0, 0, 0, 0)         # live, age and hits saturate
    s[1, :32].view(ref.HEAD)[0] = (0, 99, 0xFFFFFFFF, (1, 2, 3, 4, 5))
    boxes = [[(11, 10, 12, 12), (41, 4, 8, 8), (50, 30, 6, 6)], [(0, 0, 4, 4)]]
    return Case(prm, 64, 48, 2, sequence(2, [boxes, boxes]), state0=state)


def case_id_wrap():
    prm = P(7, 300, 0, 1, 0)
    state = np.zeros(2 * prm.stride(), np.uint8)
    state[:32].view(ref.HEAD)[0] = (0xFFFFFFFE, 0, 0, (0,) * 5)
    return Case(prm, 64, 48, 2, sequence(2, [[grid_boxes(3, 3), grid_boxes(2, 2)], [grid_boxes(3, 3, y0=20), []]]), state0=state)


def case_garbage_info_in():
    """picture 0: first + written above n_rois; picture 1: a sum that wraps 32 bits; picture 2: a slice with entries of another
    picture, a reserved word, the invalid entry of regions, empty and overhanging boxes among three valid ones; picture 3: zeros"""
    good = [(2, 4, 4, 8, 8, 0), (2, 20, 4, 8, 8, 0), (2, 40, 20, 8, 8, 0)]
    bad = [(1, 4, 4, 8, 8, 0), (2, 4, 4, 8, 8, 1), ref.INVALID_ROI, (2, 4, 4, 0, 8, 0), (2, 4, 4, 8, 0, 0), (2, 60, 4, 8, 8, 0), (2, 4, 44, 8, 8, 0),
           (0xFFFFFFFF, 4, 4, 8, 8, 0), (3, 4, 4, 8, 8, 0)]
    rois = [bad[0], good[0], bad[1], bad[2], bad[3], good[1], bad[4], bad[5], bad[6], good[2], bad[7], bad[8]]
    n_rois = len(rois)
    info = [(1, 1, 10, n_rois - 9), (1, 1, 0xFFFFFFF0, 0x18), (0, 0, 0, n_rois), (0, 0, 0, 0)]
    return Case(P(7, 300, 2, 1, 1), 64, 48, 4, [Call(rois, info), Call(rois, info)])


def case_slice_300():
    """300 valid entries in one slice: the first 256 are the detections; then the same behind 100 invalid entries in the slice, so
    that the 256th valid one is found in the gather's second step"""
    boxes = grid_boxes(300, 20, 8, 10)
    second = table(1, [[(0, 0, 0, 0, 0, 0)] * 100 + boxes])
    return Case(P(256, 300, 2, 2, 0), 4096, 4096, 1, [table(1, [boxes]), second])


def case_pictures_130():
    """130 pictures: the pack's prefix takes three steps; picture p emits p % 4 tracks a call, 193 in all, the table holds 100 and
    is full after the first of picture 67's three"""
    boxes = [grid_boxes(p % 4, 4) for p in range(130)]
    return Case(P(7, 300, 2, 1, 1), 128, 48, 130, sequence(130, [boxes, boxes]), max_out=100)


def case_no_pictures():
    return Case(P(7, 300, 2, 1, 1), 64, 48, 0, [Call([], []), Call([ref.INVALID_ROI], [])], max_out=5)


def case_no_refs():
    c = case_deaths_and_births()
    c.refs = False
    return c


def random_case(seed, n=3, max_tracks=16, calls=5, w=320, h=240, objects=12, permille=300, dense=False):
    """objects that drift, appear and vanish, noise boxes, overlapping boxes, cuts now and then"""
    rng = np.random.default_rng(seed)
    prm = P(max_tracks, permille, int(rng.integers(0, 3)), int(rng.integers(1, 4)), int(rng.integers(0, 3)))
    pos = rng.integers(0, [w - 40, h - 40], (n, objects, 2))
    size = rng.integers(8, 40, (n, objects, 2))
    out = []
    for _ in range(calls):
        per = []
        for p in range(n):
            boxes = []
            for k in range(objects):
                if rng.random() < 0.8:
                    boxes.append((int(pos[p, k, 0]), int(pos[p, k, 1]), int(size[p, k, 0]), int(size[p, k, 1])))
            for _ in range(int(rng.integers(0, 4))):
                boxes.append((int(rng.integers(0, w - 8)), int(rng.integers(0, h - 8)), int(rng.integers(1, 9)), int(rng.integers(1, 9))))
            order = rng.permutation(len(boxes))
            per.append([boxes[i] for i in order])
        c = table(n, per, pad=int(rng.integers(0, 3)), lead=int(rng.integers(0, 3)))
        if rng.random() < 0.4:
            c.cut, c.cut_count = rng.integers(0, n + 2, n + 1).astype(np.uint32), int(rng.integers(0, n + 3))
        out.append(c)
        step = 12 if dense else 5
        pos = np.clip(pos + rng.integers(-step, step + 1, pos.shape), 0, [w - 40, h - 40])
    return Case(prm, w, h, n, out, max_out=int(rng.integers(1, n * max_tracks + 1)))


CASES = {
    "ties": case_ties,
    "float_order": case_float_order,
    "threshold": case_threshold,
    "permille0": case_permille0,
    "greedy_not_argmax": case_greedy_not_argmax,
    "chain256": case_chain256,
    "greedy_not_optimal": case_greedy_not_optimal,
    "full_256": case_full_256,
    "deaths_and_births": case_deaths_and_births,
    "max_missed_2": case_max_missed_2,
    "emit_h1_p0": lambda: case_emit(1, 0), "emit_h1_p1": lambda: case_emit(1, 1), "emit_h1_p4": lambda: case_emit(1, 4),
    "emit_h3_p0": lambda: case_emit(3, 0), "emit_h3_p1": lambda: case_emit(3, 1), "emit_h3_p4": lambda: case_emit(3, 4),
    "max_tracks_1": case_max_tracks_1,
    "cuts": case_cuts,
    "garbage_state": case_garbage_state,
    "id_wrap": case_id_wrap,
    "garbage_info_in": case_garbage_info_in,
    "slice_300": case_slice_300,
    "pictures_130": case_pictures_130,
    "no_pictures": case_no_pictures,
    "no_refs": case_no_refs,
    "random_small": lambda: random_case(1),
    "random_crowded": lambda: random_case(2, n=2, max_tracks=7, objects=30, w=160, h=120, dense=True),
    "random_256": lambda: random_case(3, n=2, max_tracks=256, objects=250, calls=3, w=640, h=480, permille=50, dense=True),
}
# the cases whose matching takes more than one round
MULTI_ROUND = ["greedy_not_argmax", "chain256", "full_256", "random_small", "random_crowded", "random_256"]
MUTANT_CASES = {
    "H263MI_MUTATE_TRACKS_FLOAT_IOU": ["float_order"],
    "H263MI_MUTATE_TRACKS_ARGMAX": ["greedy_not_argmax", "chain256"],
    "H263MI_MUTATE_TRACKS_BIRTH_BEFORE_DEATH": ["deaths_and_births", "cuts"],
}


@functools.lru_cache(maxsize=None)
def build(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def expected(name):
    """the reference's outputs of every call of the case, computed once and shared"""
    return build(name).expected()


def compare(want, state, rois, refs, info, count):
    """one call's outputs against the reference's, byte for byte -> None, or what differs first"""
    w_state, w_rois, w_refs, w_info, w_count = want
    for what, a, b in (("state", w_state, state), ("rois", w_rois, rois), ("refs", w_refs, refs), ("info", w_info, info), ("count", w_count, count)):
        if b is None:
            continue
        a, b = np.ascontiguousarray(a).view(np.uint8).reshape(-1), np.ascontiguousarray(b).view(np.uint8).reshape(-1)
        if a.size != b.size:
            return "%s: %d bytes, not %d" % (what, b.size, a.size)
        if not np.array_equal(a, b):
            at = int(np.nonzero(a != b)[0][0])
            return "%s differs at byte %d" % (what, at)
    return None


def rounds_of_mutual_best(tracks, dets, permille):
    """the rounds in which the mutual-best formulation matches something, and its matching"""
    pairs = ref.eligible_pairs(tracks, dets, permille)
    key = functools.cmp_to_key(ref._order)
    m, rounds = {}, 0
    while True:
        best_t, best_d = {}, {}
        for q in pairs:
            if q[2] not in best_t or key(q) < key(best_t[q[2]]):
                best_t[q[2]] = q
            if q[3] not in best_d or key(q) < key(best_d[q[3]]):
                best_d[q[3]] = q
        took = [q for q in best_t.values() if best_d[q[3]] is q]
        if not took:
            return rounds, m
        rounds += 1
        for q in took:
            m[q[2]] = q[3]
        gone_t, gone_d = {q[2] for q in took}, {q[3] for q in took}
        pairs = [q for q in pairs if q[2] not in gone_t and q[3] not in gone_d]


def _debug(name):
    dbg = []
    out = build(name).expected(debug=dbg)
    return out, dbg


def check_hazards():
    f32 = np.float32
    slots = lambda state, p, prm: state.reshape(-1, prm.stride())[p, 32:].view(ref.TRACK)
    head = lambda state, p, prm: state.reshape(-1, prm.stride())[p, :32].view(ref.HEAD)[0]

    # ties: one track, two detections of equal IoU -> the smaller j; two tracks, one detection -> the smaller slot
    out, dbg = _debug("ties")
    d0, d1 = dbg[1]
    pairs = ref.eligible_pairs(d0["tracks"], d0["dets"], 100)
    assert len(pairs) == 2 and pairs[0][0] * pairs[1][1] == pairs[1][0] * pairs[0][1] and d0["match"] == {0: 0}
    pairs = ref.eligible_pairs(d1["tracks"], d1["dets"], 100)
    assert len(pairs) == 2 and pairs[0][0] * pairs[1][1] == pairs[1][0] * pairs[0][1] and d1["match"] == {0: 0}
    assert out[1][3]["born"].tolist() == [1, 0] and slots(out[1][0], 1, build("ties").prm)["missed"][1] == 1

    # float32 division orders two pairs wrongly, and calls two others equal; areas between 2^24 and 2^29
    out, dbg = _debug("float_order")
    (i1, u1), (i2, u2) = ref.inter_union(FLOAT_TRACK, FLOAT_INSIDE), ref.inter_union(FLOAT_TRACK, FLOAT_AROUND)
    assert all(2 ** 24 < v < 2 ** 29 for v in (i1, u1, i2, u2))
    assert i1 * u2 > i2 * u1 and f32(i1) / f32(u1) < f32(i2) / f32(u2)
    assert dbg[1][0]["match"] == {0: 1}
    (i1, u1), (i2, u2) = ref.inter_union(EQUAL_TRACK, EQUAL_LARGE), ref.inter_union(EQUAL_TRACK, EQUAL_SMALL)
    assert i1 > i2 > 2 ** 24 and u1 == u2 and f32(i1) / f32(u1) == f32(i2) / f32(u2)
    assert dbg[1][1]["match"] == {0: 1}

    # on the threshold and one pixel below
    out, dbg = _debug("threshold")
    (i1, u1), (i2, u2) = ref.inter_union((0, 0, 20, 10), (0, 0, 10, 10)), ref.inter_union((0, 0, 20, 10), (0, 0, 11, 9))
    assert i1 * 1000 == 500 * u1 and i2 * 1000 == 500 * u2 - 1000 and (i2, u2) == (99, 200)
    assert dbg[1][0]["match"] == {0: 0} and dbg[1][1]["match"] == {}

    # permille 0: one pixel, and none
    out, dbg = _debug("permille0")
    assert ref.inter_union((10, 10, 10, 10), (19, 19, 10, 10))[0] == 1 and ref.inter_union((10, 10, 10, 10), (20, 10, 10, 10))[0] == 0
    assert dbg[1][0]["match"] == {0: 0} and dbg[1][1]["match"] == {}

    # greedy is not the per-track argmax: both tracks like detection 0 best
    out, dbg = _debug("greedy_not_argmax")
    d = dbg[1][0]
    for i in (0, 1):
        assert ref.match_sorted({i: d["tracks"][i]}, d["dets"], 100) == {i: 0}
    assert d["match"] == {0: 0, 1: 1}
    assert rounds_of_mutual_best(d["tracks"], d["dets"], 100) == (2, d["match"])

    # the chain: 256 rounds, each track prefers the detection before its own
    out, dbg = _debug("chain256")
    d = dbg[1][0]
    assert len(d["tracks"]) == 256 and len(d["dets"]) == 256 and d["match"] == {k: k for k in range(256)}
    for k in range(1, 256):
        assert ref.match_sorted({k: d["tracks"][k]}, d["dets"], 100) == {k: k - 1}
    assert rounds_of_mutual_best(d["tracks"], d["dets"], 100) == (256, d["match"])
    assert all(b[0] + b[2] <= CHAIN_W and b[3] <= CHAIN_H for b in d["dets"])

    # greedy is not the optimal assignment: a matching of two pairs exists, greedy takes one
    out, dbg = _debug("greedy_not_optimal")
    d = dbg[1][0]
    ok = {(i, j) for _, _, i, j in ref.eligible_pairs(d["tracks"], d["dets"], 50)}
    assert any(all((i, j) in ok for i, j in zip((0, 1), perm)) for perm in itertools.permutations(range(2)))
    assert len(d["match"]) == 1 and out[1][3]["born"][0] == 1

    # all slots live, further detections are dropped
    out, dbg = _debug("full_256")
    prm = build("full_256").prm
    assert head(out[0][0], 0, prm)["live"] == 256 and out[1][3][0]["dropped"] == 56 and out[1][3][0]["matched"] == 200
    assert head(out[1][0], 0, prm)["live"] == 256

    # deaths and births in one call: the births take the freed slots, ascending
    out, dbg = _debug("deaths_and_births")
    prm = build("deaths_and_births").prm
    s = slots(out[1][0], 0, prm)
    assert out[1][3][0]["died"] == 3 and out[1][3][0]["born"] == 4
    assert [int(f) & 3 for f in s["flags"]] == [1, 2, 1, 2, 1, 1, 0] and [int(v) for v in s["id"]] == [6, 2, 7, 4, 8, 9, 0]
    assert prm.max_missed == 0 and prm.max_tracks == 7

    out, dbg = _debug("max_missed_2")
    prm = build("max_missed_2").prm
    assert [int(slots(o[0], 0, prm)["missed"][0]) for o in out[:3]] == [0, 1, 2] and int(slots(out[3][0], 0, prm)["id"][0]) == 1
    assert [int(o[3][0]["died"]) for o in out] == [0, 0, 0, 0, 0, 0, 1, 0] and int(slots(out[7][0], 0, prm)["id"][0]) == 2

    # the schedules of emission over 14 calls
    want = {(1, 0): [0], (1, 1): [0, 1, 2, 3, 4, 5, 8, 9, 10, 11, 12, 13], (1, 4): [0, 4, 10],
            (3, 0): [2], (3, 1): [2, 3, 4, 5, 8, 9, 10, 11, 12, 13], (3, 4): [2, 8, 12]}
    for (mh, per), calls in want.items():
        name = "emit_h%d_p%d" % (mh, per)
        out = expected(name)
        assert len(out) >= 12
        got = [k for k, o in enumerate(out) if any(r["id"] == 1 and r["picture"] == 1 for r in o[2][:int(o[4][0])])]
        assert got == calls, (name, got)

    out = expected("max_tracks_1")
    assert out[0][3][0]["dropped"] == 1 and out[1][3][0]["matched"] == 1 and out[1][3][0]["dropped"] == 1
    assert {build(n).prm.max_tracks for n in CASES} >= {1, 7, 256}

    # the cut list: indices >= n_pictures, a count above n_pictures, duplicates; all die and all are born in one call
    c = build("cuts")
    out = expected("cuts")
    assert c.calls[1].cut_count > c.n and max(c.calls[1].cut) >= c.n and list(c.calls[1].cut).count(2) == 2
    assert out[1][3]["died"].tolist() == [0, 0, 2, 0] and out[1][3]["born"].tolist() == [0, 0, 2, 0] and out[1][3]["matched"].tolist() == [2, 2, 0, 2]
    assert [int(v) for v in slots(out[1][0], 2, c.prm)["id"][:2]] == [3, 4]
    assert out[3][3]["died"].sum() == 0 and out[4][3]["died"].tolist() == [2, 2, 2, 2]

    # a garbage state: what is live in it, what is not
    c = build("garbage_state")
    out = expected("garbage_state")
    s = slots(out[0][0], 0, c.prm)
    assert int(s["id"][1]) == 77 and int(s["flags"][1]) == 6 and int(s["reserved"][1]) == 0 and int(s["hits"][1]) == 5
    assert int(s["id"][5]) == 81 and int(s["age"][5]) == 0xFFFFFFFF and int(s["hits"][5]) == 0xFFFFFFFF
    assert int(out[0][3][0]["died"]) >= 1 and int(s["id"][4]) != 80
    assert int(head(out[0][0], 1, c.prm)["next_id"]) == 2 and int(head(out[0][0], 1, c.prm)["calls"]) == 0
    assert not head(out[0][0], 1, c.prm)["reserved"].any()

    # ids wrap past 0
    c = build("id_wrap")
    out = expected("id_wrap")
    assert [int(v) for v in slots(out[0][0], 0, c.prm)["id"][:3]] == [0xFFFFFFFE, 0xFFFFFFFF, 1]
    assert int(head(out[0][0], 0, c.prm)["next_id"]) == 2 and [int(v) for v in slots(out[0][0], 1, c.prm)["id"][:2]] == [1, 2]

    c = build("garbage_info_in")
    out = expected("garbage_info_in")
    n_rois = c.calls[0].rois.size
    assert 10 + (n_rois - 9) > n_rois and (0xFFFFFFF0 + 0x18) & 0xFFFFFFFF < n_rois
    assert out[0][3]["detections"].tolist() == [0, 0, 3, 0] and out[0][3]["ignored"].tolist() == [n_rois - 9, 0x18, n_rois - 3, 0]

    c = build("slice_300")
    out = expected("slice_300")
    assert out[0][3][0]["detections"] == 256 and out[0][3][0]["ignored"] == 44 and out[1][3][0]["matched"] == 256
    assert out[1][3][0]["ignored"] == 144

    c = build("pictures_130")
    out = expected("pictures_130")
    assert out[0][4].tolist() == [100, 193] and out[0][3][67]["first"] == 99 and out[0][3][67]["written"] == 1
    assert out[0][3][68]["first"] == 100 and out[0][3][129]["written"] == 0

    out = expected("no_pictures")
    assert out[0][4].tolist() == [0, 0] and out[0][1]["reserved"].tolist() == [1] * 5
