"""The contract of the region tracks (include/h263mi.h, REGION TRACKS) in plain sequential Python, integers only: one call over the
states of n pictures.  Two formulations of the matching -- the eligible pairs sorted with integer cross-multiplication and taken
greedily (match_sorted), and the maximum over the remaining pairs taken again and again (match_bruteforce) -- and a sanity check of
a matching that needs neither (check_matching).  TEST INFRASTRUCTURE."""
import functools

import numpy as np

ROI = np.dtype([("picture", np.uint32), ("x", np.uint16), ("y", np.uint16), ("w", np.uint16), ("h", np.uint16), ("reserved", np.uint32)])
INFO_IN = np.dtype([("components", np.uint32), ("kept", np.uint32), ("first", np.uint32), ("written", np.uint32)])
TRACK = np.dtype([("id", np.uint32), ("x", np.uint16), ("y", np.uint16), ("w", np.uint16), ("h", np.uint16), ("age", np.uint32),
                  ("hits", np.uint32), ("missed", np.uint16), ("flags", np.uint16), ("det", np.uint32), ("reserved", np.uint32)])
HEAD = np.dtype([("next_id", np.uint32), ("live", np.uint32), ("calls", np.uint32), ("reserved", np.uint32, (5,))])
INFO = np.dtype([(f, np.uint32) for f in ("detections", "ignored", "matched", "born", "died", "dropped", "first", "written")])
REF = np.dtype([("id", np.uint32), ("picture", np.uint32), ("hits", np.uint32), ("slot", np.uint16), ("flags", np.uint16)])
assert (ROI.itemsize, INFO_IN.itemsize, TRACK.itemsize, HEAD.itemsize, INFO.itemsize, REF.itemsize) == (16, 16, 32, 32, 32, 16)

BORN, MATCHED, EMITTED = 1, 2, 4
NO_DET = 0xFFFFFFFF
U32 = 0xFFFFFFFF
INVALID_ROI = (0xFFFFFFFF, 0, 0, 0, 0, 1)


class Params:
    def __init__(self, max_tracks=16, iou_permille=300, max_missed=2, min_hits=2, emit_period=0):
        self.max_tracks, self.iou_permille, self.max_missed, self.min_hits, self.emit_period = \
            max_tracks, iou_permille, max_missed, min_hits, emit_period

    def stride(self):
        return 32 + 32 * self.max_tracks


def box_valid(x, y, w, h, W, H):
    return w >= 1 and h >= 1 and x + w <= W and y + h <= H


def inter_union(a, b):
    """two boxes (x, y, w, h) -> (intersection, union) in pixels"""
    iw = min(a[0] + a[2], b[0] + b[2]) - max(a[0], b[0])
    ih = min(a[1] + a[3], b[1] + b[3]) - max(a[1], b[1])
    inter = iw * ih if iw > 0 and ih > 0 else 0
    return inter, a[2] * a[3] + b[2] * b[3] - inter


def eligible_pairs(tracks, dets, permille):
    """tracks: {slot: box}, dets: [box] -> [(inter, union, i, j)] of the eligible pairs"""
    out = []
    for i, tb in tracks.items():
        for j, db in enumerate(dets):
            inter, uni = inter_union(tb, db)
            if inter >= 1 and inter * 1000 >= permille * uni:
                out.append((inter, uni, i, j))
    return out


def _order(p, q):
    """negative when pair p comes before (is better than) pair q: more inter / union, then the smaller slot, then the smaller j"""
    a, b = p[0] * q[1], q[0] * p[1]
    if a != b:
        return -1 if a > b else 1
    return -1 if (p[2], p[3]) < (q[2], q[3]) else (1 if (p[2], p[3]) > (q[2], q[3]) else 0)


def match_sorted(tracks, dets, permille):
    """-> {slot: j}: the pairs sorted from best to worst, each taken when its track and its detection are still free"""
    out, used = {}, set()
    for inter, uni, i, j in sorted(eligible_pairs(tracks, dets, permille), key=functools.cmp_to_key(_order)):
        if i not in out and j not in used:
            out[i] = j
            used.add(j)
    return out


def match_bruteforce(tracks, dets, permille):
    """-> {slot: j}: the maximum over the remaining pairs, found by a plain scan, taken again and again"""
    rest = eligible_pairs(tracks, dets, permille)
    out = {}
    while rest:
        best = rest[0]
        for q in rest[1:]:
            if _order(q, best) < 0:
                best = q
        out[best[2]] = best[3]
        rest = [q for q in rest if q[2] != best[2] and q[3] != best[3]]
    return out


def check_matching(tracks, dets, permille, m):
    """what every greedy matching is, whatever the order: one-to-one, eligible pairs only, and maximal -- no eligible pair is left
    whose track and detection are both free -- and the best pair of all is in it"""
    assert len(set(m.values())) == len(m)
    pairs = eligible_pairs(tracks, dets, permille)
    ok = {(i, j) for _, _, i, j in pairs}
    assert all((i, j) in ok for i, j in m.items())
    used = set(m.values())
    assert not [(i, j) for i, j in ok if i not in m and j not in used]
    if pairs:
        best = min(pairs, key=functools.cmp_to_key(_order))
        assert m[best[2]] == best[3]


def next_id(n, k=1):
    v = n + k
    return v - U32 if v > U32 else v


def call(state, prm, W, H, n, rois, info_in, cut, cut_count, max_out, matcher=match_sorted, debug=None):
    """One call.  state: the bytes of n states (any garbage), rois: ROI records, info_in: n INFO_IN records, cut: a list of words and
    cut_count (or None, None).  -> (state, out_rois, out_refs, info, count) as the call leaves them"""
    state = np.array(state, np.uint8).reshape(n, prm.stride()) if n else np.zeros((0, prm.stride()), np.uint8)
    new = np.zeros_like(state)
    info = np.zeros(n, INFO)
    emitted = []                                            # (picture, slot, track record)
    n_rois = len(rois)
    for p in range(n):
        head = state[p, :32].view(HEAD)[0]
        slots = state[p, 32:].view(TRACK)
        nid = int(head["next_id"]) or 1
        live = {}
        for i in range(prm.max_tracks):
            s = slots[i]
            if int(s["id"]) != 0 and box_valid(int(s["x"]), int(s["y"]), int(s["w"]), int(s["h"]), W, H):
                live[i] = dict(id=int(s["id"]), box=(int(s["x"]), int(s["y"]), int(s["w"]), int(s["h"])), age=int(s["age"]),
                               hits=int(s["hits"]), missed=int(s["missed"]), flags=0, det=NO_DET)
        died = 0
        # 1. cut
        if cut is not None and any(int(v) == p for v in cut[:min(int(cut_count), n)]):
            died += len(live)
            live = {}
        # 2. detections
        first, written = int(info_in[p]["first"]), int(info_in[p]["written"])
        dets, didx = [], []
        if first + written <= n_rois:
            for k in range(first, first + written):
                q = rois[k]
                if int(q["reserved"]) == 0 and int(q["picture"]) == p and box_valid(int(q["x"]), int(q["y"]), int(q["w"]), int(q["h"]), W, H) \
                        and len(dets) < 256:
                    dets.append((int(q["x"]), int(q["y"]), int(q["w"]), int(q["h"])))
                    didx.append(k)
        ignored = written - len(dets)
        # 3. match
        m = matcher({i: t["box"] for i, t in live.items()}, dets, prm.iou_permille)
        if debug is not None:
            debug.append(dict(picture=p, tracks={i: t["box"] for i, t in live.items()}, dets=list(dets), match=dict(m)))
        # 4. update
        for i in sorted(live):
            t = live[i]
            t["age"] = min(t["age"] + 1, U32)
            if i in m:
                t.update(box=dets[m[i]], hits=min(t["hits"] + 1, U32), missed=0, flags=MATCHED, det=didx[m[i]])
            else:
                t["missed"] += 1
                if t["missed"] > prm.max_missed:
                    del live[i]
                    died += 1
        # 5. births
        used = set(m.values())
        unmatched = [j for j in range(len(dets)) if j not in used]
        free = [i for i in range(prm.max_tracks) if i not in live]
        born = min(len(unmatched), len(free))
        for j, i in zip(unmatched, free):
            live[i] = dict(id=nid, box=dets[j], age=1, hits=1, missed=0, flags=BORN, det=didx[j])
            nid = next_id(nid)
        # 6. emitted
        out = new[p, 32:].view(TRACK)
        e = 0
        for i in sorted(live):
            t = live[i]
            if t["flags"] and t["hits"] >= prm.min_hits and \
                    (t["hits"] == prm.min_hits if prm.emit_period == 0 else (t["hits"] - prm.min_hits) % prm.emit_period == 0):
                t["flags"] |= EMITTED
                e += 1
            out[i] = (t["id"],) + t["box"] + (t["age"], t["hits"], t["missed"], t["flags"], t["det"], 0)
            if t["flags"] & EMITTED:
                emitted.append((p, i, t))
        new[p, :32].view(HEAD)[0] = (nid, len(live), (int(head["calls"]) + 1) & U32, (0,) * 5)
        info[p] = (len(dets), ignored, len(m), born, died, len(unmatched) - born, 0, e)
    # the table
    out_rois = np.zeros(max_out, ROI)
    out_refs = np.zeros(max_out, REF)
    out_rois[:] = INVALID_ROI
    before = 0
    for p in range(n):
        e = int(info[p]["written"])
        first = min(before, max_out)
        info[p]["first"], info[p]["written"] = first, min(e, max_out - first)
        before += e
    for k, (p, i, t) in enumerate(emitted[:max_out]):
        out_rois[k] = (p,) + t["box"] + (0,)
        out_refs[k] = (t["id"], p, t["hits"], i, t["flags"])
    count = np.array([min(before, max_out), before], np.uint32)
    return new.reshape(-1), out_rois, out_refs, info, count
