"""The numpy reference of the background model (include/h263mi.h, BACKGROUND MODEL), written from the header's text: a state buffer
is the bytes the header lays out (per picture a 64-byte head, then H rows of 16 * ceil(W/16) uint16 words), a call is one pass over
it in 64-bit integers.  The cells' judgement, the summaries and the selection are the change maps' (change_ref) with the counts of
foreground pixels in the place of the SADs.  Shared by the CPU checker's tests and the GPU tests."""
import numpy as np

import change_ref

VALID, INIT, WARM = 1, 2, 4          # head.mode
KEEP = 255                           # fg_learn_shift: a foreground pixel keeps its word
HEAD_BYTES = 64


class Params:
    def __init__(self, cl=4, learn=4, fg_learn=KEEP, pix_thr=24, warmup=0, cell_thr=0, min_changed=1):
        self.cl, self.learn, self.fg_learn, self.pix_thr, self.warmup = cl, learn, fg_learn, pix_thr, warmup
        self.cell_thr, self.min_changed = cell_thr, min_changed
        self.c = 1 << cl


def padded_width(w):
    return 16 * -(-w // 16)


def bpitch(w):
    return 2 * padded_width(w)


def state_stride(w, h):
    return HEAD_BYTES + h * bpitch(w)


def head_of(state, p, w, h):
    """the 16 words of picture p's head, a view"""
    at = p * state_stride(w, h)
    return state[at:at + HEAD_BYTES].view(np.uint32)


def words_of(state, p, w, h):
    """picture p's (h, padded width) uint16 words, a view"""
    at = p * state_stride(w, h) + HEAD_BYTES
    return state[at:at + h * bpitch(w)].view(np.uint16).reshape(h, padded_width(w))


def empty_state(n, w, h):
    return np.zeros(n * state_stride(w, h), np.uint8)


def is_cut(p, n, cut, cut_count):
    return cut is not None and any(int(cut[k]) == p for k in range(min(int(cut_count), n)))


def moved(c, b, s, mutant=None):
    """the words b after a step towards the pixels c at shift s (int64 arrays)"""
    if s == KEEP:
        return b
    d = (c << 7) - b
    step = d >> s                                                       # (arithmetic: numpy shifts signed integers so)
    if mutant != "H263MI_MUTATE_BG_STEP_FLOOR":
        step = np.where((step == 0) & (d != 0), np.sign(d), step)
    return b + step


def call(state, cur, prm, valid=None, cut=None, cut_count=0, mutant=None):
    """One call over the state buffer (changed in place).  cur: (n, h, w) uint8.
    -> (fg (n, h, w) bool, grid (n, gh, gw) int64, summaries [(sad, changed_cells, max_cell_sad)], selected [p])
    mutant: one of the CPU checker's two (mutants.h), to tell which cases it must fail"""
    n, h, w = cur.shape
    valid = [True] * n if valid is None else valid
    fg = np.zeros((n, h, w), bool)
    for p in range(n):
        if not valid[p]:
            continue
        head, words = head_of(state, p, w, h), words_of(state, p, w, h)
        age = int(head[0])
        init = age == 0 or is_cut(p, n, cut, cut_count)
        warm = not init and age < prm.warmup
        c = cur[p].astype(np.int64)
        if init:
            words[:, :w] = c << 7
            words[:, w:] = 0
        else:
            b = words[:, :w].astype(np.int64)
            judged = moved(c, b, prm.learn, mutant) if mutant == "H263MI_MUTATE_BG_JUDGE_AFTER" else b
            r = (judged + 64) >> 7
            if not warm:
                fg[p] = np.abs(c - r) > prm.pix_thr
            words[:, :w] = np.where(fg[p], moved(c, b, prm.fg_learn, mutant), moved(c, b, prm.learn, mutant))
        head[0] = 1 if init else min(age + 1, 0xFFFFFFFF)
        head[1] = VALID | (INIT if init else 0) | (WARM if warm else 0)
        head[2:] = 0
    grid = change_ref.cells(fg.astype(np.uint8), np.zeros_like(fg, np.uint8), prm.c)
    summ = change_ref.summaries(grid, w, h, prm.c, prm.cell_thr, valid)
    return fg, grid, summ, change_ref.select(summ, prm.min_changed, valid)
