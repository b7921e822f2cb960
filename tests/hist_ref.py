"""The numpy reference of the plane histograms (include/h263mi.h, PLANE HISTOGRAMS): np.bincount per picture, everything behind it in
Python integers -- nothing here can wrap."""
import numpy as np


def histograms(planes):
    """(n, H, W) uint8 -> (n, 256) int64"""
    return np.stack([np.bincount(p.reshape(-1), minlength=256) for p in planes]).astype(np.int64)


def pctl(hist, q, pixels):
    """the smallest v with C(v) >= 1 and 1000 * C(v) >= q * P"""
    cum = 0
    for v in range(256):
        cum += int(hist[v])
        if cum >= 1 and 1000 * cum >= q * pixels:
            return v
    raise AssertionError("a histogram of P pixels reaches every percentile")


def distance(hist, prev):
    return sum(abs(int(a) - int(b)) for a, b in zip(hist, prev))


def stats(hist, prev, lo_permille, hi_permille):
    """-> (sum, sum_sq, distance, min, max, p_lo, p_hi, mode) of one picture; prev None: distance 0"""
    h = [int(x) for x in hist]
    pixels = sum(h)
    present = [v for v in range(256) if h[v]]
    most = max(h)
    return (sum(v * h[v] for v in range(256)), sum(v * v * h[v] for v in range(256)), distance(h, prev) if prev is not None else 0,
            present[0], present[-1], pctl(h, lo_permille, pixels), pctl(h, hi_permille, pixels), h.index(most))


def is_cut(dist, cut_permille, pixels):
    return dist * 1000 > cut_permille * 2 * pixels


ZERO_STATS = (0, 0, 0, 0, 0, 0, 0, 0)


def select(all_stats, cut_permille, pixels, valid):
    return [p for p, s in enumerate(all_stats) if valid[p] and is_cut(s[2], cut_permille, pixels)]
