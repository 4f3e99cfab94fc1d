"""BRIEF test-pair tables ({y1, x1, y2, x2}, int8 [256, 4], |.| <= 24) at which a footprint table (csrc/brief_footprint.h) can go wrong:
empty rows, a single-chunk row, a full-width row, an alignment spill at both ends.  tests/cpp/test_brief_footprint.cpp checks the same
shapes against a brute-force scan on the host; here they are the patterns the GPU recovery runs under."""
import numpy as np

EXTREMES = [(-24, -24), (-24, 24), (24, -24), (24, 24), (-24, 0), (24, 0), (0, -24), (0, 24)]   # (y, x)


def _random(seed):
    return np.random.default_rng(seed).integers(-24, 25, size=(256, 4)).astype(np.int8)


def extremes(seed=21):
    """taps at the eight extreme positions (+-24, +-24), (+-24, 0), (0, +-24), the other taps random"""
    p = _random(seed)
    p[:4] = np.array(EXTREMES, np.int8).reshape(4, 4)
    return p


def row0(seed=22):
    """all taps in row 0, columns spanning -24 .. 24: one full-width row, every other row empty"""
    p = _random(seed)
    p[:, 0] = p[:, 2] = 0
    p[0, 1], p[0, 3] = -24, 24
    return p


def column0(seed=23):
    """all taps in column 0: every row a single element"""
    p = _random(seed)
    p[:, 1] = p[:, 3] = 0
    p[0, 0], p[0, 2] = -24, 24
    return p


def rows_pm24(seed=24):
    """taps only in rows -24 and +24, empty rows between them"""
    p = _random(seed)
    p[:, 0], p[:, 2] = -24, 24
    return p


def uniform(seed=25):
    """uniformly random taps over +-24"""
    return _random(seed)


# name -> table; None = the library's built-in pattern (whatever get_pattern returns before anything was set)
PATTERNS = {"built-in": None, "extremes": extremes(), "row 0": row0(), "column 0": column0(), "rows -24 and +24": rows_pm24(), "random": uniform()}
