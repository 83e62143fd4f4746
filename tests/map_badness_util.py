"""Shared by tests/test_host_map_badness.py, tests/test_gpu_map_badness.py and tools/make_map_badness_golden.py: the inputs of
the percentile cases, built by integer arithmetic so that the fixture records only what numpy answered, and the fixture loader."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refrun_map_badness.npz")

# 16384 is the longest segment the device selects with one workgroup (csrc/map_rank.hip: SEL_BLOCK_LEN)
SEGMENT_LENGTHS = (1, 2, 63, 64, 65, 16383, 16384, 16385)
WHOLE_Q = (0.0, 2.0, 25.0, 50.0, 75.0, 98.0, 100.0, 33.3)
SIZES = ((3, 1), (5, 1), (3, 3), (5, 3), (4, 3), (7, 7))


def segment(n, kind="plain"):
    """n exact doubles: 'plain' a scrambled arithmetic sequence with repeats, 'nan' the same with every 7th entry NaN (from the
    4th), 'equal' one value, 'zeros' a mix of -0, +0 and a few +-1, 'allnan' no number"""
    i = np.arange(n, dtype=np.int64)
    x = ((i * 7919 + 13) % 10007).astype(float) / 8.0 - 600.0
    if kind == "nan":
        x[3::7] = np.nan
    elif kind == "equal":
        x[:] = 1.25
    elif kind == "zeros":
        x = np.where(i % 2 == 0, -0.0, 0.0)
        x[i % 5 == 4] = 1.0
        x[i % 11 == 10] = -1.0
    elif kind == "allnan":
        x[:] = np.nan
    elif kind != "plain":
        raise ValueError(kind)
    return x


def row_case(name):
    """2-D arrays for the by-row percentiles"""
    if name == "r6x65":
        a = np.stack([segment(65, k) for k in ("plain", "nan", "equal", "zeros", "allnan", "nan")])
        a[5, :60] = np.nan
        return a
    if name == "r3x16384":
        return np.stack([segment(16384, "plain"), segment(16384, "nan"), segment(16384, "zeros")])
    if name == "r2x16385":
        return np.stack([segment(16385, "nan"), segment(16385, "plain")[::-1]])
    raise ValueError(name)


ROW_CASES = ("r6x65", "r3x16384", "r2x16385")
ROW_Q = (2.0, 98.0, 25.0, 75.0)


def rank_case(G, key):
    """(input, kind, size) of a recorded rank filter 'rank.<array>.<median|p25|p75|iqr>.<r>x<c>'"""
    _, name, kind, size = key.split(".")
    return G[f"rank.{name}.in"], kind, tuple(int(s) for s in size.split("x"))


def rank_equal(G, key, got):
    """bit for bit against scipy, NaN windows included wherever every rank involved lies strictly inside the window; at rank 0
    or size - 1 scipy switches to its minimum / maximum filter, and there only the windows without a NaN are compared"""
    a, kind, size = rank_case(G, key)
    return rank_rule_equal(a, kind, size, got, G[key])


def rank_rule_equal(a, kind, size, got, ref):
    """the rule of rank_equal for any input a, filter kind and window size, against the reference result ref"""
    from hipdrt.filters import ndfilters
    n = size[0] * size[1]
    ranks = {"median": [n // 2], "p25": [int(n * 25 / 100.0)], "p75": [int(n * 75 / 100.0)],
             "iqr": [int(n * 25 / 100.0), int(n * 75 / 100.0)]}[kind]
    if all(0 < r < n - 1 for r in ranks):
        return np.array_equal(got, ref, equal_nan=True)
    clean = ~np.isnan(ndfilters.window_values(a, list(size))).any(axis=-1)
    return np.array_equal(got[clean], ref[clean]) and bool(clean.any())


def load():
    return np.load(GOLDEN, allow_pickle=False)
