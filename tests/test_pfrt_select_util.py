"""CPU: the numpy statement of DRT.select_pfrt_candidates (hipdrt.models.pfrt: rank_peaks, shift_candidate, candidate_corr,
select_compact, select_candidates) against the reference's recorded run (tools/make_pfrt_select_golden.py) and on hand-built rows
for every quirk of upstream's rule (hybdrt/models/pfrt.py:49-213).  quirk_cases() is shared with tests/test_gpu_pfrt_select.py."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

from hipdrt.models import pfrt

DEFAULTS = (0.99, 0.01, 1e-6)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "refrun_pfrt_select.npz"))


def golden_lists(g, c, t):
    """upstream's (target_peak_indices, candidate_indices) of spectrum c at threshold set t, and the winning match_quality"""
    targets = [row[row >= 0] for row in g[f"c{c}_t{t}_targets"]] if len(g[f"c{c}_t{t}_steps"]) else []
    return targets, [int(s) for s in g[f"c{c}_t{t}_steps"]], g[f"c{c}_t{t}_match_quality"]


def same_lists(got, ref):
    return (len(got[0]) == len(ref[0]) and all(np.array_equal(a, b) for a, b in zip(got[0], ref[0]))
            and list(got[1]) == list(ref[1]))


def test_fixture_holds_what_the_tests_rely_on(golden):
    assert len(golden["sources"]) == 2 and golden["thresholds"].shape == (3, 3)
    assert tuple(golden["thresholds"][0]) == DEFAULTS
    assert any(int(golden[f"c{c}_t{t}_num_peaks"]) >= 3 and len(set(golden[f"c{c}_t{t}_steps"])) >= 2
               for c in range(2) for t in range(3))


@pytest.mark.parametrize("t", [0, 1, 2])
@pytest.mark.parametrize("c", [0, 1])
def test_statement_against_the_reference_run(golden, c, t):
    raw, steps, llh = golden[f"c{c}_raw_pfrt"], golden[f"c{c}_step_pfrt"], golden[f"c{c}_step_llh"]
    thr = tuple(golden["thresholds"][t])
    comp = pfrt.select_compact(raw, steps, llh, *thr)
    targets, chosen, quality = golden_lists(golden, c, t)
    assert same_lists(pfrt.candidates_from_compact(comp), (targets, chosen))
    assert same_lists(pfrt.select_candidates(raw, steps, llh, *thr), (targets, chosen))
    assert comp["num_peaks"] == int(golden[f"c{c}_t{t}_num_peaks"]) and comp["num_candidates"] == len(chosen)
    np.testing.assert_allclose(comp["match_quality"], quality, rtol=1e-12, atol=0, equal_nan=True)
    assert comp["magnitude"][0] == 1.0 and (np.diff(comp["magnitude"]) < 0).all()


def rows(n, entries):
    r = np.zeros(n)
    for i, v in entries.items():
        r[i] = v
    return r


def quirk_cases():
    """name -> (raw, steps (S, n), llh (S,), thresholds, expected): expected is (targets, chosen steps) worked out by hand, or
    ValueError.  Every value is a small binary fraction, so areas and magnitudes are exact."""
    cases = {}
    # a range that starts at index 0 has area 0 (upstream's pf[-1:end + 1] is empty): ranked last, below end_thresh
    raw = rows(10, {0: 0.5, 1: 0.75, 4: 0.5, 7: 0.25})
    steps = np.array([rows(10, {1: 1.0, 4: 0.5}), rows(10, {4: 1.0}), rows(10, {4: 1.0, 7: 0.5})])
    cases["range_at_index_0"] = (raw, steps, np.array([-3.0, -2.0, -2.5]), DEFAULTS, ([[4], [4, 7]], [0, 0]))
    # an entry one past a range's end (index 5 after the range [3, 5)) moves to the range's peak at 4; the entry at 6 stays
    raw = rows(12, {3: 0.25, 4: 0.5, 9: 0.25})
    steps = np.array([rows(12, {5: 1.0}), rows(12, {6: 1.0}), rows(12, {9: 1.0})])
    cases["one_past_the_end"] = (raw, steps, np.array([2.0, 2.0, 2.0]), DEFAULTS, ([[4]], [0]))
    # two entries of a step inside one range land on its peak: the one at the higher index stays (0.25, not 1)
    raw = rows(12, {2: 0.25, 3: 0.5, 4: 0.25, 9: 0.5})
    steps = np.array([rows(12, {2: 1.0, 4: 0.25, 9: 1.0}), rows(12, {3: 1.0, 9: 0.5})])
    cases["two_entries_on_one_peak"] = (raw, steps, np.array([1.0, 1.0]), DEFAULTS, ([[3]], [1]))
    # an all-zero step has correlation NaN, and np.argmax takes the first NaN whatever the other steps hold
    raw = rows(9, {2: 0.5, 6: 0.25})
    steps = np.array([rows(9, {2: 1.0}), np.zeros(9), rows(9, {2: 1.0}), np.zeros(9)])
    cases["all_zero_step"] = (raw, steps, np.array([5.0, 1.0, 7.0, 1.0]), DEFAULTS, ([[2]], [1]))
    # equal areas: the higher index ranks first (np.argsort(...)[::-1])
    raw = rows(12, {2: 0.5, 5: 0.5, 9: 0.25})
    steps = np.array([rows(12, {2: 1.0}), rows(12, {5: 1.0}), rows(12, {2: 1.0, 5: 1.0})])
    cases["equal_areas"] = (raw, steps, np.array([1.0, 1.0, 1.0]), (0.99, 0.01, 1e-6), ([[5, 2]], [2]))
    # one peak: nothing to choose between
    cases["one_peak"] = (rows(8, {3: 0.5, 4: 0.25}), np.array([rows(8, {3: 1.0})]), np.array([1.0]), DEFAULTS, ([], []))
    # end_thresh stops the loop before the fourth peak joins a target: four peaks, two candidates (not three)
    raw = rows(16, {2: 1.0, 6: 0.5, 10: 0.125, 13: 0.0625})
    steps = np.array([rows(16, {2: 1.0}), rows(16, {2: 1.0, 6: 1.0}), rows(16, {2: 1.0, 6: 1.0, 10: 1.0})])
    cases["end_thresh_stops_early"] = (raw, steps, np.array([1.0, 1.0, 1.0]), (0.99, 0.25, 1e-6), ([[2], [2, 6]], [0, 1]))
    # nothing at or above peak_thresh
    cases["no_peak"] = (rows(8, {3: 0.5}), np.array([rows(8, {3: 1.0})]), np.array([1.0]), (0.99, 0.01, 0.75), ValueError)
    return cases


@pytest.mark.parametrize("name", list(quirk_cases()))
def test_quirks_on_hand_built_rows(name):
    raw, steps, llh, thr, expected = quirk_cases()[name]
    if expected is ValueError:
        with pytest.raises(ValueError, match="peak_thresh"):
            pfrt.select_candidates(raw, steps, llh, *thr)
        return
    got = pfrt.select_candidates(raw, steps, llh, *thr)
    assert same_lists(got, expected), got


def test_the_pieces_one_by_one():
    raw = rows(10, {0: 0.5, 1: 0.75, 4: 0.5, 7: 0.25})
    idx, area = pfrt.rank_peaks(raw, 1e-6)
    assert list(idx) == [4, 7, 1] and list(area) == [0.5, 0.25, 0.0]
    # a row of a single point is one range at index 0: pf[-1:2] is that one sample and the area 0
    assert list(pfrt.rank_peaks(np.array([0.5]), 1e-6)[1]) == [0.0]
    # equal areas, more of them than numpy's insertion sort ever sees: still the higher index first
    many = np.zeros(80)
    many[1::4] = 0.5
    assert list(pfrt.rank_peaks(many, 1e-6)[0]) == list(range(1, 80, 4))[::-1]
    ranges, pk = pfrt.get_peak_ranges(raw, 1e-6), pfrt.identify_peaks(raw, 1e-6)
    sh = pfrt.shift_candidate(rows(10, {0: 0.25, 2: 0.5, 3: 1.0, 5: 0.125, 8: 0.0625, 9: 0.75}), ranges, pk)
    # 0 and 2 (one past [0, 2)) land on 1, the higher index winning; 3 stays; 5 (one past [4, 5)) -> 4; 8 (one past [7, 8)) -> 7
    assert list(sh) == list(rows(10, {1: 0.5, 3: 1.0, 4: 0.125, 7: 0.0625, 9: 0.75}))
    t = np.zeros(10)
    t[[1, 4]] = 1.0
    np.testing.assert_allclose(pfrt.candidate_corr([1, 4], sh), np.corrcoef(t, sh)[0, 1], rtol=1e-14)
    assert np.isnan(pfrt.candidate_corr([1, 4], np.zeros(10)))
    assert pfrt.candidate_corr([1, 4], 0.5 * t) == 1.0
