"""Generate the candidate-selection fixture under tests/golden/ (build container only: imports the reference through the shims of
oracle/refshim, like tools/make_pfrt_golden.py):

  refrun_pfrt_select.npz   two spectra through the reference's DRT.pfrt_fit_eis, DRT.predict_pfrt and DRT.select_pfrt_candidates
                           (hybdrt/models/drt1d.py:2860-2865 over hybdrt/models/pfrt.py:164-213) at three threshold sets
                           (start_thresh, end_thresh, peak_thresh): the defaults, (0.5, 0.1, 1e-6) and (0.99, 1e-4, 1e-3).  Per
                           spectrum c: c{c}_freq, c{c}_z, c{c}_factors, c{c}_tau_pfrt, c{c}_raw_pfrt, c{c}_step_pfrt, c{c}_step_llh;
                           per threshold set t upstream's two lists as c{c}_t{t}_targets (one row per candidate, padded with
                           -1), c{c}_t{t}_steps, and c{c}_t{t}_match_quality, the winning corr * llh of every target.

Spectra are tried in a fixed order: the reference's 71-frequency known-answer spectrum (tests/golden/ref_test_drt_fit_eis.npz),
then three-arc spectra of seeds 0, 1, 2, ... on the same frequencies: hipdrt.synth.zarc2_spectrum(seed, **TWO_ARCS) plus a third
ZARC (THIRD_ARC) -- broad arcs under 2 % noise, so that the peaks' probabilities stay below one (three sharp arcs give three
areas of exactly 1 and nothing to rank).  The first two that satisfy every condition below are kept; `sources` records which (-1: the known-answer
spectrum, else the seed).

Conditions on the reference's own values without which the spectrum is passed over -- at one threshold set at least 3 ranked peaks
and at least two distinct chosen steps, and at every threshold set:
  * no raw_pfrt value in [0.5, 2] x peak_thresh;
  * the two largest values of every range differ by more than 1e-6 relative;
  * consecutive magnitudes differ by more than 1e-6 relative;
  * no magnitude within 1e-6 relative of start_thresh or end_thresh;
  * for every target the best and the second-best match_quality differ by more than 1e-6 of the larger magnitude (a target whose
    match_quality holds a NaN is won by the first NaN, which an all-zero row gives whatever the rounding).

    python tools/make_pfrt_select_golden.py
"""
import contextlib
import io
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle", "refshim"))
import oracle_boot  # noqa: E402,F401

from hybdrt.models import DRT  # noqa: E402
from hybdrt.models import pfrt as ref_pfrt  # noqa: E402

from hipdrt import synth  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
CTOR = dict(fit_inductance=True, fit_capacitance=False, fit_dop=False, fit_ohmic=True)
THRESHOLDS = ((0.99, 0.01, 1e-6), (0.5, 0.1, 1e-6), (0.99, 1e-4, 1e-3))
TWO_ARCS = dict(sigma=0.02, beta1=0.7, beta2=0.7)
THIRD_ARC = dict(r=0.1, tau=1e-5, beta=0.7)
REL = 1e-6
MAX_SEEDS = 40


@contextlib.contextmanager
def quiet():
    with warnings.catch_warnings(), contextlib.redirect_stdout(io.StringIO()):
        warnings.simplefilter("ignore")
        yield


def three_arc(freq, seed):
    jw = 1j * 2 * np.pi * np.asarray(freq, dtype=float)
    return synth.zarc2_spectrum(freq, seed=seed, **TWO_ARCS) + THIRD_ARC["r"] / (1 + (jw * THIRD_ARC["tau"]) ** THIRD_ARC["beta"])


class PassedOver(Exception):
    """a condition of the module docstring does not hold"""


def apart(a, b):
    return abs(a - b) > REL * max(abs(a), abs(b))


def check(raw, steps, llh, start, end, thr):
    """(targets, chosen steps, winning match_quality, number of ranked peaks); PassedOver when a condition fails"""
    if ((raw >= 0.5 * thr) & (raw <= 2 * thr)).any() or not (raw >= thr).any():
        raise PassedOver(f"a raw_pfrt value within [0.5, 2] x {thr}, or none above it")
    ranges = ref_pfrt.get_peak_ranges(raw, thr)
    peak_idx = ref_pfrt.identify_peaks(raw, thr)
    for s, e in zip(*ranges):
        v = np.sort(raw[s:e])[::-1]
        if len(v) > 1 and not apart(v[0], v[1]):
            raise PassedOver(f"range {s}:{e} has two equal largest values")
    ranked, mag = ref_pfrt.rank_peaks(raw, thr)
    mag = mag / np.max(mag)
    if any(not apart(mag[i], mag[i + 1]) for i in range(len(mag) - 1)):
        raise PassedOver(f"two consecutive magnitudes too close: {mag}")
    if any(not apart(m, t) for m in mag for t in (start, end)):
        raise PassedOver(f"a magnitude on a threshold: {mag}")
    with quiet():
        targets, chosen = ref_pfrt.select_candidates(raw, steps, llh, start, end, thr)
    shifted = [ref_pfrt.shift_candidate_pfrt(c, tot_peak_ranges=ranges, tot_peak_indices=peak_idx) for c in steps]
    quality = []
    for t, c in zip(targets, chosen):
        with np.errstate(invalid="ignore", divide="ignore"):
            mq = np.array([ref_pfrt.candidate_corr(t, sh) * l for sh, l in zip(shifted, llh)])
        assert int(np.argmax(mq)) == int(c)
        if not np.isnan(mq).any():
            srt = np.sort(mq)[::-1]
            if len(srt) > 1 and not abs(srt[0] - srt[1]) > REL * max(abs(srt[0]), abs(srt[1])):
                raise PassedOver(f"target {list(t)}: best and second-best match_quality too close: {srt[:2]}")
        quality.append(mq[int(c)])
    return targets, [int(c) for c in chosen], np.array(quality, dtype=float), len(mag)


def run(freq, z):
    with quiet():
        drt = DRT(**CTOR)
        drt.pfrt_fit_eis(freq, z)
        drt.predict_pfrt()
        pr = drt.pfrt_result
        raw, steps = np.array(pr["raw_pfrt"], dtype=float), np.array(pr["step_pfrt"], dtype=float)
        llh, factors = np.array(pr["step_llh"], dtype=float), np.array(pr["factors"], dtype=float)
        own = [drt.select_pfrt_candidates(*t) for t in THRESHOLDS]
    sets = []
    for t, (own_targets, own_steps) in zip(THRESHOLDS, own):
        got = check(raw, steps, llh, *t)
        assert [list(a) for a in got[0]] == [list(a) for a in own_targets] and got[1] == [int(c) for c in own_steps]
        sets.append(got)
    if not any(n >= 3 and len(set(ch)) >= 2 for (_, ch, _, n) in sets):
        raise PassedOver(f"(ranked peaks, chosen steps) {[(n, ch) for (_, ch, _, n) in sets]}: nowhere 3 peaks and two distinct steps")
    return dict(freq=np.asarray(freq, dtype=float), z=np.asarray(z, dtype=complex), factors=factors,
                tau_pfrt=np.array(pr["tau_pfrt"], dtype=float), raw_pfrt=raw, step_pfrt=steps, step_llh=llh), sets


def main():
    g = np.load(os.path.join(GOLDEN, "ref_test_drt_fit_eis.npz"))
    freq = np.asarray(g["freq"], dtype=float)
    tries = [(-1, np.asarray(g["z"], dtype=complex))] + [(s, None) for s in range(MAX_SEEDS)]
    kept = []
    for source, z in tries:
        z = three_arc(freq, source) if z is None else z
        try:
            got = run(freq, z)
        except PassedOver as why:
            print("source", source, "passed over:", why)
            continue
        print("source", source, "kept: (ranked peaks, chosen steps)", [(n, ch) for (_, ch, _, n) in got[1]])
        kept.append((source, got))
        if len(kept) == 2:
            break
    assert len(kept) == 2, "fewer than two spectra satisfy the conditions"
    out = dict(sources=np.array([s for s, _ in kept]), thresholds=np.array(THRESHOLDS),
               two_arcs=np.array([TWO_ARCS["sigma"], TWO_ARCS["beta1"], TWO_ARCS["beta2"]]),
               third_arc=np.array([THIRD_ARC["r"], THIRD_ARC["tau"], THIRD_ARC["beta"]]))
    for c, (_, (arrays, sets)) in enumerate(kept):
        out.update({f"c{c}_{k}": v for k, v in arrays.items()})
        for t, (targets, chosen, quality, n) in enumerate(sets):
            pad = np.full((len(targets), max([len(a) for a in targets] + [1])), -1, dtype=np.int64)
            for j, a in enumerate(targets):
                pad[j, :len(a)] = a
            out.update({f"c{c}_t{t}_targets": pad, f"c{c}_t{t}_steps": np.array(chosen, dtype=np.int64),
                        f"c{c}_t{t}_match_quality": quality, f"c{c}_t{t}_num_peaks": np.int64(n)})
    path = os.path.join(GOLDEN, "refrun_pfrt_select.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < (1 << 20), os.path.getsize(path)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
