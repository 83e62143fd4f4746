"""Generate the Kramers-Kronig fixtures under tests/golden/ (build container only: imports the reference through the shims of
oracle/refshim, like oracle/make_golden.py):

  refrun_kk_stats.npz     residual vectors with the outputs of the reference's kk.get_outliers / kk.get_limits, and bare masks
                          with kk.get_limits' outputs (hybdrt/models/kk.py:21-123)
  refrun_kk_test_41.npz   DRT.kk_test(n_iter=2) (hybdrt/models/drt1d.py:1370-1391) on six spectra of 41 frequencies, every pass
                          recorded: residuals, std, outlier indices, limits, trimmed data

Margin condition: a case is accepted only if, in every outlier iteration of every pass, no point has
|ln prob - ln p_thresh| < 0.2 (n_sigma form: |ln(|e| / (n_sigma std))| < 0.2).  A residual that differs at rounding level can then
not flip a mask, so the tests compare masks and limits exactly.

    python tools/make_kk_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle", "refshim"))
import oracle_boot  # noqa: E402,F401

from hybdrt.models import DRT, kk  # noqa: E402
from hybdrt.utils import eis, stats  # noqa: E402

from hipdrt import synth  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
MARGIN = 0.2


def outlier_pass(err, n_iter, p_thresh, n_sigma, fraction):
    """kk.get_outliers iteration by iteration with the reference's own functions -> (std of the last iteration, smallest margin)"""
    mask = np.zeros(len(err), dtype=bool)
    std, margin = np.nan, np.inf
    for _ in range(n_iter):
        std = stats.robust_std(eis.complex_vector_to_concat(err[~mask]), sample_fraction=fraction)
        with np.errstate(divide="ignore"):
            if n_sigma is None:
                dist = np.abs(-np.abs(err) ** 2 / (2 * std ** 2) - np.log(p_thresh))
                mask = stats.outer_cdf_chi2(np.abs(err) ** 2, scale=std ** 2, k=2) < p_thresh
            else:
                dist = np.abs(np.log(np.abs(err) / (n_sigma * std)))
                mask = np.abs(err) > std * n_sigma
        margin = min(margin, float(np.min(dist)))
    return std, margin


def limits(freq, outliers, max_num_outliers):
    """(status, f_lim, i_lim) of kk.get_limits; status 1 = the reference raises IndexError"""
    try:
        (f_min, f_max), (i_left, i_right) = kk.get_limits(freq, outliers, max_num_outliers=max_num_outliers, return_index=True)
    except IndexError:
        return 1, np.array([np.nan, np.nan]), np.array([-1, -1])
    return 0, np.array([f_min, f_max]), np.array([int(i_left), int(i_right)])


def residuals_for(nf, positions, rng, clean_scale=0.2, size=12.0):
    """noise of `clean_scale` percent with large residuals planted at `positions` (signs and parts alternate)"""
    err = clean_scale * (rng.standard_normal(nf) + 1j * rng.standard_normal(nf))
    for i, k in enumerate(positions):
        err[k] = size * clean_scale * (1, -1, 1j, -1j)[i % 4] * (1 + 0.3 * rng.random())
    return err


def make_stats():
    out, cases = {}, []

    def add(name, freq, err, n_iter=2, p_thresh=1e-4, n_sigma=None, fraction=0.6, max_out=2, expect=None):
        std, margin = outlier_pass(err, n_iter, p_thresh, n_sigma, fraction)
        if margin < MARGIN:
            return False
        outl = kk.get_outliers(err, n_iter, p_thresh, n_sigma=n_sigma, std_sample_fraction=fraction)
        if expect is not None and not np.array_equal(outl, np.sort(expect)):
            return False
        status, f_lim, i_lim = limits(freq, outl, max_out)
        i = len(cases)
        cases.append(name)
        out[f"c{i}_freq"], out[f"c{i}_err"] = freq, err
        out[f"c{i}_opts"] = np.array([n_iter, p_thresh, -1.0 if n_sigma is None else n_sigma, fraction, max_out], dtype=float)
        out[f"c{i}_outliers"], out[f"c{i}_std"] = outl.astype(np.int64), np.float64(std)
        out[f"c{i}_status"], out[f"c{i}_flim"], out[f"c{i}_ilim"] = np.int64(status), f_lim, i_lim.astype(np.int64)
        out[f"c{i}_margin"] = np.float64(margin)
        return True

    def add_retry(name, nf, positions, ascending, seed0, **kw):
        for seed in range(seed0, seed0 + 200):
            freq = np.logspace(5, -1, nf)
            if ascending:
                freq = freq[::-1].copy()
            err = residuals_for(nf, positions, np.random.default_rng(seed))
            if add(f"{name}_nf{nf}_{'asc' if ascending else 'desc'}", freq, err, expect=np.asarray(positions, dtype=int), **kw):
                return
        raise RuntimeError(f"no seed gives case {name} nf={nf} the margin")

    seed0 = 0
    for nf in (3, 7, 41, 64):
        for asc in (False, True):
            patterns = {"none": [], "first": [0], "last": [nf - 1]}
            if nf >= 7:
                patterns["adjacent"] = [nf // 2, nf // 2 + 1]
            if nf >= 41:
                patterns["trim_mo0"] = [8, 9, 20, 31]
                patterns["trim_mo2"] = [6, 12, 18, 24, 30]
                patterns["tie_mo1"] = [10, nf - 1 - 10]
                patterns["ends_and_inside"] = [0, 1, 15, nf - 2]
            for name, pos in patterns.items():
                kw = {}
                if name == "trim_mo0":
                    kw["max_out"] = 0
                if name == "tie_mo1":
                    kw["max_out"] = 1
                add_retry(name, nf, pos, asc, seed0, **kw)
                seed0 += 200
            if nf >= 7:
                add_retry("n_sigma", nf, [2, nf - 3], asc, seed0, n_sigma=4.0)
                seed0 += 200
                add_retry("one_iteration", nf, [3], asc, seed0, n_iter=1)
                seed0 += 200
    # no clean point: every third frequency is an outlier (purely real / imaginary, alternating signs: 1/6 of the sample)
    for nf in (7, 41):
        for asc in (False, True):
            add_retry("no_clean_point", nf, list(range(1, nf, 3)), asc, seed0)
            seed0 += 200
    # the branches the fixture must hold
    names = cases
    taken = {n: int(out[f"c{i}_status"]) for i, n in enumerate(names)}
    assert any(v == 1 for n, v in taken.items() if n.startswith("no_clean_point"))
    for i, n in enumerate(names):
        if n.startswith(("trim_", "tie_")):           # the window was cut: it is narrower than first-to-last clean point
            o = np.zeros(len(out[f"c{i}_freq"]), dtype=int)
            order = np.argsort(out[f"c{i}_freq"])[::-1]
            mask = np.zeros(len(o), dtype=bool)
            mask[out[f"c{i}_outliers"]] = True
            o = mask[order].astype(int)
            pad = np.concatenate([o[:1], o, o[-1:]])
            clean = np.where(pad[:-2] + pad[1:-1] + pad[2:] == 0)[0]
            assert o[clean[0]:clean[-1]].sum() > out[f"c{i}_opts"][4], n
            assert tuple(out[f"c{i}_ilim"]) != (clean[0], clean[-1]), n
    out["case_names"] = np.array(names)

    # bare masks for get_limits
    rng = np.random.default_rng(77)
    nm = 0
    for t in range(60):
        nf = int(rng.choice([3, 7, 41, 64]))
        freq = np.logspace(5, -1, nf)
        if t % 2:
            freq = freq[::-1].copy()
        mask = rng.random(nf) < rng.choice([0.05, 0.15, 0.3, 0.6])
        mo = int(rng.integers(0, 3))
        status, f_lim, i_lim = limits(freq, np.where(mask)[0], mo)
        out[f"m{nm}_freq"], out[f"m{nm}_mask"], out[f"m{nm}_maxout"] = freq, mask, np.int64(mo)
        out[f"m{nm}_status"], out[f"m{nm}_flim"], out[f"m{nm}_ilim"] = np.int64(status), f_lim, i_lim.astype(np.int64)
        nm += 1
    out["num_masks"] = np.int64(nm)
    np.savez_compressed(os.path.join(GOLDEN, "refrun_kk_stats.npz"), **out)
    print(f"refrun_kk_stats.npz: {len(names)} residual cases, {nm} masks; smallest margin "
          f"{min(float(out[f'c{i}_margin']) for i in range(len(names))):.3f}")


def perturbed_spectrum(freq, seed, drift=False):
    """zarc2 spectrum with a few points off by about 5 %, or with a low-frequency drift instead"""
    z = synth.zarc2_spectrum(freq, seed, jitter=True)
    rng = np.random.default_rng(500 + seed)
    if drift:
        drift = np.clip(np.log10(1.0 / freq) + 0.2, 0, None)        # grows below ~1.6 Hz
        return z * (1 + 0.04 * drift)
    for k in rng.choice(len(freq), size=int(rng.integers(2, 6)), replace=False):
        z[k] *= 1 + 0.05 * (rng.choice([-1, 1]) + 0.3 * rng.standard_normal()) * np.exp(1j * rng.uniform(-0.5, 0.5))
    return z


def run_kk_test(freq, z, n_iter=2):
    """DRT.kk_test(n_iter, show_plot=False) spelled out pass by pass -> list of per-pass records, or None (margin)"""
    drt = DRT()
    passes, outl = [], None
    for _ in range(n_iter):
        drt.kk_fit(freq, z, outlier_index=outl)
        err = drt.eval_kk_residuals()
        std, margin = outlier_pass(err, 2, 1e-4, None, 0.6)
        if margin < MARGIN:
            return None, margin
        outl = drt.get_kk_outliers()
        status, f_lim, i_lim = limits(drt.get_fit_frequencies(), outl, 2)
        assert status == 0
        f_clean, z_clean = kk.trim_data(freq, z, f_lim[0], f_lim[1])
        passes.append(dict(err=err, std=std, outliers=outl, flim=f_lim, ilim=i_lim, f_clean=f_clean, z_clean=z_clean,
                           margin=margin, n=len(drt.fit_parameters["x"]) + 2,
                           outer=drt.qphb_params.get("outer_iterations", -1) if hasattr(drt, "qphb_params") else -1))
    return passes, min(p["margin"] for p in passes)


def make_kk_test():
    freq = np.logspace(6, -1, 41)
    out = {"freq": freq}
    members, seed, cut = 0, 0, 0
    while members < 6:
        z = perturbed_spectrum(freq, seed, drift=members == 3)          # the fourth member drifts
        passes, margin = run_kk_test(freq, z)
        if passes is None:
            print(f"seed {seed}: refused, margin {margin:.3f}")
            seed += 1
            continue
        b = members
        out[f"s{b}_seed"], out[f"s{b}_z"], out[f"s{b}_drift"] = np.int64(seed), z, np.int64(members == 3)
        for i, p in enumerate(passes):
            pre = f"s{b}_p{i}_"
            out[pre + "err"], out[pre + "std"], out[pre + "outliers"] = p["err"], np.float64(p["std"]), p["outliers"].astype(np.int64)
            out[pre + "flim"], out[pre + "ilim"] = p["flim"], p["ilim"].astype(np.int64)
            out[pre + "f_clean"], out[pre + "z_clean"], out[pre + "margin"] = p["f_clean"], p["z_clean"], np.float64(p["margin"])
        # was the window of the last pass cut by the trimming branch?  (more than max_num_outliers between the outer clean points)
        last = passes[-1]
        mask = np.zeros(len(freq), dtype=int)
        mask[last["outliers"]] = 1
        pad = np.concatenate([mask[:1], mask, mask[-1:]])
        clean = np.where(pad[:-2] + pad[1:-1] + pad[2:] == 0)[0]
        trimmed = mask[clean[0]:clean[-1]].sum() > 2
        cut += int(trimmed)
        print(f"seed {seed}: member {b}, n = {passes[0]['n']}, margins {[round(p['margin'], 3) for p in passes]}, "
              f"outliers {[p['outliers'].tolist() for p in passes]}, limits {last['flim']}, trimming branch {bool(trimmed)}")
        assert passes[0]["n"] == 113
        members += 1
        seed += 1
    assert cut >= 1, "no member whose window is cut by the trimming branch"
    out["num_spectra"], out["num_passes"] = np.int64(6), np.int64(2)
    np.savez_compressed(os.path.join(GOLDEN, "refrun_kk_test_41.npz"), **out)


if __name__ == "__main__":
    if "--only-kk-test" not in sys.argv:
        make_stats()
    make_kk_test()
