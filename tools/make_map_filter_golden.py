"""Generate the map-filter fixture tests/golden/refrun_map_filter.npz (build container only: imports the reference through the
shims of oracle/refshim, like tools/make_peaks_golden.py, and needs scipy).

Every case is one call of the reference's mapping.ndx.filter_ndx (hybdrt/mapping/ndx.py:261-349) with num_group_dims=0 on a
deterministic smooth two-peak surface plus 2 % noise, with one all-NaN row, a few scattered NaNs and one row scaled by 3 (the
outlier the iterated weights must suppress).  Recorded per case: the input, the keywords (JSON), the output and -- for the
iterative cases -- the final weights of iterate_gaussian_weights and, with adaptive=True, the sigma fields the last filter used.

The file is only written when no result hinges on a single rounding:
  - the argument of the ceil that sets the node count of every nonuniform filter is at least 1e-6 from an integer,
  - every rms_filter radicand is exactly 0 or above 1e-10 of its array's maximum,
  - no mask_filt of a masked filter is 0 outside the all-NaN row's neighbourhood (two rows either side).

    python tools/make_map_filter_golden.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle", "refshim"))
import oracle_boot  # noqa: E402,F401

from scipy import ndimage  # noqa: E402
from hybdrt.filters import _filters as rf  # noqa: E402
from hybdrt.mapping import ndx as rndx  # noqa: E402

from hipdrt.filters import ndfilters  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")

# name -> (shape, filter_ndx keywords).  70 rows and 130 columns: more than one tile (32 rows, 64 columns) and wavefront in either axis;
# (3, 5): radius 6 exceeds both lengths; sigma 5: radius 20, past what the device stages in LDS for an axis-0 pass.
CASES = {
    "s3x5": ((3, 5), dict(sigma=(1.5, 0.5))),
    "s23_tau_skipped": ((23, 37), dict(sigma=(1, 0))),
    "s23": ((23, 37), dict(sigma=(1.5, 0.5))),
    "s23_plain": ((23, 37), dict(sigma=(1.5, 0.5), iterative=False)),
    "s23_impute": ((23, 37), dict(sigma=(1.5, 0.5), impute=True)),
    "s23_adaptive": ((23, 37), dict(adaptive=True, max_sigma=(2, 1))),
    "s23_adaptive_plain": ((23, 37), dict(adaptive=True, max_sigma=(2, 1), iterative=False)),
    "s23_wide": ((23, 37), dict(sigma=(5, 0.5))),
    "s70": ((70, 130), dict(sigma=(1.5, 0.5))),
    "s70_plain": ((70, 130), dict(sigma=(1.5, 0.5), iterative=False)),
    "s70_impute": ((70, 130), dict(sigma=(1.5, 0.5), impute=True)),
    "s70_adaptive": ((70, 130), dict(adaptive=True, max_sigma=(2, 1))),
    "v23": ((23,), dict(sigma=(1,))),
}


def surface(shape, seed):
    """two smooth peaks over (psi, ln tau), 2 % noise; returns the array and the index of its all-NaN row (None for 1-D)"""
    rng = np.random.default_rng(seed)
    if len(shape) == 1:
        u = np.linspace(0, 1, shape[0])
        a = np.exp(-((u - 0.3) / 0.12) ** 2) + 0.6 * np.exp(-((u - 0.7) / 0.2) ** 2) + 0.05
        a = a * (1 + 0.02 * rng.standard_normal(shape))
        a[shape[0] // 2] *= 3
        a[[3, shape[0] - 4]] = np.nan
        return a, None
    r, c = shape
    psi, lt = np.meshgrid(np.linspace(0, 1, r), np.linspace(0, 1, c), indexing="ij")
    a = (np.exp(-((lt - 0.3 - 0.1 * psi) / 0.12) ** 2) + (0.4 + 0.5 * psi) * np.exp(-((lt - 0.7) / 0.2) ** 2) + 0.05)
    a = a * (1 + 0.02 * rng.standard_normal(shape))
    nan_row, big_row = (1, 2) if r < 8 else (r // 3, (2 * r) // 3)
    a[big_row] *= 3
    a[nan_row] = np.nan
    for k in range(max(1, r * c // 150)):
        a[(7 * k + 5) % r, (11 * k + 3) % c] = np.nan
    return a, nan_row


class Guards:
    """wrappers round the reference's own functions that check the margins while the reference runs"""

    def __init__(self):
        self.nan_row = None
        self.log = []
        self._nonuniform, self._rms, self._masked = rf.nonuniform_gaussian_filter1d, rf.rms_filter, rf.masked_filter

    def install(self):
        rf.nonuniform_gaussian_filter1d, rf.rms_filter, rf.masked_filter = self.nonuniform, self.rms, self.masked

    def nonuniform(self, a, sigma, *args, **kw):
        if np.max(sigma) > 0:
            sg = np.maximum(sigma, 1e-8)
            arg = ndfilters.sigma_nodes(np.min(sg), np.max(sg))[3]
            assert abs(arg - round(arg)) >= 1e-6, ("node-count ceil argument too close to an integer", arg)
            self.log.append(("ceil", float(arg)))
        return self._nonuniform(a, sigma, *args, **kw)

    def rms(self, a, size, empty=False, **kw):
        a2 = a ** 2
        rad = ndimage.uniform_filter(a2, size, **kw)
        if empty:
            n = size ** np.ndim(a) if np.isscalar(size) else np.prod(size)
            rad -= a2 / n
            rad *= n / (n - 1)
        top = np.max(np.abs(rad))
        bad = (rad != 0) & (np.abs(rad) <= 1e-10 * top)
        assert not bad.any(), ("rms_filter radicand within rounding of 0", rad[bad], top)
        return self._rms(a, size, empty, **kw)

    def masked(self, a, mask, filter_func=None, **filter_kw):
        func = ndimage.gaussian_filter if filter_func is None else filter_func
        mask_filt = func(mask.astype(float), **filter_kw)
        zero_rows = np.unique(np.nonzero(mask_filt == 0)[0])
        if len(zero_rows):
            assert self.nan_row is not None and np.all(np.abs(zero_rows - self.nan_row) <= 2), ("mask_filt == 0", zero_rows)
            self.log.append(("mask_filt zero rows", zero_rows.tolist()))
        return self._masked(a, mask, filter_func, **filter_kw)


def main():
    guards = Guards()
    guards.install()
    out = {}
    names = []
    for name, (shape, kw) in CASES.items():
        a, guards.nan_row = surface(shape, 100 + len(shape) * shape[0])
        guards.log = []
        kw = dict(kw)
        ndx_kw = {k: kw.pop(k) for k in ("iterative", "adaptive", "impute") if k in kw}
        with np.errstate(invalid="ignore", divide="ignore"):
            res = rndx.filter_ndx(a.copy(), 0, **ndx_kw, **kw)
            out[f"{name}_in"], out[f"{name}_out"] = a, res
            if ndx_kw.get("iterative", True):
                nan = np.isnan(a)
                x0 = np.nan_to_num(a)
                adaptive = ndx_kw.get("adaptive", False)
                w = rf.iterate_gaussian_weights(x0, None, adaptive, 2, 5, dev_rms_size=5, nan_mask=nan, **kw)
                out[f"{name}_weights"] = w
                if adaptive:
                    out[f"{name}_sigmas"] = np.stack(rf.get_adaptive_sigmas(x0, empty=False, weights=w, **kw))
            elif ndx_kw.get("adaptive", False):
                out[f"{name}_sigmas"] = np.stack(rf.get_adaptive_sigmas(np.nan_to_num(a), weights=(~np.isnan(a)).astype(float), **kw))
        out[f"{name}_kw"] = np.array(json.dumps(dict(ndx_kw, **kw)))
        names.append(name)
        print(name, shape, dict(ndx_kw, **kw), "nan in/out", int(np.isnan(a).sum()), int(np.isnan(res).sum()), guards.log[:4])
    out["cases"] = np.array(names)
    # an array that repeats an earlier one bit for bit (the shared inputs, the weights impute=True does not change) is stored
    # once: the later key holds the earlier key's name
    seen = {}
    for k in list(out):
        v = out[k]
        if v.dtype.kind != "f" or v.ndim == 0:
            continue
        first = seen.setdefault((v.shape, v.tobytes()), k)
        if first != k:
            out[k] = np.array("=" + first)
    path = os.path.join(GOLDEN, "refrun_map_filter.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
