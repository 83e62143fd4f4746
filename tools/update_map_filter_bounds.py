"""Rewrite tests/map_filter_bounds.json: "device" from the record of a GPU run (a JSON file label -> measured deviation of the
device from tests/golden/refrun_map_filter.npz, as tests/test_gpu_map_filter.py prints them), "numpy" from the numpy statement
(hipdrt.filters.ndfilters) measured where this runs against the same fixture.  Every figure is max |difference| / max |reference|.
--measure writes that record on a machine with the GPU: the bodies of tests/test_gpu_map_filter.py with their assertion replaced
by a recorder (nothing is compared with a bound).

bound = the measurement rounded up to the next 1-2-5 step at least 10 x above it, and never below 5e-15: about twenty spacings
of FP64 at the scale of the metric, the level at which one more or one fewer rounding in a sum of a few terms shows (a
measured 0 is one such sum landing the same way, not a promise).

    python tools/update_map_filter_bounds.py --measure measured.json      # on the GPU
    python tools/update_map_filter_bounds.py measured.json                # anywhere (numpy only)
"""
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FLOOR = 5e-15


def bound_for(measured):
    target = max(10.0 * measured, FLOOR)
    decade = 10.0 ** math.floor(math.log10(target))
    for step in (1, 2, 5, 10):
        if step * decade >= target * (1 - 1e-12):
            return float(f"{step * decade:.0e}")


def numpy_figures():
    import test_host_map_filter as t
    fx = t.load_fixture()
    out = {}
    for name in t.CASES:
        for label, (actual, ref) in t.statement_case(fx, name).items():
            out[label] = t.deviation(actual, ref)
    return out


def measure(path):
    import test_gpu_map_filter as t
    record = {}

    def recorder(section, label, actual, ref):
        record[label] = max(t.deviation(actual, ref), record.get(label, 0.0))

    t.check = recorder
    fx = t.load_fixture()
    for name in t.CASES:
        t.test_filter_ndx_matches_the_reference_run(fx, name)
        if "plain" not in name or "adaptive" in name:
            t.test_weights_and_sigmas_match_the_recorded_intermediates(fx, name)
    t.test_reexported_filters_compose_like_the_reference_chain(fx)
    t.test_drtmd_filter_observations_end_to_end()
    with open(path, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
    print(f"wrote {len(record)} figures to {path}")


def main(path):
    with open(path) as f:
        device = json.load(f)
    table = {"device": {k: [float(f"{v:.3g}"), bound_for(v)] for k, v in sorted(device.items())},
             "numpy": {k: [float(f"{v:.3g}"), bound_for(v)] for k, v in sorted(numpy_figures().items())}}
    # "kernels" (tests/test_gpu_map_kernels.py: the adaptive passes against ndfilters, by the same rule) is kept as it stands
    with open(os.path.join(ROOT, "tests", "map_filter_bounds.json")) as f:
        table.update({k: v for k, v in json.load(f).items() if k not in table})
    with open(os.path.join(ROOT, "tests", "map_filter_bounds.json"), "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    for section, rows in table.items():
        for k, (m, b) in rows.items():
            print(f"{section:7s} {k:32s} measured {m:.2e} bound {b:.0e}")


if __name__ == "__main__":
    if sys.argv[1] == "--measure":
        measure(sys.argv[2])
    else:
        main(sys.argv[1])
