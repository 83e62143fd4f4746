"""Rewrite tests/map_badness_bounds.json: per label of tests/test_gpu_map_badness.py the derived bound (cols + c) 2^-52 on the
relative deviation of a row's rss from the reference's, and the deviation measured on the GPU (taken from the lines
"map_badness <label>: measured <x> bound <y>" that the tests print; null until a run is given).

A row's rss is sum_c r_c^2 / cols with r_c = nan_to_num((a - filt) / (iqr / 1.349 + 0.1 robust_std)).  Either side adds cols
non-negative terms in some order: at most (cols - 1) 2^-53 relative each, less than cols 2^-52 between them.  c counts the other
roundings, once for either side at 2^-53 each, i.e. 2^-52 a rounding between them:
    the term: hi - lo of the IQR, / 1.349, 0.1 * robust_std, their sum, a - filt, the division, the square             7
    the division of the sum by cols                                                                                   1
    the data score only: hi + lo, 0.5 *, a - mid, / range of the scaling (drtmd.py:675-679), and 0.5 * (v + z)        6
The device's exp enters the outlier flags only, which are compared exactly (the fixture keeps every p_out 1e-9 from thresh).

    python tools/update_map_badness_bounds.py [pytest-output.txt]
"""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# label -> (cols of the widest array summed, c)
LABELS = {"chain.a23.rss": (37, 8), "chain.a70.rss": (130, 8), "fit.badness": (91, 8), "data.hybrid.badness": (200, 14),
          "data.mixed.badness": (200, 14)}


def main(path=None):
    measured = {}
    if path:
        for m in re.finditer(r"map_badness (\S+): measured (\S+) bound", open(path).read()):
            measured[m.group(1)] = max(float(m.group(2)), measured.get(m.group(1), 0.0))
    table = {k: {"cols": cols, "c": c, "bound": (cols + c) * 2.0 ** -52, "measured": measured.get(k)}
             for k, (cols, c) in LABELS.items()}
    with open(os.path.join(ROOT, "tests", "map_badness_bounds.json"), "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    for k, v in table.items():
        print(k, v)


if __name__ == "__main__":
    main(*sys.argv[1:2])
