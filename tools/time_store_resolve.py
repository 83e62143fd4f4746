"""Wall time of DRTMD.resolve_group on the store (coupled QPs assembled on the device, csrc/resolve.hip) against the host-assembled
path (DRT.batch_fits() downloads every member's P, mapping.resolve.resolve_group builds every coupled P in numpy and uploads it) on
the same fitted batch of 16 joint observations.  Every timed piece ends with its results on the host, i.e. behind a device
synchronisation.  The two paths alternate, after one untimed round of each.

    python tools/time_store_resolve.py [--grid 121|512] [--rounds 5] [--out FILE]

--grid 121: the 121-point supergrid of tests/golden/refrun_resolve_group_hybrid16.npz (about 100 unknowns per member, coupled
problems of about 700); --grid 512: the 512-point basis of tests/golden/refrun_resolve_c2grid.npz (514 unknowns per member, coupled
problems of 3598: the group kernel)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hipdrt import synth  # noqa: E402
from hipdrt.mapping import DRTMD, resolve  # noqa: E402


def build_store(grid, n_obs=16):
    if grid == 512:
        basis = np.load(os.path.join(ROOT, "tests", "golden", "refrun_resolve_c2grid.npz"))["basis_tau"]
        md = DRTMD(basis, psi_dim_names=["T"], warn=False, fixed_basis_tau=basis)
    else:
        md = DRTMD(np.logspace(-8, 4, 121), psi_dim_names=["T"], warn=False)
    for k in range(n_obs):
        m = synth.hybrid_measurement(seed=100 + k, jitter=True, n_post=100 if grid != 512 else 120, nf=31)
        md.add_observation([float(k)], (m[0], m[1], m[2]), (m[3], m[4]), group_id="g")
    return md


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=121)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch-size", type=int, default=7)
    ap.add_argument("--overlap", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    md = build_store(a.grid)
    t_fit, _ = clock(md.fit_all)
    assert md.obs_fit_status.all()
    index = md.get_group_index("g")
    tau_idx = [md.obs_tau_indices[i] for i in index]
    nsup = len(md.tau_supergrid)
    bs, starts = resolve.group_batch_starts(len(index), a.batch_size, a.overlap)
    times = dict(store_total=[], refit=[], device_solve=[], host_download=[], host_solve=[])
    x_dev = x_host = None
    for r in range(a.rounds + 1):
        t_total, _ = clock(lambda: md.resolve_group("g", batch_size=a.batch_size, overlap=a.overlap, psi_sort_dims=["T"]))
        x_dev = md.obs_x_resolved.copy()
        # the pieces of the same call, on their own
        t_refit, (plan, members) = clock(lambda: md._refit_members(index))
        t_dev, sol = clock(lambda: resolve.resolve_batches_on_plan(plan, members, tau_idx, True, starts, bs))
        its_dev = sol[3]
        # the host-assembled path on the plan the refit left
        t_down, fits = clock(md.drt1d.batch_fits)
        t_host, (x_host, _) = clock(lambda: resolve.resolve_group(fits, tau_idx, True, nsup, batch_size=a.batch_size, overlap=a.overlap))
        assert its_dev == resolve.resolve_group.last_qp["iterations"], (its_dev, resolve.resolve_group.last_qp)
        if r:                                   # round 0 warms every shape up
            for key, v in zip(times, (t_total, t_refit, t_dev, t_down, t_host)):
                times[key].append(v)
    dev = float(np.abs(x_dev - x_host).max() / np.abs(x_host).max())
    n_member = int(tau_idx[0][1] - tau_idx[0][0]) + 2
    res = dict(grid=a.grid, observations=len(index), batch_size=bs, batches=len(starts), unknowns_per_member=n_member,
               unknowns_per_problem=bs * n_member, qp_iterations=its_dev, fit_all_s=t_fit, deviation=dev,
               seconds={k: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v))) for k, v in times.items()})
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
