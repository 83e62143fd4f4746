"""Generate tests/golden/refrun_store_resolve8.npz (build container only: imports the reference through the shims of
oracle/refshim, like tools/make_map_filter_golden.py; cvxopt.solvers.qp is oracle/coneqp.py there).

The reference's own DRTMD (hybdrt/mapping/drtmd.py:186-329, 432-559) on the eight joint observations of
tests/test_gpu_store_resolve.py: add_observation, fit_all, resolve_group('g', batch_size=4, overlap=2, psi_sort_dims=['T']).
Recorded, data only: the observations (times, current, voltage, frequencies, impedance), psi, the tau supergrid, every observation's
tau indices, obs_x, obs_x_resolved, the resolved special parameters and the iteration count of every coupled QP.

    python tools/make_store_resolve_golden.py
"""
import contextlib
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle", "refshim"))
import oracle_boot  # noqa: E402,F401

import cvxopt  # noqa: E402
from hybdrt.mapping.drtmd import DRTMD  # noqa: E402

from hipdrt import synth  # noqa: E402

N_OBS, BATCH_SIZE, OVERLAP = 8, 4, 2
SUPERGRID = np.logspace(-7, 2, 91)


def observations():
    """as tests/test_gpu_store_resolve.py: small_hybrid_store"""
    out = []
    for k in range(N_OBS):
        m = synth.hybrid_measurement(seed=500 + k, jitter=True, n_pre=24, n_post=176, nf=21)
        out.append(([300.0 + 5 * k], (m[0], m[1], m[2]), (m[3], m[4])))
    return out


def main():
    obs = observations()
    with contextlib.redirect_stdout(io.StringIO()):
        dmd = DRTMD(tau_supergrid=SUPERGRID, psi_dim_names=['T'], print_progress=False, warn=False)
        for psi, chrono, eis in obs:
            dmd.add_observation(np.array(psi), chrono, eis, group_id='g')
        dmd.fit_all()
    log = []
    cvxopt.solvers.options["_oracle_log"] = log
    with contextlib.redirect_stdout(io.StringIO()):
        dmd.resolve_group('g', batch_size=BATCH_SIZE, overlap=OVERLAP, psi_sort_dims=['T'])
    cvxopt.solvers.options["_oracle_log"] = None
    out = dict(n_obs=N_OBS, batch_size=BATCH_SIZE, overlap=OVERLAP, tau_supergrid=SUPERGRID,
               psi=np.array([o[0] for o in obs]), times=np.array([o[1][0] for o in obs]), i_signal=np.array([o[1][1] for o in obs]),
               v_signal=np.array([o[1][2] for o in obs]), frequencies=np.array([o[2][0] for o in obs]),
               z=np.array([o[2][1] for o in obs]), obs_tau_indices=np.array(dmd.obs_tau_indices), obs_x=dmd.obs_x,
               obs_x_resolved=dmd.obs_x_resolved, special_names=np.array(sorted(dmd.obs_special_resolved)),
               qp_iterations=np.array([entry["iterations"] for entry in log]))
    for key, val in dmd.obs_special_resolved.items():
        out[f"{key}_resolved"] = np.asarray(val)
    path = os.path.join(ROOT, "tests", "golden", "refrun_store_resolve8.npz")
    np.savez_compressed(path, **out)
    print(f"store_resolve8: {N_OBS} obs, tau indices {sorted(set(map(tuple, out['obs_tau_indices'].tolist())))}, "
          f"qp iterations {out['qp_iterations'].tolist()}, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
