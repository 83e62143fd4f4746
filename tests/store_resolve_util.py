"""Shared by tests/test_host_store_resolve.py and tests/test_gpu_store_resolve.py: hand-made descriptions of coupled batches
(what hipdrt.mapping.resolve.resolve_args derives from fits), synthetic members, and the derived bound of an assembled q."""
import types

import numpy as np

# the supergrid of the synthetic members has 23 slots; their ranges reach each of resize_pq's four cases against these common ranges
RANGES3 = [(0, 21), (2, 23), (1, 20)]
MATCHES = {"expand": (0, 23), "truncate": (2, 20), "left_in_right_out": (1, 21), "left_out_right_in": (1, 22)}


def random_members(ranges, so, num_remove, seed):
    """one exactly symmetric P (n_b, n_b) and one q (n_b,) per member, n_b = num_remove + so + right - left"""
    rng = np.random.default_rng(seed)
    p_list, q_list = [], []
    for left, right in ranges:
        n = num_remove + so + right - left
        a = rng.standard_normal((n, n))
        p_list.append(a + a.T + 2 * n * np.eye(n))
        q_list.append(rng.standard_normal(n))
    return p_list, q_list


def hand_args(ranges, batches, nr, so, num_remove, seed, lambda_psi=0.7):
    """a description with `batches` = [(first member, (match left, match right)), ...]: my exactly symmetric, param_scale positive,
    x_remove random -- nothing in it comes from a fit"""
    rng = np.random.default_rng(seed + 1000)
    my, ps, h = [], [], []
    for _, (ml, mr) in batches:
        a = rng.standard_normal((nr, nr))
        my.append(a + a.T)
        nc = so + mr - ml
        ps.append(rng.uniform(0.5, 2.0, nc))
        h.append(np.zeros(nr * nc))
    return dict(nb=len(batches), nr=nr, num_remove=num_remove, so=so, lambda_psi=lambda_psi, tau_filter_sigma=0.0,
                special_filter_sigma=0.0, first=np.array([b[0] for b in batches], dtype=np.int32),
                match=np.array([b[1] for b in batches], dtype=np.int32).reshape(-1, 2),
                tau_indices=np.array(ranges, dtype=np.int32).reshape(-1, 2), x_remove=rng.standard_normal((len(ranges), num_remove)),
                my=np.array(my).reshape(-1, nr, nr), param_scale=ps, h=h, special={})


def q_bound(args, p_list, q_list):
    """per batch, per entry of q_k: (num_remove + 1) 2^-53 (|q| + sum_k |x_remove_k P_kj|) -- num_remove products of correctly
    rounded factors and num_remove additions, in whatever order: each of the num_remove + 1 terms is off by at most one rounding of
    a partial sum that the sum of the terms' magnitudes bounds.  Derived, nothing measured."""
    from hipdrt.mapping import resolve
    nrm, nr = args["num_remove"], args["nr"]
    out = []
    for k in range(args["nb"]):
        nc = len(args["param_scale"][k])
        bound = np.zeros(nr * nc)
        for i in range(nr):
            b = int(args["first"][k]) + i
            p, q = np.asarray(p_list[b]), np.asarray(q_list[b])
            mag = np.abs(q[nrm:]) + np.abs(args["x_remove"][b]) @ np.abs(p[:nrm, nrm:])
            src = resolve.member_columns(args, k, b)
            there = src >= 0
            bound[i * nc + np.where(there)[0]] = (nrm + 1) * 2.0 ** -53 * mag[src[there] - nrm]
        out.append(bound)
    return out


SPECIAL4 = {"v_baseline": dict(index=0, size=1, nonneg=False), "vz_offset": dict(index=1, size=1, nonneg=False),
            "R_inf": dict(index=2, size=1, nonneg=True), "inductance": dict(index=3, size=1, nonneg=True)}


def synthetic_fits(ranges, seed):
    """DRT-like objects with 2 removed + 2 kept special unknowns on the given tau ranges: what resolve reads from a fit"""
    rng = np.random.default_rng(seed)
    p_list, q_list = random_members(ranges, 2, 2, seed)
    fits = []
    for p, q in zip(p_list, q_list):
        fp = dict(p_matrix=p, q_vector=q, v_baseline=np.array([rng.normal()]), vz_offset=rng.normal(), R_inf=rng.uniform(0.5, 2.0),
                  inductance=rng.uniform(1e-7, 1e-6))
        fits.append(types.SimpleNamespace(fit_parameters=fp, special_qp_params=SPECIAL4, coefficient_scale=rng.uniform(0.5, 2.0),
                                          response_signal_scale=rng.uniform(0.5, 2.0), scaled_response_offset=rng.normal(),
                                          v_baseline_scale=np.array([rng.uniform(0.5, 2.0)]), dop_scale_vector=None,
                                          inductance_scale=1e-5))
    return fits
