"""CPU: DRTMD.resolve_observations / resolve_group on the store (hybdrt/mapping/drtmd.py:432-559) -- the description of the coupled
batches (mapping.resolve.resolve_args), the numpy statement of the device assembly (assemble_statement) against the existing host
assembly, and the store's bookkeeping around a stand-in for the device."""
import os
import types

import numpy as np
import pytest

from conftest import GOLDEN
from store_resolve_util import MATCHES, RANGES3, hand_args, q_bound, random_members, synthetic_fits

def fixture_fits(name):
    """the fitted members of a resolve_group fixture as resolve reads them, their tau ranges, batch size and overlap"""
    g = np.load(os.path.join(GOLDEN, f"refrun_resolve_group_{name}.npz"))
    special = {str(k): dict(index=int(i), size=int(s), nonneg=bool(nn))
               for k, i, s, nn in zip(g["special_names"], g["special_index"], g["special_size"], g["special_nonneg"])}
    fits = []
    for i in range(int(g["n_obs"])):
        n = int(g["n_params"][i]) if "n_params" in g else g["p_matrix"][i].shape[0]      # (stacks are zero-padded to the largest)
        fp = {k: g[k][i] for k in ("v_baseline", "vz_offset", "R_inf")}
        fp["p_matrix"], fp["q_vector"] = g["p_matrix"][i][:n, :n], g["q_vector"][i][:n]
        fits.append(types.SimpleNamespace(
            fit_parameters=fp, special_qp_params=special, coefficient_scale=float(g["coefficient_scale"][i]),
            response_signal_scale=float(g["response_signal_scale"][i]), scaled_response_offset=float(g["scaled_response_offset"][i]),
            v_baseline_scale=g["v_baseline_scale"][i], dop_scale_vector=None, inductance_scale=float(g["inductance_scale"][i])))
    tau_idx = [tuple(int(v) for v in t) for t in g["obs_tau_indices"]]
    return fits, tau_idx, int(g["batch_size"]), int(g["overlap"])


def upstream_starts(num_obs, batch_size, overlap):
    """the loop of drtmd.py:520-537, restated"""
    batch_size = min(batch_size, num_obs)
    out = []
    for start in range(0, num_obs, max(batch_size - overlap, 1)):
        if num_obs - start < batch_size:
            start = max(0, num_obs - batch_size)
        out.append(start)
        if start + batch_size >= num_obs:
            break
    return out


@pytest.mark.parametrize("name", ["hybrid16", "hybrid16_ranges"])
def test_statement_equals_the_host_assembly_on_the_reference_fits(name):
    from hipdrt.mapping import resolve
    fits, tau_idx, bs, overlap = fixture_fits(name)
    bs2, starts = resolve.group_batch_starts(len(fits), bs, overlap)
    assert bs2 == bs and starts == upstream_starts(len(fits), bs, overlap) and len(starts) == 3
    bare = [types.SimpleNamespace(**{**vars(f), "fit_parameters": {k: v for k, v in f.fit_parameters.items() if k != "p_matrix"}})
            for f in fits]                                                   # the description needs no P
    args = resolve.resolve_args(bare, tau_idx, True, starts, bs)
    p_list = [f.fit_parameters["p_matrix"] for f in fits]
    q_list = [f.fit_parameters["q_vector"] for f in fits]
    stm = resolve.assemble_statement(args, p_list, q_list)
    bounds = q_bound(args, p_list, q_list)
    for k, a in enumerate(starts):
        p_ref, q_ref, h_ref, special, match, nr, nc = resolve.resolve_observations(fits[a:a + bs], tau_idx[a:a + bs], True,
                                                                                  _assemble_only=True)
        assert (nr, nc) == (args["nr"], len(args["param_scale"][k])) and tuple(args["match"][k]) == match
        assert special == args["special"] and int(args["first"][k]) == a
        np.testing.assert_array_equal(stm[k][0], p_ref)
        assert np.all(np.abs(stm[k][1] - q_ref) <= bounds[k])
        np.testing.assert_array_equal(args["h"][k], h_ref)
    if name == "hybrid16_ranges":
        assert len({len(ps) for ps in args["param_scale"]}) == 2          # batches of two sizes


@pytest.mark.parametrize("truncate", [False, True])
def test_statement_on_synthetic_members_of_three_ranges(truncate):
    """nr = 3, 2 special unknowns kept + 2 removed, tau ranges (0, 21), (2, 23), (1, 20) on a supergrid of 23: every member is
    expanded (truncate=False) or cut (truncate=True) at one end at least"""
    from hipdrt.mapping import resolve
    fits = synthetic_fits(RANGES3, seed=3)
    args = resolve.resolve_args(fits, RANGES3, True, [0], 3, truncate=truncate, sigma=1, lambda_psi=2.5)
    assert tuple(args["match"][0]) == ((2, 20) if truncate else (0, 23)) and args["num_remove"] == 2 and args["so"] == 2
    p_list = [f.fit_parameters["p_matrix"] for f in fits]
    q_list = [f.fit_parameters["q_vector"] for f in fits]
    (p_k, q_k), = resolve.assemble_statement(args, p_list, q_list)
    p_ref, q_ref, h_ref, *_ = resolve.resolve_observations(fits, RANGES3, True, truncate=truncate, lambda_psi=2.5, _assemble_only=True)
    np.testing.assert_array_equal(p_k, p_ref)
    assert np.all(np.abs(q_k - q_ref) <= q_bound(args, p_list, q_list)[0])
    np.testing.assert_array_equal(args["h"][0], h_ref)
    assert h_ref[0] == 0 and h_ref[1] == 0                                    # both kept specials are nonneg


@pytest.mark.parametrize("case", list(MATCHES))
def test_member_columns_is_resize_pq_in_each_of_its_four_cases(case):
    """one index rule against resize_pq itself, member by member, for common ranges that expand, truncate, expand left / truncate
    right and truncate left / expand right"""
    from hipdrt.mapping import resolve
    so, nrm, match = 2, 2, MATCHES[case]
    p_list, q_list = random_members(RANGES3, so, nrm, seed=11)
    args = hand_args(RANGES3, [(0, match)], 3, so, nrm, seed=5)
    (p_k, q_k), = resolve.assemble_statement(args, p_list, q_list)
    nc = so + match[1] - match[0]
    lefts = {np.sign(r[0] - match[0]) for r in RANGES3}
    rights = {np.sign(r[1] - match[1]) for r in RANGES3}
    assert len(lefts | rights) >= 2                                           # the case moves something
    for i, (p, q, rng_) in enumerate(zip(p_list, q_list, RANGES3)):
        q_off = q[nrm:] + args["x_remove"][i] @ p[:nrm, nrm:]
        p_res, q_res = resolve.resize_pq(p[nrm:, nrm:], q_off, so, rng_, match)
        blk = p_k[i * nc:(i + 1) * nc, i * nc:(i + 1) * nc]
        expect = p_res + np.diag(args["param_scale"][0] * args["my"][0][i, i] * args["lambda_psi"])
        np.testing.assert_array_equal(blk, expect)
        np.testing.assert_array_equal(q_k[i * nc:(i + 1) * nc], q_res)
        for j in range(3):
            if j != i:
                off = p_k[i * nc:(i + 1) * nc, j * nc:(j + 1) * nc]
                np.testing.assert_array_equal(off, np.diag(args["param_scale"][0] * args["my"][0][i, j] * args["lambda_psi"]))


def test_statement_refuses_the_dense_filters():
    from hipdrt.mapping import resolve
    args = hand_args(RANGES3, [(0, (0, 23))], 3, 2, 2, seed=5)
    args["tau_filter_sigma"] = 1.0
    with pytest.raises(NotImplementedError):
        resolve.assemble_statement(args, *random_members(RANGES3, 2, 2, seed=1))


# ---- the store's bookkeeping around a stand-in for the device ---------------------------------------------------------------------
class _NoDevice:
    device = 0


def _store(n=9, nt=12):
    from hipdrt.mapping import store
    md = store.DRTMD(np.logspace(-4, 1, nt), drt=_NoDevice(), psi_dim_names=["T", "p"])
    temps = [50.0, 10.0, 30.0, 20.0, 40.0, 70.0, 60.0, 80.0, 5.0]
    for k in range(n):
        md.add_observation([temps[k], 0.0], ("t", "i", "v"), ("f", "z"), group_id="a" if k < 8 else "b")
    md.obs_x[:] = np.arange(n)[:, None] * 10.0 + np.arange(nt)[None]
    md.obs_fit_status[:] = True
    md.obs_tau_indices = [(1, 9)] * n
    md.obs_special = {"R_inf": np.arange(n) + 0.5, "vz_offset": np.arange(n) + 0.25}
    return md


@pytest.fixture
def stand_in(monkeypatch):
    """the refit and the device solve replaced: members carry their observation index as coefficient scale, batch k's solution is
    100 (k + 1) + 10 row + column in QP units, its R_inf column k + 1"""
    from hipdrt.mapping import resolve, store
    calls = dict(refit=[], solve=[], host=[])
    special = {"R_inf": dict(index=0, size=1, nonneg=True)}

    def refit(self, obs_index):
        calls["refit"].append(np.array(obs_index))
        members = [types.SimpleNamespace(coefficient_scale=1.0, dop_scale_vector=None, inductance_scale=1.0, obs=int(i)) for i in obs_index]
        return "plan", members

    def solve(plan, members, tau_idx, nonneg, starts, batch_size, truncate=False, sigma=1, lambda_psi=1):
        calls["solve"].append(dict(plan=plan, members=[m.obs for m in members], tau_idx=list(tau_idx), nonneg=nonneg, starts=list(starts),
                                   batch_size=batch_size, truncate=truncate, sigma=sigma, lambda_psi=lambda_psi))
        x, matches = [], []
        for k, a in enumerate(starts):
            m = resolve.get_tau_indices(tau_idx[a:a + batch_size], truncate=truncate)
            nc = 1 + m[1] - m[0]
            xk = 100.0 * (k + 1) + 10.0 * np.arange(batch_size)[:, None] + np.arange(nc)[None]
            xk[:, 0] = k + 1
            x.append(xk); matches.append(m)
        return x, matches, special, [7] * len(starts)

    def host_group(fits, tau_idx, nonneg, nsup, **kw):
        calls["host"].append(dict(n=len(fits), kw=kw))
        return np.full((len(fits), nsup), 3.0), {"R_inf": np.full(len(fits), 4.0)}
    host_group.last_qp = dict(iterations=[1], launches=1)

    monkeypatch.setattr(store.DRTMD, "_refit_members", refit)
    monkeypatch.setattr(resolve, "resolve_batches_on_plan", solve)
    monkeypatch.setattr(resolve, "resolve_group", host_group)
    monkeypatch.setattr(_NoDevice, "batch_fits", lambda self: ["fit"] * len(calls["refit"][-1]), raising=False)
    return calls


def test_resolve_group_selects_sorts_batches_and_averages(stand_in):
    md = _store()
    md.obs_fit_status[3] = False                      # unfitted
    md.obs_ignore_flag[6] = True                      # ignored
    md.obs_tau_indices[0] = (2, 8)
    assert md.obs_x_resolved is None and md.obs_special_resolved is None
    md.resolve_group("a", batch_size=4, overlap=2, psi_sort_dims=["T"], sigma=2, lambda_psi=3)
    order = [1, 2, 4, 0, 5, 7]                        # group a without 3 and 6, ascending T: 10, 30, 40, 50, 70, 80
    np.testing.assert_array_equal(stand_in["refit"][0], order)
    call = stand_in["solve"][0]
    assert call["members"] == order and call["starts"] == [0, 2] and call["batch_size"] == 4 and call["plan"] == "plan"
    assert call["tau_idx"] == [md.obs_tau_indices[i] for i in order] and call["nonneg"] is True
    assert (call["sigma"], call["lambda_psi"], call["truncate"]) == (2, 3, False)
    assert md.last_resolve == dict(iterations=[7, 7], path="device")
    # margins of a batch of 4: 0 1 1 0 -> weights 0.1 1.1 1.1 0.1; rows 2, 3 of the group lie in both batches
    x0 = 100.0 + 10.0 * np.arange(4)[:, None] + np.arange(1, 9)[None]
    x1 = 200.0 + 10.0 * np.arange(4)[:, None] + np.arange(1, 9)[None]
    want = np.zeros((6, 12))
    want[0:2, 1:9], want[4:6, 1:9] = x0[0:2], x1[2:4]
    w0, w1 = np.array([1.1, 0.1])[:, None], np.array([0.1, 1.1])[:, None]
    want[2:4, 1:9] = (w0 * x0[2:4] + w1 * x1[0:2]) / (w0 + w1)
    np.testing.assert_allclose(md.obs_x_resolved[order], want, rtol=1e-14)
    r_inf = np.array([1, 1, (1.1 * 1 + 0.1 * 2) / 1.2, (0.1 * 1 + 1.1 * 2) / 1.2, 2, 2])
    np.testing.assert_allclose(md.obs_special_resolved["R_inf"][order], r_inf, rtol=1e-14)
    untouched = [3, 6, 8]
    assert not md.obs_x_resolved[untouched].any() and not md.obs_special_resolved["R_inf"][untouched].any()
    assert md.obs_special_resolved["R_inf"].shape == (9,)
    assert not md.obs_special_resolved["vz_offset"].any()          # upstream's table: a key per fitted special, zeros where eliminated
    # a later observation grows the resolved arrays with the others
    md.add_observation([90.0, 0.0], None, None, group_id="a")
    assert md.obs_x_resolved.shape == (10, 12) and md.obs_special_resolved["R_inf"].shape == (10,)
    # filter_observations(resolved=True) now finds what it reads
    assert md.obs_x_resolved is not None and md.obs_special_resolved is not None


def test_resolve_group_clears_rows_and_keeps_the_one_observation_error(stand_in):
    md = _store()
    md.obs_x_resolved = np.full_like(md.obs_x, 9.0)
    md.obs_special_resolved = {}
    with pytest.raises(ValueError, match="Only one observation"):
        md.resolve_group("b")
    assert not md.obs_x_resolved[8].any() and np.all(md.obs_x_resolved[:8] == 9.0)
    assert stand_in["refit"] == []
    md.obs_ignore_flag[8] = True
    with pytest.warns(UserWarning, match="No valid observations"):
        md.resolve_group("b")


def test_resolve_observations_writes_inside_the_common_range(stand_in):
    md = _store()
    md.obs_tau_indices[2] = (0, 10)
    md.resolve_observations(np.array([4, 2, 1]), psi_sort_dims=["T"], truncate=True)
    order = [1, 2, 4]
    call = stand_in["solve"][0]
    assert call["members"] == order and call["starts"] == [0] and call["batch_size"] == 3 and call["truncate"] is True
    x0 = 100.0 + 10.0 * np.arange(3)[:, None] + np.arange(1, 9)[None]
    np.testing.assert_array_equal(md.obs_x_resolved[order, 1:9], x0)
    assert not md.obs_x_resolved[:, 0].any() and not md.obs_x_resolved[:, 9:].any()
    np.testing.assert_array_equal(md.obs_special_resolved["R_inf"][order], [1, 1, 1])
    # one observation: its raw parameters, with upstream's warning
    with pytest.warns(UserWarning, match="raw parameters will be copied"):
        md.resolve_observations(np.array([5]))
    np.testing.assert_array_equal(md.obs_x_resolved[5, 1:9], md.obs_x[5, 1:9])
    assert md.obs_special_resolved["R_inf"][5] == 5.5 and md.obs_special_resolved["vz_offset"][5] == 5.25
    assert len(stand_in["solve"]) == 1


def test_dense_filters_fall_back_to_the_host_assembly(stand_in):
    md = _store()
    md.resolve_group("a", batch_size=4, overlap=1, tau_filter_sigma=1.5)
    assert stand_in["solve"] == [] and len(stand_in["host"]) == 1
    kw = stand_in["host"][0]["kw"]
    assert stand_in["host"][0]["n"] == 8 and kw["batch_size"] == 4 and kw["overlap"] == 1 and kw["tau_filter_sigma"] == 1.5
    assert md.last_resolve["path"] == "host"
    assert np.all(md.obs_x_resolved[:8] == 3.0) and np.all(md.obs_special_resolved["R_inf"][:8] == 4.0)
    md.resolve_observations(np.arange(3), special_filter_sigma=2.0)
    assert len(stand_in["host"]) == 2 and stand_in["host"][1]["kw"]["special_filter_sigma"] == 2.0


def test_eis_only_observations_raise_upstreams_key_error():
    from hipdrt.mapping import store
    md = store.DRTMD(np.logspace(-4, 1, 7), drt=_NoDevice())
    for k in range(3):
        md.add_observation([k], None, (np.logspace(3, 0, 5), np.ones(5) + 0j), group_id="g")
    md.obs_fit_status[:] = True
    md.obs_tau_indices = [(0, 7)] * 3
    with pytest.raises(KeyError, match="v_baseline"):
        md.resolve_group("g")
