"""Device: the assembly kernels of hipdrt_plan_resolve_group (csrc/resolve.hip) alone against their numpy statement, and
DRTMD.resolve_group on the store against the host-assembled path (mapping.resolve.resolve_group on the members' downloaded P) on the
same fitted batch, and against the reference's own DRTMD (tests/golden/refrun_store_resolve8.npz).

The figure against the host-assembled path is max |difference| / max |reference|, the largest over obs_x_resolved and the resolved
special parameters, asserted at its bound in tests/store_resolve_bounds.json (bound = the next 1-2-5 step at least 10 x above the
measured value, never above 1e-7).  The two paths hand the QP the same P bit for bit and q's that may differ in the last bit of an
entry (the order of a num_remove + 1 term sum).  On the batches of these tests the q's agree as well and the figure measured on the
GPU is 0.0; the recorded value is what the same comparison measured where they do not -- 5.22e-15 on the 16-observation batch of
tools/time_store_resolve.py --grid 121 -- so that the bound does not hinge on how the host's BLAS orders a two-term sum."""
import json
import os

import numpy as np
import pytest

from conftest import ROOT
from store_resolve_util import RANGES3, hand_args, q_bound, random_members

pytestmark = pytest.mark.gpu

RANGES70 = [(0, 66), (3, 70), (2, 68)]          # on a supergrid of 70 slots
# ranges, nr, so, num_remove, [(first member, common range)]: nc = so + width of the common range
CASES = {
    # nc = 23 (less than one 64-column strip) beside 25, 20 and 22: expand left / truncate right and its mirror image, expand,
    # truncate, plain and mixed -- four problem sizes in one call
    "nc23_nr3_rm2": (RANGES3, 3, 2, 2, [(0, (1, 22)), (0, (0, 23)), (0, (2, 20)), (0, (1, 21))]),
    # two batches of one size over different members, nothing removed
    "nc23_nr2_rm0": (RANGES3, 2, 2, 0, [(0, (1, 22)), (1, (1, 22))]),
    # nc = 70: a strip and a ragged one; n = 140 leaves a padding tile row (nchp = 10 for 9 tile rows); nc = 72 beside it
    "nc70_nr2_rm2": (RANGES70, 2, 2, 2, [(0, (1, 69)), (1, (1, 69)), (0, (0, 70))]),
    "nc70_nr3_rm0": (RANGES70, 3, 2, 0, [(0, (1, 69))]),
}


@pytest.fixture(scope="module")
def ctx():
    from hipdrt import _ffi
    return _ffi.get_context(0)


@pytest.mark.parametrize("name", list(CASES))
def test_assembly_kernels_equal_their_statement(ctx, name):
    from hipdrt.mapping import resolve
    ranges, nr, so, nrm, batches = CASES[name]
    p_list, q_list = random_members(ranges, so, nrm, seed=len(name))
    args = hand_args(ranges, batches, nr, so, nrm, seed=7)
    stm = resolve.assemble_statement(args, p_list, q_list)
    bounds = q_bound(args, p_list, q_list)
    out = ctx.debug_resolve_assemble(args, p_list, q_list)
    assert len(out) == len(batches)
    for k, ((p_dev, q_dev), (p_stm, q_stm)) in enumerate(zip(out, stm)):
        assert p_dev.shape == p_stm.shape == (nr * (so + batches[k][1][1] - batches[k][1][0]),) * 2
        np.testing.assert_array_equal(p_dev, p_stm)                           # bit for bit
        assert p_dev.tobytes() == p_stm.tobytes()
        excess = np.abs(q_dev - q_stm) - bounds[k]
        print(f"resolve assemble {name} batch {k}: max |q - statement| {np.abs(q_dev - q_stm).max():.2e}, least slack {-excess.max():.2e}")
        assert np.all(excess <= 0)
    again = ctx.debug_resolve_assemble(args, p_list, q_list)
    for (p1, q1), (p2, q2) in zip(out, again):
        assert p1.tobytes() == p2.tobytes() and q1.tobytes() == q2.tobytes()


def test_assembly_refuses_what_it_does_not_build(ctx):
    from hipdrt import _ffi
    ranges, nr, so, nrm, batches = CASES["nc23_nr2_rm0"]
    p_list, q_list = random_members(ranges, so, nrm, seed=1)
    args = hand_args(ranges, batches, nr, so, nrm, seed=7)
    with pytest.raises(NotImplementedError, match="tau_filter_sigma"):
        ctx.debug_resolve_assemble(dict(args, tau_filter_sigma=1.0), p_list, q_list)
    with pytest.raises(NotImplementedError):
        ctx.debug_resolve_assemble(dict(args, special_filter_sigma=0.5), p_list, q_list)
    with pytest.raises(_ffi.HipDrtError, match="reaches outside"):
        ctx.debug_resolve_assemble(dict(args, first=np.array([0, 2], dtype=np.int32)), p_list, q_list)
    with pytest.raises(ValueError, match="member 1"):
        ctx.debug_resolve_assemble(args, [p_list[0], p_list[1][:-1, :-1], p_list[2]], [q_list[0], q_list[1][:-1], q_list[2]])


def check(label, pairs):
    """pairs: (actual, reference) arrays of one solution; the figure is the largest max |difference| / max |reference| among them"""
    with open(os.path.join(ROOT, "tests", "store_resolve_bounds.json")) as f:
        table = json.load(f)["device"]
    err = max(float(np.abs(np.asarray(a) - np.asarray(r)).max() / np.abs(r).max()) for a, r in pairs)
    print(f"store_resolve device {label}: measured {err:.2e} bound {table[label][1]:.1e}")
    assert table[label][1] <= 1e-7                                            # the project's stated promise
    assert err <= table[label][1], (label, err, table[label])


def small_hybrid_store(n_obs=8):
    """8 joint observations of jittered cells: 200 time samples (24 before the step, 176 after) and 21 frequencies each"""
    from hipdrt import synth
    from hipdrt.mapping import DRTMD
    md = DRTMD(np.logspace(-7, 2, 91), psi_dim_names=["T"], warn=False)
    for k in range(n_obs):
        m = synth.hybrid_measurement(seed=500 + k, jitter=True, n_pre=24, n_post=176, nf=21)
        md.add_observation([300.0 + 5 * k], (m[0], m[1], m[2]), (m[3], m[4]), group_id="g")
    return md


@pytest.fixture(scope="module")
def resolved_store():
    """the eight observations added, fitted and resolved once, for the tests that read the result"""
    md = small_hybrid_store()
    md.fit_all()
    assert md.obs_fit_status.all()
    md.resolve_group("g", batch_size=4, overlap=2, psi_sort_dims=["T"])
    return md


def test_store_resolve_group_equals_the_host_assembled_path(resolved_store):
    from hipdrt.mapping import resolve
    md = resolved_store
    assert md.last_resolve["path"] == "device" and len(md.last_resolve["iterations"]) == 3
    # the host-assembled path on the same fitted batch: the plan of the resolve's refit is still the DRT object's
    fits = md.drt1d.batch_fits()
    tau_idx = [md.obs_tau_indices[i] for i in range(8)]
    x_ref, sp_ref = resolve.resolve_group(fits, tau_idx, True, len(md.tau_supergrid), batch_size=4, overlap=2)
    print("store_resolve qp iterations", md.last_resolve["iterations"], resolve.resolve_group.last_qp["iterations"],
          "unknowns per member", fits[0].fit_parameters["p_matrix"].shape[0])
    assert md.last_resolve["iterations"] == resolve.resolve_group.last_qp["iterations"]
    assert set(sp_ref) == {"R_inf", "inductance"} and set(md.obs_special_resolved) == set(md.obs_special)
    check("drtmd:resolve_group", [(md.obs_x_resolved, x_ref)] + [(md.obs_special_resolved[key], sp_ref[key]) for key in sp_ref])
    scale = np.abs(x_ref).max()
    assert np.abs(md.obs_x_resolved - md.obs_x).max() > 1e-4 * scale          # the coupling moved the coefficients
    # filter_observations' default (resolved=True) now runs on what the store filled itself
    md.filter_observations(np.arange(8), psi_sort_dims=["T"], sigma=(1, 0))
    assert np.abs(md.obs_x_filt).max() > 0


def test_store_resolve_group_matches_the_reference_drtmd(resolved_store):
    """the reference's own DRTMD on the same eight observations (tools/make_store_resolve_golden.py): add_observation, fit_all,
    resolve_group(batch_size=4, overlap=2) -- same iteration counts, same margin-weighted averages"""
    from conftest import GOLDEN, parity
    g = np.load(os.path.join(GOLDEN, "refrun_store_resolve8.npz"))
    md = resolved_store
    np.testing.assert_array_equal(np.array([o[0][2] for o in md.obs_data]), g["v_signal"])          # the fixture's inputs
    np.testing.assert_array_equal(np.array([o[1][1] for o in md.obs_data]), g["z"])
    np.testing.assert_array_equal(md.tau_supergrid, g["tau_supergrid"])
    assert [tuple(t) for t in md.obs_tau_indices] == [tuple(t) for t in g["obs_tau_indices"].tolist()]
    assert md.last_resolve["iterations"] == g["qp_iterations"].tolist()
    scale = np.abs(g["obs_x_resolved"]).max()
    parity("x_res", md.obs_x_resolved, g["obs_x_resolved"], default=1e-7, scale=scale)
    assert sorted(md.obs_special_resolved) == [str(k) for k in g["special_names"]]
    for key in ("v_baseline", "vz_offset"):                                   # eliminated by the resolve: zeros, there and here
        assert not g[f"{key}_resolved"].any() and not md.obs_special_resolved[key].any()
    parity("R_inf", md.obs_special_resolved["R_inf"], g["R_inf_resolved"], default=1e-6, rel=True)
    parity("inductance", md.obs_special_resolved["inductance"], g["inductance_resolved"], default=1e-5, rel=True)
    assert np.abs(md.obs_x_resolved - g["obs_x"]).max() > 1e-4 * scale        # the coupling moved the coefficients


def test_store_resolve_observations_and_the_dense_fallback():
    """resolve_observations on four of the observations, against resolve.resolve_observations on their downloaded P; then with a tau
    filter, which the device assembly refuses and the store sends through the host-assembled path"""
    from hipdrt.mapping import resolve
    md = small_hybrid_store(4)
    md.fit_all()
    md.resolve_observations(np.arange(4), psi_sort_dims=["T"], sigma=2, lambda_psi=10)
    assert md.last_resolve["path"] == "device"
    fits = md.drt1d.batch_fits()
    tau_idx = [md.obs_tau_indices[i] for i in range(4)]
    x_drt, x_special, match = resolve.resolve_observations(fits, tau_idx, True, sigma=2, lambda_psi=10, unpack=True)
    assert md.last_resolve["iterations"] == [resolve.resolve_observations.last_qp["iterations"]]
    check("drtmd:resolve_observations", [(md.obs_x_resolved[:, match[0]:match[1]], x_drt)] +
          [(md.obs_special_resolved[key], x_special[key]) for key in x_special])
    with pytest.raises(NotImplementedError):
        md.drt1d._plan.resolve_group(resolve.resolve_args(fits, tau_idx, True, [0], 4, tau_filter_sigma=1.0))
    first = md.obs_x_resolved.copy()
    md.resolve_observations(np.arange(4), psi_sort_dims=["T"], sigma=2, lambda_psi=10, tau_filter_sigma=1.0)
    assert md.last_resolve["path"] == "host"
    assert np.abs(md.obs_x_resolved - first).max() > 0
