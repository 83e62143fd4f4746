"""Fits a fixed set of spectra (C1 golden-size and C2-size) with whatever library HIPDRT_LIB points to and saves the raw
results; two dumps compared bit for bit tell whether two builds compute the same thing.  Every path of the plan's device
loop is taken once: EIS batch fits, a sub-batched fit, outlier_p, a warm restart, a prepared joint fit with the 'weight'
factor rule and its restart with row factors, one iterate_qphb pass, the posterior entry points, the Kramers-Kronig screen
and the predictions of a fitted batch; then the post-fit DRT chain (peaks, peak and trough probabilities, per-peak resolution,
window integrals, the PFRT and candidate scores of a short PFRT fit) and its row kernels alone through their test hooks.
python tools/dump_fit.py out.npz   /   python tools/dump_fit.py --cmp a.npz b.npz"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
if sys.argv[1] == "--cmp":
    a, b = np.load(sys.argv[2]), np.load(sys.argv[3])

    def same(x, y):     # bit for bit: NaN rows of dead spectra and padding compare equal, -0.0 and 0.0 do not
        return x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()
    bad = sorted(set(a.files) ^ set(b.files)) + [k for k in a.files if k in b.files and not same(a[k], b[k])]
    print("identical" if not bad else f"DIFFERENT: {bad}")
    for k in bad:       # how far apart: iteration counts as a mismatch count, everything else relative to the largest entry
        if k not in a.files or k not in b.files or a[k].shape != b[k].shape:
            print(f"  {k}: in one dump only, or of another shape")
            continue
        x, y = np.asarray(a[k], dtype=float), np.asarray(b[k], dtype=float)
        if "iters" in k:
            print(f"  {k}: {int((x != y).sum())} of {x.size} differ")
        else:
            sc = np.abs(x).max(axis=-1, keepdims=True) if x.ndim > 1 else np.abs(x).max()
            print(f"  {k}: max |a - b| / peak = {np.max(np.abs(x - y) / np.maximum(sc, 1e-300)):.2e}")
    sys.exit(1 if bad else 0)
from hipdrt import synth
from hipdrt.models import DRT
out = {}
c2 = synth.config_c2()
z = synth.zarc2_batch(c2["freq"], 96)
d = DRT(fixed_basis_tau=c2["tau"])
r = d.fit_eis_batch(c2["freq"], z)
for k in ("x", "weights", "rho", "outer_iters", "qp_iters_total"):
    out["c2_" + k] = r[k]
v = d.estimate_distribution_var_batch(c2["tau"][::4])
out["c2_var"] = np.asarray(v[0] if isinstance(v, tuple) else v)
# model evaluation of the fitted C2 batch on the device: DRT and its first derivative, credible band, impedance, R_p
for o in (0, 1):
    out[f"c2_drt{o}"] = d.predict_drt_batch(order=o)
out["c2_ci_lo"], out["c2_ci_hi"], out["c2_ci_ok"] = d.predict_drt_ci_batch()
out["c2_z"], out["c2_r_p"] = d.predict_z_batch(), d.predict_r_p_batch()
# the same range on a finer tau grid: n > 528, the posterior variance with the inverse diagonal blocks in global memory (four
# spectra: their QPs run on the group kernel)
tf = np.geomspace(c2["tau"][0], c2["tau"][-1], 600)
df = DRT(fixed_basis_tau=tf)
rf = df.fit_eis_batch(c2["freq"], z[:4])
for k in ("x", "outer_iters", "qp_iters_total"):
    out["fine_" + k] = rf[k]
v = df.estimate_distribution_var_batch(tf[::4])
out["fine_var"] = np.asarray(v[0] if isinstance(v, tuple) else v)
c1 = synth.config_c1()
z1 = synth.zarc2_batch(c1["freq"], 16)
d1 = DRT(fixed_basis_tau=c1["tau"])
r1 = d1.fit_eis_batch(c1["freq"], z1)
for k in ("x", "weights", "outer_iters", "qp_iters_total"):
    out["c1_" + k] = r1[k]


def put(prefix, v):
    """a result of any shape the post-fit methods give -- an array, a dict or tuple of results, a per-spectrum list of ragged
    arrays (flattened, with the lengths beside it) -- under keys that start with prefix"""
    if isinstance(v, dict):
        for k in v:
            put(f"{prefix}_{k}", v[k])
    elif isinstance(v, tuple):
        for i, e in enumerate(v):
            put(f"{prefix}_{i}", e)
    elif isinstance(v, list):
        if v and isinstance(v[0], dict):
            put(prefix, {k: [e[k] for e in v] for k in v[0]})
        else:
            rows = [np.asarray(e) for e in v]
            out[prefix] = np.concatenate([e.ravel() for e in rows]) if rows else np.zeros(0)
            out[prefix + "_len"] = np.array([e.size for e in rows])
    else:
        out[prefix] = np.asarray(v)


# the post-fit DRT chain on the C1 batch: peak finding by every method, the peak and trough probabilities and the search on their
# product, the credible band, per-peak resolution from find_peaks and from windows, the window integral
put("c1_peaks_thresh", d1.find_peaks_batch(return_info=True))
put("c1_peaks_prob", d1.find_peaks_batch(method="prob", num_peaks=2, return_info=True))
out["c1_map_peak_prob"], out["c1_map_curv_prob"] = d1.peak_prob_batch(), d1.curv_prob_batch()
for bc in (True, False):
    put(f"c1_ptp_bayes{int(bc)}", d1.predict_peak_trough_probs_batch(bayes_cov=bc))
put("c1_byprob", d1.find_peaks_byprob_batch(height=0.5, prominence=0.25, return_info=True))
put("c1_byprob_ranges", d1.find_peaks_byprob_batch(peak_tau_ranges=[(1e-5, 1e-3), (1e-3, 1e-1)], return_info=True))
put("c1_ci", d1.predict_drt_ci_batch())
put("c1_quantify", d1.quantify_peaks_batch(return_info=True))
put("c1_peak_drts", d1.estimate_peak_drts_batch())
out["c1_split_resolved"] = d1.split_r_p_batch([1e-4, 1e-2], resolve_peaks=True)
out["c1_integral"] = d1.integrate_drt_batch(1e-6, 1e1)
# a short PFRT fit: the PFRT of its three recorded steps, and the steps scored as candidate models
dp = DRT(fixed_basis_tau=c1["tau"])
dp.pfrt_fit_eis_batch(c1["freq"], z1[:8], factors=np.logspace(-1, 1, 3))
put("pfrt", dp.predict_pfrt_batch(return_info=True))
put("pfrt_cand", dp._plan.score_candidates(ln_tau_find=np.log(dp.get_tau_eval(10))))
# the row kernels alone, on seeded rows: neval 3 (the smallest row with an interior sample) and 257 (a thread takes two samples,
# the sort buffer is padded), extend_var's bounds in order and crossed
from hipdrt import _ffi
ctx, rng = d1._plan.ctx, np.random.default_rng(7)
for n in (3, 257):
    f, fx, fxx = rng.normal(size=(3, 3, n))
    vf, vx, vxx = rng.uniform(0.01, 1.0, size=(3, 3, n))
    sg, ht, pr = rng.integers(-1, 2, size=(3, n)), rng.uniform(0.0, 1.0, size=(3, n)), rng.uniform(0.0, 1.0, size=(3, n))
    lt, lb = np.linspace(-8.0, 2.0, n), np.linspace(-8.0, 2.0, 16)
    put(f"hook{n}_resolve", ctx.debug_peak_resolve(np.abs(f), fxx, rng.uniform(0.1, 1.0, size=(3, 16)), lt, lb, ln_tau_out=lt,
                                                    windows=([0, n // 2], [n // 2 + 1, n])))
    for tag, (el, er) in (("ord", (n // 6, n - 1 - n // 6)), ("crossed", (n - 1 - n // 6, n // 6))):
        for m in ("thresh", "prob", "map"):
            o = _ffi.peak_opts(search=0, method=m, num_peaks=2 if m == "prob" else None, ext_left=el, ext_right=er)
            put(f"hook{n}_{tag}_peaks_{m}", ctx.debug_find_peaks(fxx, f, vxx, vf, opts=o))
        for bc in (True, False):
            o = _ffi.peak_prob_opts(bayes_cov=bc, ext_left=el, ext_right=er, search="thresh", height=0.1, prominence=0.05)
            put(f"hook{n}_{tag}_ptp_bayes{int(bc)}", ctx.debug_peak_trough_probs(f, fx, fxx, vf, vx, vxx, opts=o))
        out[f"hook{n}_{tag}_pfrt_step"] = ctx.debug_pfrt_step(sg, ht, pr, f, vf, vxx, 1e-5, el, er)
        put(f"hook{n}_{tag}_map", ctx.debug_map_prob(f, fxx, vf, vxx, ext=np.tile(np.int32([el, er]), (3, 1)), search=0))
# Kramers-Kronig screen of the C1 spectra: two rounds of fit -> screen, the second fit with the first screen's row factors
kk = DRT(fixed_basis_tau=c1["tau"]).kk_test_batch(c1["freq"], z1)
for k in ("outlier_mask", "clean_mask", "f_min", "f_max", "residuals", "std", "status", "z_hat"):
    out["kk_" + k] = kk[k]
f = np.logspace(5.5, -0.5, 60)
r3 = DRT(basis_tau_ppd=8).fit_eis_batch(f, synth.zarc2_batch(f, 8))      # n = 61: odd number of block columns etc.
for k in ("x", "outer_iters", "qp_iters_total"):
    out["d_" + k] = r3[k]

# the staged batch fitted as three ranges side by side (hipdrt_plan_set_subbatches)
ds = DRT(fixed_basis_tau=c2["tau"])
ds.stage_batch(c2["freq"], synth.zarc2_batch(c2["freq"], 384, first_seed=5000)).set_subbatches(3)
ds.fit_staged()
rs = ds.collect_staged()
for k in ("x", "weights", "rho", "s_vectors", "q_vector", "outer_iters", "qp_iters_total"):
    out["sub_" + k] = rs[k]
out["sub_launches"] = np.array(list(rs["launches"].values()))

# outlier_p: two initial QPs, outlier-aware weights in every iteration
ro = DRT(fixed_basis_tau=c1["tau"]).fit_eis_batch(c1["freq"], z1, outlier_p=0.05)
for k in ("x", "weights", "outer_iters", "qp_iters_total"):
    out["outl_" + k] = ro[k]
out["outl_launches"] = np.array(list(ro["launches"].values()))

# warm restart of the C2 batch with a changed l2_lambda_0
rc = d.continue_from_init(l2_lambda_0=142.0 / 4.0)
for k in ("x", "weights", "rho", "q_vector", "outer_iters", "qp_iters_total"):
    out["cont_" + k] = rc[k]
out["cont_launches"] = np.array(list(rc["launches"].values()))

# prepared joint fit: initial weights per block, row factors by the 'weight' rule; then a restart with row factors and the
# posterior entry points on the state it leaves
dj = DRT(warn=False)
fj = dj.fit_hybrid(*synth.hybrid_measurement(seed=0), init_weights_separately=True, hybrid_weight_factor_method='weight')
qp = dj.qphb_params
out["joint_x"], out["joint_weights"], out["joint_p"] = dj.cvx_result["x"], qp["true_weights"], fj["p_matrix"]
out["joint_factors"] = np.array([qp["chrono_weight_factor"], qp["eis_weight_factor"]])
out["joint_launches"] = np.array(list(dj._plan.timings()[1].values()))      # (fit_hybrid's result does not carry them)
rj = dj.continue_from_init(weight_factor=1.3, eis_weight_factor=1.7, chrono_weight_factor=0.6, max_iter=3)
for k in ("x", "weights", "rho", "q_vector", "outer_iters", "qp_iters_total"):
    out["jcont_" + k] = rj[k]
out["jcont_launches"] = np.array(list(rj["launches"].values()))
pc = dj.estimate_param_cov()
out["jcont_param_cov"] = np.asarray(np.nan if pc is None else pc)
dc = dj.estimate_distribution_cov(ppd=10)
out["jcont_dist_cov"] = np.asarray(np.nan if dc is None else dc)
v = dj.estimate_distribution_var_batch(ppd=10)
out["jcont_var"] = np.asarray(v[0] if isinstance(v, tuple) else v)
out["jcont_p"] = dj._plan.p_matrix(0)

# one iterate_qphb pass from the start state of _qphb_fit_core on the joint fit's matrices
from hipdrt.models import qphb
from oracle import drt_oracle as orc
n = qp["rm"].shape[1]
it = qphb.iterate_qphb(np.zeros(n) + 1e-6, np.ones((3, n)), np.ones(3), None, qp["rv"], qp["true_weights"], qp["est_weights"],
                       None, qp["rm"], qp["vmm"], qp["penalty_matrices"], "integral", qp["l1_lambda_vector"],
                       orc.get_default_hypers(), True, np.ones(3), None, None, None, None, True, dj.special_qp_params, 1e-2, 1, None)
for i, k in ((0, "x"), (1, "s_vectors"), (2, "rho"), (4, "weights")):
    out["iter_" + k] = np.asarray(it[i])
out["iter_qp"] = np.array([it[7]["iterations"], it[7]["primal objective"], it[8]], dtype=float)
np.savez(sys.argv[1], **out)
print("saved", sys.argv[1], {k: v.shape for k, v in out.items() if k.endswith("_x")})
