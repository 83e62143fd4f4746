"""The observation store around the batch driver: what DRTMD keeps between calls (hybdrt/mapping/drtmd.py:102-160, 186-329).

``mapping.fit_observations`` is a function -- it fits what it is handed.  ``DRTMD.fit_all(refit=False)`` is a method of an object
that REMEMBERS: observations are added one by one (``add_observation``, drtmd.py:186-241), each carries a fit status, an ignore
flag and the error that made it fail, and ``fit_all`` fits only the ones that are neither fitted nor ignored (drtmd.py:321-329)
-- the resume-after-interruption path of a long map.  This class is that bookkeeping on top of the device batches: the
observations selected by a call are fitted as ONE list (mapping.fit_observations groups them by data type and sampling grid, one
device batch per group), results are scattered into the per-observation arrays, and the status / ignore / error rules are the
reference's:

    fit succeeded                          obs_fit_status True
    fit failed, ignore_errors=True         obs_fit_status False, obs_ignore_flag True, obs_fit_errors[i] = the error
                                           (drtmd.py:292-299) -- a later fit_all(refit=False) skips it
    fit failed, ignore_errors=False        the error is raised (drtmd.py:300-301); observations of the same call that were
                                           fitted on the device before the failed one keep their results, as in the
                                           reference's serial loop, later ones stay unfitted

Fitted observations can be smoothed across psi and tau on the device: ``filter_observations`` / ``filter_group``
(drtmd.py:561-635) write ``obs_x_filt`` / ``obs_special_filt`` through mapping.ndx.filter_ndx.  Before that, a group's raw data
and fitted DRTs can be scored against their neighbours in psi: ``score_group_data_badness`` / ``score_group_fit_badness``
(drtmd.py:642-783) write ``obs_data_badness`` / ``obs_fit_badness`` through mapping.nddata.score_rows.

The fitted map is read through the prediction block (drtmd.py:788-1106): ``predict_x``, ``predict_r_p``, ``predict_drt``,
``predict_drt_var``, ``predict_peak_prob`` and ``predict_curv_prob`` run csrc/map_predict.hip on the store's arrays (statement=True:
mapping.predict, the same arithmetic in numpy).  The store keeps no fits and no covariances: with ``store_eval_var=True`` every
device batch also leaves the raw variances of the DRT and of its curvature on get_tau_eval(10) in ``obs_f_var`` / ``obs_fxx_var``.

Neighbouring observations can be re-optimised coherently: ``resolve_observations`` / ``resolve_group`` (drtmd.py:432-559) write
``obs_x_resolved`` / ``obs_special_resolved``, which ``filter_observations(resolved=True)`` then reads.  The store keeps no fits, so a
resolve refits its observations as ONE prepared device batch and hands that plan to mapping.resolve.resolve_batches_on_plan: the
coupled QPs are assembled from the members' final P and q where they lie (csrc/resolve.hip) and solved there.

Not here (out of scope): file readers, psi interpolation, pickling."""
import warnings

import numpy as np

from . import drtmd as _driver
from . import nddata
from . import predict as _predict
from .ndx import filter_ndx
from . import resolve as _resolve
from .resolve import get_tau_indices
from .table import new_special, tau_slots


class DRTMD:
    def __init__(self, tau_supergrid, drt=None, fit_kw=None, fit_type='drt', pfrt_factors=None, drt_var=True, llh_kw=None,
                 rss_kw=None, psi_dim_names=None, store_eval_var=False, **drt_kw):
        from ..models import DRT
        self.tau_supergrid = np.asarray(tau_supergrid, dtype=float)
        self.drt1d = drt if drt is not None else DRT(tau_supergrid=self.tau_supergrid, **drt_kw)      # drtmd.py:52-58
        if fit_type not in ('drt', 'pfrt'):
            raise ValueError(f"Invalid fit_type {fit_type}. Options: ['drt', 'pfrt']")          # drtmd.py:1479-1482
        self.fit_type = fit_type
        defaults = {'nonneg': True}                                                                # drtmd.py:89-96
        defaults.update(fit_kw or {})
        self.fit_kw = defaults
        # (upstream's attribute says logspace(-0.7, 0.7, 11), drtmd.py:98-100, but its fits never receive it and run with
        # _pfrt_fit_core's own logspace(-1, 1, 11) -- mapping.fit_observations_pfrt's docstring; None = that behaviour)
        self.pfrt_factors = None if pfrt_factors is None else np.asarray(pfrt_factors, dtype=float)
        n_steps = 11 if self.pfrt_factors is None else len(self.pfrt_factors)
        self.drt_var = bool(drt_var)
        self.llh_kw, self.rss_kw = _driver._metric_kw(llh_kw, rss_kw)                            # drtmd.py:127-129
        self.psi_dim_names = psi_dim_names
        self.obs_psi = None if psi_dim_names is None else np.zeros((0, len(psi_dim_names)))
        self.obs_data, self.obs_group_id, self.obs_fit_errors, self.obs_tau_indices = [], [], [], []
        self.obs_ignore_flag = np.zeros(0, dtype=bool)
        self.obs_fit_status = np.zeros(0, dtype=bool)
        nt = len(self.tau_supergrid)
        self.obs_x = np.zeros((0, nt)) if fit_type == 'drt' else np.zeros((0, n_steps, nt))
        self.obs_drt_var = np.zeros_like(self.obs_x)
        self.obs_x_filt = np.zeros_like(self.obs_x)
        self.obs_special = None
        self.obs_special_filt = {}
        # None until the first resolve_observations / resolve_group (or until a caller that resolved elsewhere sets them)
        self.obs_x_resolved, self.obs_special_resolved = None, None
        self.obs_llh, self.obs_rss = np.zeros(0), np.zeros(0)
        self.obs_data_badness, self.obs_fit_badness = np.zeros(0), np.zeros(0)                   # drtmd.py:121-122
        self.last_fit_index = np.zeros(0, dtype=int)          # what the last fit_observations call sent to the device
        # the raw (unclamped) variances of f and fxx on get_tau_eval(10), NaN until the observation is fitted; only on request: a
        # store built without the keyword has neither attribute
        self.store_eval_var = bool(store_eval_var)
        if self.store_eval_var:
            if fit_type == 'pfrt':
                raise NotImplementedError("store_eval_var with fit_type='pfrt': one variance per factor is not built")
            neval = len(self.get_tau_eval(_predict.DEFAULT_PPD))
            self.obs_f_var, self.obs_fxx_var = np.zeros((0, neval)), np.zeros((0, neval))

    @property
    def num_obs(self):
        return len(self.obs_data)

    def add_observation(self, psi, chrono_data, eis_data, group_id=None, fit=False):
        """drtmd.py:186-241: append one observation (unfitted, not ignored); ``fit=True`` fits it right away"""
        psi = np.atleast_1d(psi).astype(float).flatten()
        if self.obs_psi is None:
            self.obs_psi = np.zeros((0, len(psi)))
        if len(psi) != self.obs_psi.shape[1]:
            raise ValueError(f'psi must have length {self.obs_psi.shape[1]}')
        self.obs_psi = np.vstack([self.obs_psi, psi[None]])
        self.obs_data.append((chrono_data, eis_data))
        self.obs_group_id.append(group_id)
        self.obs_ignore_flag = np.append(self.obs_ignore_flag, False)
        self.obs_fit_status = np.append(self.obs_fit_status, False)
        self.obs_fit_errors.append(None)
        self.obs_tau_indices.append(None)
        self.obs_x = np.concatenate([self.obs_x, np.zeros((1,) + self.obs_x.shape[1:])])
        self.obs_drt_var = np.concatenate([self.obs_drt_var, np.zeros((1,) + self.obs_drt_var.shape[1:])])
        self.obs_x_filt = np.concatenate([self.obs_x_filt, np.zeros((1,) + self.obs_x_filt.shape[1:])])
        for key, val in self.obs_special_filt.items():
            self.obs_special_filt[key] = np.concatenate([val, np.zeros((1,) + val.shape[1:])])
        if self.obs_x_resolved is not None:
            self.obs_x_resolved = np.concatenate([self.obs_x_resolved, np.zeros((1,) + self.obs_x_resolved.shape[1:])])
        for key, val in (self.obs_special_resolved or {}).items():
            self.obs_special_resolved[key] = np.concatenate([val, np.zeros((1,) + val.shape[1:])])
        self.obs_llh, self.obs_rss = np.append(self.obs_llh, 0.0), np.append(self.obs_rss, 0.0)
        self.obs_data_badness, self.obs_fit_badness = np.append(self.obs_data_badness, 0.0), np.append(self.obs_fit_badness, 0.0)
        if self.obs_special is not None:
            for key in self.obs_special:
                val = self.obs_special[key]
                self.obs_special[key] = np.concatenate([val, np.zeros((1,) + val.shape[1:])])
        if self.store_eval_var:
            nan_row = np.full((1, self.obs_f_var.shape[1]), np.nan)
            self.obs_f_var, self.obs_fxx_var = np.concatenate([self.obs_f_var, nan_row]), np.concatenate([self.obs_fxx_var, nan_row])
        if fit:
            self.fit_observation(self.num_obs - 1)

    def get_obs_data(self, obs_index):
        return self.obs_data[obs_index]

    def fit_observation(self, obs_index, ignore_errors=False):
        self.fit_observations([obs_index], ignore_errors=ignore_errors)

    def fit_observations(self, obs_index, ignore_errors=False):
        """drtmd.py:303-319: the listed observations, as one device job"""
        idx = np.asarray(obs_index, dtype=int).ravel()
        self.last_fit_index = idx
        if len(idx) == 0:
            return
        eval_kw = dict(eval_var_tau=self.get_tau_eval(_predict.DEFAULT_PPD)) if self.store_eval_var else {}
        obs_x, obs_special, res = _driver.fit_observations(
            self.drt1d, observations=[self.obs_data[i] for i in idx], tau_supergrid=self.tau_supergrid, drt_var=self.drt_var,
            ignore_errors=True, llh_kw=self.llh_kw, rss_kw=self.rss_kw, fit_type=self.fit_type,
            pfrt_factors=self.pfrt_factors if self.fit_type == 'pfrt' else None, **eval_kw, **self.fit_kw)
        ok = np.asarray(res['obs_fit_status'], dtype=bool)
        first_bad = int(np.argmin(ok)) if not ok.all() else len(idx)
        # without ignore_errors the reference's loop stops at the first failure: what came before it is stored, the rest is not
        seen = np.arange(len(idx)) if ignore_errors else np.arange(first_bad)
        good, bad = seen[ok[seen]], seen[~ok[seen]]
        if len(good):
            rows = idx[good]
            self.obs_x[rows] = obs_x[good]
            self.obs_llh[rows], self.obs_rss[rows] = res['obs_llh'][good], res['obs_rss'][good]
            if self.drt_var and 'obs_drt_var' in res:
                self.obs_drt_var[rows] = res['obs_drt_var'][good]
            if self.store_eval_var:
                self.obs_f_var[rows], self.obs_fxx_var[rows] = res['obs_f_var'][good], res['obs_fxx_var'][good]
            if self.obs_special is None:                          # initialize_obs_special, drtmd.py:270-271
                self.obs_special = {}
            for key, val in obs_special.items():
                if key not in self.obs_special:
                    self.obs_special[key] = new_special(self.num_obs, val)
                self.obs_special[key][rows] = np.asarray(val)[good]
            self.obs_fit_status[rows] = True
            slots = tau_slots(res['obs_tau_indices'], len(idx))
            for j in good:
                self.obs_tau_indices[idx[j]] = tuple(slots[j].tolist())
                self.obs_fit_errors[idx[j]] = None
        self.obs_fit_status[idx[bad]], self.obs_ignore_flag[idx[bad]] = False, True          # drtmd.py:292-299
        for j in bad:
            self.obs_fit_errors[idx[j]] = res['obs_fit_errors'][j]
        if not ignore_errors and first_bad < len(idx):
            print(f"Error encountered at obs_index {idx[first_bad]}")
            raise res['obs_fit_errors'][first_bad]

    def fit_all(self, refit=False, ignore_errors=False):
        """drtmd.py:321-329: everything (refit=True) or only what is neither fitted nor ignored"""
        if refit:
            fit_index = np.arange(self.num_obs)
        else:
            fit_index = np.where(~self.obs_fit_status & ~self.obs_ignore_flag)[0]
        self.fit_observations(fit_index, ignore_errors=ignore_errors)
        return fit_index

    def get_group_index(self, group_id, psi_sort_dims=None, exclude_flagged=False):
        """drtmd.py:1194-1225: observation indices of a group (a string) or of several (a list), optionally sorted by psi
        dimensions -- within groups when several are given"""
        ids = np.array(self.obs_group_id)
        single = type(group_id) == str                                                           # noqa: E721 (as upstream)
        obs_index = np.where(ids == group_id)[0] if single else np.where(np.isin(ids, group_id))[0]
        if psi_sort_dims is not None:
            sort_vals = [self.obs_psi[obs_index, self.psi_dim_names.index(d)] for d in psi_sort_dims]
            if not single:
                sort_vals = [ids[obs_index]] + sort_vals
            obs_index = obs_index[np.lexsort(sort_vals[::-1])]
        if exclude_flagged:
            obs_index = obs_index[~self.obs_ignore_flag[obs_index]]
        return obs_index

    # ---- resolution (drtmd.py:432-559) ----
    def _resolve_selection(self, obs_index, psi_sort_dims):
        """fitted and not ignored, in the order of psi_sort_dims (drtmd.py:436-443, 492-505)"""
        obs_index = np.asarray(obs_index, dtype=int).ravel()
        obs_index = obs_index[self.obs_fit_status[obs_index] & ~self.obs_ignore_flag[obs_index]]
        if psi_sort_dims is not None:
            sort_vals = [self.obs_psi[obs_index, self.psi_dim_names.index(d)] for d in psi_sort_dims][::-1]
            obs_index = obs_index[np.lexsort(sort_vals)]
        return obs_index

    def _resolved_arrays(self):
        if self.fit_type == 'pfrt':
            raise NotImplementedError("fit_type='pfrt': resolve takes one DRT per observation")
        if self.obs_x_resolved is None:
            self.obs_x_resolved = np.zeros_like(self.obs_x)
        if self.obs_special_resolved is None:
            # initialize_obs_special (drtmd.py:1160-1166): zeros under every fitted special parameter -- v_baseline and vz_offset,
            # which a resolve eliminates, keep them
            self.obs_special_resolved = {key: np.zeros_like(val) for key, val in (self.obs_special or {}).items()}

    def _write_resolved_special(self, obs_index, special):
        for key, val in special.items():
            if key not in self.obs_special_resolved:
                self.obs_special_resolved[key] = new_special(self.num_obs, val)
            self.obs_special_resolved[key][obs_index] = val

    def _refit_members(self, obs_index):
        """The store keeps no fits: the selected observations once more, as ONE prepared device batch through the driver.  Returns
        the plan, still holding that batch, and one view per observation of what resolve reads from a fit beside P and q
        (DRT.batch_fits).  Nothing of the store is written.  EIS-only observations raise upstream's KeyError: get_offset_pq needs
        the v_baseline / vz_offset of a joint fit."""
        observations = [self.obs_data[i] for i in obs_index]
        if all(kind == 'eis' for kind, _ in _driver.observation_groups(observations)):
            raise KeyError('v_baseline')
        _, _, res = _driver.fit_observations(self.drt1d, observations=observations, tau_supergrid=self.tau_supergrid, drt_var=False,
                                             ignore_errors=True, llh_kw=self.llh_kw, rss_kw=self.rss_kw, **self.fit_kw)
        if len(res['groups']) != 1:
            raise NotImplementedError("resolve on the store takes observations that share one protocol (data type, sampling grids): "
                                      f"these fall into {len(res['groups'])} device batches; use mapping.resolve.resolve_group on "
                                      "their fits")
        if not np.all(res['obs_fit_status']):
            raise RuntimeError(f"observation {obs_index[int(np.argmin(res['obs_fit_status']))]} was fitted before and failed now")
        return self.drt1d._plan, self.drt1d.batch_fits(with_p=False)

    def _resolve_batches(self, obs_index, starts, batch_size, overlap, truncate, sigma, lambda_psi, tau_filter_sigma,
                         special_filter_sigma):
        """the batches of sorted observations obs_index -> (obs_x_resolved rows (len(obs_index), num_tau), specials) averaged over the
        overlaps.  Assembled and solved on the device from the refitted plan; with a tau or special filter the coupled P is dense
        across its blocks, which the device assembly does not build: those go through the host-assembled path
        (mapping.resolve.resolve_group on the members' downloaded P)."""
        tau_indices = [self.obs_tau_indices[i] for i in obs_index]
        nonneg, nsup = self.fit_kw['nonneg'], len(self.tau_supergrid)
        plan, members = self._refit_members(obs_index)
        if tau_filter_sigma > 0 or special_filter_sigma > 0:
            fits = self.drt1d.batch_fits()
            out = _resolve.resolve_group(fits, tau_indices, nonneg, nsup, batch_size=batch_size, overlap=overlap, truncate=truncate,
                                         sigma=sigma, lambda_psi=lambda_psi, tau_filter_sigma=tau_filter_sigma,
                                         special_filter_sigma=special_filter_sigma, device=self.drt1d.device)
            self.last_resolve = dict(_resolve.resolve_group.last_qp, path='host')
            return out
        x_sol, matches, special, iterations = _resolve.resolve_batches_on_plan(
            plan, members, tau_indices, nonneg, starts, batch_size, truncate=truncate, sigma=sigma, lambda_psi=lambda_psi)
        self.last_resolve = dict(iterations=iterations, path='device')
        return _resolve.average_batches(members, starts, batch_size, overlap, nsup, x_sol, matches, special)

    def resolve_observations(self, obs_index, psi_sort_dims=None, truncate=False, sigma=1, lambda_psi=1, tau_filter_sigma=0,
                             special_filter_sigma=0):
        """drtmd.py:432-484: the listed observations (fitted, not ignored, sorted along psi_sort_dims) re-optimised as ONE coupled
        problem, into obs_x_resolved (inside their common tau range) and obs_special_resolved.  One observation: its raw parameters
        are copied, with upstream's warning.  tau_filter_sigma / special_filter_sigma > 0 fall back to the host-assembled path
        (_resolve_batches).  Raises ValueError when the QP breaks down (cvxopt's error), KeyError for EIS-only observations."""
        obs_index = self._resolve_selection(obs_index, psi_sort_dims)
        if len(obs_index) == 0:
            warnings.warn("No valid observations included in resolution group")
            return
        self._resolved_arrays()
        if len(obs_index) == 1:
            warnings.warn("Only one observation included in resolution group; raw parameters will be copied")
            left, right = self.obs_tau_indices[obs_index[0]]
            self.obs_x_resolved[obs_index, left:right] = self.obs_x[obs_index, left:right]
            self._write_resolved_special(obs_index, {k: v[obs_index] for k, v in (self.obs_special or {}).items()})
            return
        left, right = get_tau_indices([self.obs_tau_indices[i] for i in obs_index], truncate=truncate)
        x_res, sp_res = self._resolve_batches(obs_index, [0], len(obs_index), 0, truncate, sigma, lambda_psi, tau_filter_sigma,
                                              special_filter_sigma)
        self.obs_x_resolved[obs_index, left:right] = x_res[:, left:right]
        self._write_resolved_special(obs_index, sp_res)

    def resolve_group(self, group_id, batch_size=7, overlap=2, psi_sort_dims=None, truncate=False, sigma=1, lambda_psi=1,
                      tau_filter_sigma=0, special_filter_sigma=0):
        """drtmd.py:486-559: the group's observations (fitted, not ignored, sorted along psi_sort_dims) in overlapping batches of
        batch_size, every batch one coupled problem, the overlaps averaged with weights growing with the distance from the batch
        edge (mapping.resolve.group_batch_starts, average_batches); obs_x_resolved rows of the group are cleared first.  All batches
        are assembled on the device from one refit of the group and solved there, one launch per problem size.  Raises ValueError
        for a group of one observation and when a QP breaks down, KeyError for EIS-only observations."""
        obs_index = self._resolve_selection(self.get_group_index(group_id), psi_sort_dims)
        if len(obs_index) == 0:
            warnings.warn("No valid observations included in resolution group")
            return
        self._resolved_arrays()
        self.obs_x_resolved[obs_index] = 0
        if len(obs_index) == 1:
            raise ValueError("Only one observation included in resolution group")
        batch_size, starts = _resolve.group_batch_starts(len(obs_index), batch_size, overlap)
        x_res, sp_res = self._resolve_batches(obs_index, starts, batch_size, overlap, truncate, sigma, lambda_psi, tau_filter_sigma,
                                              special_filter_sigma)
        self.obs_x_resolved[obs_index] = x_res
        self._write_resolved_special(obs_index, sp_res)

    def filter_observations(self, obs_index, psi_sort_dims=None, truncate=False, resolved=True, special_kw=None, **kw):
        """drtmd.py:561-628: smooth the fitted coefficients of the listed observations across psi (rows, in the order of
        psi_sort_dims) and tau with mapping.ndx.filter_ndx(**kw) on the device, into obs_x_filt / obs_special_filt.  x_dop is
        filtered with kw, the other specials with special_kw (None: kw without the tau entry of a non-scalar sigma / max_sigma);
        vz_offset and v_baseline are data-dependent and copied."""
        obs_index = np.asarray(obs_index, dtype=int).ravel()
        obs_index = obs_index[self.obs_fit_status[obs_index] & ~self.obs_ignore_flag[obs_index]]
        if psi_sort_dims is not None:
            sort_vals = [self.obs_psi[obs_index, self.psi_dim_names.index(d)] for d in psi_sort_dims][::-1]
            obs_index = obs_index[np.lexsort(sort_vals)]
        if resolved and (self.obs_x_resolved is None or self.obs_special_resolved is None):
            raise ValueError("resolved=True needs obs_x_resolved / obs_special_resolved: run resolve_group / resolve_observations "
                             "first (or set them), or pass resolved=False to filter the fitted parameters")
        x_drt_in = self.obs_x_resolved if resolved else self.obs_x
        special_in = (self.obs_special_resolved if resolved else self.obs_special) or {}
        if special_kw is None:
            special_kw = kw.copy()
            for key in ("max_sigma", "sigma"):
                if key in special_kw and not np.isscalar(special_kw[key]):
                    special_kw[key] = special_kw[key][:-1]                  # the tau axis
        if len(obs_index) == 0:
            warnings.warn("No valid observations included in resolution group")
            return
        obs_tau_indices = [self.obs_tau_indices[i] for i in obs_index]
        if len(obs_index) == 1:
            warnings.warn("Only one observation included in filter; raw parameters will be copied")
            left, right = obs_tau_indices[0]
            x_drt = x_drt_in[obs_index, left:right]
            special = {k: v[obs_index] for k, v in special_in.items()}
        else:
            left, right = get_tau_indices(obs_tau_indices, truncate=truncate)
            x_drt = filter_ndx(x_drt_in[obs_index, left:right], num_group_dims=0, **kw)
            special = {}
            for k, v in special_in.items():
                if k in ("vz_offset", "v_baseline"):
                    special[k] = v[obs_index]
                else:
                    special[k] = filter_ndx(v[obs_index], num_group_dims=0, **(kw if k == "x_dop" else special_kw))
        self.obs_x_filt[obs_index, left:right] = x_drt
        for key, val in special.items():
            if key not in self.obs_special_filt:
                self.obs_special_filt[key] = new_special(self.num_obs, val)
            self.obs_special_filt[key][obs_index] = val

    def filter_group(self, group_id, psi_sort_dims=None, truncate=False, resolved=True, special_kw={}, **kw):   # noqa: B006
        """drtmd.py:630-635.  special_kw is forwarded as given: with upstream's default {} the special parameters are filtered
        without a sigma, which fails there and here -- pass special_kw=None for the derived keywords"""
        return self.filter_observations(self.get_group_index(group_id), psi_sort_dims, truncate=truncate, resolved=resolved,
                                        special_kw=special_kw, **kw)

    # ---- data / fit validation (drtmd.py:639-783) ----
    @staticmethod
    def _score_rows(statement, device):
        if statement:
            return nddata.score_rows_statement
        return lambda *a, **kw: nddata.score_rows(*a, device=device, **kw)

    def score_group_data_badness(self, group_id, psi_sort_dims, median_filter_size=(3, 1), std_size=(5, 3), ignore_outliers=True,
                                 impute=False, statement=False, device=0):
        """drtmd.py:642-735: the badness of every observation's raw data within a group, into obs_data_badness -- the mean
        squared deviation of its chrono voltage (centred and scaled by its 2 % / 98 % percentiles) and of its impedance from
        the median across neighbouring observations (rows in the order of psi_sort_dims), in units of the local robust spread;
        with ignore_outliers, single outlier points are dropped first where they are fewer than 5 % of an observation.

        Where upstream runs (every observation has EIS data, at least one has chrono data) the result is upstream's.  Beyond
        that: a group without chrono data is scored on its EIS part alone, one without EIS data on its chrono
        part alone, and an observation that lacks one part is a NaN row of that array.  impute=True fails upstream and is not
        built.  statement=True evaluates the numpy statement (mapping.nddata.score_rows_statement) instead of the device chain."""
        if impute:
            raise NotImplementedError("impute=True is not built (upstream raises TypeError there: impute_nans without a sigma)")
        score = self._score_rows(statement, device)
        obs_index = self.get_group_index(group_id, psi_sort_dims=psi_sort_dims)
        if len(obs_index) == 0:
            return
        data_list = [self.get_obs_data(i) for i in obs_index]
        iv_data = [dl[0] for dl in data_list]
        z_list = [None if dl[1] is None else dl[1][1] for dl in data_list]

        v_len = np.array([0 if tup is None or tup[0] is None else len(tup[0]) for tup in iv_data])
        has_chrono = v_len > 0
        has_eis = np.array([z is not None for z in z_list])
        v_len = np.unique(v_len[v_len > 0])
        if len(v_len) > 1:
            raise ValueError(f'Found chrono data with different lengths: {v_len}')
        v_rss, z_rss = np.zeros(len(obs_index)), np.zeros(len(obs_index))
        if has_chrono.any():
            nan_row = np.full(v_len[0], np.nan)
            i_array = np.stack([np.asarray(tup[1], dtype=float) if ok else nan_row for tup, ok in zip(iv_data, has_chrono)], axis=0)
            v_array = np.stack([np.asarray(tup[2], dtype=float) if ok else nan_row for tup, ok in zip(iv_data, has_chrono)], axis=0)
            v_rss = score(v_array, median_filter_size, std_size, scale_src=i_array, ignore_outliers=ignore_outliers)
        if has_eis.any():
            # EIS data: truncated to the shortest length (hybrid measurements)
            z_len = min(len(z) for z in z_list if z is not None)
            nan_row = np.full(2 * z_len, np.nan)
            z_array = np.stack([nan_row if z is None else np.concatenate([np.real(z[:z_len]), np.imag(z[:z_len])]) for z in z_list],
                               axis=0)
            z_rss = score(z_array, median_filter_size, std_size, ignore_outliers=ignore_outliers)

        tot_rss = np.zeros(len(obs_index))
        hybrid_index = has_eis & has_chrono
        eis_index = has_eis & ~has_chrono
        chrono_index = has_chrono & ~has_eis
        tot_rss[hybrid_index] = 0.5 * (v_rss[hybrid_index] + z_rss[hybrid_index])
        tot_rss[eis_index] = z_rss[eis_index]
        tot_rss[chrono_index] = v_rss[chrono_index]
        self.obs_data_badness[obs_index] = tot_rss

    def score_group_fit_badness(self, group_id, psi_sort_dims, median_size=(3, 3), std_size=(5, 3), include_special=False,
                                statement=False, device=0):
        """drtmd.py:737-783: the badness of every observation's fitted DRT within a group, into obs_fit_badness -- its mean
        squared deviation from the median across neighbouring observations and tau, in units of the local robust spread.
        Ignored and unfitted observations are NaN rows and score 0.  include_special=True fails upstream for scalar special
        parameters and is not built."""
        if include_special:
            raise NotImplementedError("include_special=True is not built (upstream raises RuntimeError for any scalar special "
                                      "parameter: a 2-D median_size on a 1-D array)")
        obs_index = self.get_group_index(group_id, psi_sort_dims=psi_sort_dims)
        if len(obs_index) == 0:
            return
        x_array = self.obs_x[obs_index].copy()
        if x_array.ndim != 2:
            raise NotImplementedError("fit_type='pfrt': the fit score takes one DRT per observation")
        ignore = self.obs_ignore_flag[obs_index] | ~self.obs_fit_status[obs_index]
        x_array[ignore] = np.nan
        self.obs_fit_badness[obs_index] = self._score_rows(statement, device)(x_array, median_size, std_size)

    # ---- prediction (drtmd.py:788-1106) ----
    def validate_psi(self, psi):
        """drtmd.py:1168-1184"""
        if self.psi_dim_names is not None:
            psi_len = len(self.psi_dim_names)
        elif self.obs_psi is not None:
            psi_len = self.obs_psi.shape[1]
        else:
            psi_len = None
        psi = np.atleast_2d(psi)
        if psi_len is not None and psi_len != np.shape(psi)[1]:
            raise ValueError(f'Dimensions of provided psi ({np.shape(psi)[1]}) do not match shape of existing psi array '
                             f'({None if self.obs_psi is None else self.obs_psi.shape})')
        return psi

    def get_psi_index(self, psi):
        """drtmd.py:1186-1188: the observation index of every row of psi (8 significant digits), -1 where it was not observed"""
        psi = np.asarray(self.validate_psi(psi), dtype=float)
        return _predict.row_match_index(self.obs_psi, psi, precision=8)

    def get_tau_eval(self, ppd, extend_decades=0):
        """drtmd.py:1252-1263"""
        return _predict.tau_eval(self.tau_supergrid, ppd, extend_decades)

    @property
    def tau_basis_area(self):
        """drtmd.py:1292-1293 (gaussian basis)"""
        return float(np.sqrt(np.pi) / self.drt1d.tau_epsilon)

    def _map_rows(self, psi, percentile=None, factor_index=None):
        """the checks every prediction shares -> (observation indices, their coefficient rows with NaN rows for what is unfitted or
        ignored)"""
        if self.fit_type == 'pfrt':
            raise NotImplementedError("fit_type='pfrt': the prediction block takes one DRT per observation (factor_index is not built)")
        if percentile is not None:
            raise NotImplementedError("percentile= needs the parameter covariances, which the store does not keep")
        index = self.get_psi_index(psi)
        if len(index) == 0 or np.min(index) < 0:
            raise NotImplementedError("psi that is not an observed coordinate: resampling between observations is not built")
        x = self.obs_x[index].copy()
        x[self.obs_ignore_flag[index] | ~self.obs_fit_status[index]] = np.nan
        return index, x

    def _tables(self, ndfilter, filter_func, filter_kw):
        """the device filter's tables (None: no filter, or a callable that the host applies)"""
        return _predict.filter_tables(ndfilter and filter_func is None, filter_kw)

    @staticmethod
    def _host_filter(a, ndfilter, filter_func, filter_kw):
        """apply_filter (_filters.py:506-518) with a callable: filter_func(a, **filter_kw), as upstream calls it"""
        if ndfilter and filter_func is not None:
            return filter_func(a, **filter_kw)
        return a

    def _map_predict(self, statement, device, x, tau, want, normalize=False, tables=None, f_var=None, fxx_var=None, var_stored=False,
                     ext=None, search=1, height=1e-3, prominence=5e-3, peak_spread_sigma=None):
        """one pass of the chain on rows x: the device call, or with statement=True the same stages in numpy"""
        eps, area = self.drt1d.tau_epsilon, self.tau_basis_area
        ln_sup, ln_ev = np.log(self.tau_supergrid), np.log(tau)
        if not statement:
            from .. import _ffi
            spread = {}
            if peak_spread_sigma is not None:
                spread = dict(spread_table=_predict.gaussian_tables((peak_spread_sigma,))[0],
                              spread_factor=_predict.spread_factor(peak_spread_sigma))
            return _ffi.get_context(device).map_predict(x, ln_sup, ln_ev, eps, area, normalize, tables, f_var, fxx_var, var_stored, ext,
                                                        search, height, prominence, want=want, **spread)
        res = {}
        xf = _predict.map_x_statement(x, area, normalize, tables)
        res['x'] = xf
        if any(w in want for w in ('f', 'fxx', 'peak_prob', 'curv_prob')):
            res['f'], res['fxx'] = (_predict.map_drt_statement(xf, ln_sup, ln_ev, eps, o) for o in (0, 2))
        if f_var is not None:
            vf, vxx = np.array(f_var, dtype=float), np.array(fxx_var, dtype=float)
            if var_stored:
                if ext is not None:
                    vf, vxx = _predict.clamp_rows(vf, ext), _predict.clamp_rows(vxx, ext)
                vf, vxx = _predict.correlate_tables(vf, tables), _predict.correlate_tables(vxx, tables)
            res['f_var'], res['fxx_var'] = vf, vxx
            with np.errstate(invalid='ignore', divide='ignore'):
                if 'peak_prob' in want:
                    pk = _predict.peak_rows(res['f'], res['fxx'], vf, vxx, search, height, prominence)
                    if peak_spread_sigma is not None:
                        pk = _predict.spread_statement(pk, peak_spread_sigma)
                    res['peak_prob'] = pk * np.sign(res['f'])
                if 'curv_prob' in want:
                    from ..models import peaks
                    res['curv_prob'] = peaks.curv_prob_row(res['f'], res['fxx'], vf, vxx)
        return {w: res[w] for w in want}

    def predict_x(self, psi, factor_index=None, percentile=None, normalize=False, ndfilter=False, filter_func=None, resample_dims=None,
                  filter_kw=None, statement=False, device=0):
        """drtmd.py:797-835: the coefficient rows of the observations at psi, in the order of psi -- normalised by their absolute
        R_p first, then filtered.  filter_func=None filters on the device: gaussian_filter(sigma=(1, 0)) with no filter_kw, else
        filter_kw={'sigma': ...}; a callable is applied on the host as apply_filter applies it.  Rows of unfitted or ignored
        observations are NaN (and spread through a psi filter as scipy spreads them)."""
        _, x = self._map_rows(psi, percentile, factor_index)
        tables = self._tables(ndfilter, filter_func, filter_kw)
        if normalize or tables is not None:
            x = self._map_predict(statement, device, x, self.tau_supergrid, ('x',), normalize=normalize, tables=tables)['x']
        return self._host_filter(x, ndfilter, filter_func, filter_kw)

    def predict_r_p(self, psi=None, x=None, factor_index=None, absolute=False, **kw):
        """drtmd.py:788-795"""
        if x is None:
            x = self.predict_x(psi, factor_index=factor_index, **kw)
        if absolute:
            x = np.abs(x)
        return np.sum(x, axis=-1) * self.tau_basis_area

    def predict_drt(self, psi=None, tau=None, x=None, order=0, factor_index=None, normalize=False, statement=False, device=0, **kw):
        """drtmd.py:837-851: x E' on tau (None: the supergrid) for order 0 or 2 (statement=True: any order); normalize divides the
        filtered x by its absolute R_p"""
        if x is None:
            x = self.predict_x(psi, factor_index=factor_index, normalize=False, statement=statement, device=device, **kw)
        tau = self.tau_supergrid if tau is None else np.asarray(tau, dtype=float)
        if statement:
            xn = _predict.map_x_statement(x, self.tau_basis_area, normalize)
            return _predict.map_drt_statement(xn, np.log(self.tau_supergrid), np.log(tau), self.drt1d.tau_epsilon, order)
        if order not in (0, 2):
            raise NotImplementedError("the device chain evaluates orders 0 and 2; pass statement=True for order 1")
        name = 'f' if order == 0 else 'fxx'
        return self._map_predict(False, device, np.asarray(x, dtype=float), tau, (name,), normalize=normalize)[name]

    def _stored_var(self, obs_index, tau, order):
        if not self.store_eval_var:
            raise NotImplementedError("the store keeps no covariances: build it with store_eval_var=True to keep the variances of "
                                      "every fit on get_tau_eval(10)")
        stored = self.get_tau_eval(_predict.DEFAULT_PPD)
        if tau is not None and not (np.shape(tau) == stored.shape and np.array_equal(np.asarray(tau, dtype=float), stored)):
            raise NotImplementedError("the variances are stored on get_tau_eval(10) only: another grid needs the covariances")
        if order not in (0, 2):
            raise NotImplementedError("the variances are stored for orders 0 and 2 only")
        obs_index = np.atleast_1d(np.asarray(obs_index, dtype=int))
        return obs_index, stored, (self.obs_f_var if order == 0 else self.obs_fxx_var)[obs_index]

    def predict_drt_var(self, obs_index, tau=None, x_cov=None, order=0, factor_index=None, extend_var=True, ndfilter=False,
                        filter_func=None, filter_kw=None, statement=False, device=0):
        """drtmd.py:1012-1021 from the stored rows (store_eval_var=True): the variance of the DRT (order 0) or of its curvature
        (order 2) on get_tau_eval(10) -- tau=None means that grid here -- with the map clamp (extend_var) and the filter"""
        if x_cov is not None:
            raise NotImplementedError("x_cov=: the device chain starts from the stored variance rows, not from covariances")
        if self.fit_type == 'pfrt':
            raise NotImplementedError("fit_type='pfrt': the prediction block takes one DRT per observation")
        obs_index, tau, var = self._stored_var(obs_index, tau, order)
        ext = _predict.clamp_index_rows(tau, self.tau_supergrid, [self.obs_tau_indices[i] for i in obs_index]) if extend_var else None
        tables = self._tables(ndfilter, filter_func, filter_kw)
        if ext is not None or tables is not None:
            var = self._map_predict(statement, device, self.obs_x[obs_index], tau, ('f_var',), tables=tables, f_var=var, fxx_var=var,
                                    var_stored=True, ext=ext)['f_var']
        return self._host_filter(var, ndfilter, filter_func, filter_kw)

    def _prob_map(self, which, psi, x, f_var, fxx_var, tau, factor_index, extend_var, ndfilter, filter_func, filter_kw, normalize,
                  statement, device, **peak_kw):
        tau = self.get_tau_eval(_predict.DEFAULT_PPD) if tau is None else np.asarray(tau, dtype=float)
        if self.fit_type == 'pfrt':
            raise NotImplementedError("fit_type='pfrt': the prediction block takes one DRT per observation")
        if x is None and f_var is None and fxx_var is None and filter_func is None:
            # everything comes from the store: one upload, one download
            index, xr = self._map_rows(psi, None, factor_index)
            _, tau, vf = self._stored_var(index, tau, 0)
            vxx = self.obs_fxx_var[index]
            ext = _predict.clamp_index_rows(tau, self.tau_supergrid, [self.obs_tau_indices[i] for i in index]) if extend_var else None
            return self._map_predict(statement, device, xr, tau, (which,), normalize=normalize, tables=self._tables(ndfilter, None, filter_kw),
                                     f_var=vf, fxx_var=vxx, var_stored=True, ext=ext, **peak_kw)[which]
        filt = dict(ndfilter=ndfilter, filter_func=filter_func, filter_kw=filter_kw, statement=statement, device=device)
        if x is None:
            x = self.predict_x(psi, factor_index=factor_index, normalize=normalize, **filt)
        if f_var is None or fxx_var is None:
            index = self.get_psi_index(psi)
            if f_var is None:
                f_var = self.predict_drt_var(index, tau=tau, order=0, factor_index=factor_index, extend_var=extend_var, **filt)
            if fxx_var is None:
                fxx_var = self.predict_drt_var(index, tau=tau, order=2, factor_index=factor_index, extend_var=extend_var, **filt)
        return self._map_predict(statement, device, np.asarray(x, dtype=float), tau, (which,), f_var=f_var, fxx_var=fxx_var,
                                 **peak_kw)[which]

    def predict_peak_prob(self, psi, x=None, f_var=None, fxx_var=None, tau=None, factor_index=None, extend_var=True, prominence=5e-3,
                          height=1e-3, peak_spread_sigma=None, ndfilter=False, filter_func=None, filter_kw=None, sign=1,
                          statement=False, device=0):
        """drtmd.py:1023-1064: the signed probability of a peak at every point of tau (None: get_tau_eval(10)) for the observations
        at psi.  x is normalised and filtered, the variances are not divided by r_p^2; f_var / fxx_var passed here are used as given
        (neither clamped nor filtered), otherwise the stored rows are taken (store_eval_var=True) with the map clamp and the filter."""
        peak_kw = dict(search=_predict.search_kind(self.fit_kw['nonneg'], sign), height=height, prominence=prominence,
                       peak_spread_sigma=peak_spread_sigma)
        return self._prob_map('peak_prob', psi, x, f_var, fxx_var, tau, factor_index, extend_var, ndfilter, filter_func, filter_kw,
                              True, statement, device, **peak_kw)

    def predict_curv_prob(self, psi=None, x=None, f_var=None, fxx_var=None, tau=None, factor_index=None, extend_var=True,
                          ndfilter=False, filter_func=None, filter_kw=None, statement=False, device=0):
        """drtmd.py:1066-1106: the signed probability that the curvature is negative where f is positive (x unnormalised)"""
        if psi is None and (x is None or f_var is None or fxx_var is None):
            raise ValueError('If psi is not provided, all of x, f_var, and fxx_var must be provided')
        return self._prob_map('curv_prob', psi, x, f_var, fxx_var, tau, factor_index, extend_var, ndfilter, filter_func, filter_kw,
                              False, statement, device)

    def predict_dop(self, *args, **kw):
        raise NotImplementedError("predict_dop: the store keeps no distribution of phasances (upstream marks its x as a TODO)")

    def predict_param_cov(self, *args, **kw):
        raise NotImplementedError("predict_param_cov: the store keeps no fits and no covariances")

    predict_x_cov = predict_x_var = predict_drt_cov = predict_param_cov
