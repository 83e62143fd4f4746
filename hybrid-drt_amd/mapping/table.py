"""The per-observation result table of the mapping drivers: what a map keeps for every observation (DRTMD's obs_x, obs_special,
llh / rss, tau slots, fit status and error: hybdrt/mapping/drtmd.py:245-301), how a fitted group is scattered into it, the error
a failed fit stands for, the rows of doubles a table travels as between ranks, and the merge of consecutive chunks of one map."""
import numpy as np


def failed_fit_error():
    """what the reference raises for an observation whose fit broke down (cvxopt's ValueError at a singular start point)"""
    return ValueError("Rank(A) < p or Rank([P; A; G]) < n")


def fit_errors(ok):
    """one entry per observation: None, or the error of a failed fit"""
    return [None if good else failed_fit_error() for good in ok]


def raise_first_error(res, ignore_errors):
    """fit_observation's error contract (drtmd.py:292-301): without ignore_errors the first failed observation raises"""
    if not ignore_errors and not np.all(res['obs_fit_status']):
        bad = int(np.flatnonzero(~np.asarray(res['obs_fit_status']))[0])
        print(f"Error encountered at obs_index {bad}")
        raise res['obs_fit_errors'][bad]


def zero_failed(ok, val):
    """`val` (leading axis: observations; any rank) with zeros in the rows of failed fits"""
    return np.where(ok.reshape((-1,) + (1,) * (np.ndim(val) - 1)), val, 0.0)


def new_special(num, val):
    """initialize_obs_special / the "key is new" branch of drtmd.py:281-285: zeros for every observation that does not report it"""
    return np.zeros((num,) + np.shape(val)[1:])


def tau_slots(tau_indices, num):
    """obs_tau_indices as (num, 2): one (left, right) for the whole map (shared-grid form) or one per observation"""
    return np.broadcast_to(np.asarray(tau_indices).reshape(-1, 2), (num, 2))


class ObsTable:
    """`num` observations: obs_x (num, *row_shape) with row_shape = (nsup,) or (S, nsup), obs_special, and res with obs_llh, obs_rss,
    obs_fit_status, the path's own ``columns`` {name: dtype | (dtype, trailing shape)}, with ``groups`` obs_group and the list of
    fitted groups, and with ``drt_var`` obs_drt_var / obs_drt_var_ok; obs_tau_indices and obs_fit_errors join them in result()."""

    def __init__(self, num, row_shape, drt_var=False, columns=None, groups=False):
        self.obs_x = np.zeros((num,) + tuple(row_shape))
        self.obs_special = {}
        self.slots = np.zeros((num, 2), dtype=np.int64)
        self.res = dict(obs_llh=np.zeros(num), obs_rss=np.zeros(num), obs_fit_status=np.zeros(num, dtype=bool))
        for name, spec in (columns or {}).items():
            dtype, shape = spec if isinstance(spec, tuple) else (spec, ())
            self.res[name] = np.zeros((num,) + shape, dtype=dtype)
        if groups:
            self.res.update(obs_group=np.zeros(num, dtype=int), groups=[])
        if drt_var:
            self.res.update(obs_drt_var=np.zeros_like(self.obs_x), obs_drt_var_ok=np.zeros(num, dtype=bool))

    def scatter(self, idx, ok, x, span, specials, llh, rss, columns, var=None, vok=None, group=None):
        """The fitted block of the observations `idx` (`ok`: which fits succeeded; failed ones keep zeros everywhere):
        coefficients `x` into the supergrid columns span = (left, right), which become the rows' obs_tau_indices, ``specials``
        {key: (len(idx), ...)}, llh / rss, the block's ``columns`` as they are, `var` (anything that broadcasts to the rows) where
        `vok` and the fit are good; ``group`` = (kind, basis_tau) of the fitted group the block is."""
        res, idx = self.res, np.asarray(idx)
        fill = zero_failed if not ok.all() else (lambda _, val: val)          # (no fit failed: nothing to zero, no copy made)
        self.obs_x[idx, ..., span[0]:span[1]] = fill(ok, x)
        for key, val in specials.items():
            val = np.asarray(val, dtype=float)
            if key not in self.obs_special:
                self.obs_special[key] = new_special(len(self.slots), val)
            self.obs_special[key][idx] = fill(ok, val)
        res['obs_llh'][idx], res['obs_rss'][idx] = fill(ok, llh), fill(ok, rss)
        res['obs_fit_status'][idx] = ok
        for name, val in columns.items():
            res[name][idx] = val
        self.slots[idx] = span
        if group is not None:
            res['obs_group'][idx] = len(res['groups'])
            res['groups'].append(dict(kind=group[0], indices=idx, basis_tau=group[1], tau_indices=span))
        if var is not None:
            vok = np.asarray(vok, dtype=bool) & ok
            res['obs_drt_var'][idx], res['obs_drt_var_ok'][idx] = zero_failed(vok, var), vok

    def scatter_rows(self, idx, block):
        """one rank's packed block (pack_rows) -> the rows `idx`: the fit status is read from the status column"""
        x, special, cols, ti, var, vok = unpack_block(block)
        # (shapes as fit_observations returns them: (num,) for scalar specials, (num, width) for vector-valued ones)
        specials = {key: val if nd > 1 else val[:, 0] for key, (val, nd) in special.items()}
        self.scatter(idx, cols['status'] >= 0, x, (0, x.shape[1]), specials, cols.pop('obs_llh'), cols.pop('obs_rss'), cols,
                     var=var, vok=vok)
        self.slots[idx] = ti                       # (the rows bring the slots their own fits found)

    def result(self, ignore_errors):
        """(obs_x, obs_special, res) with obs_tau_indices as a list of (left, right) and the error every failed fit stands for;
        raises the first of them unless ``ignore_errors``"""
        self.res['obs_tau_indices'] = [tuple(pair) for pair in self.slots.tolist()]
        self.res['obs_fit_errors'] = fit_errors(self.res['obs_fit_status'])
        raise_first_error(self.res, ignore_errors)
        return self.obs_x, self.obs_special, self.res


# ---- a table as rows of doubles (the gather of the sharded driver) -----------------------------------------------------------
GATHER_KEYS = ('obs_llh', 'obs_rss', 'outer_iters', 'qp_iters_total', 'status')
GATHER_COLUMNS = {k: np.int64 for k in GATHER_KEYS[2:]}
# every special parameter a fit can report (x layout of drt1d.py:377-408); the gathered rows name them by position here
SPECIAL_REGISTRY = ('v_baseline', 'vz_offset', 'R_inf', 'inductance', 'C_inv', 'x_dop')


def pack_rows(obs_x, obs_special, res, drt_var):
    """One rank's results as rows of doubles behind ONE header row that describes them, so that `dst` can unpack blocks from
    ranks whose fits reported other special parameters (or none at all) without a second collective:
        header = [nsup, drt_var, n_specials, (registry index, width, ndim) x n_specials, 0 ...]
        row    = [obs_x (nsup) | specials at their real widths | GATHER_KEYS | left, right | obs_drt_var (nsup), ok]
    A result that carries obs_f_var / obs_fxx_var (fit_observations(eval_var_tau=)) adds 2 to the header's drt_var entry, their
    width after the last special's triple and the two blocks at the end of the row; without them nothing changes."""
    num, nsup = obs_x.shape
    unknown = [k for k in obs_special if k not in SPECIAL_REGISTRY]
    if unknown:
        raise NotImplementedError(f'special parameters {unknown} are not known to the sharded driver')
    cols, head = [obs_x], [float(nsup), float(bool(drt_var)), 0.0]
    for ki, key in enumerate(SPECIAL_REGISTRY):
        if obs_special.get(key) is None:
            continue
        raw = np.asarray(obs_special[key], dtype=float)
        val = raw.reshape(num, -1)
        cols.append(val)
        head += [float(ki), float(val.shape[1]), float(raw.ndim)]
        head[2] += 1
    cols += [np.asarray(res[k], dtype=float)[:, None] for k in GATHER_KEYS]
    cols.append(tau_slots(res.get('obs_tau_indices', (0, nsup)), num).astype(float))
    if drt_var:
        cols += [res['obs_drt_var'], np.asarray(res['obs_drt_var_ok'], dtype=float)[:, None]]
    if res.get('obs_f_var') is not None:
        head[1] += 2.0
        head.append(float(res['obs_f_var'].shape[1]))
        cols += [res['obs_f_var'], res['obs_fxx_var']]
    body = np.concatenate(cols, axis=1)
    width = max(body.shape[1], len(head))
    packed = np.zeros((num + 1, width))
    packed[0, :len(head)] = head
    packed[1:, :body.shape[1]] = body
    return packed


def unpack_block(block):
    """inverse of pack_rows for one rank's block (header row first): (obs_x, {special: (2-d array, ndim of the original)}, {key: column}, ti, var, vok)"""
    head, body = block[0], block[1:]
    nsup, drt_var, eval_var, nsp = int(head[0]), bool(int(head[1]) & 1), bool(int(head[1]) & 2), int(head[2])
    obs_x = body[:, :nsup]
    pos = nsup
    special = {}
    for j in range(nsp):
        key, w, nd = SPECIAL_REGISTRY[int(head[3 + 3 * j])], int(head[4 + 3 * j]), int(head[5 + 3 * j])
        special[key] = (body[:, pos:pos + w], nd)
        pos += w
    cols = {k: body[:, pos + j] for j, k in enumerate(GATHER_KEYS)}
    pos += len(GATHER_KEYS)
    ti = body[:, pos:pos + 2]
    pos += 2
    var = vok = None
    if drt_var:
        var, vok = body[:, pos:pos + nsup], body[:, pos + nsup] > 0.5
        pos += nsup + 1
    if eval_var:                                   # (two more columns of the table: they travel with `cols`)
        neval = int(head[3 + 3 * nsp])
        cols['obs_f_var'], cols['obs_fxx_var'] = body[:, pos:pos + neval], body[:, pos + neval:pos + 2 * neval]
    return obs_x, special, cols, ti, var, vok


# ---- consecutive chunks of one shared-grid map -------------------------------------------------------------------------------
NOT_PER_OBS = ('basis_tau', 'timings_ms', 'launches', 'obs_tau_indices', 'obs_fit_errors')


def merge_chunk_results(outs, chunks, ignore_errors):
    """results of fit_observations on consecutive chunks of one map -> the result for the whole map: arrays whose leading length
    is the (first) chunk's are concatenated, everything else is the first chunk's"""
    obs_x = np.concatenate([o[0] for o in outs])
    obs_special = {k: np.concatenate([o[1][k] for o in outs]) for k in outs[0][1]}
    res = {}
    for k, v in outs[0][2].items():
        per_obs = k not in NOT_PER_OBS and isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == len(chunks[0])
        res[k] = np.concatenate([o[2][k] for o in outs]) if per_obs else v
    res['obs_fit_errors'] = [e for o in outs for e in o[2]['obs_fit_errors']]
    raise_first_error(res, ignore_errors)
    return obs_x, obs_special, res
