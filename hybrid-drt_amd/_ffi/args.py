"""Bound: an argument structure together with the numpy arrays its pointer fields refer to.

A ctypes pointer field does not keep its array alive, so every array goes through here: converted, checked against the shapes
the entry point takes, stored in the field and held in ``keep`` for as long as the Bound lives."""
import numpy as np

from .abi import PFRT_SELECT_COMPACT, PFRT_SELECT_ROWS, PfrtSelectOut, ResolveArgs, _p, _pi


class Bound:
    def __init__(self, struct):
        self.c = struct
        self.keep = []

    def hold(self, a):
        """keep `a` alive with the structure (an array that goes into a positional argument, an options structure)"""
        self.keep.append(a)
        return a

    def _store(self, field, v, shapes):
        if shapes is not None:
            allowed = [tuple(s) for s in (shapes if isinstance(shapes, list) else [shapes])]
            if v.shape not in allowed:
                raise ValueError(f"{field}: expected shape {' or '.join(map(str, allowed))}, got {v.shape}")
        setattr(self.c, field, _pi(v) if v.dtype == np.int32 else _p(v))
        return self.hold(v)

    def array(self, field, v, shapes=None, dtype=np.float64, copy=False):
        """`v` as a C-contiguous `dtype` (float64 or int32) array behind pointer field `field`; None leaves the field NULL.
        shapes: one shape or a list of allowed ones; copy: a fresh writable copy, the caller's array stays untouched"""
        if v is None:
            return None
        return self._store(field, np.array(v, dtype=dtype, order="C") if copy else np.ascontiguousarray(v, dtype=dtype), shapes)

    def output(self, field, v, shape):
        """a caller-filled in/out array: it must be writable C-contiguous float64 of `shape` already, nothing is copied"""
        if v is None:
            return None
        if not (isinstance(v, np.ndarray) and v.dtype == np.float64 and v.flags.c_contiguous and v.flags.writeable):
            raise ValueError(f"{field}: a writeable C-contiguous float64 array")
        return self._store(field, v, shape)

    def table(self, slot, full):
        """centre and right half of the full symmetric table `full` into `slot`, a FilterTable or the (NodeTables, k) of node k;
        None: radius -1, which skips the axis"""
        r, w = -1, None
        if full is not None:
            r = len(full) // 2
            w = _p(self.hold(np.ascontiguousarray(np.asarray(full, dtype=np.float64)[r:])))
        if isinstance(slot, tuple):
            tables, k = slot
            tables.radius[k] = r
            if w is not None:
                tables.w[k] = w
        else:
            slot.radius = r
            if w is not None:
                slot.w = w


def resolve_bound(args, num_members):
    """a description of coupled batches (mapping.resolve.resolve_args) as hipdrt_resolve_args, with the sizes it implies:
    -> (Bound, [nc_k], [doubles before batch k in x and h])"""
    b = Bound(ResolveArgs())
    c = b.c
    nb, nr, nrm = int(args["nb"]), int(args["nr"]), int(args["num_remove"])
    c.nb, c.nr, c.num_remove, c.so, c.lambda_psi = nb, nr, nrm, int(args["so"]), float(args["lambda_psi"])
    c.tau_filter_sigma, c.special_filter_sigma = float(args["tau_filter_sigma"]), float(args["special_filter_sigma"])
    b.array("first", args["first"], (nb,), dtype=np.int32)
    match = b.array("match", args["match"], (nb, 2), dtype=np.int32)
    b.array("tau_indices", args["tau_indices"], (num_members, 2), dtype=np.int32)
    b.array("my", args["my"], (nb, nr, nr))
    if nrm > 0:
        b.array("x_remove", args["x_remove"], (num_members, nrm))
    nc = [int(c.so + m[1] - m[0]) for m in match]
    if [len(v) for v in args["param_scale"]] != nc or [len(v) for v in args["h"]] != [nr * v for v in nc]:
        raise ValueError("param_scale: so + match width entries per batch; h: nr times as many")
    b.array("param_scale", np.concatenate([np.asarray(v, dtype=np.float64) for v in args["param_scale"]]))
    b.array("h", np.concatenate([np.asarray(v, dtype=np.float64) for v in args["h"]]))
    return b, nc, np.concatenate([[0], np.cumsum([nr * v for v in nc])]).astype(int)


def pfrt_select_bound(B, S, npf, max_peaks, want=None, rows=True, nout=0):
    """hipdrt_pfrt_select_out with its host arrays, poisoned so that anything the kernel leaves unwritten shows (-77 / 7e77: -1
    and NaN are the padding of unused slots): the compact form (num_peaks, first, num_candidates (B,); ranked_index, step_index,
    magnitude, match_quality (B, max_peaks)) and, with `rows`, raw_pfrt (B, np), step_pfrt (S, B, np), post_prob (S, B); pfrt
    (B, nout) only when `want` names it.  want: the names to form and download (None: all but pfrt) -> (Bound, dict of the arrays)"""
    mp = max(1, min(int(max_peaks), 4096))          # (a count the library refuses still gets arrays to point at)
    shapes = dict(num_peaks=(B,), ranked_index=(B, mp), first=(B,), num_candidates=(B,), step_index=(B, mp), magnitude=(B, mp),
                  match_quality=(B, mp), raw_pfrt=(B, npf), step_pfrt=(S, B, npf), post_prob=(S, B), pfrt=(B, nout))
    b = Bound(PfrtSelectOut())
    out = {}
    for k in PFRT_SELECT_COMPACT + (PFRT_SELECT_ROWS if rows else ()):
        if (want is None and k == "pfrt") or (want is not None and k not in want):
            continue
        integer = k in PFRT_SELECT_COMPACT[:5]
        out[k] = b.array(k, np.full(shapes[k], -77, dtype=np.int32) if integer else np.full(shapes[k], 7e77), shapes[k],
                         dtype=np.int32 if integer else np.float64)
    return b, out
