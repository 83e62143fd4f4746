"""ctypes binding of libhipdrt.so (C-ABI declared in include/hipdrt.h).  numpy in, numpy out.

There is deliberately no CPU fallback: if the shared library is missing, or no gfx950 device is visible,
every compute entry point raises ``HipDrtError``.  This file only re-exports: the imports below are the surface and say which
module holds what (debug: the DebugHooks that Context mixes in).  Callers write ``_ffi.NAME`` and so resolve a name here at call time.
"""
from . import abi
from .abi import *                                                   # noqa: F401,F403 (every public name of the headers' mirror)
from .abi import _HERE, _RESTYPES, _check, _dp, _f64, _i32, _ip, _lock, _p, _pi, _vp      # noqa: F401
from .args import Bound, pfrt_select_bound                                              # noqa: F401
from .opts import (default_fit_opts, kk_opts, PEAK_METHODS, peak_opts, pfrt_opts, pfrt_select_opts, pfrt_bytes_per_spectrum,    # noqa: F401
                   peak_resolve_opts, _resolve_outputs, _resolve_out_struct, _PEAK_INT, _PEAK_F64, _peak_outputs, _peak_out_args,
                   _kk_outputs, PEAK_PROB_SEARCH, peak_prob_opts, _peak_prob_outputs, _peak_prob_out_args, _index_windows)
from .context import Context, _default_ctx, device_usable, get_context      # noqa: F401
from .plan import Plan, PreparedPlan                                 # noqa: F401
from .comm import Comm, comm_unique_id                               # noqa: F401


def __getattr__(name):
    if name == "_lib":              # load_library rebinds it: read it where it lives
        return abi._lib
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
