"""hipdrt._ffi.args.Bound and the return-code mapping of _check: host only, no device.

Bound is the one place where a numpy array gets behind a ctypes pointer field: converted, checked against the shapes the entry
point takes, and kept alive for as long as the argument structure is in use."""
import gc

import numpy as np
import pytest

from hipdrt import _ffi


def _read(ptr, n):
    return [ptr[i] for i in range(n)]


def test_array_converts_to_the_asked_type_and_stores_the_pointer():
    b = _ffi.Bound(_ffi.MapPredictArgs())
    v = b.array("f_var", [[1, 2, 3], [4, 5, 6]], (2, 3))
    assert v.dtype == np.float64 and v.flags.c_contiguous and v.shape == (2, 3)
    assert _read(b.c.f_var, 6) == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]
    e = b.array("ext", [[0, 2], [1, 2]], (2, 2), np.int32)
    assert e.dtype == np.int32 and _read(b.c.ext, 4) == [0, 2, 1, 2]
    b.array("fxx_var", np.arange(6.0).reshape(3, 2).T, (2, 3))       # not contiguous: the field gets the rows laid out in C order
    assert _read(b.c.fxx_var, 6) == [0.0, 2.0, 4.0, 1.0, 3.0, 5.0]


def test_array_none_leaves_the_field_null():
    b = _ffi.Bound(_ffi.MapPredictArgs())
    assert b.array("f_var", None, (2, 3)) is None and b.array("ext", None, dtype=np.int32) is None
    assert not b.c.f_var and not b.c.ext and b.keep == []


def test_array_shape_error_names_the_field_and_both_shapes():
    b = _ffi.Bound(_ffi.MapPredictArgs())
    with pytest.raises(ValueError, match=r"^f_var: expected shape \(2, 3\), got \(3, 2\)$"):
        b.array("f_var", np.zeros((3, 2)), (2, 3))
    with pytest.raises(ValueError, match=r"^f_var: expected shape \(3,\) or \(2, 3\), got \(2,\)$"):
        b.array("f_var", np.zeros(2), [(3,), (2, 3)])
    assert not b.c.f_var and b.keep == []                # a refused array is neither stored nor held


def test_array_accepts_each_of_a_list_of_shapes():
    b = _ffi.Bound(_ffi.MapPredictArgs())
    assert b.array("f_var", np.ones(3), [(3,), (2, 3)]).shape == (3,)
    assert b.array("f_var", np.ones((2, 3)), [(3,), (2, 3)]).shape == (2, 3)


def test_array_copy_does_not_alias_the_input():
    b = _ffi.Bound(_ffi.MapPredictArgs())
    src = np.arange(6.0).reshape(2, 3)
    assert np.shares_memory(b.array("f_var", src), src)              # without copy a fitting array goes in as it is
    v = b.array("fxx_var", src, (2, 3), copy=True)
    assert not np.shares_memory(v, src) and v.flags.writeable
    b.c.fxx_var[4] = -1.0
    assert v[1, 1] == -1.0 and src[1, 1] == 4.0


def test_bound_keeps_temporaries_alive():
    b = _ffi.Bound(_ffi.MapPredictArgs())
    b.array("f_var", np.arange(6).reshape(2, 3) + 0.5, (2, 3))
    b.array("ext", np.array([[3, 1], [4, 1]], dtype=np.int64) * 2, (2, 2), np.int32)
    b.table(b.c.spread, [float(i) for i in range(5)])
    held = np.arange(3.0) + 10
    ptr = _ffi._p(b.hold(held + 1))
    del held
    gc.collect()
    junk = [np.full(6, -1.0) for _ in range(64)]         # what a freed block of that size would be handed out for next
    assert _read(b.c.f_var, 6) == [0.5, 1.5, 2.5, 3.5, 4.5, 5.5]
    assert _read(b.c.ext, 4) == [6, 2, 8, 2]
    assert _read(b.c.spread.w, 3) == [2.0, 3.0, 4.0]
    assert _read(ptr, 3) == [11.0, 12.0, 13.0]
    assert len(b.keep) == 4 and len(junk) == 64


def test_table_takes_centre_and_right_half():
    # the figures are what filters.mapfilter._Args.table gave before Bound: r = len // 2, w = full[r:]
    b = _ffi.Bound(_ffi.MapPredictArgs())
    b.table(b.c.spread, [0.1, 0.2, 0.4, 0.2, 0.1])
    assert b.c.spread.radius == 2 and _read(b.c.spread.w, 3) == [0.4, 0.2, 0.1]
    b.table(b.c.x_filter[1], np.array([1, 2, 3, 4]))     # an even length: the same arithmetic, radius 2 and two values
    assert b.c.x_filter[1].radius == 2 and _read(b.c.x_filter[1].w, 2) == [3.0, 4.0]
    assert b.c.x_filter[0].radius == 0 and not b.c.x_filter[0].w     # untouched


def test_table_none_skips_the_axis():
    b = _ffi.Bound(_ffi.MapPredictArgs())
    b.table(b.c.spread, None)
    assert b.c.spread.radius == -1 and not b.c.spread.w and b.keep == []


def test_table_fills_a_node_of_node_tables():
    b = _ffi.Bound(_ffi.NodeTables())
    b.table((b.c, 3), [0.1, 0.2, 0.4, 0.2, 0.1])
    b.table((b.c, 4), None)
    assert b.c.radius[3] == 2 and _read(b.c.w[3], 3) == [0.4, 0.2, 0.1]
    assert b.c.radius[4] == -1 and not b.c.w[4] and b.c.radius[0] == 0


def test_output_takes_only_a_writable_contiguous_float64_array_of_the_shape():
    b = _ffi.Bound(_ffi.DebugGramArgs())
    q = np.full((2, 3), 7.0)
    assert b.output("q", q, (2, 3)) is q and b.c.q[5] == 7.0         # nothing is copied
    assert b.output("P", None, (2, 3)) is None and not b.c.P
    read_only = np.zeros((2, 3))
    read_only.flags.writeable = False
    for bad in (np.zeros((3, 2)).T, read_only, np.zeros((2, 3), dtype=np.float32), [[0.0] * 3] * 2):
        with pytest.raises(ValueError, match="P: a writeable C-contiguous float64 array"):
            b.output("P", bad, (2, 3))
    with pytest.raises(ValueError, match=r"^P: expected shape \(2, 3\), got \(3, 2\)$"):
        b.output("P", np.zeros((3, 2)), (2, 3))
    assert not b.c.P


def test_check_maps_a_return_code_only_where_asked():
    _ffi._check(0)
    _ffi._check(0, {_ffi.E_UNSUPPORTED: NotImplementedError})
    with pytest.raises(NotImplementedError) as e:
        _ffi._check(_ffi.E_UNSUPPORTED, {_ffi.E_UNSUPPORTED: NotImplementedError})
    assert not isinstance(e.value, _ffi.HipDrtError)
    with pytest.raises(ValueError):
        _ffi._check(_ffi.E_NUMERIC, {_ffi.E_NUMERIC: ValueError})
    for raises in (None, {_ffi.E_NUMERIC: ValueError}):              # unmapped: the generic error, with the code in it
        with pytest.raises(_ffi.HipDrtError, match="hipdrt error -5"):
            _ffi._check(_ffi.E_UNSUPPORTED, raises)
