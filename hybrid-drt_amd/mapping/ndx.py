"""mapping.ndx.filter_ndx (hybdrt/mapping/ndx.py:261-349) for an ungrouped 1-D or 2-D array, filtered on the device
(csrc/map_filter.hip through hipdrt.filters).  The NaN rules are the reference's (267-299): NaNs are zero-filled before the
filter so that they do not spread, every entry comes back filled, and NaNs are then restored per impute / impute_groups."""
import numpy as np

from .. import filters
from ..filters import ndfilters


def _check(ndx, num_group_dims, filter_func, by_group, impute_groups):
    if impute_groups and by_group:
        raise ValueError('Group imputation cannot be performed when filtering by group')
    if filter_func is not None:
        raise NotImplementedError("filter_func: only the built-in Gaussian filters (filter_func=None) run on the device")
    if by_group:
        raise NotImplementedError("by_group=True: grouped maps are not built")
    if num_group_dims != 0:
        raise NotImplementedError("num_group_dims > 0: grouped maps are not built")
    if np.ndim(ndx) not in (1, 2):
        raise NotImplementedError("more than two dimensions: filter_ndx takes 1-D and 2-D arrays")


def _restore_nans(out, nan_obs_index, nan_group_index, impute, impute_groups):
    if impute:
        if not impute_groups:
            out[nan_group_index] = np.nan          # (num_group_dims = 0: the one group is the whole array)
    else:
        out[nan_obs_index] = np.nan
    return out


def filter_ndx(ndx, num_group_dims, impute=False, impute_groups=False, iterative=True, adaptive=False, mask_nans=True,
               filter_func=None, by_group=False, device=0, **filter_kw):
    _check(ndx, num_group_dims, filter_func, by_group, impute_groups)
    ndx = np.asarray(ndx, dtype=float)
    nan_obs_index = np.isnan(ndx)
    nan_group_index = bool(np.all(nan_obs_index))
    out = filters.filter_array(ndx, iterative=iterative, adaptive=adaptive, mask_nans=mask_nans, device=device, **filter_kw)
    return _restore_nans(out, nan_obs_index, nan_group_index, impute, impute_groups)


def filter_ndx_statement(ndx, num_group_dims, impute=False, impute_groups=False, iterative=True, adaptive=False, mask_nans=True,
                         filter_func=None, by_group=False, **filter_kw):
    """the same call stated in numpy (filters/ndfilters.py): what the device path is read against"""
    _check(ndx, num_group_dims, filter_func, by_group, impute_groups)
    ndx = np.asarray(ndx, dtype=float)
    nan_obs_index = np.isnan(ndx)
    nan_group_index = bool(np.all(nan_obs_index))
    x = np.nan_to_num(ndx) if mask_nans else ndx
    weights = (~nan_obs_index).astype(float) if mask_nans else None
    if iterative:
        out = ndfilters.iterative_gaussian_filter(x, adaptive=adaptive, nan_mask=nan_obs_index if mask_nans else None, fill_nans=True,
                                                  **filter_kw)
    elif adaptive:
        sigmas = ndfilters.get_adaptive_sigmas(x, weights=weights, **filter_kw)

        def func(a_in, **kw):
            return ndfilters.adaptive_gaussian_filter(a_in, sigmas=sigmas, **kw)
        out = ndfilters.masked_filter(x, weights, filter_func=func, **filter_kw) if mask_nans else func(x, **filter_kw)
    elif mask_nans:
        out = ndfilters.masked_filter(x, weights, **filter_kw)
    else:
        out = ndfilters.gaussian_filter(x, **filter_kw)
    return _restore_nans(out, nan_obs_index, nan_group_index, impute, impute_groups)
