"""RCCL communicator behind the C ABI."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .abi import HipDrtError, _check, _f64, _p, _vp, load_library


def comm_unique_id() -> bytes:
    """128 opaque bytes of a fresh RCCL communicator id (rank 0 makes them, every rank passes them to Comm)"""
    buf = C.create_string_buffer(128)
    _check(load_library().hipdrt_comm_unique_id(buf))
    return buf.raw


class Comm:
    """RCCL communicator behind the C ABI (include/hipdrt.h: hipdrt_comm_*): one per process, numpy in / numpy out"""

    def __init__(self, device, rank, world, unique_id):
        self._lib = load_library()
        self._h = _vp()
        self.rank, self.world, self.device = int(rank), int(world), int(device)
        if len(unique_id) != 128:
            raise HipDrtError("a RCCL unique id has 128 bytes")
        _check(self._lib.hipdrt_comm_create(self.device, self.rank, self.world, C.c_char_p(bytes(unique_id)), C.byref(self._h)))

    def close(self):
        if self._h:
            self._lib.hipdrt_comm_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:       # noqa: BLE001 (interpreter shutdown)
            pass

    def broadcast(self, array, root=0):
        """`array` (contiguous float64) of `root` into every rank's `array`, in place"""
        if not (isinstance(array, np.ndarray) and array.dtype == np.float64 and array.flags.c_contiguous):
            raise HipDrtError("broadcast needs a C-contiguous float64 array (it is filled in place)")
        _check(self._lib.hipdrt_comm_broadcast(self._h, _p(array), array.size, int(root)))
        return array

    def gather(self, block, root=0):
        """every rank's `block` (same size everywhere) to `root`: returns (world, block.size) there, None elsewhere"""
        block = _f64(block).ravel()
        out = np.empty((self.world, block.size)) if self.rank == root else None
        _check(self._lib.hipdrt_comm_gather(self._h, _p(block), block.size, _p(out), int(root)))
        return out

    def allreduce_max(self, value):
        v = C.c_double(float(value))
        _check(self._lib.hipdrt_comm_allreduce_max(self._h, C.byref(v)))
        return v.value

    def barrier(self):
        _check(self._lib.hipdrt_comm_barrier(self._h))
