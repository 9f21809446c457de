"""
Batched number-theoretic transform over a curve's scalar field on the GPU: ctypes callers of ctt_hip_fr_ntt_plan_create /
ctt_hip_fr_ntt (include/ctt_msm_hip.h part 5; kernels constantine_amd/csrc/ntt.hip).  Nothing is computed in
Python: a numpy array is copied to the device (torch does the plumbing), transformed there and copied back; a torch CUDA tensor or a
raw device address is transformed where it is.

    plan = NttPlan("bls12_381_g1", 12, omega)             # omega: int or 32 little-endian bytes, omega^(n/2) == -1
    cells = plan.ntt(coeffs, out_brp=True, shift=g)       # coeffs: (batch, n, 32) or (n, 32) uint8, canonical little-endian
    back = plan.ntt(cells, inverse=True, in_brp=True, shift=g)

Forward out[k] = sum_i (g^i in[i]) omega^(ik), inverse out[i] = g^-i / n * sum_k in[k] omega^(-ik); in_brp / out_brp: that side is
in bit-reversed order; in_mont / out_mont: that side holds Montgomery residues instead of canonical scalars.
"""
import ctypes

import numpy as np

from . import _lib
from ._arrays import ptr
from .curves import CURVES

INVERSE, IN_BRP, OUT_BRP, IN_MONT, OUT_MONT = 1, 2, 4, 8, 16


class NttRefused(RuntimeError):
    """ctt_hip_fr_ntt / _plan_create returned an error: `code` is ctt_hip_last_error() (-1 refused, -2 out of device memory, ...)."""

    def __init__(self, what):
        L = _lib.lib()
        self.code = int(L.ctt_hip_last_error())
        msg = L.ctt_hip_last_error_message()
        super().__init__(f"{what} ({self.code}): {msg.decode(errors='replace') if msg else ''}")


def _scalar(v):
    """int or 32 bytes -> a ctypes buffer of 32 little-endian bytes (range checks are the library's)"""
    b = int(v).to_bytes(32, "little") if isinstance(v, int) else bytes(v)
    if len(b) != 32:
        raise ValueError("a scalar is 32 bytes")
    return (ctypes.c_uint8 * 32).from_buffer_copy(b)


class NttPlan:
    """ctt_hip_ntt_plan: the twiddle table of (the curve's scalar field, log2n, omega) on one context.  `device`: a device index (the
    plan makes a context of its own) or a DeviceMsm, whose context -- and stream order with its MSMs -- the plan shares."""

    def __init__(self, curve, log2n, omega, device=0, tile_log2=0):
        self.L = _lib.lib()
        self.curve, self.log2n, self.n = curve, int(log2n), 1 << int(log2n)
        self._own_ctx = not hasattr(device, "ctx")
        self.ctx = self.L.ctt_hip_msm_ctx_create(int(device)) if self._own_ctx else device.ctx
        self.plan = None
        if not self.ctx:
            raise _lib.GpuUnavailable("NTT context")
        self.device = int(device) if self._own_ctx else int(device.device)
        self.plan = self.L.ctt_hip_fr_ntt_plan_create(self.ctx, CURVES[curve].cid, int(log2n), _scalar(omega), int(tile_log2))
        if not self.plan:
            err = NttRefused("ctt_hip_fr_ntt_plan_create")
            self.close()
            raise err

    def close(self):
        if self.plan:
            self.L.ctt_hip_fr_ntt_plan_destroy(self.ctx, self.plan)
            self.plan = None
        if self.ctx and self._own_ctx:
            self.L.ctt_hip_msm_ctx_destroy(self.ctx)
        self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:   # noqa: BLE001  (interpreter shutdown)
            pass

    def info(self):
        """{'log2n', 'tile_log2', 'passes', 'table_bytes'} of the plan"""
        v = (ctypes.c_size_t * 4)()
        if self.L.ctt_hip_fr_ntt_plan_info(self.plan, v) != 0:
            raise NttRefused("ctt_hip_fr_ntt_plan_info")
        return dict(zip(("log2n", "tile_log2", "passes", "table_bytes"), map(int, v)))

    def ntt_ptr(self, d_out, d_in, batch, flags=0, shift=None):
        """the C call on raw device addresses; -> its return value"""
        return self.L.ctt_hip_fr_ntt(self.ctx, self.plan, ptr(d_out), ptr(d_in), int(batch), int(flags),
                                     None if shift is None else _scalar(shift))

    def ntt(self, x, inverse=False, in_brp=False, out_brp=False, in_mont=False, out_mont=False, shift=None, out=None):
        """x: a numpy uint8 array of batch * n * 32 bytes (-> a new numpy array of the same shape) or a torch CUDA uint8 tensor (-> `out`,
        a tensor of the same size, or x itself when out is None: in place)."""
        flags = (INVERSE if inverse else 0) | (IN_BRP if in_brp else 0) | (OUT_BRP if out_brp else 0) | (IN_MONT if in_mont else 0) | \
                (OUT_MONT if out_mont else 0)
        import torch
        host = isinstance(x, np.ndarray)
        if host:
            if x.dtype != np.uint8:
                raise TypeError("uint8 bytes expected")
            t = torch.from_numpy(np.ascontiguousarray(x)).to(f"cuda:{self.device}")
            out = t
        else:
            t = x
            out = x if out is None else out
            if not (t.is_cuda and t.is_contiguous() and out.is_cuda and out.is_contiguous() and t.dtype == torch.uint8 and out.dtype == torch.uint8):
                raise TypeError("contiguous CUDA uint8 tensors expected")
            if out.numel() != t.numel():
                raise ValueError("out and x differ in size")
        if t.numel() % (32 * self.n):
            raise ValueError(f"{t.numel()} bytes are not whole rows of {self.n} elements of 32 bytes")
        torch.cuda.synchronize(t.device)     # (the engine's stream is not torch's: what produced x is done before the transform starts)
        rc = self.ntt_ptr(out.data_ptr(), t.data_ptr(), t.numel() // (32 * self.n), flags, shift)
        if rc != 0:
            raise NttRefused("ctt_hip_fr_ntt")
        return out.cpu().numpy().reshape(x.shape) if host else out
