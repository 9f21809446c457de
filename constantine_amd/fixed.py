"""Batched fixed-base MSM over BLS12-381 G1 and BN254 G1 (include/ctt_msm_hip_fixed.h, libctt_msm_hip_fixed.so): a table of window
multiples of up to 65536 fixed points, and m MSMs over it in one kernel pass -- no sort, no buckets, no tickets.  It pays where the
engine's MSM is launch-bound: many MSMs of a few thousand pairs over the same points."""
import ctypes

import numpy as np

from . import _lib
from ._arrays import is_cuda, ptr
from .curves import COEF_BIG, COEF_FR, CURVES

COEFS_ON_DEVICE, OUT_ON_DEVICE = 1, 2


class FixedMsmRefused(RuntimeError):
    """a call the library refused; `code` is its return value: -1 an argument (checked before anything is launched), -2 a failed
    allocation, -3 a HIP error or no usable device.  Outputs are untouched."""

    def __init__(self, what, code):
        super().__init__(f"{what}: refused ({code})")
        self.code = code


class FixedBaseMsm:
    def __init__(self, curve, points, c=None, device=0):
        """curve: "bls12_381_g1" or "bn254_snarks_g1"; points: (n, 96 | 64) uint8 affine Montgomery coordinates, (0, 0) the neutral, a numpy
        array or a torch device tensor, 1 <= n <= 65536; c: window bits 2 .. 12 (None: the library's default)"""
        self.L = _lib.fixed_lib()
        self.info_curve = CURVES[curve]
        self.handle = None
        if tuple(points.shape[1:]) != (self.info_curve.aff_bytes,):
            raise ValueError(f"points: (n, {self.info_curve.aff_bytes}) uint8 expected")
        if is_cuda(points):
            import torch
            points = points.contiguous()
            torch.cuda.current_stream(points.device).synchronize()   # the handle works on a stream of its own
        else:
            points = np.ascontiguousarray(points, dtype=np.uint8)
        self.n = int(points.shape[0])
        h = self.L.ctt_hip_fixed_bases_create(int(device), self.info_curve.cid, ptr(points), self.n, 0 if c is None else int(c))
        if not h:
            raise FixedMsmRefused("ctt_hip_fixed_bases_create", int(self.L.ctt_hip_fixed_last_error()))
        self.handle = ctypes.c_void_p(h)

    def info(self):
        """-> dict: n, c, windows, records_per_base, table_bytes, build_us"""
        v = (ctypes.c_size_t * 6)()
        if self.L.ctt_hip_fixed_bases_info(self.handle, v) != 0:
            raise FixedMsmRefused("ctt_hip_fixed_bases_info", -1)
        return dict(zip(("n", "c", "windows", "records_per_base", "table_bytes", "build_us"), (int(x) for x in v)))

    def last_timings(self):
        """device ms of the last batch: (the sum kernel, the finish)"""
        ms = (ctypes.c_float * 2)()
        if self.L.ctt_hip_fixed_last_timings(self.handle, ms) != 0:
            raise FixedMsmRefused("ctt_hip_fixed_last_timings", -1)
        return float(ms[0]), float(ms[1])

    def msm_batch(self, coefs, fr=False, out=None):
        """coefs: (m, n, 32) uint8, a numpy array or a torch device tensor -- canonical little-endian scalars below 2^bits, not reduced
        mod r, or with fr=True Montgomery residues of the scalar field.  -> (m, 96 | 64) affine Montgomery bytes, the neutral (0, 0): a
        numpy array, or a device tensor when given one (`out`: where to write them, of the same kind).  The call returns when the
        result is written; a refusal raises FixedMsmRefused and leaves `out` untouched."""
        if len(coefs.shape) != 3 or tuple(coefs.shape[1:]) != (self.n, 32):
            raise ValueError(f"coefs: (m, {self.n}, 32) uint8 expected")
        m, ab = int(coefs.shape[0]), self.info_curve.aff_bytes
        on_device = is_cuda(coefs)
        if on_device:
            import torch
            coefs = coefs.contiguous()
            if out is None:
                out = torch.empty((m, ab), dtype=torch.uint8, device=coefs.device)
            assert is_cuda(out) and out.is_contiguous() and out.numel() == m * ab
            torch.cuda.current_stream(coefs.device).synchronize()    # the handle works on a stream of its own
            flags = COEFS_ON_DEVICE | OUT_ON_DEVICE
        else:
            coefs = np.ascontiguousarray(coefs, dtype=np.uint8)
            if out is None:
                out = np.zeros((m, ab), dtype=np.uint8)
            assert isinstance(out, np.ndarray) and out.flags.c_contiguous and out.size == m * ab
            flags = 0
        rc = self.L.ctt_hip_fixed_msm_batch(self.handle, COEF_FR if fr else COEF_BIG, ptr(coefs), m, ptr(out), flags)
        if rc != 0:
            raise FixedMsmRefused("ctt_hip_fixed_msm_batch", rc)
        return out

    def close(self):
        if self.handle:
            self.L.ctt_hip_fixed_bases_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
