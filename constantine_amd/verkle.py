"""
Batched Verkle commitments over a fixed Banderwagon basis (include/ctt_msm_hip.h part 4).

  VerkleCrs(points).commit(coefs)        m commitments of n scalars each against the n <= 256 cached points, and of every commitment
                                         the projective point, its 32-byte serialisation and its map to the scalar field
  VerkleCrs(points).update(deltas, idx, row_ptr, base)
                                         m sparse updates in one pass: old commitment + sum of delta * P_idx over the few changed slots
                                         of every row (CSR: row_ptr, idx), and of every result the same outputs plus "dfr", the delta
                                         map(new) - map(old) that the parent node takes
  batchMapToScalarField(points_prj)      constantine/ethereum_verkle_ipa.nim:247-281
  serializeBatch_vartime(points_prj)     constantine/serialization/codecs_banderwagon.nim:239-266

Arrays are numpy uint8 buffers, or torch CUDA uint8 tensors, in the C-API layout: points (n, 64) affine Montgomery, coefs (m, n, 32)
BigInt canonical little-endian below 2^253 (Fr Montgomery with fr_coefs=True), projective points (m, 96).  Results: "prj" (m, 96)
with Z = 1, "ser" (m, 32) big-endian, "fr" (m, 32) Montgomery.  Like the reference nothing is validated: the points must be
Banderwagon elements.  Shape errors raise ValueError before the library is touched; a call the GPU cannot serve raises
GpuUnavailable, any other refusal MsmRefused.
"""
import numpy as np

from . import _lib
from ._arrays import is_cuda, order, ptr
from .msm import MsmRefused

_WANT = ("prj", "ser", "fr")
_WANT_UPDATE = _WANT + ("dfr",)
_BYTES = {"prj": 96, "ser": 32, "fr": 32, "dfr": 32}
MAX_BASES = 256


def _shaped(a, tail, what):
    """`a` as a contiguous uint8 array / tensor whose trailing dimensions are `tail`"""
    if is_cuda(a):
        import torch
        if a.dtype != torch.uint8:
            raise ValueError(f"{what} must be a uint8 tensor")
        a = a.contiguous()
    else:
        a = np.ascontiguousarray(a, dtype=np.uint8)
    if a.ndim != len(tail) + 1 or tuple(a.shape[1:]) != tuple(tail):
        raise ValueError(f"{what} must have shape (m, {', '.join(str(t) for t in tail)})")
    return a


def _empty_like(src, m, width):
    if is_cuda(src):
        import torch
        return torch.empty((m, width), dtype=torch.uint8, device=src.device)
    return np.zeros((m, width), dtype=np.uint8)


def _refused(L, rc, what):
    if L.ctt_hip_last_error() in (-2, -3, -4, -5):
        raise _lib.GpuUnavailable(what)
    raise MsmRefused(rc)


class VerkleCrs:
    """A table of precomputed multiples of n <= 256 Banderwagon points, resident on the GPU (ctt_hip_verkle_crs_*).
    window_bits: 0 = the library's default, else 2 .. 10.  `ctx` is a ctt_hip_msm_ctx* (DeviceMsm.ctx) or None for the default context."""

    def __init__(self, points, ctx=None, window_bits=0, on_device=False):
        if on_device != is_cuda(points):
            raise ValueError("on_device=True takes a CUDA tensor, on_device=False a host array")
        points = _shaped(points, (64,), "points")
        n = int(points.shape[0])
        if not 1 <= n <= MAX_BASES:
            raise ValueError(f"a CRS has 1 .. {MAX_BASES} points, not {n}")
        if int(window_bits) != 0 and not 2 <= int(window_bits) <= 10:
            raise ValueError("window_bits is 0 (default) or 2 .. 10")
        self.L = _lib.lib()
        self.ctx = ctx
        self.n = n
        self.handle = None
        if on_device:
            import torch
            torch.cuda.current_stream(points.device).synchronize()   # the table is made from the tensor as it is now
        self.handle = self.L.ctt_hip_verkle_crs_create(ctx, ptr(points), n, int(window_bits), 1 if on_device else 0)
        if not self.handle:
            _refused(self.L, -1, "ctt_hip_verkle_crs_create")
        self.window_bits = self.L.ctt_hip_verkle_crs_window_bits(self.handle)

    def commit(self, coefs, fr_coefs=False, want=_WANT):
        """{"prj": (m, 96), "ser": (m, 32), "fr": (m, 32)} (the keys of `want`) for the m rows of coefs (m, n, 32); arrays for a host
        array, tensors on the same device for a CUDA tensor."""
        want = tuple(want)
        if not want or any(w not in _WANT for w in want):
            raise ValueError(f"want is a non-empty subset of {_WANT}")
        coefs = _shaped(coefs, (self.n, 32), "coefs")
        if not self.handle:
            raise ValueError("this VerkleCrs is closed")
        m = int(coefs.shape[0])
        out = {w: _empty_like(coefs, m, _BYTES[w]) for w in _WANT if w in want}
        if m == 0:
            return out
        order(self.L, self.ctx, coefs)
        rc = self.L.ctt_hip_verkle_commit_batch(self.ctx, self.handle, 1 if fr_coefs else 0, ptr(out.get("prj")), ptr(out.get("ser")),
                                                ptr(out.get("fr")), ptr(coefs), m, 1 if is_cuda(coefs) else 0)
        if rc != 0:
            _refused(self.L, rc, "ctt_hip_verkle_commit_batch")
        return out

    def update(self, deltas, idx, row_ptr, base=None, fr_coefs=False, want=_WANT):
        """Row k = base[k] + sum of deltas[e] * P_idx[e] over e in [row_ptr[k], row_ptr[k + 1]): {"prj", "ser", "fr", "dfr"} (the keys of
        `want`), "dfr" (m, 32) being map(row k) - map(base[k]) mod r in Montgomery form.  deltas (E, 32) host array or CUDA tensor,
        base (m, 96) projective of the same kind or None (the neutral); idx (E,) and row_ptr (m + 1,) are host integers.  Entries of a
        row may repeat a base; a row may be empty.  No dispatch to commit() happens here, however long the rows are."""
        want = tuple(want)
        if not want or any(w not in _WANT_UPDATE for w in want):
            raise ValueError(f"want is a non-empty subset of {_WANT_UPDATE}")
        deltas = _shaped(deltas, (32,), "deltas")
        E = int(deltas.shape[0])
        idx, row_ptr = np.asarray(idx), np.asarray(row_ptr)
        if idx.ndim != 1 or idx.shape[0] != E or (E and idx.dtype.kind not in "iu"):
            raise ValueError("idx is one integer per row of deltas")
        if row_ptr.ndim != 1 or row_ptr.shape[0] < 1 or (row_ptr.dtype.kind not in "iu"):
            raise ValueError("row_ptr is (m + 1,) integers")
        m = int(row_ptr.shape[0]) - 1
        if int(row_ptr[0]) != 0 or int(row_ptr[-1]) != E or (m and bool(np.any(np.diff(row_ptr.astype(np.int64)) < 0))):
            raise ValueError("row_ptr rises monotonically from 0 to the number of entries")
        if E and (int(idx.min()) < 0 or int(idx.max()) >= self.n):
            raise ValueError(f"idx holds indices in [0, {self.n})")
        if base is not None:
            if is_cuda(base) != is_cuda(deltas):
                raise ValueError("base and deltas are both host arrays or both CUDA tensors")
            base = _shaped(base, (96,), "base")
            if int(base.shape[0]) != m:
                raise ValueError(f"base has {int(base.shape[0])} rows, row_ptr {m}")
            if is_cuda(base) and base.device != deltas.device:
                raise ValueError("base and deltas are on different devices")
        if not self.handle:
            raise ValueError("this VerkleCrs is closed")
        idx = np.ascontiguousarray(idx, dtype=np.uint8)
        row_ptr = np.ascontiguousarray(row_ptr, dtype=np.uint32)
        out = {w: _empty_like(deltas, m, _BYTES[w]) for w in _WANT_UPDATE if w in want}
        if m == 0:
            return out
        order(self.L, self.ctx, deltas, base)   # both on one device: one current stream
        rc = self.L.ctt_hip_verkle_update_batch(self.ctx, self.handle, 1 if fr_coefs else 0, ptr(out.get("prj")), ptr(out.get("ser")),
                                                ptr(out.get("fr")), ptr(out.get("dfr")), ptr(base), ptr(row_ptr), ptr(idx),
                                                ptr(deltas), m, 1 if is_cuda(deltas) else 0)
        if rc != 0:
            _refused(self.L, rc, "ctt_hip_verkle_update_batch")
        return out

    def last_timings(self):
        """ms of the context's last commit (or update) batch (after DeviceMsm.enable_timings) and of its last table build"""
        ms = np.zeros(3, dtype=np.float32)
        self.L.ctt_hip_verkle_last_timings(self.ctx, ptr(ms), 3)
        return dict(zip(("commit", "finish", "table"), (float(x) for x in ms)))

    def close(self):
        if self.handle:
            self.L.ctt_hip_verkle_crs_destroy(self.ctx, self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _finish(symbol, points_prj, ctx):
    points_prj = _shaped(points_prj, (96,), "points_prj")
    m = int(points_prj.shape[0])
    out = _empty_like(points_prj, m, 32)
    if m == 0:
        return out
    L = _lib.lib()
    order(L, ctx, points_prj)
    rc = getattr(L, symbol)(ctx, ptr(out), ptr(points_prj), m, 1 if is_cuda(points_prj) else 0)
    if rc != 0:
        _refused(L, rc, symbol)
    return out


def batchMapToScalarField(points_prj, ctx=None):
    """((x / y) mod p) mod r of every projective point (m, 96), as (m, 32) Montgomery residues of the scalar field"""
    return _finish("ctt_hip_banderwagon_map_to_fr_batch", points_prj, ctx)


def serializeBatch_vartime(points_prj, ctx=None):
    """the 32-byte big-endian serialisation of every projective point (m, 96): x if y >= (p-1)/2 else p - x"""
    return _finish("ctt_hip_banderwagon_serialize_batch", points_prj, ctx)
