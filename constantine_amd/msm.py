"""
Host-side mirror of the reference's MSM entry points, over the C ABI of libctt_msm_hip.so.

Names and argument meaning follow the reference:
  multiScalarMul_vartime(r, coefs, points)                 constantine/math/elliptic/ec_multi_scalar_mul.nim:525-568
  multiScalarMul_vartime_parallel(tp, r, coefs, points)    constantine/math/elliptic/ec_multi_scalar_mul_parallel.nim:588-639
  CttEngine.msm(coeffs, bases)                             constantine-rust/constantine-halo2-zal/src/lib.rs:22-58
    (Halo2-ZAL MsmAccel: BN254 G1, Fr coefficients, projective result; descriptors at lib.rs:60-95)

Arrays are numpy uint8 buffers in the C-API memory layout (include/ctt_msm_hip.h): coefs (n,32) --
BigInt canonical little-endian, or Fr Montgomery when fr_coefs=True -- and points (n, 2*coord) affine
Montgomery.  Like the reference, nothing is validated (no on-curve / subgroup checks) and the functions are
variable-time: public inputs only.  coefs and points must have the same length (the reference asserts it in
debug builds, ec_multi_scalar_mul.nim:536).
"""
import ctypes

import numpy as np

from . import _lib
from ._arrays import is_cuda, order, ptr, result_buffer
from .curves import COEF_BIG, COEF_FR, CURVES, OUT_AFF, OUT_JAC, OUT_PRJ

_COORD = {"jac": OUT_JAC, "prj": OUT_PRJ, "aff": OUT_AFF}


def _check(curve, coefs, points):
    info = CURVES[curve]
    coefs = np.ascontiguousarray(coefs, dtype=np.uint8)
    points = np.ascontiguousarray(points, dtype=np.uint8)
    if coefs.ndim != 2 or coefs.shape[1] != 32:
        raise ValueError("coefs must have shape (n, 32)")
    if points.ndim != 2 or points.shape[1] != info.aff_bytes:
        raise ValueError(f"points must have shape (n, {info.aff_bytes})")
    if coefs.shape[0] != points.shape[0]:
        raise ValueError("coefs and points must have the same length")
    return info, coefs, points


def _out_kind(info, coord):
    """CTT_HIP_OUT_* of `coord`; Banderwagon (twisted Edwards) has no Jacobian coordinates"""
    if coord not in _COORD or (coord == "jac" and info.cid == CURVES["banderwagon"].cid):
        raise ValueError(f"no {coord!r} coordinates for {info.name}")
    return _COORD[coord]


def multiScalarMul_vartime(curve, coefs, points, coord="jac", fr_coefs=False):
    """r <- sum coefs[i]*points[i], via ctt_<curve>_<coord>_multi_scalar_mul_{big,fr}_coefs_vartime.
    Returns r as a uint8 array of 3 coordinates (X,Y,Z) in `coord` ("jac" or "prj")."""
    info, coefs, points = _check(curve, coefs, points)
    if curve == "banderwagon":   # the companion library: projective only, the affine form is its Z = 1 representative
        _out_kind(info, coord)
        fn = getattr(_lib.banderwagon_lib(), f"ctt_banderwagon_ec_prj_multi_scalar_mul_{'fr' if fr_coefs else 'big'}_coefs_vartime")
        r = np.zeros(info.jac_bytes, dtype=np.uint8)
        fn(ptr(r), ptr(coefs), ptr(points), coefs.shape[0])
        return r[:info.aff_bytes].copy() if coord == "aff" else r
    L = _lib.lib()
    fn = getattr(L, f"ctt_{info.sym}_{coord}_multi_scalar_mul_{'fr' if fr_coefs else 'big'}_coefs_vartime")
    r = np.zeros(info.jac_bytes, dtype=np.uint8)
    fn(ptr(r), ptr(coefs), ptr(points), coefs.shape[0])
    return r


def multiScalarMul_vartime_parallel(tp, curve, coefs, points, coord="jac", fr_coefs=False):
    """Same through the *_vartime_parallel symbol; `tp` (a ctt_threadpool* or None) is accepted and ignored,
    the GPU replaces the pool.  Groups without an upstream parallel symbol (G2) raise AttributeError."""
    info, coefs, points = _check(curve, coefs, points)
    if not info.has_parallel:
        raise AttributeError(f"the reference exports no *_vartime_parallel MSM for {curve}")
    L = _lib.lib()
    fn = getattr(L, f"ctt_{info.sym}_{coord}_multi_scalar_mul_{'fr' if fr_coefs else 'big'}_coefs_vartime_parallel")
    r = np.zeros(info.jac_bytes, dtype=np.uint8)
    fn(ptr(tp), ptr(r), ptr(coefs), ptr(points), coefs.shape[0])
    return r


class MsmRefused(RuntimeError):
    """A neutral host-pointer symbol returned an error code: -1 refused (bad id / length / all slots busy), -2 out of device
    memory.  The caller that has a CPU implementation next to it (the Nim binding of INTEGRATION.md part B) falls back to it."""

    def __init__(self, code):
        super().__init__(f"ctt_hip_msm_host refused the call: {code}")
        self.code = code


def msm_available():
    """ctt_hip_msm_available(): 1 when a HIP device is present, never aborts."""
    return bool(_lib.lib().ctt_hip_msm_available())


def msm_host(curve, coefs, points, coord="jac", fr_coefs=False, typed=True):
    """The neutral host-pointer symbols (include/ctt_msm_hip.h part 1c): ctt_hip_msm_<curve>_<coord>_<big|fr> (typed=True,
    "jac" / "prj") or the generic ctt_hip_msm_host (also "aff").  Same arguments and result as multiScalarMul_vartime; raises
    MsmRefused with the symbol's status instead of aborting."""
    info, coefs, points = _check(curve, coefs, points)
    L = _lib.lib()
    r = result_buffer(info, coord)
    if typed and coord != "aff":
        rc = getattr(L, f"ctt_hip_msm_{info.sym}_{coord}_{'fr' if fr_coefs else 'big'}")(ptr(r), ptr(coefs), ptr(points), coefs.shape[0])
    else:
        rc = L.ctt_hip_msm_host(info.cid, COEF_FR if fr_coefs else COEF_BIG, _COORD[coord], ptr(r), ptr(coefs), ptr(points),
                                coefs.shape[0])
    if rc != 0:
        raise MsmRefused(rc)
    return r


class DeviceMsm:
    """Device-resident MSM: inputs already in HBM (torch CUDA tensors or raw device pointers)."""

    def __init__(self, device=0):
        self.L = _lib.lib()
        self.device = device
        self.ctx = self.L.ctt_hip_msm_ctx_create(device)
        if not self.ctx:
            raise RuntimeError("ctt_hip_msm_ctx_create failed")

    def close(self):
        if self.ctx:
            self.L.ctt_hip_msm_ctx_destroy(self.ctx)
            self.ctx = None

    def set_option(self, key, value):
        """ctt_hip_msm_set_option: "c", "K", "S", "chunks", "horner_bits", "host_window_sums", "sort_staged", "sort_xcd", "timings", "timings_every",
        and the forms of the head merge and the stream placements of a pipelined MSM: "merge_chain", "merge_lmax", "merge_queue_quad",
        "early_tail" (default 1), "front_side", "pyr0_tail", and "glv" -- the endomorphism split of BLS12-381 G1: 0 at the curve's measured
        sizes, 1 always, 2 never --, "accum_handover" -- the priority hand-over of the accumulate kernel: 0 off, 1 the curve's drop distance
        (default), n >= 2 that distance -- (include/ctt_msm_hip.h); 0 = automatic / off.  KeyError for an unknown key."""
        if self.L.ctt_hip_msm_set_option(self.ctx, key.encode(), int(value)) != 0:
            raise KeyError(key)

    def wait_stream(self, stream):
        """Everything the engine enqueues from now on waits for the work `stream` (a hipStream_t address) holds now."""
        if self.L.ctt_hip_msm_wait_stream(self.ctx, ptr(stream)) != 0:
            raise RuntimeError("ctt_hip_msm_wait_stream failed")

    def msm(self, curve, d_coefs, d_points, n, coord="aff", fr_coefs=False):
        info = CURVES[curve]
        r = result_buffer(info, coord)
        order(self.L, self.ctx, d_coefs, d_points)
        rc = self.L.ctt_hip_msm_device(self.ctx, info.cid, COEF_FR if fr_coefs else COEF_BIG, _out_kind(info, coord), ptr(r),
                                       ptr(d_coefs), ptr(d_points), n)
        if rc != 0:
            raise RuntimeError("ctt_hip_msm_device failed")
        return r

    def submit(self, curve, d_coefs, d_points, n, fr_coefs=False):
        """Enqueue one MSM and return a ticket at once (at most three outstanding per curve: a fourth raises)."""
        info = CURVES[curve]
        order(self.L, self.ctx, d_coefs, d_points)
        t = self.L.ctt_hip_msm_device_submit(self.ctx, info.cid, COEF_FR if fr_coefs else COEF_BIG,
                                             ptr(d_coefs), ptr(d_points), n)
        if t < 0:
            raise RuntimeError("ctt_hip_msm_device_submit failed (bad arguments, or three tickets already outstanding)")
        return (curve, t)

    def finish(self, ticket, coord="aff"):
        """Wait for a submitted MSM, run the host tail, return the result."""
        curve, t = ticket
        info = CURVES[curve]
        r = result_buffer(info, coord)
        if self.L.ctt_hip_msm_device_finish(self.ctx, t, _out_kind(info, coord), ptr(r)) != 0:
            raise RuntimeError("ctt_hip_msm_device_finish failed (ticket not outstanding)")
        return r

    def sync(self):
        """Wait until everything enqueued on the engine's stream(s) has completed."""
        self.L.ctt_hip_msm_sync(self.ctx)

    def gen_points(self, curve, seed, n, d_out, first=0):
        order(self.L, self.ctx, d_out)
        rc = self.L.ctt_hip_gen_points(self.ctx, CURVES[curve].cid, seed & (2**64 - 1), first, n, ptr(d_out))
        if rc != 0:
            raise RuntimeError("ctt_hip_gen_points failed")

    def field_op(self, curve, op, d_a, d_b, d_r, n):
        order(self.L, self.ctx, d_a, d_b, d_r)
        rc = self.L.ctt_hip_field_op(self.ctx, CURVES[curve].cid, op, ptr(d_a), ptr(d_b), ptr(d_r), n)
        if rc != 0:
            raise RuntimeError("ctt_hip_field_op failed")

    SORT_PROBE_IN = ("bits", "c", "log2_ng", "slice", "cap", "big", "staged", "xcd_map", "merged", "id_stride", "zero_bytes")
    SORT_PROBE_USED = ("cb", "r", "W", "Wd", "B", "NG", "gshift", "gshift_narrow", "nblk", "jbits", "nent")

    def sort_probe(self, d_scalars, n, d_entries, d_bstart, d_maxcount, d_buckets=None, log2_ng=-1, kwords=8, **sizing):
        """ctt_hip_sort_probe_words: the digit sort alone on n device scalars of `kwords` words each (8, or 4: the half scalars of the
        endomorphism split), sized by `sizing` (the names of SORT_PROBE_IN; what is left out is 0 = the engine's default).  The outputs are
        uint32 / uint8 device tensors whose sizes go along as the capacities the call checks.
        Returns the derived shape (SORT_PROBE_USED) as a dict, or None when the call was refused (nothing launched, nothing written)."""
        unknown = set(sizing) - set(self.SORT_PROBE_IN)
        if unknown:
            raise KeyError(sorted(unknown))
        sizing["log2_ng"] = log2_ng
        cap = [t.numel() * t.element_size() if t is not None else 0 for t in (d_entries, d_bstart, d_buckets)]
        args = np.array([int(sizing.get(k, 0)) for k in self.SORT_PROBE_IN] + [cap[0] // 4, cap[1] // 4, cap[2]], dtype=np.int32)
        used = np.zeros(len(self.SORT_PROBE_USED), dtype=np.uint32)
        order(self.L, self.ctx, d_scalars, d_entries, d_bstart, d_maxcount, d_buckets)
        rc = self.L.ctt_hip_sort_probe_words(self.ctx, ptr(d_scalars), kwords, n, ptr(args), ptr(used), ptr(d_entries),
                                             ptr(d_bstart), ptr(d_maxcount), ptr(d_buckets))
        return dict(zip(self.SORT_PROBE_USED, (int(x) for x in used))) if rc == 0 else None

    def glv_front_probe(self, curve, d_scalars, d_points, n, d_records, d_half):
        """ctt_hip_glv_front_probe: the front kernel of the endomorphism split alone -- n canonical scalars [n][8] and n affine points in,
        the records [2n] and the half scalars [2n][4] out (include/ctt_msm_hip.h).  False when the call was refused (nothing launched)."""
        order(self.L, self.ctx, d_scalars, d_points, d_records, d_half)
        return self.L.ctt_hip_glv_front_probe(self.ctx, CURVES[curve].cid, ptr(d_scalars), ptr(d_points), n, ptr(d_records), ptr(d_half)) == 0

    def sum_reduce(self, curve, d_points, n, coord="aff"):
        """r = sum of n affine points resident in HBM (sum_reduce_vartime)."""
        info = CURVES[curve]
        r = result_buffer(info, coord)
        order(self.L, self.ctx, d_points)
        if self.L.ctt_hip_sum_reduce(self.ctx, info.cid, _COORD[coord], ptr(r), ptr(d_points), n, 1) != 0:
            raise RuntimeError("ctt_hip_sum_reduce failed")
        return r

    def batch_affine(self, curve, d_dst, d_src, n, src_coord="jac"):
        """d_dst[i] = affine(d_src[i]); both in HBM (batchAffine_vartime).  Returns when d_dst is complete."""
        order(self.L, self.ctx, d_src, d_dst)
        if self.L.ctt_hip_batch_affine(self.ctx, CURVES[curve].cid, _COORD[src_coord], ptr(d_dst),
                                       ptr(d_src), n, 1) != 0:
            raise RuntimeError("ctt_hip_batch_affine failed")

    def enable_timings(self, on=True):
        """Record the per-stage HIP events that last_timings() reads (off by default: they are host time per MSM and barrier
        packets in the queue).  on = 2: the accumulate stage and the total only (what a roofline needs)."""
        self.set_option("timings", int(on))

    def last_timings(self):
        ms = np.zeros(6, dtype=np.float32)
        self.L.ctt_hip_msm_last_timings(self.ctx, ptr(ms), 6)
        return dict(zip(("digits", "sort", "accumulate", "merge", "reduce", "total"), (float(x) for x in ms)))

    def last_plan(self):
        """c, W = accumulations per input pair (the digit windows of the scalar; twice the bucket sets when the endomorphism split
        ran), K, G, S, lanes, bucket_sets and glv (1 = the split ran)."""
        p = np.zeros(8, dtype=np.int32)
        self.L.ctt_hip_msm_last_plan(self.ctx, ptr(p), 8)
        return dict(zip(("c", "W", "K", "G", "S", "lanes", "bucket_sets", "glv"), (int(x) for x in p)))


def set_devices(devices):
    """GPUs the host-pointer entry points (multiScalarMul_vartime[_parallel], CttEngine.msm) shard a call over, by points
    (ctt_hip_msm_set_devices; the reference's msm-level split, ec_multi_scalar_mul_parallel.nim:386-431).  A device id may
    repeat (one context each); fewer than two ids turns sharding off."""
    arr = (ctypes.c_int * max(1, len(devices)))(*devices)
    if _lib.lib().ctt_hip_msm_set_devices(arr, len(devices)) != 0:
        raise ValueError(f"device id out of range in {list(devices)}")


def set_shard_min(pairs_per_device):
    _lib.lib().ctt_hip_msm_set_shard_min(int(pairs_per_device))


def subgroup_check(curve, points, ctx=None):
    """ok[i] = ([r]points[i] is the neutral element), r = the curve order, for all points in one launch
    (ctt_hip_subgroup_check; the reference checks deserialised points one by one: isInSubgroup)."""
    info = CURVES[curve]
    pts = np.ascontiguousarray(points, dtype=np.uint8).reshape(-1, info.aff_bytes)
    ok = np.zeros(pts.shape[0], dtype=np.uint8)
    if _lib.lib().ctt_hip_subgroup_check(ctx, info.cid, ptr(ok), ptr(pts), pts.shape[0], 0) != 0:
        raise RuntimeError("ctt_hip_subgroup_check failed")
    return ok.astype(bool)


def ec_sum_affine(curve, pts_aff, coord="aff"):
    """Host-only sum of affine points (combining per-GPU partial MSMs)."""
    info = CURVES[curve]
    pts = np.ascontiguousarray(pts_aff, dtype=np.uint8).reshape(-1, info.aff_bytes)
    r = result_buffer(info, coord)
    rc = _lib.lib().ctt_hip_ec_sum_affine(info.cid, _COORD[coord], ptr(r), ptr(pts), pts.shape[0])
    if rc != 0:
        raise RuntimeError("ctt_hip_ec_sum_affine failed")
    return r


def sum_reduce_vartime(curve, points, coord="jac"):
    """Mirror of sum_reduce_vartime(r, points) (ec_shortweierstrass_batch_ops.nim:649-663), host arrays in, GPU sum."""
    info = CURVES[curve]
    pts = np.ascontiguousarray(points, dtype=np.uint8).reshape(-1, info.aff_bytes)
    r = result_buffer(info, coord)
    if _lib.lib().ctt_hip_sum_reduce(None, info.cid, _COORD[coord], ptr(r), ptr(pts), pts.shape[0], 0) != 0:
        raise RuntimeError("ctt_hip_sum_reduce failed")
    return r


def batchAffine_vartime(curve, points, coord="jac"):
    """Mirror of batchAffine_vartime(affs, projs) through the Constantine C symbol `ctt_<curve>_<coord>_batch_affine`
    (bindings/c_curve_decls.nim:395-396): [n][3 coordinates] Montgomery bytes -> [n] affine points."""
    info = CURVES[curve]
    src = np.ascontiguousarray(points, dtype=np.uint8).reshape(-1, 3 * info.coord_bytes)
    dst = np.zeros((src.shape[0], info.aff_bytes), dtype=np.uint8)
    fn = getattr(_lib.lib(), f"ctt_{info.sym}_{coord}_batch_affine")
    fn(ptr(dst), ptr(src), src.shape[0])
    return dst


class CachedBases:
    """Base points resident in HBM in the device representation (ctt_hip_msm_bases_*).

    table=True also keeps their multiples 2^(c*w) * P for every digit window (ctt_hip_msm_bases_create_table): (bits/c + 1)
    times the memory, and every later MSM over these bases needs bits/c + 1 accumulations per pair into one bucket set
    with a larger c than a table-less MSM (window_bits = 0: chosen from the number of bases), and no window combine."""

    def __init__(self, curve, points, ctx=None, on_device=False, table=False, window_bits=0):
        self.L = _lib.lib()
        self.curve = curve
        self.info = CURVES[curve]
        self.ctx = ctx
        if on_device:
            import torch
            self.n = int(points.shape[0])
            torch.cuda.current_stream(points.device).synchronize()  # the records are made from the tensor as it is now
        else:
            points = np.ascontiguousarray(points, dtype=np.uint8)
            if points.ndim != 2 or points.shape[1] != self.info.aff_bytes:
                raise ValueError(f"points must have shape (n, {self.info.aff_bytes})")
            self.n = points.shape[0]
        if table:
            self.handle = self.L.ctt_hip_msm_bases_create_table(ctx, self.info.cid, ptr(points), self.n, 1 if on_device else 0,
                                                                int(window_bits))
        else:
            self.handle = self.L.ctt_hip_msm_bases_create(ctx, self.info.cid, ptr(points), self.n, 1 if on_device else 0)
        if not self.handle:
            raise RuntimeError("ctt_hip_msm_bases_create failed")
        self.window_bits = self.L.ctt_hip_msm_bases_window_bits(self.handle)  # 0 = plain records

    def submit(self, d_coefs, n, fr_coefs=False):
        """Coefficients resident on the device (torch CUDA tensor or raw address): enqueue and return a ticket for
        DeviceMsm.finish / CachedBases.finish (at most three outstanding per curve)."""
        if n > self.n:
            raise AssertionError("more coefficients than cached bases")
        order(self.L, self.ctx, d_coefs)
        t = self.L.ctt_hip_msm_with_bases_submit(self.ctx, self.handle, COEF_FR if fr_coefs else COEF_BIG,
                                                 ptr(d_coefs), n)
        if t < 0:
            raise RuntimeError("ctt_hip_msm_with_bases_submit failed (wrong context, or three tickets already outstanding)")
        return (self.curve, t)

    def finish(self, ticket, coord="prj"):
        curve, t = ticket
        r = result_buffer(self.info, coord)
        if self.L.ctt_hip_msm_device_finish(self.ctx, t, _out_kind(self.info, coord), ptr(r)) != 0:
            raise RuntimeError("ctt_hip_msm_device_finish failed (ticket not outstanding)")
        return r

    def msm(self, coefs, coord="prj", fr_coefs=False):
        if is_cuda(coefs):
            return self.finish(self.submit(coefs, int(coefs.shape[0]), fr_coefs=fr_coefs), coord=coord)
        coefs = np.ascontiguousarray(coefs, dtype=np.uint8)
        if coefs.ndim != 2 or coefs.shape[1] != 32:
            raise ValueError("coefs must have shape (n, 32)")
        if coefs.shape[0] > self.n:
            raise AssertionError("more coefficients than cached bases")
        r = result_buffer(self.info, coord)
        rc = self.L.ctt_hip_msm_with_bases(self.ctx, self.handle, COEF_FR if fr_coefs else COEF_BIG, _out_kind(self.info, coord), ptr(r),
                                           ptr(coefs), coefs.shape[0], 0)
        if rc != 0:
            raise RuntimeError("ctt_hip_msm_with_bases failed")
        return r

    def close(self):
        if self.handle:
            self.L.ctt_hip_msm_bases_destroy(self.ctx, self.handle)
            self.handle = None


class CttEngine:
    """Mirror of the Halo2-ZAL engine (constantine-halo2-zal/src/lib.rs:22-96): BN254-Snarks G1,
    coefficients are Fr elements in Montgomery form, result is a projective point."""

    CURVE = "bn254_snarks_g1"

    def __init__(self, num_threads=0):
        self.num_threads = num_threads  # kept for signature parity; the GPU path has no thread pool

    def msm(self, coeffs, bases):
        # lib.rs:42-58 -> ctt_bn254_snarks_g1_prj_multi_scalar_mul_fr_coefs_vartime_parallel
        if len(coeffs) != len(bases):
            raise AssertionError("coeffs and bases must have the same length")  # assert_eq! at lib.rs:43
        return multiScalarMul_vartime_parallel(None, self.CURVE, coeffs, bases, coord="prj", fr_coefs=True)

    # descriptor API (lib.rs:60-95). Upstream these are pass-throughs with a "put device specific preprocessing
    # here" note; the base descriptor here uploads + converts the points once and keeps them in HBM.
    def get_coeffs_descriptor(self, coeffs):
        return np.ascontiguousarray(coeffs, dtype=np.uint8)

    TABLE_BYTES_AUTO = 2 << 30

    def get_base_descriptor(self, bases, table=None):
        # table=True: the window table (CachedBases) -- bits/c + 1 multiples of every base resident in HBM (13-17x the plain
        # records) and c*(bits/c) doublings per base to build, one bucket set per MSM afterwards.  Automatic (None): only while
        # the table stays below TABLE_BYTES_AUTO; the library itself falls back to plain records when a table does not fit.
        if table is None:
            # rows of the table the library would build: one per digit window, bits/c + 1 with c ~ log2(n) (choose_table_window_bits,
            # msm_plan.h: 13 rows of 128-byte records at 2^20 bases = 1.74 GB; round 3 estimated 17 rows and dropped the table
            # for exactly that size)
            n = max(1, len(bases))
            c_est = min(22, max(8, int(np.ceil(np.log2(n)))))
            rows = -(-(CURVES[self.CURVE].scalar_bits + 1) // c_est)
            table = n * rows * 128 <= self.TABLE_BYTES_AUTO
        return CachedBases(self.CURVE, bases, table=table)

    def msm_with_cached_scalars(self, coeffs_desc, bases):
        return self.msm(coeffs_desc, bases)

    def msm_with_cached_base(self, coeffs, base_desc):
        if len(coeffs) != base_desc.n:
            raise AssertionError("coeffs and bases must have the same length")
        return base_desc.msm(coeffs, coord="prj", fr_coefs=True)

    def msm_with_cached_inputs(self, coeffs_desc, base_desc):
        return self.msm_with_cached_base(coeffs_desc, base_desc)
