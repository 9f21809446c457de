"""
constantine_amd -- MI355X-native multi-scalar-multiplication engine behind Constantine's MSM API.

Only what the MSM hot path needs lives here:
  csrc/     HIP kernels (gfx950) + the C ABI  (include/ctt_msm_hip.h)  -> libctt_msm_hip.so
  _lib.py   ctypes loader (fails loudly if the HIP library is missing) and the prototype tables of both libraries
  _arrays.py  the pointer, result-buffer and stream-ordering helpers of every caller below
  msm.py    host-side mirror of the reference's entry points (multiScalarMul_vartime[_parallel],
            Halo2-ZAL CttEngine.msm) over the C ABI
  parallel.py  point-sharded multi-GPU MSM, one process per GPU (torch.distributed / RCCL); the in-library form, one
            process driving several GPUs, is ctt_hip_msm_set_devices / $CTT_HIP_DEVICES (msm.set_devices)
  synth.py  synthetic benchmark inputs (seeded scalars)
  verkle.py  batched Verkle commitments over a fixed Banderwagon basis: VerkleCrs.commit, batchMapToScalarField, serializeBatch_vartime
  fixed.py  batched fixed-base MSM over BLS12-381 G1 / BN254 G1 (FixedBaseMsm; include/ctt_msm_hip_fixed.h -> libctt_msm_hip_fixed.so)
  ntt.py    batched NTT over a curve's scalar field (NttPlan); the EIP-7594 cells and cell proofs of kzg.py run on it
  peerdas.py  EIP-7594 recovery batched over blobs (Recovery; include/ctt_msm_hip_peerdas.h -> libctt_msm_hip_peerdas.so)
  kzg.py, evm.py  ctypes callers of the reference's KZG / EIP-2537 MSM-precompile C symbols (csrc/protocols.hip: host side in C++)
"""
from .curves import CURVES, CurveInfo  # noqa: F401
from .msm import (  # noqa: F401
    CachedBases,
    CttEngine,
    DeviceMsm,
    MsmRefused,
    msm_available,
    msm_host,
    batchAffine_vartime,
    sum_reduce_vartime,
    multiScalarMul_vartime,
    multiScalarMul_vartime_parallel,
    set_devices,
    set_shard_min,
)
from .verkle import VerkleCrs, batchMapToScalarField, serializeBatch_vartime  # noqa: F401
from .fixed import FixedBaseMsm, FixedMsmRefused  # noqa: F401
