// ntt.h -- the scalar-field NTT's operation table: one per scalar field, instantiated once in ntt.hip (BLS12-381 G1 and G2 share
// theirs, as do BN254-Snarks G1 and G2); a curve's CurveOps points at the table of its C::Fr (hip_backend.h).  Bodies: ntt_bodies.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "field_params.h"
#include "ntt_plan.h"

namespace ctt {

struct NttOps {
  int two_adicity;   // of the field's multiplicative group: log2n <= min(NTT_MAX_LOG2N, two_adicity)
  // A plan: the twiddle table omega^i, i < n/2 (16 * n bytes), built by a kernel on `s`.  omega: 32 canonical little-endian bytes, host.
  // -> 0 and *plan; -1 omega is not below the modulus or omega^(n/2) != -1 (nothing allocated, nothing launched); -2 out of device
  // memory (*oom_bytes = the request)
  int (*plan_create)(hipStream_t s, int log2n, const void* omega, int tile_log2, void** plan, size_t* oom_bytes);
  void (*plan_destroy)(void* plan);
  // batch rows of n elements from d_in to d_out (may be equal); shift: NULL or 32 canonical bytes, host.  Enqueued on `s`, not waited for.
  // -> 0; -1 a shift of zero or not below the modulus (nothing launched); -2 out of device memory (the shift's n multipliers)
  int (*run)(hipStream_t s, void* plan, void* d_out, const void* d_in, size_t batch, int flags, const void* shift, size_t* oom_bytes);
  // info[0..3] = log2n, tile_log2, passes of a natural-order-in transform, bytes of the twiddle table
  void (*plan_info)(const void* plan, size_t info[4]);
};

template <class PP>
const NttOps* ntt_ops_for();
template <> const NttOps* ntt_ops_for<BLS12_381_Fr>();
template <> const NttOps* ntt_ops_for<BN254_Fr>();
template <> const NttOps* ntt_ops_for<Vesta_Fp>();      // Pallas' scalar field
template <> const NttOps* ntt_ops_for<Pallas_Fp>();     // Vesta's
template <> const NttOps* ntt_ops_for<Banderwagon_Fr>();

}  // namespace ctt
