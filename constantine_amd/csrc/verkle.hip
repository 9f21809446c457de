// verkle.hip -- kernels of the batched Verkle commitment over a fixed Banderwagon basis (bodies: verkle_bodies.h).
#include "verkle.h"

#include "hip_errors.h"

namespace ctt {

#define VK_HIP_CHECK(expr)                                                                            \
  do {                                                                                               \
    hipError_t e_ = (expr);                                                                          \
    if (e_ != hipSuccess)                                                                            \
      ::ctt::hip_failed(#expr, hipGetErrorString(e_), e_ == hipErrorOutOfMemory, __FILE__, __LINE__); \
  } while (0)

using VkF = Banderwagon::F;
using VkFr = Banderwagon::Fr;

static constexpr int VK_TABLE_BLOCK = 64;
static constexpr int VK_FINISH_BLOCK = 64;
static constexpr uint32_t VK_TREE_SLOTS = VK_MAX_BASES / 2;
static constexpr uint32_t VK_UPDATE_G = 64;                       // lanes per row of an update: one wavefront
static constexpr uint32_t VK_UPDATE_ROWS = 4;                     // rows per workgroup
static constexpr uint32_t VK_UPDATE_BLOCK = VK_UPDATE_G * VK_UPDATE_ROWS;
static constexpr uint32_t VK_UPDATE_SLOTS = VK_UPDATE_G / 2;

__global__ void __launch_bounds__(VK_TABLE_BLOCK) k_vk_table(VkTableArgs a) {
  vk_table_body<VkF>(a, blockIdx.x * blockDim.x + threadIdx.x);
}

// One workgroup per commitment, lane i owns base i: W gathers and mixed additions in registers, then the lanes are summed pairwise
// through LDS -- in every step the upper half of the live lanes hands its point to the lower half (128 slots of 128 bytes, stored
// word-major so that a wave's accesses fall into consecutive banks).  Lanes without a base or without a non-zero digit hold the
// in-memory neutral, which ed_add passes through.
__global__ void __launch_bounds__(VK_MAX_BASES) k_vk_commit(VkCommitArgs a) {
  __shared__ uint32_t slots[VK_EXT_WORDS * VK_TREE_SLOTS];
  const uint32_t k = blockIdx.x, lane = threadIdx.x;
  XYZZ<VkF> acc = vk_lane_sum<VkF, VkFr>(a, k, lane);
  uint32_t live = 1;
  while (live < a.n) live <<= 1;
#pragma unroll 1
  for (uint32_t s = live >> 1; s >= 1; s >>= 1) {
    if (lane >= s && lane < 2 * s) {
      uint32_t* o = slots + (lane - s);
#pragma unroll
      for (int t = 0; t < 8; t++) {
        o[t * VK_TREE_SLOTS] = acc.x.l[t];
        o[(8 + t) * VK_TREE_SLOTS] = acc.y.l[t];
        o[(16 + t) * VK_TREE_SLOTS] = acc.zz.l[t];
        o[(24 + t) * VK_TREE_SLOTS] = acc.zzz.l[t];
      }
    }
    __syncthreads();
    if (lane < s) {
      const uint32_t* o = slots + lane;
      XYZZ<VkF> q;
#pragma unroll
      for (int t = 0; t < 8; t++) {
        q.x.l[t] = o[t * VK_TREE_SLOTS];
        q.y.l[t] = o[(8 + t) * VK_TREE_SLOTS];
        q.zz.l[t] = o[(16 + t) * VK_TREE_SLOTS];
        q.zzz.l[t] = o[(24 + t) * VK_TREE_SLOTS];
      }
      acc = ed_add<VkF>(acc, q);
    }
    __syncthreads();
  }
  if (lane == 0) vk_store_ext<VkF>(a.out, k, acc);
}

// One wavefront per row, four rows per workgroup: the lanes of a wave share the row's entries x windows (vk_update_lane_sum), then six
// ed_add levels through the wave's own 32 slots of LDS, word-major as above.  Every wave runs the same six levels, so the barriers
// are uniform; a wave without a row loads nothing and holds neutrals.
__global__ void __launch_bounds__(VK_UPDATE_BLOCK) k_vk_update(VkUpdateArgs a) {
  __shared__ uint32_t slots[VK_UPDATE_ROWS * VK_EXT_WORDS * VK_UPDATE_SLOTS];
  const uint32_t wave = threadIdx.x / VK_UPDATE_G, lane = threadIdx.x % VK_UPDATE_G;
  const uint32_t k = blockIdx.x * VK_UPDATE_ROWS + wave;
  XYZZ<VkF> acc = vk_update_lane_sum<VkF, VkFr>(a, k, lane, VK_UPDATE_G);
  uint32_t* mine = slots + wave * (VK_EXT_WORDS * VK_UPDATE_SLOTS);
#pragma unroll 1
  for (uint32_t s = VK_UPDATE_SLOTS; s >= 1; s >>= 1) {
    if (lane >= s && lane < 2 * s) {
      uint32_t* o = mine + (lane - s);
#pragma unroll
      for (int t = 0; t < 8; t++) {
        o[t * VK_UPDATE_SLOTS] = acc.x.l[t];
        o[(8 + t) * VK_UPDATE_SLOTS] = acc.y.l[t];
        o[(16 + t) * VK_UPDATE_SLOTS] = acc.zz.l[t];
        o[(24 + t) * VK_UPDATE_SLOTS] = acc.zzz.l[t];
      }
    }
    __syncthreads();
    if (lane < s) {
      const uint32_t* o = mine + lane;
      XYZZ<VkF> q;
#pragma unroll
      for (int t = 0; t < 8; t++) {
        q.x.l[t] = o[t * VK_UPDATE_SLOTS];
        q.y.l[t] = o[(8 + t) * VK_UPDATE_SLOTS];
        q.zz.l[t] = o[(16 + t) * VK_UPDATE_SLOTS];
        q.zzz.l[t] = o[(24 + t) * VK_UPDATE_SLOTS];
      }
      acc = ed_add<VkF>(acc, q);
    }
    __syncthreads();
  }
  if (lane == 0 && k < a.m) vk_update_store<VkF>(a, k, acc);
}

__global__ void __launch_bounds__(VK_FINISH_BLOCK) k_vk_finish(VkFinishArgs a) {
  vk_finish_body<VkF, VkFr>(a, blockIdx.x * blockDim.x + threadIdx.x);
}

__global__ void __launch_bounds__(VK_FINISH_BLOCK) k_vk_delta(VkDeltaArgs a) {
  vk_delta_body<VkFr>(a, blockIdx.x * blockDim.x + threadIdx.x);
}

void vk_launch_table(hipStream_t stream, const VkTableArgs& a) {
  const uint32_t lanes = a.n * a.W;
  hipLaunchKernelGGL(k_vk_table, dim3((lanes + VK_TABLE_BLOCK - 1) / VK_TABLE_BLOCK), dim3(VK_TABLE_BLOCK), 0, stream, a);
  VK_HIP_CHECK(hipGetLastError());
}
void vk_launch_commit(hipStream_t stream, const VkCommitArgs& a) {
  hipLaunchKernelGGL(k_vk_commit, dim3(a.m), dim3(VK_MAX_BASES), 0, stream, a);
  VK_HIP_CHECK(hipGetLastError());
}
void vk_launch_update(hipStream_t stream, const VkUpdateArgs& a) {
  hipLaunchKernelGGL(k_vk_update, dim3((a.m + VK_UPDATE_ROWS - 1) / VK_UPDATE_ROWS), dim3(VK_UPDATE_BLOCK), 0, stream, a);
  VK_HIP_CHECK(hipGetLastError());
}
void vk_launch_delta(hipStream_t stream, const VkDeltaArgs& a) {
  hipLaunchKernelGGL(k_vk_delta, dim3((a.m + VK_FINISH_BLOCK - 1) / VK_FINISH_BLOCK), dim3(VK_FINISH_BLOCK), 0, stream, a);
  VK_HIP_CHECK(hipGetLastError());
}
void vk_launch_finish(hipStream_t stream, const VkFinishArgs& a) {
  const uint32_t lanes = (a.m + a.K - 1) / a.K;
  hipLaunchKernelGGL(k_vk_finish, dim3((lanes + VK_FINISH_BLOCK - 1) / VK_FINISH_BLOCK), dim3(VK_FINISH_BLOCK), 0, stream, a);
  VK_HIP_CHECK(hipGetLastError());
}

}  // namespace ctt
