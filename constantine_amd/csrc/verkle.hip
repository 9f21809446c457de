// verkle.hip -- kernels of the batched Verkle commitment and update over a fixed Banderwagon basis (bodies: verkle_bodies.h, DESIGN.md
// sections 11 and 12).  The commit and the update kernel share the LDS tree vk_tree.
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

// The pairwise sum of a group of lanes through its SLOTS slots of LDS (vk_tree_put / vk_tree_take, verkle_bodies.h), from level `first`
// down to 1: afterwards lane 0 holds the sum of the lanes below 2 * first.  Every lane of the workgroup runs the same levels, so
// the barriers are uniform.
template <uint32_t SLOTS>
__device__ __forceinline__ void vk_tree(uint32_t* slots, uint32_t lane, uint32_t first, XYZZ<VkF>& acc) {
#pragma unroll 1
  for (uint32_t s = first; s >= 1; s >>= 1) {
    vk_tree_put<VkF, SLOTS>(slots, lane, s, acc);
    __syncthreads();
    vk_tree_take<VkF, SLOTS>(slots, lane, s, acc);
    __syncthreads();
  }
}

// One workgroup per commitment, lane i owns base i: W gathers and mixed additions in registers, then the tree over the live lanes
// (128 slots of 128 bytes).  Lanes without a base or without a non-zero digit hold the in-memory neutral.
__global__ void __launch_bounds__(VK_MAX_BASES) k_vk_commit(VkCommitArgs a) {
  __shared__ uint32_t slots[VK_EXT_WORDS * VK_TREE_SLOTS];
  const uint32_t k = blockIdx.x, lane = threadIdx.x;
  XYZZ<VkF> acc = vk_lane_sum<VkF, VkFr>(a, k, lane);
  uint32_t live = 1;
  while (live < a.n) live <<= 1;
  vk_tree<VK_TREE_SLOTS>(slots, lane, live >> 1, acc);
  if (lane == 0) vk_store_ext<VkF>(a.out, k, acc);
}

// One wavefront per row, four rows per workgroup: the lanes of a wave share the row's entries x windows (vk_update_lane_sum), then the
// six levels of the tree through the wave's own 32 slots.  A wave without a row loads nothing and holds neutrals.
__global__ void __launch_bounds__(VK_UPDATE_BLOCK) k_vk_update(VkUpdateArgs a) {
  __shared__ uint32_t slots[VK_UPDATE_ROWS * VK_EXT_WORDS * VK_UPDATE_SLOTS];
  const uint32_t wave = threadIdx.x / VK_UPDATE_G, lane = threadIdx.x % VK_UPDATE_G;
  const uint32_t k = blockIdx.x * VK_UPDATE_ROWS + wave;
  XYZZ<VkF> acc = vk_update_lane_sum<VkF, VkFr>(a, k, lane, VK_UPDATE_G);
  vk_tree<VK_UPDATE_SLOTS>(slots + wave * (VK_EXT_WORDS * VK_UPDATE_SLOTS), lane, VK_UPDATE_SLOTS, acc);
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
