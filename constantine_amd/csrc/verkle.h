// verkle.h -- launchers of the batched Verkle commitment and update kernels (verkle.hip) for the engine's C ABI (msm_engine.hip).  The
// table, commit and update arguments each begin with the VkTable view of the CRS handle (verkle_bodies.h).
#pragma once
#include <hip/hip_runtime.h>

#include "verkle_bodies.h"

namespace ctt {

static constexpr int VK_DEFAULT_WINDOW_BITS = 10;   // measured best of 6, 8, 10 at every batch size

void vk_launch_table(hipStream_t stream, const VkTableArgs& a);     // a.n * a.W lanes
void vk_launch_commit(hipStream_t stream, const VkCommitArgs& a);   // a.m workgroups of VK_MAX_BASES lanes
void vk_launch_update(hipStream_t stream, const VkUpdateArgs& a);   // ceil(a.m / 4) workgroups of 256 lanes: one wavefront per row
void vk_launch_delta(hipStream_t stream, const VkDeltaArgs& a);     // a.m lanes
void vk_launch_finish(hipStream_t stream, const VkFinishArgs& a);   // ceil(a.m / a.K) lanes

}  // namespace ctt
