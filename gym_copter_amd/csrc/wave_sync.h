// wave_sync.h -- the wavefront-wide LDS hand-over of the kernels that stage values for their neighbours' lanes
// (cov_tile.h's users, copterstep_ppo_grad.hip, copterstep_mlp_grad.hip): what the lanes wrote before it, every lane of
// the wavefront may read after it.  Device code, no dependence on the other device headers.
#pragma once

namespace cs {
namespace {

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

}  // namespace
}  // namespace cs
