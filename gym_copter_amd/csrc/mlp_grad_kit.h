// mlp_grad_kit.h -- the split-K parameter reduction that cs_mlp_param_grad and both heads of cs_ppo_grad share
// (copterstep_mlp_grad.hip, copterstep_ppo_grad.hip).  A "skinny GEMM": the inner dimension is R rows, the output one
// theta of P <= 1092 numbers.  Every wavefront takes tiles of 64 rows and keeps its share of the output in registers:
// lane = (row slot s, hidden unit j) with HP = the hidden width rounded up to a power of two (0 = the linear network, one
// row per lane) and 64 / HP rows in flight; lane (s, j) owns gW1[j][.], gb1[j], gW2[.][j] (and a copy of gb2).  The slots
// of a wavefront are summed by a fixed shuffle tree, the four wavefronts of a workgroup through the LDS, and each
// workgroup writes one partial in theta's layout; a sum kernel of the translation unit adds the partials in a fixed
// order.  No floating-point atomics: the order of summation depends on (R, shape) alone.  NOUT = the network's outputs
// (A for a policy, 1 for a value function).  Included inside the translation unit's floating-point-contraction pragma,
// after copterstep_jacobian.h; not a stand-alone header, and no dev_*.h (those are the step kernels' sources, whose hash
// stamps the committed profiles).  DESIGN.md sections 12 and 18.
#pragma once

#include <type_traits>

#include "mlp_policy.h"
#include "wave_sync.h"

namespace cs {
namespace {

constexpr int kGradWaves = 4;                    // wavefronts per workgroup
constexpr int kGradBlock = 64 * kGradWaves;
constexpr int kGradChunk = 8;                    // accumulators reduced per pass through the LDS
constexpr uint32_t kGradMaxGroups = 1024;        // workgroups (= partials) at most: 4 per CU

// lanes of a wavefront that hold its sums after the slot reduction, and a lane's accumulators:
// HP > 0: [gW1[j][0..OBS), gb1[j], gW2[0..NOUT)[j], gb2[0..NOUT)];  HP = 0: [gW[c][i] at c OBS + i, gb[c] at NOUT OBS + c]
constexpr int grad_live(int HP) { return HP == 0 ? 1 : HP; }
constexpr int grad_nacc(int OBS, int NOUT, int HP) { return HP == 0 ? NOUT * (OBS + 1) : OBS + 1 + 2 * NOUT; }
// the LDS doubles of the workgroup's reduction: [kGradWaves][kGradChunk][64]
constexpr int kGradRed = kGradWaves * kGradChunk * 64;

// lane (s, j)'s weights in float64: W1[j][.], b1[j], W2[.][j]; zero for the idle lanes j >= H (they add zeros) and for
// the linear network
template <int OBS, int NOUT, int HP>
__device__ __forceinline__ void grad_lane_weights(const float* __restrict__ params, const int H, const int j,
                                                  double (&w1)[OBS], double& b1, double (&w2)[NOUT]) {
  b1 = 0.0;
#pragma unroll
  for (int i = 0; i < OBS; ++i) w1[i] = 0.0;
#pragma unroll
  for (int c = 0; c < NOUT; ++c) w2[c] = 0.0;
  if (HP != 0 && j < H) {
    const MlpLayout at = mlp_layout(OBS, NOUT, H);
#pragma unroll
    for (int i = 0; i < OBS; ++i) w1[i] = (double)params[j * OBS + i];
    b1 = (double)params[at.b1 + j];
#pragma unroll
    for (int c = 0; c < NOUT; ++c) w2[c] = (double)params[at.w2 + c * H + j];
  }
}

// One row through hidden unit j, backwards (HP > 0): from the row's observation o, the cotangent g on the outputs and
// the unit's value h = tanh(pre), gp = (sum_c W2[c][j] g[c]) (1 - h^2) and the lane's sums, every one an fma chain
template <int OBS, int NOUT>
__device__ __forceinline__ void grad_unit_accumulate(const double (&w2)[NOUT], const double (&o)[OBS],
                                                     const double (&g)[NOUT], const double h,
                                                     double (&acc)[OBS + 1 + 2 * NOUT]) {
  double gh = 0.0;
#pragma unroll
  for (int c = 0; c < NOUT; ++c) gh = fma(w2[c], g[c], gh);
  const double gp = gh * (1.0 - h * h);
#pragma unroll
  for (int i = 0; i < OBS; ++i) acc[i] = fma(gp, o[i], acc[i]);
  acc[OBS] += gp;
#pragma unroll
  for (int c = 0; c < NOUT; ++c) {
    acc[OBS + 1 + c] = fma(g[c], h, acc[OBS + 1 + c]);
    acc[OBS + 1 + NOUT + c] += g[c];
  }
}

// The workgroup's partial: the slots of a wavefront by a fixed shuffle tree, the wavefronts through the LDS (`red`,
// kGradRed doubles, which may be the memory the rows were staged in), written to `out` in theta's layout.  Called by
// every thread of the workgroup.
template <int OBS, int NOUT, int HP>
__device__ __forceinline__ void grad_partial_reduce(const double (&acc)[grad_nacc(OBS, NOUT, HP)], double* const red,
                                                    double* const out, const int H) {
  constexpr int LIVE = grad_live(HP), NACC = grad_nacc(OBS, NOUT, HP);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int q0 = 0; q0 < NACC; q0 += kGradChunk) {
    __syncthreads();  // (the staged rows, or the previous pass's sums, have been read)
#pragma unroll
    for (int ql = 0; ql < kGradChunk; ++ql) {
      if (q0 + ql < NACC) {
        double v = acc[q0 + ql];
#pragma unroll
        for (int off = 32; off >= LIVE; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane < LIVE) red[(wave * kGradChunk + ql) * 64 + lane] = v;
      }
    }
    __syncthreads();
    for (int idx = tid; idx < kGradChunk * LIVE; idx += kGradBlock) {
      const int ql = idx / LIVE, jj = idx % LIVE, q = q0 + ql;
      if (q >= NACC) continue;
      double t = red[ql * 64 + jj];
#pragma unroll
      for (int w = 1; w < kGradWaves; ++w) t += red[(w * kGradChunk + ql) * 64 + jj];
      if constexpr (HP == 0) {
        out[q] = t;
      } else if (jj < H) {  // theta's layout: [W1 (H x OBS), b1 (H), W2 (NOUT x H), b2 (NOUT)]
        if (q < OBS)
          out[jj * OBS + q] = t;
        else if (q == OBS)
          out[H * OBS + jj] = t;
        else if (q < OBS + 1 + NOUT)
          out[H * OBS + H + (q - OBS - 1) * H + jj] = t;
        else if (jj == 0)
          out[H * OBS + H + NOUT * H + (q - OBS - 1 - NOUT)] = t;
      }
    }
  }
}

// ---- host side ----
// the row tiles of a launch over its workgroups: at most kGradMaxGroups of them, `per_group` consecutive tiles each
struct GradSplit {
  uint32_t per_group, groups;
};
inline GradSplit grad_split(const uint64_t rows) {
  const uint64_t tiles = (rows + 63) / 64;
  const uint32_t per_group = (uint32_t)((tiles + kGradMaxGroups - 1) / kGradMaxGroups);
  return {per_group, (uint32_t)((tiles + per_group - 1) / per_group)};
}

template <int V>
using Int = std::integral_constant<int, V>;

// f(Int<HP>) for the hidden width H: HP = 0, or H rounded up to 8, 16, 32 or 64 lanes per row
template <class F>
hipError_t for_grad_width(const int H, F&& f) {
  if (H == 0) return f(Int<0>{});
  if (H <= 8) return f(Int<8>{});
  if (H <= 16) return f(Int<16>{});
  if (H <= 32) return f(Int<32>{});
  return f(Int<64>{});
}

// f(Int<OBS>, Int<A>) for the task: the four (OBS, A) shapes of the six tasks
template <class F>
hipError_t for_task_shape(const int task, F&& f) {
  switch (task_obs_dim(task)) {
    case 10:
      return f(Int<10>{}, Int<4>{});
    case 12:
      return f(Int<12>{}, Int<4>{});
    case 6:
      return f(Int<6>{}, Int<2>{});
    case 2:
      return f(Int<2>{}, Int<1>{});
    default:
      return hipErrorInvalidValue;
  }
}

}  // namespace
}  // namespace cs
