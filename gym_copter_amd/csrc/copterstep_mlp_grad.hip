// copterstep_mlp_grad.hip -- the policy-parameter gradient of the closed-loop rollouts on gfx950 (cs_mlp_param_grad,
// include/copterstep.h): g_theta = sum_{k,n} J_theta pi(o_{k-1,n})^T g_a_{k,n}, the reduction that follows
// cs_rollout_mlp_vjp, over the forward's obs tape and the backward's g_actions.  DESIGN.md section 12.
//
// The loop replaced: the backward of lander.py:40-65 under a policy, the part of it that a training step needs for the
// policy's own weights (gym_copter_amd.mlp.param_grad is the same sum as torch matrix products).
//
// The split-K reduction of mlp_grad_kit.h over R = K N rows: lane = (row slot s, hidden unit j), its sums in registers,
// one [P] partial per workgroup, which mlp_grad_sum_kernel adds in a fixed order.  A tile's 64 consecutive rows come in
// coalesced and go through the LDS as float64, so a lane reads its slot's row at a slot-uniform address.
#include <string>

#include "copterstep_jacobian.h"

// the sums are explicit fma chains (the arithmetic include/copterstep.h documents), whatever the compiler would contract
#pragma clang fp contract(off)

#include "mlp_grad_kit.h"

namespace cs {
namespace {

// HP: 0 = the linear policy (one row per lane), else the hidden width rounded up (8, 16, 32 or 64 lanes per row)
template <int OBS, int A, int HP>
__global__ __launch_bounds__(kGradBlock) void mlp_param_grad_kernel(const float* __restrict__ params, const int H,
                                                                    const float* __restrict__ obs,
                                                                    const void* __restrict__ g_actions,
                                                                    const uint32_t ga_f32, const uint64_t rows,
                                                                    const uint32_t tiles_per_group,
                                                                    const uint32_t P, double* __restrict__ partials) {
  constexpr int LIVE = grad_live(HP), NACC = grad_nacc(OBS, A, HP);
  [[maybe_unused]] constexpr int SLOTS = 64 / LIVE;        // (HP > 0) rows in flight per wavefront
  constexpr int ROW = OBS + A;            // float64 values of a staged row
  constexpr int STAGE = kGradWaves * 64 * ROW;
  __shared__ __attribute__((aligned(16))) double smem[STAGE > kGradRed ? STAGE : kGradRed];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t tile_index = blockIdx.x;  // (the workgroup: its share of the row tiles, its partial; no state tiles here)
  double* const od = smem + wave * 64 * ROW;  // the wavefront's tile: obs [64][OBS] ...
  double* const gd = od + 64 * OBS;           // ... and g_a [64][A], float64

  // lane (s, j)'s weights in float64 and its sums (mlp_grad_kit.h)
  [[maybe_unused]] const int j = HP == 0 ? 0 : lane & (LIVE - 1), s = HP == 0 ? 0 : lane / LIVE;
  [[maybe_unused]] double w1[OBS], b1, w2[A];
  grad_lane_weights<OBS, A, HP>(params, H, j, w1, b1, w2);
  double acc[NACC];
#pragma unroll
  for (int q = 0; q < NACC; ++q) acc[q] = 0.0;

  const uint64_t tiles = (rows + 63) / 64;
  const uint64_t first = (uint64_t)tile_index * tiles_per_group;
  const uint64_t last = first + tiles_per_group < tiles ? first + tiles_per_group : tiles;
#pragma clang loop unroll(disable)
  for (uint64_t tile = first + wave; tile < last; tile += kGradWaves) {
    // ---- the tile's rows, coalesced, into the LDS as float64 (64-bit offsets: the tapes pass 4 GiB at 1 M envs); rows
    // past the end are zeros and add zeros ----
    const uint64_t row0 = tile * 64;
    const uint32_t nrows = rows - row0 < 64 ? (uint32_t)(rows - row0) : 64u;
    const float* osrc = obs + row0 * OBS;
#pragma unroll
    for (int v = 0; v < OBS; ++v) {
      const uint32_t e = v * 64 + lane;
      od[e] = e < nrows * OBS ? (double)osrc[e] : 0.0;
    }
#pragma unroll
    for (int v = 0; v < A; ++v) {
      const uint32_t e = v * 64 + lane;
      double g = 0.0;
      if (e < nrows * A)
        g = ga_f32 ? (double)(reinterpret_cast<const float*>(g_actions) + row0 * A)[e]
                   : (reinterpret_cast<const double*>(g_actions) + row0 * A)[e];
      gd[e] = g;
    }
    wave_sync();
    if constexpr (HP == 0) {  // lane = row
      const double* o = od + lane * OBS;
      const double* g = gd + lane * A;
#pragma unroll
      for (int c = 0; c < A; ++c) {
#pragma unroll
        for (int i = 0; i < OBS; ++i) acc[c * OBS + i] = fma(g[c], o[i], acc[c * OBS + i]);
        acc[A * OBS + c] += g[c];
      }
    } else {
#pragma clang loop unroll(disable)
      for (int it = 0; it < LIVE; ++it) {  // 64 / SLOTS rows per slot
        const int r = it * SLOTS + s;
        double o[OBS], g[A];
#pragma unroll
        for (int i = 0; i < OBS; ++i) o[i] = od[r * OBS + i];
#pragma unroll
        for (int c = 0; c < A; ++c) g[c] = gd[r * A + c];
        double pre = b1;
#pragma unroll
        for (int i = 0; i < OBS; ++i) pre = fma(w1[i], o[i], pre);
        grad_unit_accumulate<OBS, A>(w2, o, g, tanh(pre), acc);
      }
    }
    wave_sync();  // (the next tile overwrites these rows)
  }

  // ---- the workgroup's partial ----
  grad_partial_reduce<OBS, A, HP>(acc, smem, partials + (size_t)tile_index * P, H);
}

// g_params[p] = the sum of parameter p's partials in a fixed order: four wavefronts take a quarter of the workgroups
// each, in index order (their loads independent of the running sum, 16 in flight), and the quarters are added in order
__global__ __launch_bounds__(kGradBlock) void mlp_grad_sum_kernel(const double* __restrict__ partials,
                                                                  const uint32_t groups, const uint32_t P,
                                                                  double* __restrict__ g_params) {
  __shared__ double quarter[kGradWaves][64];
  const uint32_t tile_index = blockIdx.x;  // (elementwise: 64 parameters per workgroup, no state tiles touched)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t p = tile_index * 64 + lane;
  double t = 0.0;
  if (p < P) {
    const uint32_t per = (groups + kGradWaves - 1) / kGradWaves;
    const uint32_t g0 = wave * per, g1 = g0 + per < groups ? g0 + per : groups;
#pragma unroll 16
    for (uint32_t g = g0; g < g1; ++g) t += partials[(size_t)g * P + p];
  }
  quarter[wave][lane] = t;
  __syncthreads();
  if (wave == 0 && p < P) {
    double sum = quarter[0][lane];
#pragma unroll
    for (int w = 1; w < kGradWaves; ++w) sum += quarter[w][lane];
    g_params[p] = sum;
  }
}

struct GradArgs {
  const float* params;
  int hidden;
  const float* obs;
  const void* g_actions;
  uint32_t ga_f32;
  uint64_t rows;
  uint32_t P;
  double* partials;
  double* g_params;
};

template <int OBS, int A, int HP>
hipError_t grad_launch(const GradArgs& a, hipStream_t stream) {
  const GradSplit split = grad_split(a.rows);
  hipLaunchKernelGGL((mlp_param_grad_kernel<OBS, A, HP>), dim3(split.groups), dim3(kGradBlock), 0, stream, a.params,
                     a.hidden, a.obs, a.g_actions, a.ga_f32, a.rows, split.per_group, a.P, a.partials);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(mlp_grad_sum_kernel, dim3((a.P + 63) / 64), dim3(kGradBlock), 0, stream, a.partials, split.groups,
                     a.P, a.g_params);
  return hipGetLastError();
}

hipError_t launch_mlp_param_grad(int task, const GradArgs& a, hipStream_t stream) {
  return for_task_shape(task, [&](auto obs, auto act) {
    return for_grad_width(a.hidden, [&](auto hp) { return grad_launch<obs(), act(), hp()>(a, stream); });
  });
}

}  // namespace
}  // namespace cs

extern "C" int cs_mlp_param_grad(cs_ctx* ctx, const cs_mlp_grad_io* io, void* stream) {
  const std::string w("cs_mlp_param_grad");
  // the argument block, checked before the context (a caller's layout error is reported as such, without a device)
  if (io == nullptr) return cs::report_error(CS_ERR_ARG, (w + ": null io").c_str());
  if (io->struct_size != sizeof(cs_mlp_grad_io))
    return cs::report_error(CS_ERR_ABI, (w + ": io->struct_size " + std::to_string(io->struct_size) + " != " +
                                         std::to_string(sizeof(cs_mlp_grad_io)) + " (sizeof(cs_mlp_grad_io))").c_str());
  if (io->ga_dtype != CS_JAC_F64 && io->ga_dtype != CS_JAC_F32)
    return cs::report_error(CS_ERR_ARG, (w + ": unknown ga_dtype (CS_JAC_F64 or CS_JAC_F32)").c_str());
  if (int rc_ = cs::check_hidden(w.c_str(), "hidden", io->hidden)) return rc_;
  if (io->num_steps < 1) return cs::report_error(CS_ERR_ARG, (w + ": num_steps must be >= 1").c_str());
  if (io->params_dev == nullptr) return cs::report_error(CS_ERR_ARG, (w + ": params_dev is required").c_str());
  if (io->obs_dev == nullptr) return cs::report_error(CS_ERR_ARG, (w + ": obs_dev (the obs tape) is required").c_str());
  if (io->g_actions_dev == nullptr) return cs::report_error(CS_ERR_ARG, (w + ": g_actions_dev is required").c_str());
  if (io->g_params_dev == nullptr) return cs::report_error(CS_ERR_ARG, (w + ": g_params_dev is required").c_str());
  cs::ContextView v;
  if (int rc_ = cs::enter_context(ctx, w.c_str(), stream, &v)) return rc_;
  double* partials = nullptr;
  if (int rc_ = cs::grad_scratch(ctx, cs::kScratchMlpGrad, w.c_str(), stream,
                                 (size_t)cs::kGradMaxGroups * cs::kMlpMaxParams * sizeof(double), &partials))
    return rc_;
  const int H = io->hidden;
  const uint32_t P = cs::mlp_param_count(cs::task_obs_dim(v.task), cs::task_act_dim(v.task), H);
  const cs::GradArgs a{io->params_dev, H, io->obs_dev, io->g_actions_dev, io->ga_dtype == CS_JAC_F32 ? 1u : 0u,
                       (uint64_t)io->num_steps * v.s->n, P, partials, io->g_params_dev};
  const hipError_t e = cs::launch_mlp_param_grad(v.task, a, (hipStream_t)stream);
  if (e != hipSuccess) return cs::report_hip(e, (w + ": kernel launch").c_str());
  return CS_OK;
}
