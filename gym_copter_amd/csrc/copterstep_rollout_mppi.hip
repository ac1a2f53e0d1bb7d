// copterstep_rollout_mppi.hip -- MPPI on gfx950 (cs_rollout_mppi_costs / cs_rollout_mppi_update, include/copterstep.h):
// P noisy copies of an action tape rolled out per env with the cost accumulated in registers, and the cost-weighted
// average of the perturbations.  Neither a state nor a noise value is written to memory: the noise is a counter-based
// draw (mppi_noise.h) that the update makes again.  Nothing of the env state is written.  DESIGN.md section 14.
//
// Upstream lines replaced: lander.py:40-65 (the action loop) with sampled actions; the step is rollout_step
// (rollout_step.h), the one cs_rollout_states runs.
//
// Costs: one lane per env on the tile layout of the step kernels (tile t -> workgroup t in x), the sample in grid y.
// The loop is rollout_forward's (rollout_sweep.h) with the noise as the action source and no stores but one float64 per
// lane at the end.  Update: one lane per env, the step in grid y; every wavefront recomputes its 64 envs' weights from
// the cost columns ([P,N]: each row a coalesced load) and accumulates the A components of its step.  A step's cost terms
// and the update's body are rollout_mppi.h's (mppi_step_cost, mppi_update_lane), shared with the knot-noise kernels.
#include "copterstep_jacobian.h"

// the samples' states must be cs_rollout_states' bit for bit; the cost's float64 arithmetic is not contracted either
#pragma clang fp contract(off)

#include "dev_tile.h"
#include "dev_codec.h"
#include "dev_math.h"
#include "dev_physics.h"
#include "dev_task.h"
#include "jacobian_tangents.h"
#include "rollout_adjoint.h"
#include "rollout_step.h"
#include "mppi_noise.h"
#include "dev_launch.h"
#include "rollout_mppi.h"

namespace cs {
namespace {

template <int TASK, int MODE>
__global__ __launch_bounds__(kBlock, 2) void rollout_mppi_costs_kernel(const DevConst c, const DevState s,
                                                                    const cs_rollout_io io, const MppiArgs m) {
  constexpr int A = task_act_dim(TASK);
  __shared__ __attribute__((aligned(16))) double wts[2 * tri_size(12) + tri_size(A)];  // Q, Q at the last step, R
  const int lane = threadIdx.x;
  const uint32_t tile_index = blockIdx.x, p = blockIdx.y;  // tile t -> workgroup t in x; the sample in y
  stage_triangle<12>(m.Q, wts, lane);
  stage_triangle<12>(m.Qf, wts + tri_size(12), lane);
  stage_triangle<A>(m.R, wts + 2 * tri_size(12), lane);
  __syncthreads();
  const uint32_t i = tile_index * kBlock + threadIdx.x;
  const uint32_t n = s.n;
  const bool valid = i < n;
  const uint32_t ii = valid ? i : 0u;  // (padding lanes roll env 0's actions out and store nothing)

  Coef q = uniform_coef(c);
  if (s.veh != nullptr) q = load_coef(s.veh, s.veh_stride, ii);
  // the start point, decoded as rollout_forward decodes it
  using TILE = TileIO<MODE>;
  const TILE tile(s, tile_index, lane);
  Env<MODE> e;
  unpack_env<MODE, TILE>(c, tile.load_group(0), tile.load_group(1), tile.load_group(2), tile.load_group(3), e);
  resolve_episode<MODE>(c, tile, e);
  double px, py, pz;
  rollout_start<TASK, MODE>(c, q, io, tile, i, n, valid, e, px, py, pz);

  float sig[A];
  double aref[A];
#pragma unroll
  for (int j = 0; j < A; ++j) {
    sig[j] = m.sigma[j];
    aref[j] = m.aref != nullptr ? m.aref[j] : 0.0;
  }
  const uint32_t gid = c.id_lo + ii;
  const float* abar = io.actions_dev + (size_t)ii * A;
  const size_t astep = (size_t)n * A;
  const double* xr = m.xref + (size_t)ii * 12;
  const size_t xstep = m.xref_steps ? (size_t)n * 12 : 0;
  const int K = io.num_steps;
  double S = 0.0;
#pragma clang loop unroll(disable)
  for (int k = 0; k < K; ++k) {
    // the sample's action: abar + sigma eps in float32, one multiply and one add; sample 0 is abar itself
    const float4 ab = load_action_at<TASK>(abar);
    abar += astep;
    const float abv[4] = {ab.x, ab.y, ab.z, ab.w};
    float a[A];
#pragma unroll
    for (int j = 0; j < A; ++j) a[j] = abv[j];
    if (p != 0u) {  // (uniform: the sample is the workgroup's)
#pragma unroll
      for (int j = 0; j < A; ++j) {
        const float da = sig[j] * mppi_noise(m.key, gid, m.nonce, (uint32_t)k + 1u, p, (uint32_t)j);
        a[j] = abv[j] + da;
      }
    }
    const bool resetting = e.reset_pending;
    double reward;
    bool term, trunc;
    rollout_step<TASK, MODE>(c, q, e, fan_out<A>(a), px, py, pz, reward, term, trunc);
    next_perturbation<MODE>(c, q, tile, i, resetting, e, px, py, pz);
    mppi_step_cost<A>(wts, xr, xstep, e.x, a, [&](int j) { return aref[j]; }, k == K - 1, m.wr, reward, S);
  }
  if (valid) m.costs[(size_t)p * n + i] = S;  // (64-bit: P x N doubles pass 4 GiB)
}

template <int TASK>
__global__ __launch_bounds__(kBlock) void rollout_mppi_update_kernel(uint32_t n, uint32_t id_lo, const float* abar_dev,
                                                                     const MppiArgs m) {
  constexpr int A = task_act_dim(TASK);
  const uint32_t tile = blockIdx.x, k0 = blockIdx.y;  // tile t -> workgroup t in x; step k0 + 1 in y
  const uint32_t i = tile * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t gid = id_lo + i;
  // (the scalar temperature is checked by the entry point: always warm)
  mppi_update_lane<A>(n, i, k0, abar_dev, m, m.lambda, true,
                      [&](uint32_t p, uint32_t j) { return mppi_noise(m.key, gid, m.nonce, k0 + 1u, p, j); });
}

template <int TASK, int MODE>
hipError_t mppi_costs_t(const DevConst& c, const DevState& s, const cs_rollout_io& io, const MppiArgs& m,
                        hipStream_t stream) {
  hipLaunchKernelGGL((rollout_mppi_costs_kernel<TASK, MODE>), dim3(grid_for(s.n), m.samples), dim3(kBlock), 0, stream,
                     c, s, io, m);
  return hipGetLastError();
}

template <int TASK, int MODE>
hipError_t mppi_update_t(const DevConst& c, const DevState& s, const cs_rollout_io& io, const MppiArgs& m,
                         hipStream_t stream) {
  hipLaunchKernelGGL((rollout_mppi_update_kernel<TASK>), dim3(grid_for(s.n), (uint32_t)io.num_steps), dim3(kBlock), 0,
                     stream, s.n, c.id_lo, io.actions_dev, m);
  return hipGetLastError();
}

hipError_t launch_mppi_costs(int task, int mode, const DevConst& c, const DevState& s, const cs_rollout_io& io,
                             const MppiArgs& m, hipStream_t stream) {
  CS_DISPATCH(mppi_costs_t, c, s, io, m, stream)
}

hipError_t launch_mppi_update(int task, int mode, const DevConst& c, const DevState& s, const cs_rollout_io& io,
                              const MppiArgs& m, hipStream_t stream) {
  CS_DISPATCH(mppi_update_t, c, s, io, m, stream)
}

}  // namespace
}  // namespace cs

extern "C" int cs_rollout_mppi_costs(cs_ctx* ctx, const cs_rollout_io* io, const cs_rollout_mppi_io* mio,
                                     void* stream) {
  const char* who = "cs_rollout_mppi_costs";
  if (int rc_ = cs::check_rollout_io(io, who, false)) return rc_;
  if (int rc_ = cs::check_mppi_io(mio, who)) return rc_;
  if (int rc_ = cs::check_mppi_costs_io(mio, who)) return rc_;
  cs::ContextView v;
  if (int rc_ = cs::enter_context(ctx, who, stream, &v)) return rc_;
  const cs::MppiArgs m = cs::mppi_args(ctx, *mio);
  const hipError_t e = cs::launch_mppi_costs(v.task, v.mode, *v.c, *v.s, *io, m, (hipStream_t)stream);
  if (e != hipSuccess) return cs::report_hip(e, "cs_rollout_mppi_costs: kernel launch");
  return cs::launch_mppi_best(m, v.s->n, (hipStream_t)stream, who);
}

extern "C" int cs_rollout_mppi_update(cs_ctx* ctx, const cs_rollout_io* io, const cs_rollout_mppi_io* mio,
                                      void* stream) {
  const char* who = "cs_rollout_mppi_update";
  if (int rc_ = cs::check_rollout_io(io, who, false)) return rc_;
  if (int rc_ = cs::check_mppi_io(mio, who)) return rc_;
  if (int rc_ = cs::check_mppi_update_io(io, mio, who)) return rc_;
  cs::ContextView v;
  if (int rc_ = cs::enter_context(ctx, who, stream, &v)) return rc_;
  const hipError_t e = cs::launch_mppi_update(v.task, v.mode, *v.c, *v.s, *io, cs::mppi_args(ctx, *mio),
                                              (hipStream_t)stream);
  if (e != hipSuccess) return cs::report_hip(e, "cs_rollout_mppi_update: kernel launch");
  return CS_OK;
}
