// copterstep_rollout_lqg.hip -- output-feedback (LQG) rollouts on gfx950 (cs_rollout_lqg, include/copterstep.h): per env
// and step the affine feedback law at the filter's estimate, one true env step under that action, the measurement of
// the true state, and the extended Kalman filter's predict under the same action and update on that measurement -- K
// steps in one launch.  Nothing of the env state is written.  DESIGN.md section 22.
//
// Upstream lines composed: those of copterstep_rollout_grad.hip's forward (envs/task.py:77-137 step,
// dynamics/__init__.py:114-197 setMotors) for the truth, and those of copterstep_rollout_ekf.hip (the lines
// copterstep_jacobian.hip differentiates: setMotors, the state derivative, step) for the filter.
//
// One lane per env on the tile layout of the step kernels (tile t -> workgroup t).  Per step:
//   law      lqg_law.h at the posterior mean of the step before (the lane's LDS column X)
//   truth    rollout_step / next_perturbation (rollout_step.h) from the lane's parked truth, as rollout_forward makes it
//   filter   the calls copterstep_rollout_ekf.hip makes (filter_step.h): ekf_predict, filter_update -- its measurement
//            lqg_measure (lqg_law.h) on the parked true state, not a tape's entry -- and filter_store_row; the filter is
//            cs_rollout_ekf's by construction, not by two texts that agree
// The filter's LDS rows are copterstep_rollout_ekf.hip's (P 78, W 144 + 1, the step's start mean 12, the mean 12); the
// truth does not fit in registers across cov_predict and is parked behind them in 18 more lane-private rows (x 12, the
// pending force 3, prev_shaping, and two rows of packed integers) between its step and the next: 265 rows x 512 B =
// 132.5 KiB, one wavefront per CU (profiles/rollout_lqg_resources.txt).
#include <cmath>
#include <string>

#include "copterstep_jacobian.h"

// the truth must round as the step kernels do (its tapes are cs_rollout_states' bit for bit), the filter as
// cs_rollout_ekf does, and the law's and the measurement's float64 arithmetic is fixed (one multiply and one add per
// term, no fma)
#pragma clang fp contract(off)

#include "dev_tile.h"
#include "dev_codec.h"
#include "dev_math.h"
#include "dev_physics.h"
#include "dev_task.h"
#include "jacobian_tangents.h"
#include "rollout_adjoint.h"
#include "rollout_step.h"
#include "rollout_sweep.h"
#include "ekf_update.h"
#include "lqg_law.h"
#include "cov_tile.h"
#include "filter_step.h"
#include "dev_launch.h"

namespace cs {
namespace {

// the lane's LDS rows (row j at [j * kBlock]): the filter's as in copterstep_rollout_ekf.hip, then the parked truth
constexpr int kRowW = kEkfSym;
constexpr int kRowX0 = kRowW + kStageStride;
constexpr int kRowX = kRowX0 + 12;
constexpr int kRowT = kRowX + 12;   // the true state x [12] ...
constexpr int kRowTp = kRowT + 12;  // ... its pending perturbation (px, py, pz) and prev_shaping ...
constexpr int kRowTi = kRowTp + 4;  // ... and two rows of integers: {status and flags, steps}, {episode, its far flag}
constexpr int kLqgRows = kRowTi + 2;
static_assert(kLqgRows * kBlock * sizeof(double) <= 160 * 1024, "the LDS of one CU");

enum : uint32_t { kParkPend = 1u << 8, kParkExpl = 1u << 9, kParkReset = 1u << 10 };

// the truth between its step and the next: everything rollout_step and next_perturbation read or write
template <int MODE>
__device__ __forceinline__ void park_truth(double* T, const Env<MODE>& e, double px, double py, double pz) {
#pragma unroll
  for (int j = 0; j < 12; ++j) T[j * kBlock] = e.x[j];
  double* p = T + 12 * kBlock;
  p[0 * kBlock] = px;
  p[1 * kBlock] = py;
  p[2 * kBlock] = pz;
  p[3 * kBlock] = e.prev_sh;
  uint2* w = reinterpret_cast<uint2*>(T + 16 * kBlock);
  w[0 * kBlock] = make_uint2((uint32_t)e.fs | (e.pend ? kParkPend : 0u) | (e.expl ? kParkExpl : 0u) |
                                 (e.reset_pending ? kParkReset : 0u),
                             (uint32_t)e.steps);
  w[1 * kBlock] = make_uint2(e.episode, e.ep_far);
}

template <int MODE>
__device__ __forceinline__ void unpark_truth(const double* T, Env<MODE>& e, double& px, double& py, double& pz) {
#pragma unroll
  for (int j = 0; j < 12; ++j) e.x[j] = T[j * kBlock];
  const double* p = T + 12 * kBlock;
  px = p[0 * kBlock];
  py = p[1 * kBlock];
  pz = p[2 * kBlock];
  e.prev_sh = p[3 * kBlock];
  const uint2* w = reinterpret_cast<const uint2*>(T + 16 * kBlock);
  const uint2 a = w[0 * kBlock], b = w[1 * kBlock];
  e.fs = (int)(a.x & 0xFFu);
  e.pend = (a.x & kParkPend) != 0u;
  e.expl = (a.x & kParkExpl) != 0u;
  e.reset_pending = (a.x & kParkReset) != 0u;
  e.steps = (int)a.y;
  e.episode = b.x;
  e.ep_far = b.y;
  e.ep_hi = 0u;  // (resolved before the loop: the episode number is whole)
  e.ticks = 0u;
  e.ep_ret = 0.f;
}

template <int TASK, int MODE, bool GYRO>
__global__ __launch_bounds__(kBlock) void rollout_lqg_kernel(const DevConst c, const DevState s, const cs_rollout_io io,
                                                             const cs_rollout_lqg_io g) {
  constexpr int A = task_act_dim(TASK);
  constexpr bool FULL = MODE == CS_STATE_F64 || kFullTrigInEveryMode;
  using TILE = TileIO<MODE>;
  __shared__ __attribute__((aligned(16))) double lds[kLqgRows * kBlock];
  const int lane = threadIdx.x;
  const uint32_t tile_index = blockIdx.x;
  const uint32_t i = tile_index * kBlock + threadIdx.x;
  const uint32_t n = s.n;
  const uint32_t env0 = i - lane;
  const RowOut ro{lane, i, env0, i < n, env0 + (uint32_t)kWave <= n};
  const uint32_t ii = ro.valid ? i : 0u;  // (padding lanes read env 0's inputs and store nothing)
  const int K = io.num_steps;
  const int M = g.num_meas;
  const FilterTapes t = filter_tapes(io, g);

  Coef q = uniform_coef(c);
  if (s.veh != nullptr) q = load_coef(s.veh, s.veh_stride, ii);
  double* const P = lds + lane;
  double* const W = P + kRowW * kBlock;
  double* const X0 = P + kRowX0 * kBlock;
  double* const X = P + kRowX * kBlock;
  double* const T = P + kRowT * kBlock;
  double* const stage = lds + kRowW * kBlock;

  // ---- the truth's start, as rollout_forward decodes it: the stored env or io's explicit start ----
  {
    const TILE tile(s, tile_index, lane);
    Env<MODE> e;
    unpack_env<MODE, TILE>(c, tile.load_group(0), tile.load_group(1), tile.load_group(2), tile.load_group(3), e);
    resolve_episode<MODE>(c, tile, e);
    double px, py, pz;
    rollout_start<TASK, MODE>(c, q, io, tile, i, n, ro.valid, e, px, py, pz);
    park_truth<MODE>(T, e, px, py, pz);
  }

  // ---- the caller's filter state: xhat_0, its status, the upper triangle of P0 ----
  int fs = filter_load_start(X, P, g.xhat0_dev, g.status0_dev, g.P0_dev, n, ii);
  EkfStats st{0.0, 0.0, true};

#pragma clang loop unroll(disable)
  for (int k = 0; k < K; ++k) {
    const size_t row = (size_t)k * n;  // 64-bit: K x N x 144 doubles pass 4 GiB at 1 M envs

    // ---- the law at the posterior mean of the step before ----
    float4 act;
    {
      const size_t at = (row + ii) * A;
      double dx[12];
      lqg_deviation(X, kBlock, g.xbar_dev + (row + ii) * 12, 1, dx);
      float a[A];
#pragma unroll
      for (int m = 0; m < A; ++m) a[m] = lqg_law(io.actions_dev[at + m], g.K_dev + (at + m) * 12, 1, dx);
      if (ro.valid) {
#pragma unroll
        for (int m = 0; m < A; ++m) g.actions_out_dev[at + m] = a[m];
      }
      if constexpr (A == 4)  // the task's motor fan-out, as load_action_at()
        act = make_float4(a[0], a[1], a[2], a[3]);
      else if constexpr (A == 2)
        act = make_float4(a[0], a[1], a[1], a[0]);
      else
        act = make_float4(a[0], a[0], a[0], a[0]);
    }

    // ---- the truth: one step of rollout_forward's loop from the parked state (W is dead: its rows are the stage) ----
    {
      const TILE tile(s, tile_index, lane);
      Env<MODE> e;
      double px, py, pz;
      unpark_truth<MODE>(T, e, px, py, pz);
      const bool resetting = e.reset_pending;
      double reward;
      bool term, trunc;
      rollout_step<TASK, MODE>(c, q, e, act, px, py, pz, reward, term, trunc);
      next_perturbation<MODE>(c, q, tile, i, resetting, e, px, py, pz);
      park_truth<MODE>(T, e, px, py, pz);
      if (io.x_dev != nullptr) store_x_row(stage, io.x_dev, row, ro, e.x);
      if (ro.valid) {
        if (io.reward_dev != nullptr) io.reward_dev[row + i] = reward;
        if (io.terminated_dev != nullptr) io.terminated_dev[row + i] = term ? 1 : 0;
        if (io.truncated_dev != nullptr) io.truncated_dev[row + i] = trunc ? 1 : 0;
        if (io.status_dev != nullptr) io.status_dev[row + i] = (uint8_t)e.fs;
      }
    }

    // ---- the filter's step under the same action: copterstep_rollout_ekf.hip's calls (filter_step.h), the measurement
    //      formed from the parked true state and written out on the way ----
    const uint32_t bits = ekf_predict<FULL, GYRO>(c, q, act, fs, X, X0, P, W, g.Q_dev, stage, t.x_pred, row, ro);
    const double* er = g.e_dev + (row + ii) * (size_t)M;
    filter_update(X, P, g.H_dev, g.r_dev, M, st, [&](int m) {
      const double z = lqg_measure(g.H_dev + m * 12, T, kBlock, er[m]);
      if (g.z_dev != nullptr && ro.valid) g.z_dev[(row + i) * (size_t)M + m] = z;
      return z;
    });
    filter_store_row<false>(t, stage, X, P, row, ro, k == K - 1, fs, bits, st.nis);
  }
  filter_store_end(t, ro, st);
}

template <int TASK, int MODE>
hipError_t lqg_t(const DevConst& c, const DevState& s, const cs_rollout_io& io, const cs_rollout_lqg_io& g,
                 hipStream_t stream) {
  CS_GYRO_LAUNCH(rollout_lqg_kernel, io, g);
}

hipError_t launch_rollout_lqg(int task, int mode, const DevConst& c, const DevState& s, const cs_rollout_io& io,
                              const cs_rollout_lqg_io& g, hipStream_t stream) {
  CS_DISPATCH(lqg_t, c, s, io, g, stream)
}

}  // namespace
}  // namespace cs

extern "C" int cs_rollout_lqg(cs_ctx* ctx, const cs_rollout_io* io, const cs_rollout_lqg_io* lio, void* stream) {
  using cs::report_error;
  const char* who = "cs_rollout_lqg";
  if (int rc_ = cs::check_rollout_io(io, who, false)) return rc_;
  if (lio == nullptr) return report_error(CS_ERR_ARG, "cs_rollout_lqg: null lio");
  if (lio->struct_size != sizeof(cs_rollout_lqg_io))
    return report_error(CS_ERR_ABI, ("cs_rollout_lqg: lio->struct_size " + std::to_string(lio->struct_size) + " != " +
                                     std::to_string(sizeof(cs_rollout_lqg_io)) + " (sizeof(cs_rollout_lqg_io))").c_str());
  if (io->gx_dev != nullptr || io->gr_dev != nullptr || io->g_actions_dev != nullptr || io->g_x0_dev != nullptr)
    return report_error(CS_ERR_ARG, "cs_rollout_lqg: the cotangent and gradient pointers must be NULL");
  if (lio->out_dtype != CS_JAC_F64 && lio->out_dtype != CS_JAC_F32)
    return report_error(CS_ERR_ARG, "cs_rollout_lqg: unknown lio->out_dtype (CS_JAC_F64 or CS_JAC_F32)");
  const bool no_law =
      lio->K_dev == nullptr || lio->xbar_dev == nullptr || lio->e_dev == nullptr || lio->actions_out_dev == nullptr;
  if (int rc_ = cs::check_filter_model(
          who, lio->num_meas, no_law ? "K_dev, xbar_dev, e_dev and actions_out_dev are required" : nullptr,
          {lio->H_dev, lio->r_dev, lio->Q_dev, lio->P0_dev, lio->xhat0_dev, lio->status0_dev},
          "H_dev, r_dev, Q_dev, P0_dev, xhat0_dev and status0_dev"))
    return rc_;
  cs::ContextView v;
  if (int rc_ = cs::enter_filter_context(
          ctx, who, stream, lio->out_dtype,
          {io->start_x_dev, io->start_force_dev, io->start_prev_shaping_dev, io->x_dev, io->reward_dev, lio->K_dev,
           lio->xbar_dev, lio->e_dev, lio->H_dev, lio->r_dev, lio->Q_dev, lio->P0_dev, lio->xhat0_dev, lio->z_dev,
           lio->xhat_dev, lio->x_pred_dev},
          {lio->P_dev, lio->P_tape_dev, lio->var_dev, lio->nis_dev, lio->loglik_dev},
          {io->actions_dev, lio->actions_out_dev}, "actions_dev / actions_out_dev", &v))
    return rc_;
  const hipError_t e = cs::launch_rollout_lqg(v.task, v.mode, *v.c, *v.s, *io, *lio, (hipStream_t)stream);
  if (e != hipSuccess) return cs::report_hip(e, "cs_rollout_lqg: kernel launch");
  return CS_OK;
}
