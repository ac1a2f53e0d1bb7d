// copterstep_rollout_ekf.hip -- an extended Kalman filter over the env step on gfx950 (cs_rollout_ekf,
// include/copterstep.h): K predict / update steps per env in one launch, with a 12 x 12 symmetric covariance per env and
// the step Jacobian applied on the fly, never stored.  The filter's mean and covariance are the caller's: nothing of the
// env state is read but the constants and the vehicle table, and nothing is written.  DESIGN.md section 19.
//
// Upstream lines differentiated: those of copterstep_jacobian.hip (setMotors, the state derivative, step).
//
// One lane per env on the tile layout of the step kernels (tile t -> workgroup t).  Per step:
//   mean        the physics of rollout_step (clip, motor law, physics_substeps) from the filter's own mean and status
//   covariance  P- = A P A^T + Q by cov_predict (cov_tile.h: jacobian_block with zero wrench tangents -- the actions are
//               known -- in two passes of 6 blocks of 2 directions), the function the smoother calls for the same prior
//   update      M sequential scalar updates (ekf_update.h)
// The kernel is a start, a loop of predict / update / store and an end, every piece of it filter_step.h's: the functions
// copterstep_rollout_lqg.hip calls for its filter and, but for the predict, copterstep_rollout_ukf.hip for its own.
// P (78 rows, packed upper triangle), W (144 rows and one row of stage padding behind it), the mean at the start of the
// step (12 rows) and the prior / posterior mean (12 rows) live in lane-private LDS columns (element j of a lane at
// [j * 64 + lane], as section 13's): 247 rows x 512 B = 123.5 KiB, one wavefront per CU
// (profiles/rollout_ekf_resources.txt).  After the second pass W is dead: the wavefront's 12 x 12 outputs and its mean
// rows are staged there and leave as linear runs.
#include <cmath>
#include <string>

#include "copterstep_jacobian.h"

// the mean must round as the step kernels do: x_pred is cs_rollout_states' row from the same point bit for bit, and the
// update's float64 arithmetic is fixed (one multiply and one add per term, no fma)
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
#include "cov_tile.h"
#include "filter_step.h"
#include "dev_launch.h"

namespace cs {
namespace {

// the lane's LDS rows (row j at [j * kBlock]): the packed upper triangle of P, W = A P (W[i][c] at i * 12 + c) with one
// row of padding behind it (the stage of the 12 x 12 stores, cov_tile.h), the mean at the start of the step (the
// Jacobian's point) and the prior / posterior mean
constexpr int kRowW = kEkfSym;
constexpr int kRowX0 = kRowW + kStageStride;
constexpr int kRowX = kRowX0 + 12;
constexpr int kEkfRows = kRowX + 12;
static_assert(kEkfRows * kBlock * sizeof(double) <= 160 * 1024, "the LDS of one CU");

template <int TASK, int MODE, bool GYRO>
__global__ __launch_bounds__(kBlock) void rollout_ekf_kernel(const DevConst c, const DevState s, const cs_rollout_io io,
                                                             const cs_rollout_ekf_io e) {
  constexpr int A = task_act_dim(TASK);
  constexpr bool FULL = MODE == CS_STATE_F64 || kFullTrigInEveryMode;
  __shared__ __attribute__((aligned(16))) double lds[kEkfRows * kBlock];
  const int lane = threadIdx.x;
  const uint32_t tile_index = blockIdx.x;
  const uint32_t i = tile_index * kBlock + threadIdx.x;
  const uint32_t n = s.n;
  const uint32_t env0 = i - lane;
  const RowOut ro{lane, i, env0, i < n, env0 + (uint32_t)kWave <= n};
  const uint32_t ii = ro.valid ? i : 0u;  // (padding lanes filter env 0 and store nothing)
  const int K = io.num_steps;
  const int M = e.num_meas;
  const FilterTapes t = filter_tapes(io, e);

  Coef q = uniform_coef(c);
  if (s.veh != nullptr) q = load_coef(s.veh, s.veh_stride, ii);
  double* const P = lds + lane;
  double* const W = P + kRowW * kBlock;
  double* const X0 = P + kRowX0 * kBlock;
  double* const X = P + kRowX * kBlock;
  double* const stage = lds + kRowW * kBlock;

  // ---- the caller's filter state: xhat_0, its status, the upper triangle of P0 ----
  int fs = filter_load_start(X, P, io.start_x_dev, io.start_status_dev, e.P0_dev, n, ii);
  EkfStats st{0.0, 0.0, true};

#pragma clang loop unroll(disable)
  for (int k = 0; k < K; ++k) {
    const size_t row = (size_t)k * n;  // 64-bit: K x N x 144 doubles pass 4 GiB at 1 M envs
    const float4 act = load_action_at<TASK>(io.actions_dev + (row + ii) * A);
    const uint32_t bits = ekf_predict<FULL, GYRO>(c, q, act, fs, X, X0, P, W, e.Q_dev, stage, t.x_pred, row, ro);
    const double* zr = e.z_dev + (row + ii) * (size_t)M;
    filter_update(X, P, e.H_dev, e.r_dev, M, st, [zr](int m) { return zr[m]; });
    filter_store_row<false>(t, stage, X, P, row, ro, k == K - 1, fs, bits, st.nis);
  }
  filter_store_end(t, ro, st);
}

template <int TASK, int MODE>
hipError_t ekf_t(const DevConst& c, const DevState& s, const cs_rollout_io& io, const cs_rollout_ekf_io& e,
                 hipStream_t stream) {
  CS_GYRO_LAUNCH(rollout_ekf_kernel, io, e);
}

hipError_t launch_rollout_ekf(int task, int mode, const DevConst& c, const DevState& s, const cs_rollout_io& io,
                              const cs_rollout_ekf_io& e, hipStream_t stream) {
  CS_DISPATCH(ekf_t, c, s, io, e, stream)
}

}  // namespace
}  // namespace cs

extern "C" int cs_rollout_ekf(cs_ctx* ctx, const cs_rollout_io* io, const cs_rollout_ekf_io* eio, void* stream) {
  using cs::report_error;
  const char* who = "cs_rollout_ekf";
  if (int rc_ = cs::check_rollout_io(io, who, false)) return rc_;
  const bool no_start = io->start_x_dev == nullptr || io->start_status_dev == nullptr;
  const bool extra = io->reward_dev != nullptr || io->terminated_dev != nullptr || io->truncated_dev != nullptr ||
                     io->gx_dev != nullptr || io->gr_dev != nullptr || io->g_actions_dev != nullptr ||
                     io->g_x0_dev != nullptr;
  if (int rc_ = cs::check_filter_io(io, who, {"eio", "cs_rollout_ekf_io", eio, sizeof(cs_rollout_ekf_io)},
                                    no_start ? "start_x_dev (the mean) and start_status_dev are required" : nullptr,
                                    extra ? "the reward, flag, cotangent and gradient pointers must be NULL" : nullptr))
    return rc_;
  if (int rc_ = cs::check_filter_model(who, eio->num_meas, nullptr,
                                       {eio->H_dev, eio->r_dev, eio->Q_dev, eio->P0_dev, eio->z_dev},
                                       "H_dev, r_dev, Q_dev, P0_dev and z_dev"))
    return rc_;
  cs::ContextView v;
  if (int rc_ = cs::enter_filter_context(
          ctx, who, stream, eio->out_dtype,
          {io->start_x_dev, io->x_dev, eio->H_dev, eio->r_dev, eio->Q_dev, eio->P0_dev, eio->z_dev, eio->x_pred_dev},
          {eio->P_dev, eio->P_tape_dev, eio->var_dev, eio->nis_dev, eio->loglik_dev}, {io->actions_dev}, "actions_dev",
          &v))
    return rc_;
  const hipError_t e = cs::launch_rollout_ekf(v.task, v.mode, *v.c, *v.s, *io, *eio, (hipStream_t)stream);
  if (e != hipSuccess) return cs::report_hip(e, "cs_rollout_ekf: kernel launch");
  return CS_OK;
}
