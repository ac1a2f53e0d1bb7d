// copterstep_rollout_lqr.hip -- the iLQR backward pass and feedback rollout on gfx950 (cs_rollout_lqr /
// cs_rollout_feedback_states, include/copterstep.h): the Riccati sweep over a rollout's tape with a 12 x 12 value
// Hessian per env, and the line search's forward pass under the time-varying affine feedback it returns.  Nothing of the
// env state is written.  DESIGN.md section 13.
//
// Upstream lines differentiated: those of copterstep_rollout_grad.hip (setMotors, the state derivative, step).
//
// One lane per env on the tile layout of the step kernels (tile t -> workgroup t).  The backward never forms the step
// Jacobians A, B: every product with them is a call of step_adjoint (rollout_step.h) with no reward cotangent, which
// returns (A^T lambda, B^T lambda) under every branch rule the rollout backward obeys.  Per step, with V = S + Q:
//   1 call   on v                       -> Qx, Qu
//   12 calls on the columns of V        -> W = A^T V and B^T V
//   A calls  on the columns of V B      -> B^T V B
//   12 calls on the columns of V A = W^T -> A^T V A and B^T V A
// All matrices live in lane-private LDS columns (element j of a lane at [j * 64 + lane], as section 11's accumulators):
// the adjoint's primal recompute already needs the whole register file.  302 rows x 512 B = 151 KiB for A = 4: one
// wavefront per CU (profiles/rollout_lqr_resources.txt).  The step and the sweep are lqr_step.h's, shared with the
// control-limited pass of copterstep_ilqr_box.hip; the feedback law is lqr_feedback.h's, shared with its forward.
#include <cmath>
#include <string>

#include "copterstep_jacobian.h"

// the primal must round as the step kernels do: the recomputed primal is the tape bit for bit, and the feedback law's
// float64 arithmetic is fixed (one multiply and one add per term, no fma)
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
#include "lqr_solve.h"
#include "cov_tile.h"
#include "lqr_step.h"
#include "lqr_feedback.h"
#include "dev_launch.h"

namespace cs {
namespace {

// the backward kernel: lqr_step.h's sweep with the unconstrained solve (LqrArgs, the LDS rows and the step are there)
template <int TASK, int MODE, bool GYRO>
__global__ __launch_bounds__(kBlock) void rollout_lqr_kernel(const DevConst c, const DevState s,
                                                             const cs_rollout_io io, const LqrArgs l) {
  __shared__ __attribute__((aligned(16))) double lds[lqr_rows(task_act_dim(TASK)) * kBlock];
  lqr_sweep<TASK, MODE, GYRO, LqrFreeSolve>(c, s, io, l, {}, lds);
}

// ---------------------------------------------------------------------------------------------------------------------
// the forward under the feedback
// ---------------------------------------------------------------------------------------------------------------------
// (rollout_forward's action source is lqr_feedback.h's FeedbackLaw, here without a clamp)
template <int TASK, int MODE>
__global__ __launch_bounds__(kBlock) void rollout_feedback_kernel(const DevConst c, const DevState s,
                                                                  const cs_rollout_io io,
                                                                  const cs_rollout_feedback_io f) {
  __shared__ __attribute__((aligned(16))) double xrow[kBlock * 12];  // 6 KiB: the wavefront's state rows of a step
  rollout_forward<TASK, MODE>(c, s, io, xrow,
                              FeedbackLaw<TASK, FeedbackNoClamp>{io.actions_dev, f.xbar_dev, f.K_dev, f.d_dev,
                                                                 f.alpha_dev, f.actions_out_dev, {}, 0u, 0u, 0.0});
}

template <int TASK, int MODE>
hipError_t lqr_t(const DevConst& c, const DevState& s, const cs_rollout_io& io, const LqrArgs& l, hipStream_t stream) {
  CS_GYRO_LAUNCH(rollout_lqr_kernel, io, l);
}

template <int TASK, int MODE>
hipError_t feedback_t(const DevConst& c, const DevState& s, const cs_rollout_io& io, const cs_rollout_feedback_io& f,
                      hipStream_t stream) {
  hipLaunchKernelGGL((rollout_feedback_kernel<TASK, MODE>), dim3(grid_for(s.n)), dim3(kBlock), 0, stream, c, s, io, f);
  return hipGetLastError();
}

hipError_t launch_rollout_lqr(int task, int mode, const DevConst& c, const DevState& s, const cs_rollout_io& io,
                              const LqrArgs& l, hipStream_t stream) {
  CS_DISPATCH(lqr_t, c, s, io, l, stream)
}

hipError_t launch_rollout_feedback(int task, int mode, const DevConst& c, const DevState& s, const cs_rollout_io& io,
                                   const cs_rollout_feedback_io& f, hipStream_t stream) {
  CS_DISPATCH(feedback_t, c, s, io, f, stream)
}

}  // namespace
}  // namespace cs

extern "C" int cs_rollout_lqr(cs_ctx* ctx, const cs_rollout_io* io, const cs_rollout_lqr_io* lio, void* stream) {
  const char* who = "cs_rollout_lqr";
  if (int rc_ = cs::check_rollout_io(io, who, true)) return rc_;
  if (lio == nullptr) return cs::report_error(CS_ERR_ARG, "cs_rollout_lqr: null lio");
  if (lio->struct_size != sizeof(cs_rollout_lqr_io))
    return cs::report_error(CS_ERR_ABI, ("cs_rollout_lqr: lio->struct_size " + std::to_string(lio->struct_size) +
                                         " != " + std::to_string(sizeof(cs_rollout_lqr_io)) +
                                         " (sizeof(cs_rollout_lqr_io))").c_str());
  if (lio->out_dtype != CS_JAC_F64 && lio->out_dtype != CS_JAC_F32)
    return cs::report_error(CS_ERR_ARG, "cs_rollout_lqr: unknown lio->out_dtype (CS_JAC_F64 or CS_JAC_F32)");
  if (lio->Q_dev == nullptr || lio->R_dev == nullptr)
    return cs::report_error(CS_ERR_ARG, "cs_rollout_lqr: Q_dev and R_dev are required");
  if (!(lio->mu >= 0.0) || !std::isfinite(lio->mu))
    return cs::report_error(CS_ERR_ARG, "cs_rollout_lqr: mu must be finite and >= 0");
  cs::ContextView v;
  if (int rc_ = cs::enter_context(ctx, who, stream, &v)) return rc_;
  const cs::LqrArgs l{lio->q_dev, lio->r_dev, lio->Q_dev, lio->Q_final_dev != nullptr ? lio->Q_final_dev : lio->Q_dev,
                      lio->R_dev, lio->mu, lio->K_dev, lio->d_dev, lio->dV_dev, lio->S0_dev, lio->s0_dev, lio->ok_dev,
                      lio->out_dtype == CS_JAC_F32 ? 1u : 0u};
  const hipError_t e = cs::launch_rollout_lqr(v.task, v.mode, *v.c, *v.s, *io, l, (hipStream_t)stream);
  if (e != hipSuccess) return cs::report_hip(e, "cs_rollout_lqr: kernel launch");
  return CS_OK;
}

extern "C" int cs_rollout_feedback_states(cs_ctx* ctx, const cs_rollout_io* io, const cs_rollout_feedback_io* fio,
                                          void* stream) {
  const char* who = "cs_rollout_feedback_states";
  if (int rc_ = cs::check_rollout_io(io, who, false)) return rc_;
  if (fio == nullptr) return cs::report_error(CS_ERR_ARG, "cs_rollout_feedback_states: null fio");
  if (fio->struct_size != sizeof(cs_rollout_feedback_io))
    return cs::report_error(CS_ERR_ABI,
                            ("cs_rollout_feedback_states: fio->struct_size " + std::to_string(fio->struct_size) +
                             " != " + std::to_string(sizeof(cs_rollout_feedback_io)) +
                             " (sizeof(cs_rollout_feedback_io))").c_str());
  if (fio->K_dev == nullptr || fio->d_dev == nullptr || fio->alpha_dev == nullptr || fio->actions_out_dev == nullptr)
    return cs::report_error(CS_ERR_ARG,
                            "cs_rollout_feedback_states: K_dev, d_dev, alpha_dev and actions_out_dev are required");
  if (fio->xbar_dev == nullptr && io->num_steps > 1)
    return cs::report_error(CS_ERR_ARG, "cs_rollout_feedback_states: xbar_dev (the nominal tape) is required for K > 1");
  cs::ContextView v;
  if (int rc_ = cs::enter_context(ctx, who, stream, &v)) return rc_;
  const hipError_t e = cs::launch_rollout_feedback(v.task, v.mode, *v.c, *v.s, *io, *fio, (hipStream_t)stream);
  if (e != hipSuccess) return cs::report_hip(e, "cs_rollout_feedback_states: kernel launch");
  return CS_OK;
}
