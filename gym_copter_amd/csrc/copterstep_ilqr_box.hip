// copterstep_ilqr_box.hip -- control-limited iLQR on gfx950 (cs_ilqr_box_backward / cs_ilqr_box_forward,
// include/copterstep.h): the Riccati sweep of cs_rollout_lqr with the A x A solve of each step replaced by a
// box-constrained quadratic programme over lo <= abar + d <= hi (boxqp_solve.h: projected Newton, in registers), and the
// feedback forward of cs_rollout_feedback_states with the rounded action clamped into the same box.  Nothing of the env
// state is written.  DESIGN.md section 24.
//
// Upstream lines differentiated: those of copterstep_rollout_grad.hip (setMotors, the state derivative, step).
//
// The sweep, its LDS rows and its stores are lqr_step.h's, the feedback law lqr_feedback.h's: this translation unit
// instantiates them with the box policies, beside copterstep_rollout_lqr.hip's instantiations and not behind them.  The
// programme's iteration count differs from lane to lane: it runs between the sweep's synchronisation points, touches
// no LDS, and every loop of it has a compile-time trip bound (16 iterations of at most 30 trials).
#include <cmath>
#include <string>

#include "copterstep_jacobian.h"

// the primal must round as the step kernels do: the recomputed primal is the tape bit for bit, and the arithmetic of the
// programme and of the feedback law is fixed (one multiply and one add per term, no fma)
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
#include "boxqp_solve.h"
#include "cov_tile.h"
#include "lqr_step.h"
#include "lqr_feedback.h"
#include "dev_launch.h"

namespace cs {
namespace {

// what the launch carries of cs_ilqr_box_io: the same four pointers whatever A is
struct BoxArgs {
  const float* lo;
  const float* hi;
  uint8_t* clamped;
  uint8_t* iters;
};

template <int TASK, int MODE, bool GYRO>
__global__ __launch_bounds__(kBlock) void ilqr_box_backward_kernel(const DevConst c, const DevState s,
                                                                   const cs_rollout_io io, const LqrArgs l,
                                                                   const BoxArgs b) {
  constexpr int A = task_act_dim(TASK);
  __shared__ __attribute__((aligned(16))) double lds[lqr_rows(A) * kBlock];
  lqr_sweep<TASK, MODE, GYRO, LqrBoxSolve>(c, s, io, l, typename LqrBoxSolve<A>::Args{b.lo, b.hi, b.clamped, b.iters},
                                           lds);
}

template <int TASK, int MODE>
__global__ __launch_bounds__(kBlock) void ilqr_box_forward_kernel(const DevConst c, const DevState s,
                                                                  const cs_rollout_io io,
                                                                  const cs_rollout_feedback_io f, const BoxArgs b) {
  __shared__ __attribute__((aligned(16))) double xrow[kBlock * 12];  // 6 KiB: the wavefront's state rows of a step
  rollout_forward<TASK, MODE>(c, s, io, xrow,
                              FeedbackLaw<TASK, FeedbackBoxClamp>{io.actions_dev, f.xbar_dev, f.K_dev, f.d_dev,
                                                                  f.alpha_dev, f.actions_out_dev,
                                                                  FeedbackBoxClamp{b.lo, b.hi, b.clamped}, 0u, 0u, 0.0});
}

template <int TASK, int MODE>
hipError_t box_backward_t(const DevConst& c, const DevState& s, const cs_rollout_io& io, const LqrArgs& l,
                          const BoxArgs& b, hipStream_t stream) {
  CS_GYRO_LAUNCH(ilqr_box_backward_kernel, io, l, b);
}

template <int TASK, int MODE>
hipError_t box_forward_t(const DevConst& c, const DevState& s, const cs_rollout_io& io,
                         const cs_rollout_feedback_io& f, const BoxArgs& b, hipStream_t stream) {
  hipLaunchKernelGGL((ilqr_box_forward_kernel<TASK, MODE>), dim3(grid_for(s.n)), dim3(kBlock), 0, stream, c, s, io, f,
                     b);
  return hipGetLastError();
}

hipError_t launch_box_backward(int task, int mode, const DevConst& c, const DevState& s, const cs_rollout_io& io,
                               const LqrArgs& l, const BoxArgs& b, hipStream_t stream) {
  CS_DISPATCH(box_backward_t, c, s, io, l, b, stream)
}

hipError_t launch_box_forward(int task, int mode, const DevConst& c, const DevState& s, const cs_rollout_io& io,
                              const cs_rollout_feedback_io& f, const BoxArgs& b, hipStream_t stream) {
  CS_DISPATCH(box_forward_t, c, s, io, f, b, stream)
}

// the checks of cs_ilqr_box_io that need no context
int check_box_io(const cs_ilqr_box_io* bio, const std::string& who, bool forward) {
  if (bio == nullptr) return report_error(CS_ERR_ARG, (who + ": null bio").c_str());
  if (bio->struct_size != sizeof(cs_ilqr_box_io))
    return report_error(CS_ERR_ABI, (who + ": bio->struct_size " + std::to_string(bio->struct_size) +
                                     " != " + std::to_string(sizeof(cs_ilqr_box_io)) + " (sizeof(cs_ilqr_box_io))").c_str());
  if (bio->reserved_ != 0) return report_error(CS_ERR_ARG, (who + ": bio->reserved_ must be 0").c_str());
  if (bio->lo_dev == nullptr || bio->hi_dev == nullptr)
    return report_error(CS_ERR_ARG, (who + ": lo_dev and hi_dev are required").c_str());
  if (forward && bio->iters_dev != nullptr)
    return report_error(CS_ERR_ARG, (who + ": iters_dev is the backward pass's output and must be NULL here").c_str());
  return CS_OK;
}

}  // namespace
}  // namespace cs

extern "C" int cs_ilqr_box_backward(cs_ctx* ctx, const cs_rollout_io* io, const cs_rollout_lqr_io* lio,
                                    const cs_ilqr_box_io* bio, void* stream) {
  const char* who = "cs_ilqr_box_backward";
  if (int rc_ = cs::check_rollout_io(io, who, true)) return rc_;
  if (lio == nullptr) return cs::report_error(CS_ERR_ARG, "cs_ilqr_box_backward: null lio");
  if (lio->struct_size != sizeof(cs_rollout_lqr_io))
    return cs::report_error(CS_ERR_ABI, ("cs_ilqr_box_backward: lio->struct_size " + std::to_string(lio->struct_size) +
                                         " != " + std::to_string(sizeof(cs_rollout_lqr_io)) +
                                         " (sizeof(cs_rollout_lqr_io))").c_str());
  if (lio->out_dtype != CS_JAC_F64 && lio->out_dtype != CS_JAC_F32)
    return cs::report_error(CS_ERR_ARG, "cs_ilqr_box_backward: unknown lio->out_dtype (CS_JAC_F64 or CS_JAC_F32)");
  if (lio->Q_dev == nullptr || lio->R_dev == nullptr)
    return cs::report_error(CS_ERR_ARG, "cs_ilqr_box_backward: Q_dev and R_dev are required");
  if (!(lio->mu >= 0.0) || !std::isfinite(lio->mu))
    return cs::report_error(CS_ERR_ARG, "cs_ilqr_box_backward: mu must be finite and >= 0");
  if (int rc_ = cs::check_box_io(bio, who, false)) return rc_;
  cs::ContextView v;
  if (int rc_ = cs::enter_context(ctx, who, stream, &v)) return rc_;
  const cs::LqrArgs l{lio->q_dev, lio->r_dev, lio->Q_dev, lio->Q_final_dev != nullptr ? lio->Q_final_dev : lio->Q_dev,
                      lio->R_dev, lio->mu, lio->K_dev, lio->d_dev, lio->dV_dev, lio->S0_dev, lio->s0_dev, lio->ok_dev,
                      lio->out_dtype == CS_JAC_F32 ? 1u : 0u};
  const cs::BoxArgs b{bio->lo_dev, bio->hi_dev, bio->clamped_dev, bio->iters_dev};
  const hipError_t e = cs::launch_box_backward(v.task, v.mode, *v.c, *v.s, *io, l, b, (hipStream_t)stream);
  if (e != hipSuccess) return cs::report_hip(e, "cs_ilqr_box_backward: kernel launch");
  return CS_OK;
}

extern "C" int cs_ilqr_box_forward(cs_ctx* ctx, const cs_rollout_io* io, const cs_rollout_feedback_io* fio,
                                   const cs_ilqr_box_io* bio, void* stream) {
  const char* who = "cs_ilqr_box_forward";
  if (int rc_ = cs::check_rollout_io(io, who, false)) return rc_;
  if (fio == nullptr) return cs::report_error(CS_ERR_ARG, "cs_ilqr_box_forward: null fio");
  if (fio->struct_size != sizeof(cs_rollout_feedback_io))
    return cs::report_error(CS_ERR_ABI, ("cs_ilqr_box_forward: fio->struct_size " + std::to_string(fio->struct_size) +
                                         " != " + std::to_string(sizeof(cs_rollout_feedback_io)) +
                                         " (sizeof(cs_rollout_feedback_io))").c_str());
  if (fio->K_dev == nullptr || fio->d_dev == nullptr || fio->alpha_dev == nullptr || fio->actions_out_dev == nullptr)
    return cs::report_error(CS_ERR_ARG, "cs_ilqr_box_forward: K_dev, d_dev, alpha_dev and actions_out_dev are required");
  if (fio->xbar_dev == nullptr && io->num_steps > 1)
    return cs::report_error(CS_ERR_ARG, "cs_ilqr_box_forward: xbar_dev (the nominal tape) is required for K > 1");
  if (int rc_ = cs::check_box_io(bio, who, true)) return rc_;
  cs::ContextView v;
  if (int rc_ = cs::enter_context(ctx, who, stream, &v)) return rc_;
  const cs::BoxArgs b{bio->lo_dev, bio->hi_dev, bio->clamped_dev, nullptr};
  const hipError_t e = cs::launch_box_forward(v.task, v.mode, *v.c, *v.s, *io, *fio, b, (hipStream_t)stream);
  if (e != hipSuccess) return cs::report_hip(e, "cs_ilqr_box_forward: kernel launch");
  return CS_OK;
}
