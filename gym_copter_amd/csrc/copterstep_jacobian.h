// Internal declarations between the C-ABI layer (copterstep_api.hip: contexts, error reporting) and
// copterstep_jacobian.hip (cs_step_jacobian and its kernels).  Not installed; the public ABI is include/copterstep.h.
#pragma once

#include <initializer_list>

#include "copterstep_internal.h"

namespace cs {

// what an entry point launches on: the context's task, storage mode, constants and device state
struct ContextView {
  int task, mode;
  const DevConst* c;
  const DevState* s;
};
// (copterstep_api.hip) check the context as every entry point does (null, served session, draining) and describe it
int enter_context(cs_ctx* ctx, const char* who, void* stream, ContextView* out);
// (copterstep_api.hip) set cs_last_error() and return `code` / CS_ERR_HIP
int report_error(int code, const char* message);
int report_hip(hipError_t e, const char* what);
// (copterstep_api.hip) the context's 64-bit seed (cs_seed): the MPPI noise key is a mix of it (mppi_noise.h)
uint64_t context_seed(const cs_ctx* ctx);

// (copterstep_rollout_grad.hip) the cs_rollout_io checks of cs_rollout_states / cs_rollout_vjp (vjp: the backward's),
// made before the context; also those of cs_rollout_mlp_* (copterstep_rollout_mlp.hip)
int check_rollout_io(const cs_rollout_io* io, const char* who, bool vjp);

// (copterstep_rollout_grad.hip) what cs_rollout_ekf, cs_rollout_rts and cs_rollout_pf check alike, in two calls because
// their own checks stand between.  Their second block opens with uint32_t struct_size, out_dtype.
struct FilterExt {
  const char* name;   // the argument's name ("eio") and its type's, as the messages spell them
  const char* type;
  const void* block;
  size_t size;        // sizeof the type
};
// After check_rollout_io: the block is there and of its size; `start_missing` (the entry point's text if a start pointer
// it requires is NULL, else nullptr); no start force or shaping; `must_be_null` (its text if a pointer of io it forbids
// is set, else nullptr); out_dtype is known.
int check_filter_io(const cs_rollout_io* io, const char* who, const FilterExt& ext, const char* start_missing,
                    const char* must_be_null);
// The model checks of cs_rollout_ekf, cs_rollout_ukf and cs_rollout_lqg, in the order they always made them: num_meas
// is 1 .. CS_EKF_MAX_MEAS; `own_failed` (the entry point's text if a check of its own that stands here fails, else
// nullptr); none of `required` (`required_names` in the message) is NULL.
int check_filter_model(const char* who, int32_t num_meas, const char* own_failed,
                       std::initializer_list<const void*> required, const char* required_names);
// After the entry point's own checks: the float64 arrays are 8-B aligned, the out_dtype arrays to their element, the
// 32-bit ones (`w32_names` in the message) to 4 B; then enter_context, and the float32 motor law is refused.
int enter_filter_context(cs_ctx* ctx, const char* who, void* stream, uint32_t out_dtype,
                         std::initializer_list<const void*> f64s, std::initializer_list<const void*> outs,
                         std::initializer_list<const void*> w32s, const char* w32_names, ContextView* out);

constexpr int kVehicleRows = 12;  // cs_set_vehicle_params' raw rows: B, D, M, L, Ix, Iy, Iz, Jr, maxrpm, G, rho, C_L

// what cs_rollout_states_ex / cs_rollout_vjp_ex need beyond ContextView: the configuration's motor
// law, the vehicle's raw parameters and the context's scratch tables
struct ParamView {
  int lift, gyro;
  uint32_t n, stride;                 // envs, the padded stride of DevState::veh
  double uniform_raw[kVehicleRows];   // cs_config's vehicle and world, in cs_set_vehicle_params' row order
  const double* raw_dev;              // [kVehicleRows][n] the installed per-env table, nullptr = uniform
  double* coef_dev;                   // [kCoefRows][stride] an override's folded columns (allocated on first use)
  double* gcoef_dev;                  // [kCoefRows][n] the coefficient adjoints (allocated on first use)
};
// (copterstep_api.hip) refuse the float32 motor law and describe the context; allocates the scratch tables asked for
// (outside stream order: the first call with an override or a parameter gradient allocates)
int param_view(cs_ctx* ctx, const char* who, bool want_coef, bool want_gcoef, ParamView* out);

// (copterstep_rollout_grad.hip) the DevState a call with a vehicle override launches on: `vehicle_dev` [12, n] folded
// into pv.coef_dev on `stream` (nullptr: *out = s0), as cs_rollout_states_ex folds it
int override_vehicle(const ParamView& pv, const double* vehicle_dev, const DevState& s0, hipStream_t stream,
                     const char* who, DevState* out);

// (copterstep_api.hip) a context's scratch of workgroup partials, one buffer per user: cs_mlp_param_grad
// (copterstep_mlp_grad.hip), cs_es_gradient (copterstep_rollout_es.hip) and cs_ppo_grad (copterstep_ppo_grad.hip).
// `bytes` is what the first call allocates (refused while `stream` is being captured) and cs_destroy releases; every
// call of a user asks for the same `bytes`, its largest case's partials.
enum GradScratch { kScratchMlpGrad, kScratchEsGrad, kScratchPpoGrad };
int grad_scratch(cs_ctx* ctx, GradScratch slot, const char* who, void* stream, size_t bytes, double** out);

// (copterstep_api.hip) the hidden width `value` of the MLP argument blocks' field `field` is in [0, CS_MLP_MAX_HIDDEN]
int check_hidden(const char* who, const char* field, int value);

}  // namespace cs
