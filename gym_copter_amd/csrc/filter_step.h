// filter_step.h -- the filter step that copterstep_rollout_ekf.hip, copterstep_rollout_lqg.hip and
// copterstep_rollout_ukf.hip share: the start (mean, status, P0), the extended filter's predict (ekf and lqg), the M
// sequential scalar updates, and the tapes of a row with the closing stores.  LQG's filter is the EKF's, and the UKF's
// update and tapes are the EKF's, because they are these functions of the same arguments.  All of it works on the
// lane-private LDS columns of cov_tile.h (element j of a lane at [j * kBlock]).  Device code of those translation units
// (included there, inside their floating-point-contraction pragma, after cov_tile.h); not a stand-alone header, and no
// dev_*.h (cov_tile.h says why).  DESIGN.md section 19.
#pragma once

#include "cov_tile.h"

namespace cs {
namespace {

// the outputs the three filters have in common, whatever their io blocks call them (any may be NULL)
struct FilterTapes {
  double* x;        // [K,N,12] the posterior means
  double* x_pred;   // [K,N,12] the priors
  void* P;          // [N,12,12] the last posterior
  void* P_tape;     // [K,N,12,12]
  void* var;        // [K,N,12]
  void* nis;        // [K,N]
  void* loglik;     // [N]
  uint8_t* status;  // [K,N] of the filter's own mean
  uint8_t* aux;     // [K,N] the step's byte: the EKF's branch bits, the UKF's spread
  uint8_t* ok;      // [N]
  uint32_t f32;     // P, P_tape, var, nis and loglik are float32
};
#define CS_FILTER_TAPES(X, B, STATUS, AUX)                                                                    \
  FilterTapes {                                                                                               \
    X, B.x_pred_dev, B.P_dev, B.P_tape_dev, B.var_dev, B.nis_dev, B.loglik_dev, STATUS, B.AUX, B.ok_dev,      \
        B.out_dtype == CS_JAC_F32 ? 1u : 0u                                                                   \
  }
__device__ __forceinline__ FilterTapes filter_tapes(const cs_rollout_io& io, const cs_rollout_ekf_io& e) {
  return CS_FILTER_TAPES(io.x_dev, e, io.status_dev, branch_dev);
}
__device__ __forceinline__ FilterTapes filter_tapes(const cs_rollout_io&, const cs_rollout_lqg_io& g) {
  return CS_FILTER_TAPES(g.xhat_dev, g, g.fstatus_dev, branch_dev);
}
__device__ __forceinline__ FilterTapes filter_tapes(const cs_rollout_io& io, const cs_rollout_ukf_io& u) {
  return CS_FILTER_TAPES(io.x_dev, u, io.status_dev, spread_dev);
}
#undef CS_FILTER_TAPES

// The caller's filter state of env ii: xhat_0 from x0_dev [12,N] into X, the upper triangle of P0_dev [N,12,12] into the
// packed triangle P; returns the status of the mean.  (The triangle's loops are rolled: this runs once a launch;
// load_triangle's unrolling is a speed decision of the smoother's, which loads a triangle every step.)
__device__ __forceinline__ int filter_load_start(double* X, double* P, const double* x0_dev, const uint8_t* status0_dev,
                                                 const double* P0_dev, uint32_t n, uint32_t ii) {
#pragma unroll
  for (int j = 0; j < 12; ++j) X[j * kBlock] = x0_dev[(size_t)j * n + ii];
  const int fs = (int)status0_dev[ii];
  const double* p0 = P0_dev + (size_t)ii * 144;
#pragma clang loop unroll(disable)
  for (int j = 0; j < 12; ++j) {
#pragma clang loop unroll(disable)
    for (int a = 0; a <= j; ++a) P[(j * (j + 1) / 2 + a) * kBlock] = p0[a * 12 + j];
  }
  return fs;
}

// The prior mean out through the stage.  What lived in the stage's rows (W; the UKF's factor and moment sum) is dead by
// now: the sync puts the wavefront's last accesses to it before the staging writes.
__device__ __forceinline__ void filter_store_prior(const double* X, double* stage, double* x_pred_dev, size_t row,
                                                   const RowOut& ro) {
  double x[12];
#pragma unroll
  for (int j = 0; j < 12; ++j) x[j] = X[j * kBlock];
  wave_sync();
  if (x_pred_dev != nullptr) store_x_row(stage, x_pred_dev, row, ro, x);
}

// The extended filter's predict under the action `act`: the mean X through rollout_step's physics from (xhat, fs) with
// no storage rounding (fs becomes the status after the step; xhat is kept in X0 as the Jacobian's point), P- = A P A^T +
// Q at that point (cov_predict), and the prior mean out through the stage (W is dead by then: its rows are the stage).
// Returns step_jacobian's branch bits of the step.
template <bool FULL, bool GYRO>
__device__ __forceinline__ uint32_t ekf_predict(const DevConst& c, const Coef& q, const float4& act, int& fs, double* X,
                                                double* X0, double* P, double* W, const double* Q_dev, double* stage,
                                                double* x_pred_dev, size_t row, const RowOut& ro) {
  bool clipped;
  const Wrench w = step_wrench(q, act, &clipped);
  const int fs0 = fs;
  uint32_t bits = (fs0 == CS_STATUS_LANDED ? (uint32_t)kJacLanded : 0u) | (clipped ? (uint32_t)kJacClipped : 0u);
  double x[12];
#pragma unroll
  for (int j = 0; j < 12; ++j) {
    x[j] = X[j * kBlock];
    X0[j * kBlock] = x[j];
  }
  if (fs0 != CS_STATUS_LANDED) {
    bool pend = false;
    physics_substeps<FULL, GYRO, false, true>(c, q, w, x, fs, pend, -0.0, -0.0, -0.0);
  }
#pragma unroll
  for (int j = 0; j < 12; ++j) X[j * kBlock] = x[j];
  bits |= cov_predict<FULL, GYRO>(c, q, w, fs0, X0, kBlock, P, W, Q_dev);
  filter_store_prior(X, stage, x_pred_dev, row, ro);
  return bits;
}

// The step's update: M scalar measurements in order (ekf_update.h), measurement m from z_of(m) -- a tape's entry, or
// one formed on the spot.  st.nis restarts; st.loglik and st.ok go on.
template <class Z>
__device__ __forceinline__ void filter_update(double* X, double* P, const double* H_dev, const double* r_dev, int M,
                                              EkfStats& st, Z&& z_of) {
  st.nis = 0.0;
#pragma clang loop unroll(disable)
  for (int m = 0; m < M; ++m) {
    const double z = z_of(m);
    ekf_scalar_update(X, P, kBlock, H_dev + m * 12, r_dev[m], z, st);
  }
}

// The tapes of row k (`row` = k * N): the posterior mean, P (to P_tape, and to t.P on the last step) through the stage,
// its diagonal, the step's nis, the status of the mean and the step's byte.
// The trailing wave_sync() is the write-after-read side of the stage: the lanes' reads of their neighbours' staged
// values come before it, the next step's writes into those rows (LDS columns of the lanes again) after it.
// STAGE_ALWAYS_REUSED = false (ekf, lqg): the sync follows the matrix stores only, inside their branch -- the next step's
// x row and W are written over the stage.  true (ukf): its next step's factor and moment sum overwrite the stage even
// when no matrix was stored, so the sync is unconditional.  Each kernel's sequence of syncs is what it always was; an LDS
// hazard cannot be tested for on purpose, so do not merge the two.
template <bool STAGE_ALWAYS_REUSED>
__device__ __forceinline__ void filter_store_row(const FilterTapes& t, double* stage, const double* X, const double* P,
                                                 size_t row, const RowOut& ro, bool last, int fs, uint32_t aux,
                                                 double nis) {
  {
    double x[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) x[j] = X[j * kBlock];
    if (t.x != nullptr) store_x_row(stage, t.x, row, ro, x);
  }
  if (t.P_tape != nullptr || (last && t.P != nullptr)) {
    stage_triangle(stage + ro.lane * kStageStride, P);
    wave_sync();
    if (t.P_tape != nullptr) store_matrix(t.P_tape, row, stage, ro, t.f32);
    if (last && t.P != nullptr) store_matrix(t.P, 0, stage, ro, t.f32);
    if constexpr (!STAGE_ALWAYS_REUSED) wave_sync();
  }
  if constexpr (STAGE_ALWAYS_REUSED) wave_sync();
  if (ro.valid) {
    if (t.var != nullptr) {
#pragma unroll
      for (int j = 0; j < 12; ++j) store_out(t.var, (row + ro.i) * 12 + j, P[(j * (j + 1) / 2 + j) * kBlock], t.f32);
    }
    if (t.nis != nullptr) store_out(t.nis, row + ro.i, nis, t.f32);
    if (t.status != nullptr) t.status[row + ro.i] = (uint8_t)fs;
    if (t.aux != nullptr) t.aux[row + ro.i] = (uint8_t)aux;
  }
}

// the closing stores of a launch
__device__ __forceinline__ void filter_store_end(const FilterTapes& t, const RowOut& ro, const EkfStats& st) {
  if (ro.valid) {
    if (t.loglik != nullptr) store_out(t.loglik, ro.i, st.loglik, t.f32);
    if (t.ok != nullptr) t.ok[ro.i] = st.ok ? 1 : 0;
  }
}

}  // namespace
}  // namespace cs
