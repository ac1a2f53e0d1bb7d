// lqr_feedback.h -- the action source of the iLQR forward passes (cs_rollout_feedback_states, copterstep_rollout_lqr.hip,
// and cs_ilqr_box_forward, copterstep_ilqr_box.hip): the time-varying affine feedback law in fixed float64 arithmetic,
// rounded once to float32, then the CLAMP policy -- none, or the box of the control-limited forward.  Device code of
// those two translation units (included there, inside their floating-point-contraction pragma, after rollout_sweep.h);
// not a stand-alone header.  DESIGN.md sections 13 and 24.
#pragma once

namespace cs {
namespace {

// no clamp (cs_rollout_feedback_states)
struct FeedbackNoClamp {
  template <int A>
  __device__ __forceinline__ void apply(float (&)[A], size_t, bool) const {}
};

// a = a < lo ? lo : (a > hi ? hi : a) in float32 (a NaN stays a NaN), and the optional flag byte of the step and env at
// `row` = step index x N + env: bit c = action c raised to its lower bound, bit 4 + c = lowered to its upper
struct FeedbackBoxClamp {
  const float* lo;
  const float* hi;
  uint8_t* flags;
  template <int A>
  __device__ __forceinline__ void apply(float (&a)[A], size_t row, bool valid) const {
    unsigned bits = 0u;
#pragma unroll
    for (int c = 0; c < A; ++c) {
      const float l = lo[c], h = hi[c], v = a[c];
      if (v < l) bits |= 1u << c;
      else if (v > h) bits |= 16u << c;
      a[c] = v < l ? l : (v > h ? h : v);
    }
    if (valid && flags != nullptr) flags[row] = (uint8_t)bits;
  }
};

// rollout_forward's action source: a_k = clamp(fl32(abar_k + alpha d_k + K_k (x - xbar_{k-1}))), stored to the action tape
template <int TASK, class CLAMP>
struct FeedbackLaw {
  const float* abar;
  const double* xbar;
  const double* K;
  const double* d;
  const double* alpha;
  float* out;
  CLAMP clamp;
  uint32_t i, n;
  double al;
  __device__ __forceinline__ void begin(uint32_t env, uint32_t envs) {
    i = env;
    n = envs;
    al = alpha[env];
  }
  __device__ __forceinline__ float4 next(const double (&x)[12], size_t row, const RowOut& r) {
    constexpr int A = task_act_dim(TASK);
    const size_t at = (row + i) * A;
    double t[A];
#pragma unroll
    for (int c = 0; c < A; ++c) t[c] = (double)abar[at + c] + al * d[at + c];
    if (row != 0) {  // (step 1's deviation is zero: x0 is the nominal's start)
      const double2* xb = reinterpret_cast<const double2*>(xbar + (row - n + i) * 12);
      double dx[12];
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        const double2 v = xb[j];
        dx[2 * j] = x[2 * j] - v.x;
        dx[2 * j + 1] = x[2 * j + 1] - v.y;
      }
#pragma unroll
      for (int c = 0; c < A; ++c) {
        const double2* kr = reinterpret_cast<const double2*>(K + (at + c) * 12);
#pragma unroll
        for (int j = 0; j < 6; ++j) {
          const double2 v = kr[j];
          t[c] += v.x * dx[2 * j];
          t[c] += v.y * dx[2 * j + 1];
        }
      }
    }
    float a[A];
#pragma unroll
    for (int c = 0; c < A; ++c) a[c] = (float)t[c];
    clamp.template apply<A>(a, row + i, r.valid);
    if (r.valid) {
#pragma unroll
      for (int c = 0; c < A; ++c) out[at + c] = a[c];
    }
    if constexpr (A == 4)  // the task's motor fan-out, as load_action_at()
      return make_float4(a[0], a[1], a[2], a[3]);
    else if constexpr (A == 2)
      return make_float4(a[0], a[1], a[1], a[0]);
    else
      return make_float4(a[0], a[0], a[0], a[0]);
  }
};

}  // namespace
}  // namespace cs
