// mlp_policy.h -- the MLP policy of the closed-loop kernels in one place: theta's layout and parameter count, the
// scalar-unit weight load, the float32 forward of cs_rollout_mlp_states, cs_rollout_actor_critic and
// cs_rollout_mlp_population (copterstep_rollout_mlp.hip, copterstep_rollout_ac.hip, copterstep_rollout_es.hip -- one
// definition, so those three agree bit for bit by construction), the float64 vector-Jacobian product of the closed-loop
// backward, and the fan-out of an action onto the four motors.  The layout and the count also serve the parameter
// reductions (mlp_grad_kit.h).  Included inside a translation unit's floating-point-contraction pragma, after
// copterstep_jacobian.h; not a stand-alone header.  It is no dev_*.h: those are the step kernels' sources, whose hash
// stamps the committed profiles.  DESIGN.md sections 12, 16 and 17.
#pragma once

namespace cs {
namespace {

// theta = [W1 (H x OBS), b1 (H), W2 (A x H), b2 (A)], or [W (A x OBS), b (A)] for the linear policy H = 0
// (include/copterstep.h): where b1, W2 and b2 begin; W1[h][j] is at h OBS + j, W2[c][h] at w2 + c H + h
struct MlpLayout {
  int b1, w2, b2;
};
__host__ __device__ constexpr MlpLayout mlp_layout(int OBS, int A, int H) {
  return {H * OBS, H * OBS + H, H * OBS + H + A * H};
}
// the length of theta
__host__ __device__ constexpr uint32_t mlp_param_count(int OBS, int A, int H) {
  return (uint32_t)(H == 0 ? A * (OBS + 1) : H * (OBS + 1) + A * (H + 1));
}
// the widest policy (Hover3D, H = 64: 1 092) and the widest value function
constexpr uint32_t kMlpMaxParams = mlp_param_count(12, 4, CS_MLP_MAX_HIDDEN);
constexpr uint32_t kMlpMaxValueParams = mlp_param_count(12, 1, CS_MLP_MAX_HIDDEN);

// A weight: the address is wave-uniform (one theta per launch, or a population member's row of the table, which is a
// function of blockIdx alone), and the constant address space lets the compiler fetch it with a scalar load (the
// parameters are never written by these kernels).  Staging a member's row in the LDS instead was measured and lost
// (DESIGN.md section 16).
typedef __attribute__((address_space(4))) const float ConstF32;
__device__ __forceinline__ float weight(const float* p, int idx) { return ((ConstF32*)p)[idx]; }

// pi_theta(o) in float32, the arithmetic include/copterstep.h documents: every sum an fmaf chain that starts from the
// bias and adds the terms in index order; tanhf the device library's.  Streams over the hidden units (pre_j -> h_j ->
// a[0..A) += W2[., j] h_j), so a lane holds O(OBS + A) policy values whatever the width.
template <int OBS, int A>
__device__ __forceinline__ void mlp_forward(const float* P, int H, const float (&o)[OBS], float (&a)[A]) {
  if (H == 0) {  // [W (A x OBS), b (A)]
#pragma unroll
    for (int c = 0; c < A; ++c) {
      float s = weight(P, A * OBS + c);
#pragma unroll
      for (int j = 0; j < OBS; ++j) s = fmaf(weight(P, c * OBS + j), o[j], s);
      a[c] = s;
    }
    return;
  }
  const MlpLayout at = mlp_layout(OBS, A, H);
#pragma unroll
  for (int c = 0; c < A; ++c) a[c] = weight(P, at.b2 + c);
#pragma clang loop unroll(disable)
  for (int h = 0; h < H; ++h) {
    float pre = weight(P, at.b1 + h);
#pragma unroll
    for (int j = 0; j < OBS; ++j) pre = fmaf(weight(P, h * OBS + j), o[j], pre);
    const float t = tanhf(pre);
#pragma unroll
    for (int c = 0; c < A; ++c) a[c] = fmaf(weight(P, at.w2 + c * H + h), t, a[c]);
  }
}

// lam[FIRST + j] += (J_o pi(o)^T ga)_j in float64: o = the float32 observation of x (its rounding straight-through), the
// hidden units recomputed in float64 (tanh' = 1 - h^2).  Streams over the hidden units as mlp_forward does.
template <int TASK>
__device__ __forceinline__ void mlp_vjp(const float* P, int H, const double (&x)[12], const double (&ga)[4],
                                        double (&lam)[12]) {
  constexpr int OBS = task_obs_dim(TASK), FIRST = task_obs_first(TASK), A = task_act_dim(TASK);
  double o[OBS];
#pragma unroll
  for (int j = 0; j < OBS; ++j) o[j] = (double)(float)x[FIRST + j];
  if (H == 0) {
#pragma unroll
    for (int c = 0; c < A; ++c) {
#pragma unroll
      for (int j = 0; j < OBS; ++j) lam[FIRST + j] = fma((double)weight(P, c * OBS + j), ga[c], lam[FIRST + j]);
    }
    return;
  }
  const MlpLayout at = mlp_layout(OBS, A, H);
#pragma clang loop unroll(disable)
  for (int h = 0; h < H; ++h) {
    double pre = (double)weight(P, at.b1 + h);
#pragma unroll
    for (int j = 0; j < OBS; ++j) pre = fma((double)weight(P, h * OBS + j), o[j], pre);
    const double t = tanh(pre);
    double gh = 0.0;
#pragma unroll
    for (int c = 0; c < A; ++c) gh = fma((double)weight(P, at.w2 + c * H + h), ga[c], gh);
    const double gp = gh * (1.0 - t * t);
#pragma unroll
    for (int j = 0; j < OBS; ++j) lam[FIRST + j] = fma(gp, (double)weight(P, h * OBS + j), lam[FIRST + j]);
  }
}

// the action as the step takes it (load_action_at's fan-out of the task's A columns onto the four motors)
template <int A>
__device__ __forceinline__ float4 motors_of(const float (&a)[A]) {
  if constexpr (A == 4) return make_float4(a[0], a[1], a[2], a[3]);
  else if constexpr (A == 2) return make_float4(a[0], a[1], a[1], a[0]);
  else return make_float4(a[0], a[0], a[0], a[0]);
}

}  // namespace
}  // namespace cs
