// rollout_sweep.h -- the loops of the differentiable rollouts: the forward over K steps (rollout_forward:
// cs_rollout_states) and the one reverse sweep (rollout_vjp_sweep: cs_rollout_vjp, the parameter-gradient
// cs_rollout_vjp_ex and the closed-loop cs_rollout_mlp_vjp).  The kernels are wrappers that say where the forward's
// actions come from and what the sweep adds.  Device code of copterstep_rollout_grad.hip and
// copterstep_rollout_mlp.hip (included there, inside their floating-point-contraction pragma, after rollout_step.h); not
// a stand-alone header.  DESIGN.md sections 10 to 12.
#pragma once

namespace cs {
namespace {

// A lane's place in the [.., N, W] rows its wavefront writes: env i (valid: i < N), the wavefront's first env env0, and
// whether all 64 of the wavefront's envs exist (whole: its rows go out through the LDS)
struct RowOut {
  int lane;
  uint32_t i, env0;
  bool valid, whole;
};

// Row `row` of x_dev [.., N, 12]: a whole wavefront's 64 rows of 96 B through the LDS (xrow, 6 KiB), six 1 KiB stores of
// 16 B per lane; a partial one lane by lane.
__device__ __forceinline__ void store_x_row(double* xrow, double* x_dev, size_t row, const RowOut& r,
                                            const double (&x)[12]) {
  if (r.whole) {
#pragma unroll
    for (int j = 0; j < 12; j += 2)
      *reinterpret_cast<double2*>(xrow + r.lane * 12 + j) = make_double2(x[j], x[j + 1]);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const double2* src = reinterpret_cast<const double2*>(xrow);
    double2* dst = reinterpret_cast<double2*>(x_dev + (row + r.env0) * 12);
#pragma unroll
    for (int v = 0; v < 6; ++v) dst[v * kWave + r.lane] = src[v * kWave + r.lane];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  } else if (r.valid) {
    double* dst = x_dev + (row + r.i) * 12;
#pragma unroll
    for (int j = 0; j < 12; ++j) dst[j] = x[j];
  }
}

// The open-loop actions: the caller's [K, N, A] io.actions_dev, row k - 1 in step k
template <int TASK>
struct OpenLoop {
  const float* a;  // after begin(): the lane's action of the next step
  size_t step;
  __device__ __forceinline__ void begin(uint32_t i, uint32_t n) {
    a += (size_t)i * task_act_dim(TASK);
    step = (size_t)n * task_act_dim(TASK);
  }
  __device__ __forceinline__ float4 next(const double (&)[12], size_t, const RowOut&) {
    const float4 v = load_action_at<TASK>(a);
    a += step;
    return v;
  }
};

// K steps of rollout_step from the start point (the stored env, or io's explicit start), step k's outputs stored to row
// k - 1 of io's arrays.  The action of each step is act.next(x, row, r) at the state before it (ACT: OpenLoop; the
// closed-loop forward keeps its own loop, copterstep_rollout_mlp.hip), after act.begin(i, n) with the lane's env (env 0
// for padding lanes).  xrow: the kernel's 6 KiB of LDS for the x rows.
template <int TASK, int MODE, class ACT>
__device__ __forceinline__ void rollout_forward(const DevConst& c, const DevState& s, const cs_rollout_io& io,
                                                double* xrow, ACT act) {
  const int lane = threadIdx.x;
  const uint32_t tile_index = blockIdx.x;
  const uint32_t i = tile_index * kBlock + threadIdx.x;
  const uint32_t n = s.n;
  const uint32_t env0 = i - lane;
  const RowOut r{lane, i, env0, i < n, env0 + (uint32_t)kWave <= n};

  Coef q = uniform_coef(c);
  if (s.veh != nullptr) q = load_coef(s.veh, s.veh_stride, r.valid ? i : 0u);
  // the stored env, decoded as step_many_kernel decodes it (its counters are the rollout's in both start forms)
  using TILE = TileIO<MODE>;
  const TILE tile(s, tile_index, lane);
  Env<MODE> e;
  unpack_env<MODE, TILE>(c, tile.load_group(0), tile.load_group(1), tile.load_group(2), tile.load_group(3), e);
  resolve_episode<MODE>(c, tile, e);
  double px, py, pz;
  rollout_start<TASK, MODE>(c, q, io, tile, i, n, r.valid, e, px, py, pz);

  act.begin(r.valid ? i : 0u, n);
#pragma clang loop unroll(disable)
  for (int k = 0; k < io.num_steps; ++k) {
    const size_t row = (size_t)k * n;  // 64-bit: K x N x 12 doubles pass 4 GiB at 1 M envs
    const float4 a = act.next(e.x, row, r);
    const bool resetting = e.reset_pending;
    double reward;
    bool term, trunc;
    rollout_step<TASK, MODE>(c, q, e, a, px, py, pz, reward, term, trunc);
    next_perturbation<MODE>(c, q, tile, i, resetting, e, px, py, pz);
    if (io.x_dev != nullptr) store_x_row(xrow, io.x_dev, row, r, e.x);
    if (r.valid) {
      if (io.reward_dev != nullptr) io.reward_dev[row + i] = reward;
      if (io.terminated_dev != nullptr) io.terminated_dev[row + i] = term ? 1 : 0;
      if (io.truncated_dev != nullptr) io.truncated_dev[row + i] = trunc ? 1 : 0;
      if (io.status_dev != nullptr) io.status_dev[row + i] = (uint8_t)e.fs;
    }
  }
}

// Where the parameter-gradient backward writes (cs_rollout_vjp_ex): g_coef [kCoefRows, N] float64 (the adjoints of
// Coef's rows, for unfold_vehicle_kernel), g_force [3, N] (newtons; float32 when f32) or nullptr.
struct ParamGradOut {
  double* g_coef;
  void* g_force;
  uint32_t f32;
};

// What a sweep adds to the plain one (rollout_vjp_sweep's EXT):
//   kParam   the coefficient adjoints (cs_rollout_vjp_ex): step_adjoint's PARAM terms, accumulated in the lane's LDS
//            columns `acc` (2 x kAccRows rows: step 0 has its own set), the pending force in newtons at steps 1 and 0,
//            and the g_coef / g_force stores to `po`
//   kPolicy  the caller's cotangent on the action tape, ext.add_action_cotangent(row, env, ga) (cs_rollout_mlp_vjp_ex:
//            g_a += g_actions_in, before g_a is stored), then the policy's vector-Jacobian product ext.vjp(x, ga, lam)
//            after each step's adjoint (cs_rollout_mlp_vjp: lambda_o += J_o pi^T g_a), skipped on a resetting step 0
struct SweepPlain {
  static constexpr bool kParam = false, kPolicy = false;
};
struct SweepParam {
  static constexpr bool kParam = true, kPolicy = false;
  const ParamGradOut& po;
  double* acc;
};

// pending_perturbation() with the force kept: f = the pending force in newtons (0 when none), (px, py, pz) = f two_inv_M
// with the same bits as pending_perturbation's (f x 1.0 is f, and -0.0 x 1.0 is -0.0)
template <int MODE, class TILE>
__device__ __forceinline__ void pending_force(const DevConst& c, const Coef& q, const TILE& tile, uint32_t i,
                                              uint32_t episode, uint32_t ep_far, bool pend, bool expl, double (&f)[3],
                                              double& px, double& py, double& pz) {
  Coef unit = q;
  unit.two_inv_M = 1.0;
  pending_perturbation<MODE, true>(c, unit, tile, i, episode, ep_far, pend, expl, f[0], f[1], f[2]);
  px = f[0] * q.two_inv_M;
  py = f[1] * q.two_inv_M;
  pz = f[2] * q.two_inv_M;
#pragma unroll
  for (int j = 0; j < 3; ++j) f[j] = pend ? f[j] : 0.0;
}

// The backward: sweeps k = K .. 1 with the adjoint lam in registers, each step's primal recomputed from the caller's
// tape (io.x_dev / status_dev; io.actions_dev is the actions, the action tape of a closed-loop rollout).  g_a of step k
// is complete when its adjoint returns it: every later step's dependence on a_k runs through x_k, whose adjoint lam
// already holds.  EXT: SweepPlain, SweepParam or the closed-loop rollouts' policy.
template <int TASK, int MODE, bool GYRO, class EXT>
__device__ __forceinline__ void rollout_vjp_sweep(const DevConst& c, const DevState& s, const cs_rollout_io& io,
                                                  const EXT& ext) {
  constexpr int A = task_act_dim(TASK);
  constexpr bool PARAM = EXT::kParam;
  const int lane = threadIdx.x;
  const uint32_t tile_index = blockIdx.x;
  const uint32_t i = tile_index * kBlock + threadIdx.x;
  const uint32_t n = s.n;
  const bool valid = i < n;
  const uint32_t ii = valid ? i : 0u;  // (padding lanes recompute env 0's steps and store nothing)
  const int K = io.num_steps;
  const bool f32out = io.out_dtype == CS_JAC_F32;
  auto store_actions = [&](size_t row, const double (&ga)[4]) {
    if (f32out)
      store_ga<float, A>(io.g_actions_dev, row, i, ga);
    else
      store_ga<double, A>(io.g_actions_dev, row, i, ga);
  };

  Coef q = uniform_coef(c);
  if (s.veh != nullptr) q = load_coef(s.veh, s.veh_stride, ii);
  double lam[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) lam[k] = 0.0;
  double ga[4];
  double* acc = nullptr;
  if constexpr (PARAM) {
    acc = ext.acc;
#pragma unroll
    for (int j = 0; j < 2 * kAccRows; ++j) acc[j * kBlock] = 0.0;
  }

  // ---- steps K-1 .. 2: starts from the tape, the next step's inputs fetched while this one computes ----
  StepIn cur;
  if (K > 1) load_tape_step<TASK>(io, n, ii, K - 1, cur);
#pragma clang loop unroll(disable)
  for (int k = K - 1; k >= 2; --k) {
    StepIn nxt;  // (the earlier step's tape row and action, in flight while this step computes)
    load_tape_step<TASK>(io, n, ii, k - 1, nxt);
    const double gr = add_cotangents(io, (size_t)k * n, ii, lam);
    const double* tape_next = nullptr;
#ifdef CS_DEBUG_ROLLOUT
    tape_next = io.x_dev + ((size_t)k * n + ii) * 12;
#endif
    step_adjoint<TASK, MODE, GYRO, PARAM>(c, q, cur, gr, -0.0, -0.0, -0.0, false, true, false, tape_next, lam, ga,
                                          acc);
    if constexpr (EXT::kPolicy) ext.add_action_cotangent((size_t)k * n, ii, ga);
    if (valid && io.g_actions_dev != nullptr) store_actions((size_t)k * n, ga);
    if constexpr (EXT::kPolicy) ext.vjp(cur.x, ga, lam);
    cur = nxt;
  }

  // ---- step 1 (peeled: the loop's steps have no perturbation) ----
  // A stored-start lane with a NEXT_STEP reset pending resets in step 0, and the new episode's perturbation (the draw
  // step() makes) enters the first call of step 1: its recompute needs it, or its x' is not the tape's.  Every other
  // perturbation is consumed in step 0 or only ever meets calls that do not integrate.
  if (K > 1) {
    double px = -0.0, py = -0.0, pz = -0.0;
    double f1[3] = {0.0, 0.0, 0.0};  // (PARAM) that draw in newtons: px = f1[0] two_inv_M
    if (io.start_x_dev == nullptr) {
      using TILE = TileIO<MODE>;
      const TILE tile(s, tile_index, lane);
      Env<MODE> e;
      unpack_env<MODE, TILE>(c, tile.load_group(0), tile.load_group(1), tile.load_group(2), tile.load_group(3), e);
      if (e.reset_pending) {  // (rollout_step's masked reset, then the forward's draw for the new episode)
        resolve_episode<MODE>(c, tile, e);
        next_episode<MODE, true>(e);
        if constexpr (PARAM) {
          pending_force<MODE>(c, q, tile, i, e.episode, e.ep_far, true, false, f1, px, py, pz);
        } else {
          pending_perturbation<MODE, true>(c, q, tile, i, e.episode, e.ep_far, true, false, px, py, pz);
        }
      }
    }
    const double gr = add_cotangents(io, (size_t)n, ii, lam);
    const double* tape_next = nullptr;
#ifdef CS_DEBUG_ROLLOUT
    tape_next = io.x_dev + ((size_t)n + ii) * 12;
#endif
    step_adjoint<TASK, MODE, GYRO, PARAM>(c, q, cur, gr, px, py, pz, false, true, false, tape_next, lam, ga, acc);
    if constexpr (PARAM) {  // the new episode's draw is a constant, 2 / M multiplies it: only two_inv_M's adjoint
      acc[8 * kBlock] += (acc[(kAccPe + 0) * kBlock] * f1[0] + acc[(kAccPe + 1) * kBlock] * f1[1]) +
                         acc[(kAccPe + 2) * kBlock] * f1[2];
    }
    if constexpr (EXT::kPolicy) ext.add_action_cotangent((size_t)n, ii, ga);
    if (valid && io.g_actions_dev != nullptr) store_actions((size_t)n, ga);
    if constexpr (EXT::kPolicy) ext.vjp(cur.x, ga, lam);
  }

  // ---- step 0: from the start point, decoded as the forward decoded it ----
  StepIn in;
  double px, py, pz;
  double f0[3] = {0.0, 0.0, 0.0};  // (PARAM) the start's pending force in newtons: px = f0[0] two_inv_M
  bool fpend = false;              // (PARAM) a force is pending at the start: only then has it a gradient
  bool resetting = false, prev_diff = false, prev_none = false;
  if (io.start_x_dev != nullptr) {
    bool pend;
    double prev_sh;
    explicit_start<TASK, MODE>(c, q, io, i, n, valid, in.x, in.fs, pend, px, py, pz, prev_sh);
    prev_diff = io.start_prev_shaping_dev == nullptr;
    prev_none = prev_sh != prev_sh;
    if constexpr (PARAM) {
      fpend = pend && valid;
      if (fpend) {
#pragma unroll
        for (int j = 0; j < 3; ++j) f0[j] = io.start_force_dev[(size_t)j * n + i];
      }
    }
  } else {
    using TILE = TileIO<MODE>;
    const TILE tile(s, tile_index, lane);
    Env<MODE> e;
    unpack_env<MODE, TILE>(c, tile.load_group(0), tile.load_group(1), tile.load_group(2), tile.load_group(3), e);
    resolve_episode<MODE>(c, tile, e);
    if constexpr (PARAM) {
      pending_force<MODE>(c, q, tile, i, e.episode, e.ep_far, e.pend, e.expl, f0, px, py, pz);
      fpend = e.pend;
    } else {
      pending_perturbation<MODE, true>(c, q, tile, i, e.episode, e.ep_far, e.pend, e.expl, px, py, pz);
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) in.x[k] = e.x[k];
    in.fs = e.fs;
    resetting = e.reset_pending;
    prev_none = e.prev_sh != e.prev_sh;
  }
  in.act = load_action_at<TASK>(io.actions_dev + (size_t)ii * A);
  const double gr0 = add_cotangents(io, 0, ii, lam);
  const double* tape_next = nullptr;
#ifdef CS_DEBUG_ROLLOUT
  if (!resetting) tape_next = io.x_dev + (size_t)ii * 12;  // (a resetting step is not recomputed: its gradient is 0)
#endif
  // (PARAM) step 0 accumulates into the second set of rows, added unless the step is a NEXT_STEP reset: that step
  // computes nothing (dt = 0), but its pre-reset state need not be finite
  step_adjoint<TASK, MODE, GYRO, PARAM>(c, q, in, gr0, px, py, pz, resetting, prev_diff, prev_none, tape_next, lam,
                                        ga, PARAM ? acc + kAccRows * kBlock : nullptr);
  if constexpr (PARAM) {
    double* acc0 = acc + kAccRows * kBlock;
    // the perturbation's adjoint, where there is a perturbation: none pending (consumed, or an explicit start without
    // start_force_dev) and a NEXT_STEP reset (its new draw is a constant) give a force gradient of exactly 0
    const bool live = fpend && !resetting;
    const double pe[3] = {live ? acc0[(kAccPe + 0) * kBlock] : 0.0, live ? acc0[(kAccPe + 1) * kBlock] : 0.0,
                          live ? acc0[(kAccPe + 2) * kBlock] : 0.0};
    acc[8 * kBlock] += (pe[0] * f0[0] + pe[1] * f0[1]) + pe[2] * f0[2];
    if (valid) {  // the coefficient adjoints [11, N] for the unfold kernel, the force's [3, N] in the caller's dtype
#pragma unroll
      for (int j = 0; j < kCoefRows; ++j)
        ext.po.g_coef[(size_t)j * n + i] = resetting ? acc[j * kBlock] : acc[j * kBlock] + acc0[j * kBlock];
      if (ext.po.g_force != nullptr) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const double g = q.two_inv_M * pe[j];
          if (ext.po.f32)
            reinterpret_cast<float*>(ext.po.g_force)[(size_t)j * n + i] = (float)g;
          else
            reinterpret_cast<double*>(ext.po.g_force)[(size_t)j * n + i] = g;
        }
      }
    }
  }
  // (a resetting lane: the step's ga = lam = 0, so ga is the caller's cotangent alone; the policy's product is skipped
  // -- its pre-reset state need not be finite, and a stored start returns no g_x0)
  if constexpr (EXT::kPolicy) {
    ext.add_action_cotangent(0, ii, ga);
    if (!resetting) ext.vjp(in.x, ga, lam);
  }
  if (valid) {
    if (io.g_actions_dev != nullptr) store_actions(0, ga);
    if (io.g_x0_dev != nullptr) {
#pragma unroll
      for (int k = 0; k < 12; ++k) {
        if (f32out)
          reinterpret_cast<float*>(io.g_x0_dev)[(size_t)k * n + i] = (float)lam[k];
        else
          reinterpret_cast<double*>(io.g_x0_dev)[(size_t)k * n + i] = lam[k];
      }
    }
  }
}

}  // namespace
}  // namespace cs
