// copterstep_rollout_ac.hip -- on-policy actor-critic collection and generalised advantage estimation on gfx950
// (cs_rollout_actor_critic / cs_gae, include/copterstep.h): K closed-loop steps under the env's own auto-reset mode in
// which step k takes a_k = mu(o_{k-1}) + sigma eps_k with the noise drawn from its counter (ppo_noise.h), and the
// tapes a PPO / A2C learner needs of them -- observations, actions, means, log-probabilities, values, rewards, flags
// and the live mask -- written as the steps are made; then the advantages and returns of those tapes.  The stored env
// state advances exactly as under cs_step_many with the same actions.  DESIGN.md section 17.
//
// Upstream lines replaced: lander.py:40-65 (observe, act, step) under a stochastic policy with a value head -- the
// collection loop of the on-policy trainers; the step is advance() (dev_task.h), the one cs_step runs.
//
// One lane per env on the tile layout of the step kernels (tile t -> workgroup t).  The loop is a sibling of
// rollout_custom_kernel's (include/copterstep_rollout.h), in a lean and a full-featured form: that kernel's policy
// functor does not see a pending NEXT_STEP reset, which the live mask needs.  The weights of both networks are wave-uniform and are read
// by the scalar unit, streamed one hidden unit at a time, as copterstep_rollout_mlp.hip reads its one theta.
#include <cmath>
#include <string>

#include "copterstep_jacobian.h"

// the step must round as the step kernels do (copterstep_kernels.hip), and the policy's float32 arithmetic is
// cs_rollout_mlp_states': the explicit fmaf chains of mlp_policy.h, nothing contracted
#pragma clang fp contract(off)

#include "dev_tile.h"
#include "dev_codec.h"
#include "dev_math.h"
#include "dev_physics.h"
// the two networks may need every register there is: no late row conversion (dev_task.h: ROW_LATE)
#define CS_NO_ROW_LATE 1
#include "dev_task.h"
#include "dev_pid.h"
#include "ppo_noise.h"
#include "mlp_policy.h"
#include "dev_launch.h"

namespace cs {
namespace {

// what the collection kernel takes of cs_rollout_ac_io
struct AcArgs {
  const float* actor;    // [P]
  const float* critic;   // [Pv] or nullptr
  const float* log_std;  // [A]
  float* obs;            // [K+1,N,OBS]
  float* actions;        // [K,N,A]
  float* means;          // [K,N,A] or nullptr
  float* logp;           // [K,N]
  float* values;         // [K+1,N] or nullptr (with critic)
  float* reward;         // [K,N]
  uint8_t* flags;        // [K,N,2]
  uint8_t* live;         // [K,N]
  int num_steps, hidden, critic_hidden;
  uint32_t key, nonce, deterministic;
};

// one float32 row of W values of this lane, [.., N, W] at env `at` (64-bit): one 16 / 8 / 4-byte store where W allows
template <int W>
__device__ __forceinline__ void store_row(float* base, size_t at, const float (&v)[W]) {
  float* dst = base + at * W;
  if constexpr (W == 4) {
    *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
  } else if constexpr (W == 2) {
    *reinterpret_cast<float2*>(dst) = make_float2(v[0], v[1]);
  } else {
#pragma unroll
    for (int j = 0; j < W; ++j) dst[j] = v[j];
  }
}

constexpr double kHalfLog2Pi = 0.91893853320467274178032973640562;  // ln(2 pi) / 2

// LEAN: the common configuration's form (dev_launch.h: lean_config, and one physics call per step): advance() with its
// optional features compiled out, as step_many_kernel's lean instantiations; every other configuration runs the
// full-featured form.  The same steps either way.  Timed against the full-featured form alone: 22 % faster per step at
// 2^20 envs and H >= 32, 6-9 % at 65 536 (profiles/rollout_ac_bench.txt, rows "full").
template <int TASK, int MODE, bool LEAN = false>
__global__ __launch_bounds__(kBlock) void rollout_ac_kernel(const DevConst c_arg, const DevState s, const AcArgs m) {
  constexpr int OBS = task_obs_dim(TASK), FIRST = task_obs_first(TASK), A = task_act_dim(TASK);
  DevConst c = c_arg;
  park_constants<MODE == CS_STATE_F64 || kFullTrigInEveryMode>(c);  // the deep constants out of the scalar registers' way
  const uint32_t n = s.n;
  const uint32_t tile_index = blockIdx.x;
  const int lane = threadIdx.x;
  const uint32_t i = tile_index * kBlock + lane;
  const bool valid = i < n;
  using TILE = TileIO<MODE>;
  const TILE tile(s, tile_index, lane);

  Env<MODE> e;
  {
    const typename TILE::Group t2 = tile.load_group(1);
    const typename TILE::Group r1 = tile.load_group(2);
    const typename TILE::Group r2 = tile.load_group(3);
    const typename TILE::Group t1 = tile.load_group(0);
    unpack_env<MODE, TILE>(c, t1, t2, r1, r2, e);
  }
  resolve_episode<MODE>(c, tile, e);  // the reset draws inside the loop are keyed by the whole episode number
  StepOpts o;
#ifdef CS_KSTAMPS
  o.kst = nullptr;
#endif
  o.stats = !LEAN && c.stats;
  o.ticks = !LEAN && c.ticks;
  o.trunc = !LEAN && c.tl_trunc;
  o.done_list = false;
  o.same_step = !LEAN && c.autoreset == CS_AUTORESET_SAME_STEP;
  o.gyro = !LEAN && c.gyro;
  o.act_f32 = !LEAN && c.act_f32;
  e.ep_ret = o.stats ? tile.load_ret() : 0.f;
  e.ticks = o.ticks ? tile.load_ticks() : 0u;
  cs_step_io io;  // no optional outputs in the K-step forms
  io.actions_dev = nullptr;
  io.output_form = CS_OUTPUT_PLAIN;
  io.reserved_ = 0;
  io.obs_dev = io.reward_dev = io.final_obs_dev = io.done_return_dev = nullptr;
  io.terminated_dev = io.truncated_dev = nullptr;
  io.done_count_dev = io.done_ids_dev = io.done_length_dev = nullptr;
  Coef q = uniform_coef(c);
  if constexpr (!LEAN) {
    if (s.veh != nullptr) q = load_coef(s.veh, s.veh_stride, i);
  }

  // sigma_c = expf(log_std[c]) and, for the log-probability, exp(-log_std[c]) and sum_c log_std[c] in float64: once
  float sigma[A];
  double inv_sigma[A], sum_log_std = 0.0;
#pragma unroll
  for (int j = 0; j < A; ++j) {
    const float ls = weight(m.log_std, j);
    sigma[j] = expf(ls);
    inv_sigma[j] = exp(-(double)ls);
    sum_log_std = sum_log_std + (double)ls;
  }
  const uint32_t g = c.id_lo + i;  // the global env id of the reset draw (dev_codec.h: draw_force)

  float seen[OBS];
#pragma unroll
  for (int j = 0; j < OBS; ++j) seen[j] = (float)e.x[FIRST + j];
  if (valid) store_row_direct<OBS>(m.obs + (size_t)i * OBS, seen);  // row 0: the stored state's observation

  const int K = m.num_steps;
  // Everything loaded so far (the env, log_std) is taken delivery of HERE, once, as rollout_custom_kernel does
  // (include/copterstep_rollout.h): a wait left inside the loop would sit out the previous step's stores.
#if defined(__gfx950__) || defined(__gfx942__) || defined(__gfx940__) || defined(__gfx90a__) || defined(__gfx908__) || defined(__gfx906__) || defined(__gfx900__)
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0) in the gfx9 encoding
#else
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
#pragma clang loop unroll(disable)
  for (int k = 0; k < K; ++k) {
    const size_t row = (size_t)k * n;  // 64-bit uniform offsets: K * N can exceed 32 bits
    // ---- actor and critic on o_{k-1} ----
    float mu[A], a[A];
    mlp_forward<OBS, A>(m.actor, m.hidden, seen, mu);
    if (m.critic != nullptr) {
      float v[1];
      mlp_forward<OBS, 1>(m.critic, m.critic_hidden, seen, v);
      if (valid) m.values[row + i] = v[0];
    }
    // ---- the action: a_c = fl32(mu_c + fl32(sigma_c eps_c)), and its log-probability from the stored values ----
    double zz = 0.0;  // sum_c z_c^2, c ascending
    if (m.deterministic != 0u) {
#pragma unroll
      for (int j = 0; j < A; ++j) a[j] = mu[j];
    } else {
      float eps[(A + 1) / 2 * 2];
#pragma unroll
      for (int p = 0; p < (A + 1) / 2; ++p)
        ppo_noise_pair(m.key, g, m.nonce, (uint32_t)k + 1u, (uint32_t)p, eps[2 * p], eps[2 * p + 1]);
#pragma unroll
      for (int j = 0; j < A; ++j) {
        const float d = sigma[j] * eps[j];
        a[j] = mu[j] + d;
        const double z = ((double)a[j] - (double)mu[j]) * inv_sigma[j];
        zz = zz + z * z;
      }
    }
    const float logp = (float)((-0.5 * zz - sum_log_std) - (double)A * kHalfLog2Pi);
    const bool resetting = e.reset_pending;  // NEXT_STEP: this step is the reset, the env ignores the action
    if (valid) {
      store_row<A>(m.actions, row + i, a);
      if (m.means != nullptr) store_row<A>(m.means, row + i, mu);
      m.logp[row + i] = logp;
      m.live[row + i] = resetting ? (uint8_t)0 : (uint8_t)1;
    }

    StepOut<OBS> out;
    advance<TASK, MODE, OBS, LEAN, LEAN, true, true>(c, q, o, e, motors_of<A>(a), io, i, lane, valid, tile, out);
#pragma unroll
    for (int j = 0; j < OBS; ++j) seen[j] = out.row[j];
    if (valid) {
      m.reward[row + i] = (float)out.reward;
      const uint16_t both = (uint16_t)((out.term ? 1u : 0u) | (out.trunc ? 0x100u : 0u));
      *reinterpret_cast<uint16_t*>(m.flags + 2 * (row + i)) = both;
      store_row_direct<OBS>(m.obs + (row + n + i) * OBS, out.row);  // row k + 1
    }
  }
  // V of the bootstrap observation, row K
  if (m.critic != nullptr) {
    float v[1];
    mlp_forward<OBS, 1>(m.critic, m.critic_hidden, seen, v);
    if (valid) m.values[(size_t)K * n + i] = v[0];
  }

  split_episode<MODE>(c, tile, e);
  store_env<MODE, TILE>(c, tile, e);
  if (o.stats) tile.store_ret(e.ep_ret);
  if (o.ticks) tile.store_ticks(e.ticks);
}

template <int TASK, int MODE>
hipError_t rollout_ac_t(const DevConst& c, const DevState& s, const AcArgs& m, hipStream_t stream) {
#ifndef CS_EXP_AC_FULL  // (A/B timing build, make exp NAME=ac_full DEFS=-DCS_EXP_AC_FULL: the full-featured form alone)
  if (lean_config(c, s) && c.nsub == 1) {
    hipLaunchKernelGGL((rollout_ac_kernel<TASK, MODE, true>), dim3(grid_for(s.n)), dim3(kBlock), 0, stream, c, s, m);
    return hipGetLastError();
  }
#endif
  hipLaunchKernelGGL((rollout_ac_kernel<TASK, MODE>), dim3(grid_for(s.n)), dim3(kBlock), 0, stream, c, s, m);
  return hipGetLastError();
}

hipError_t launch_rollout_ac(int task, int mode, const DevConst& c, const DevState& s, const AcArgs& m,
                             hipStream_t stream) {
  CS_DISPATCH(rollout_ac_t, c, s, m, stream)
}

// ---- generalised advantage estimation: lane = env, k descending, [K,N] rows (64 consecutive elements per wavefront) ----
__global__ __launch_bounds__(kBlock) void gae_kernel(const float* __restrict__ reward, const float* __restrict__ values,
                                                    const uint8_t* __restrict__ term, const uint8_t* __restrict__ trunc,
                                                    const uint32_t flag_stride, const int K, const uint32_t n,
                                                    const float g, const float gl, float* __restrict__ adv,
                                                    float* __restrict__ ret) {
  const uint32_t tile_index = blockIdx.x;  // (64 envs: no state tiles touched)
  const uint32_t i = tile_index * kBlock + threadIdx.x;
  if (i >= n) return;
  float next_v = values[(size_t)K * n + i], next_adv = 0.0f;
#pragma clang loop unroll(disable)
  for (int k = K - 1; k >= 0; --k) {
    const size_t at = (size_t)k * n + i;
    const float nd = (term[at * flag_stride] | trunc[at * flag_stride]) != 0 ? 0.0f : 1.0f;
    const float v = values[at];
    const float boot = (g * next_v) * nd;
    const float delta = (reward[at] + boot) - v;
    const float carry = (gl * nd) * next_adv;
    const float a = delta + carry;
    adv[at] = a;
    ret[at] = a + v;
    next_adv = a;
    next_v = v;
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// the argument block, checked before the context
int check_ac_io(const cs_rollout_ac_io* aio, const char* who) {
  const std::string w(who);
  if (aio == nullptr) return report_error(CS_ERR_ARG, (w + ": null aio").c_str());
  if (aio->struct_size != sizeof(cs_rollout_ac_io))
    return report_error(CS_ERR_ABI, (w + ": aio->struct_size " + std::to_string(aio->struct_size) + " != " +
                                     std::to_string(sizeof(cs_rollout_ac_io)) + " (sizeof(cs_rollout_ac_io))").c_str());
  if (aio->num_steps < 1) return report_error(CS_ERR_ARG, (w + ": num_steps must be >= 1").c_str());
  if (int rc_ = check_hidden(who, "hidden", aio->hidden)) return rc_;
  if (int rc_ = check_hidden(who, "critic_hidden", aio->critic_hidden)) return rc_;
  if (aio->deterministic > 1u) return report_error(CS_ERR_ARG, (w + ": deterministic must be 0 or 1").c_str());
  if (aio->actor_dev == nullptr) return report_error(CS_ERR_ARG, (w + ": actor_dev is required").c_str());
  if (aio->log_std_dev == nullptr) return report_error(CS_ERR_ARG, (w + ": log_std_dev is required").c_str());
  if (aio->obs_dev == nullptr) return report_error(CS_ERR_ARG, (w + ": obs_dev is required").c_str());
  if (aio->actions_dev == nullptr) return report_error(CS_ERR_ARG, (w + ": actions_dev is required").c_str());
  if (aio->logp_dev == nullptr) return report_error(CS_ERR_ARG, (w + ": logp_dev is required").c_str());
  if (aio->reward_dev == nullptr) return report_error(CS_ERR_ARG, (w + ": reward_dev is required").c_str());
  if (aio->flags_dev == nullptr) return report_error(CS_ERR_ARG, (w + ": flags_dev is required").c_str());
  if (aio->live_dev == nullptr) return report_error(CS_ERR_ARG, (w + ": live_dev is required").c_str());
  if (aio->critic_dev != nullptr && aio->values_dev == nullptr)
    return report_error(CS_ERR_ARG, (w + ": values_dev is required with critic_dev").c_str());
  if (aio->critic_dev == nullptr && aio->values_dev != nullptr)
    return report_error(CS_ERR_ARG, (w + ": values_dev must be NULL without critic_dev").c_str());
  const void* outs[] = {aio->obs_dev,    aio->actions_dev, aio->means_dev, aio->logp_dev,
                        aio->values_dev, aio->reward_dev,  aio->flags_dev, aio->live_dev};
  for (const void* p : outs)
    if (!aligned16(p)) return report_error(CS_ERR_ARG, (w + ": every output must be 16-byte aligned").c_str());
  if (((reinterpret_cast<uintptr_t>(aio->actor_dev) | reinterpret_cast<uintptr_t>(aio->critic_dev) |
        reinterpret_cast<uintptr_t>(aio->log_std_dev)) & 3u) != 0)
    return report_error(CS_ERR_ARG, (w + ": actor_dev, critic_dev and log_std_dev must be 4-byte aligned").c_str());
  return CS_OK;
}

int check_gae_io(const cs_gae_io* gio, const char* who) {
  const std::string w(who);
  if (gio == nullptr) return report_error(CS_ERR_ARG, (w + ": null gio").c_str());
  if (gio->struct_size != sizeof(cs_gae_io))
    return report_error(CS_ERR_ABI, (w + ": gio->struct_size " + std::to_string(gio->struct_size) + " != " +
                                     std::to_string(sizeof(cs_gae_io)) + " (sizeof(cs_gae_io))").c_str());
  if (gio->num_steps < 1) return report_error(CS_ERR_ARG, (w + ": num_steps must be >= 1").c_str());
  if (gio->flag_stride != 1u && gio->flag_stride != 2u)
    return report_error(CS_ERR_ARG, (w + ": flag_stride must be 1 or 2").c_str());
  if (gio->reserved_ != 0u) return report_error(CS_ERR_ARG, (w + ": reserved_ must be 0").c_str());
  if (!std::isfinite(gio->gamma)) return report_error(CS_ERR_ARG, (w + ": gamma must be finite").c_str());
  if (!std::isfinite(gio->lam)) return report_error(CS_ERR_ARG, (w + ": lam must be finite").c_str());
  // the kernel takes fl32(gamma) and fl32(fl32(gamma) fl32(lam)): a finite double past FLT_MAX narrows to infinity
  if (!std::isfinite((float)gio->gamma) || !std::isfinite((float)gio->lam) ||
      !std::isfinite((float)gio->gamma * (float)gio->lam))
    return report_error(CS_ERR_ARG, (w + ": gamma, lam and gamma x lam must be finite in float32").c_str());
  if (gio->reward_dev == nullptr) return report_error(CS_ERR_ARG, (w + ": reward_dev is required").c_str());
  if (gio->values_dev == nullptr) return report_error(CS_ERR_ARG, (w + ": values_dev is required").c_str());
  if (gio->terminated_dev == nullptr) return report_error(CS_ERR_ARG, (w + ": terminated_dev is required").c_str());
  if (gio->truncated_dev == nullptr) return report_error(CS_ERR_ARG, (w + ": truncated_dev is required").c_str());
  if (gio->advantages_dev == nullptr) return report_error(CS_ERR_ARG, (w + ": advantages_dev is required").c_str());
  if (gio->returns_dev == nullptr) return report_error(CS_ERR_ARG, (w + ": returns_dev is required").c_str());
  return CS_OK;
}

}  // namespace
}  // namespace cs

extern "C" int cs_rollout_actor_critic(cs_ctx* ctx, const cs_rollout_ac_io* aio, void* stream) {
  const char* who = "cs_rollout_actor_critic";
  if (int rc_ = cs::check_ac_io(aio, who)) return rc_;
  cs::ContextView v;
  if (int rc_ = cs::enter_context(ctx, who, stream, &v)) return rc_;  // (refuses an open served session)
  // (Packed rows -- reward_dev == obs_dev + OBS, the flags in the word after it: cs_step_io -- cannot reach this point:
  // OBS + 1 floats past a 16-byte aligned obs_dev is never 16-byte aligned for OBS in {2, 6, 10, 12}, and check_ac_io
  // has refused an unaligned output.)
  const cs::AcArgs m{aio->actor_dev, aio->critic_dev, aio->log_std_dev, aio->obs_dev,    aio->actions_dev,
                     aio->means_dev, aio->logp_dev,   aio->values_dev,  aio->reward_dev, aio->flags_dev,
                     aio->live_dev,  aio->num_steps,  aio->hidden,      aio->critic_hidden,
                     cs::ppo_noise_key(cs::context_seed(ctx)), aio->nonce, aio->deterministic};
  const hipError_t e = cs::launch_rollout_ac(v.task, v.mode, *v.c, *v.s, m, (hipStream_t)stream);
  if (e != hipSuccess) return cs::report_hip(e, "cs_rollout_actor_critic: kernel launch");
  return CS_OK;
}

extern "C" int cs_gae(cs_ctx* ctx, const cs_gae_io* gio, void* stream) {
  const char* who = "cs_gae";
  if (int rc_ = cs::check_gae_io(gio, who)) return rc_;
  cs::ContextView v;
  if (int rc_ = cs::enter_context(ctx, who, stream, &v)) return rc_;
  const float g = (float)gio->gamma;
  const float gl = g * (float)gio->lam;  // (float32 product: contraction is off in this file)
  hipLaunchKernelGGL(cs::gae_kernel, dim3(cs::grid_for(v.s->n)), dim3(cs::kBlock), 0, (hipStream_t)stream,
                     gio->reward_dev, gio->values_dev, gio->terminated_dev, gio->truncated_dev, gio->flag_stride,
                     gio->num_steps, v.s->n, g, gl, gio->advantages_dev, gio->returns_dev);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return cs::report_hip(e, "cs_gae: kernel launch");
  return CS_OK;
}
