// copterstep_rollout_es.hip -- population rollouts and evolution strategies for the MLP policy on gfx950
// (cs_rollout_mlp_population / cs_es_perturb / cs_es_gradient, include/copterstep.h): M parameter vectors, each rolled
// out closed-loop on its own envs with the discounted return kept in a register, the mirrored population around a
// centre, and the search gradient with the noise drawn again from its counter (es_noise.h).  Neither a tape nor a noise
// value is written to memory, and nothing of the env state is written.  DESIGN.md section 16.
//
// Upstream lines replaced: lander.py:40-65 (observe, act, step) under a policy, once per population member -- the
// evaluation loop of the neuroevolution and model-free trainers; the step is rollout_step (rollout_step.h), the one
// cs_rollout_mlp_states runs.
//
// Population: one lane per env on the tile layout of the step kernels (tile t -> workgroup t), env i under member
// i / E with E a multiple of 64: a wavefront never mixes members, and its member's row of the table is a function of
// blockIdx alone, so the weights stay wave-uniform and are read by the scalar unit as cs_rollout_mlp_states reads its
// one theta.  The loop is rollout_mlp_states_kernel's (copterstep_rollout_mlp.hip) without its stores.
#include <cmath>
#include <string>

#include "copterstep_jacobian.h"

// the steps must be cs_rollout_mlp_states' bit for bit: the policy's fmaf chains, the step, and the return's float64
// products and sums, none contracted
#pragma clang fp contract(off)

#include "dev_tile.h"
#include "dev_codec.h"
#include "dev_math.h"
#include "dev_physics.h"
#include "dev_task.h"
#include "jacobian_tangents.h"
#include "rollout_adjoint.h"
#include "rollout_step.h"
#include "es_noise.h"
#include "mlp_policy.h"
#include "dev_launch.h"

namespace cs {
namespace {

// what the kernels take of cs_rollout_population_io
struct PopArgs {
  const float* table;  // [M,P] float32
  double* returns;     // [N]
  int32_t* lengths;    // [N] or nullptr
  uint8_t* flags;      // [N] or nullptr
  uint8_t* status;     // [N] or nullptr
  double* member;      // [M] or nullptr
  double gamma;
  uint32_t E, P;       // envs per member, parameters per member
  int hidden;
};

// 3 wavefronts per SIMD: the kernel needs 163 VGPRs without its tapes' staging, and with per-wavefront weights the
// third wavefront covers their scalar-load misses: 4 929 against 6 177 us at 2^20 envs, H = 32, K = 64
// (profiles/rollout_es_bench.txt, rows "default" and "waves2").
// N = M E is a multiple of 64 (checked by the entry point): every lane of every wavefront has an env.
template <int TASK, int MODE>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(3, 3)))
void rollout_mlp_population_kernel(const DevConst c, const DevState s, const cs_rollout_io io, const PopArgs m) {
  constexpr int A = task_act_dim(TASK), OBS = task_obs_dim(TASK), FIRST = task_obs_first(TASK);
  const int lane = threadIdx.x;
  const uint32_t tile_index = blockIdx.x;
  const uint32_t i = tile_index * kBlock + threadIdx.x;
  const uint32_t n = s.n;
  const bool valid = i < n;
  // the wavefront's member: its row of the table is a function of blockIdx alone, so its weights are wave-uniform
  const float* const theta = m.table + (size_t)((tile_index * (uint32_t)kBlock) / m.E) * m.P;

  Coef q = uniform_coef(c);
  if (s.veh != nullptr) q = load_coef(s.veh, s.veh_stride, valid ? i : 0u);
  using TILE = TileIO<MODE>;
  const TILE tile(s, tile_index, lane);
  Env<MODE> e;
  unpack_env<MODE, TILE>(c, tile.load_group(0), tile.load_group(1), tile.load_group(2), tile.load_group(3), e);
  resolve_episode<MODE>(c, tile, e);
  double px, py, pz;
  rollout_start<TASK, MODE>(c, q, io, tile, i, n, valid, e, px, py, pz);

  const int K = io.num_steps;
  double ret = 0.0, disc = 1.0;
  int d = K, end_fs = e.fs;
  uint32_t end_flags = 0u;
  bool done = false;
#pragma clang loop unroll(disable)
  for (int k = 0; k < K; ++k) {
    // ---- the policy: o_{k-1} = what step() returned for the state before this step ----
    float o[OBS], a[A];
#pragma unroll
    for (int j = 0; j < OBS; ++j) o[j] = (float)e.x[FIRST + j];
    mlp_forward<OBS, A>(theta, m.hidden, o, a);

    const bool resetting = e.reset_pending;
    double reward;
    bool term, trunc;
    rollout_step<TASK, MODE>(c, q, e, motors_of<A>(a), px, py, pz, reward, term, trunc);
    next_perturbation<MODE>(c, q, tile, i, resetting, e, px, py, pz);

    if (!done) {  // the episode's return up to and including its last step d
      const double term_k = disc * reward;
      ret = ret + term_k;
      disc = disc * m.gamma;
      if (term || trunc) {
        done = true;
        d = k + 1;
        end_flags = (term ? 1u : 0u) | (trunc ? 2u : 0u);
        end_fs = e.fs;
      }
    }
    if (__builtin_amdgcn_ballot_w64(!done) == 0ull) break;  // (uniform) no output depends on a later step
  }
  if (!done) end_fs = e.fs;  // status_K

  if (valid) {  // one row per output: 64 consecutive elements per wavefront
    m.returns[i] = ret;
    if (m.lengths != nullptr) m.lengths[i] = d;
    if (m.flags != nullptr) m.flags[i] = (uint8_t)end_flags;
    if (m.status != nullptr) m.status[i] = (uint8_t)end_fs;
  }
}

// member_returns[m] = the mean of the member's E returns: one wavefront per member, lanes striding over E in index
// order, then the fixed shuffle tree include/copterstep.h documents
__global__ __launch_bounds__(kBlock) void member_mean_kernel(const double* __restrict__ returns, const uint32_t E,
                                                            double* __restrict__ member) {
  const uint32_t tile_index = blockIdx.x;  // (the member: no state tiles touched)
  const double* r = returns + (size_t)tile_index * E;
  double v = 0.0;
#pragma clang loop unroll(disable)
  for (uint32_t t = threadIdx.x; t < E; t += kBlock) v = v + r[t];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_down(v, off, 64);
  if (threadIdx.x == 0) member[tile_index] = v / (double)E;
}

template <int TASK, int MODE>
hipError_t population_t(const DevConst& c, const DevState& s, const cs_rollout_io& io, const PopArgs& m,
                        hipStream_t stream) {
  hipLaunchKernelGGL((rollout_mlp_population_kernel<TASK, MODE>), dim3(grid_for(s.n)), dim3(kBlock), 0, stream, c, s,
                     io, m);
  return hipGetLastError();
}

hipError_t launch_population(int task, int mode, const DevConst& c, const DevState& s, const cs_rollout_io& io,
                             const PopArgs& m, hipStream_t stream) {
  CS_DISPATCH(population_t, c, s, io, m, stream)
}

// ---- the mirrored population and the search gradient ----
constexpr int kEsBlock = 256;
constexpr uint32_t kEsMaxChunks = CS_ES_MAX_MEMBERS / 2 / CS_ES_PAIR_CHUNK;
// the context's scratch of partial sums (grad_scratch): [chunks, P] of the largest population and policy, 8.9 MB
constexpr size_t kEsScratchBytes = (size_t)kEsMaxChunks * CS_ES_MAX_PARAMS * sizeof(double);
static_assert(CS_ES_MAX_PARAMS == kMlpMaxParams, "Hover3D, H = 64");

// table[2i] = theta + sigma eps_i, table[2i+1] = theta - sigma eps_i: the pair in grid x, 256 parameters per workgroup in y
__global__ __launch_bounds__(kEsBlock) void es_perturb_kernel(const float* __restrict__ theta, float* __restrict__ table,
                                                             const uint32_t P, const float sigma, const uint32_t key,
                                                             const uint32_t nonce, const uint32_t pair_base) {
  const uint32_t tile_index = blockIdx.x, part = blockIdx.y;  // (the pair, 256 parameters: no state tiles touched)
  const uint32_t p = part * kEsBlock + threadIdx.x;
  if (p >= P) return;
  const float dlt = sigma * es_noise(key, pair_base + tile_index, nonce, p);
  const float t = theta[p];
  float* out = table + (size_t)(2u * tile_index) * P + p;
  out[0] = t + dlt;
  out[P] = t - dlt;
}

// partials[chunk][p] = sum over the chunk's pairs, i ascending, of (w[2i] - w[2i+1]) eps(i, p): lane = parameter
__global__ __launch_bounds__(kBlock) void es_gradient_kernel(const double* __restrict__ w, const uint32_t pairs,
                                                            const uint32_t P, const uint32_t key, const uint32_t nonce,
                                                            const uint32_t pair_base, double* __restrict__ partials) {
  const uint32_t tile_index = blockIdx.x, chunk = blockIdx.y;  // (64 parameters, 32 pairs: no state tiles touched)
  const uint32_t p = tile_index * kBlock + threadIdx.x;
  if (p >= P) return;
  const uint32_t i0 = chunk * CS_ES_PAIR_CHUNK;
  const uint32_t i1 = i0 + CS_ES_PAIR_CHUNK < pairs ? i0 + CS_ES_PAIR_CHUNK : pairs;
  double acc = 0.0;
#pragma clang loop unroll(disable)
  for (uint32_t i = i0; i < i1; ++i) {
    const double dw = w[2u * i] - w[2u * i + 1u];
    const double term = dw * (double)es_noise(key, pair_base + i, nonce, p);
    acc = acc + term;
  }
  partials[(size_t)chunk * P + p] = acc;
}

__global__ __launch_bounds__(kBlock) void es_gradient_sum_kernel(const double* __restrict__ partials,
                                                                const uint32_t chunks, const uint32_t P,
                                                                double* __restrict__ grad) {
  const uint32_t tile_index = blockIdx.x;  // (64 parameters: no state tiles touched)
  const uint32_t p = tile_index * kBlock + threadIdx.x;
  if (p >= P) return;
  double t = 0.0;
#pragma clang loop unroll(disable)
  for (uint32_t g = 0; g < chunks; ++g) t = t + partials[(size_t)g * P + p];
  grad[p] = t;
}

// the two argument blocks, checked before the context.  Of cs_rollout_io the call reads num_steps and the start point:
// those rules are check_rollout_io's (copterstep_rollout_grad.hip), restated here because that check requires an
// actions_dev, which this call refuses.
int check_population_io(const cs_rollout_io* io, const cs_rollout_population_io* pio, const char* who) {
  const std::string w(who);
  if (io == nullptr) return report_error(CS_ERR_ARG, (w + ": null io").c_str());
  if (pio == nullptr) return report_error(CS_ERR_ARG, (w + ": null pio").c_str());
  if (io->struct_size != sizeof(cs_rollout_io))
    return report_error(CS_ERR_ABI, (w + ": io->struct_size " + std::to_string(io->struct_size) + " != " +
                                     std::to_string(sizeof(cs_rollout_io)) + " (sizeof(cs_rollout_io))").c_str());
  if (io->num_steps < 1) return report_error(CS_ERR_ARG, (w + ": num_steps must be >= 1").c_str());
  if (io->actions_dev != nullptr)
    return report_error(CS_ERR_ARG, (w + ": io->actions_dev must be NULL (the policy makes the actions)").c_str());
  if (io->start_x_dev == nullptr &&
      (io->start_status_dev != nullptr || io->start_force_dev != nullptr || io->start_prev_shaping_dev != nullptr))
    return report_error(CS_ERR_ARG,
                        (w + ": start_status_dev / start_force_dev / start_prev_shaping_dev describe an explicit start: "
                             "start_x_dev is required").c_str());
  if (io->start_x_dev != nullptr && io->start_status_dev == nullptr)
    return report_error(CS_ERR_ARG, (w + ": an explicit start needs start_status_dev").c_str());
  if (pio->struct_size != sizeof(cs_rollout_population_io))
    return report_error(CS_ERR_ABI, (w + ": pio->struct_size " + std::to_string(pio->struct_size) + " != " +
                                     std::to_string(sizeof(cs_rollout_population_io)) +
                                     " (sizeof(cs_rollout_population_io))").c_str());
  if (int rc_ = check_hidden(who, "hidden", pio->hidden)) return rc_;
  if (pio->members < 1) return report_error(CS_ERR_ARG, (w + ": members must be >= 1").c_str());
  if (pio->envs_per_member < 64 || pio->envs_per_member % 64 != 0)
    return report_error(CS_ERR_ARG, (w + ": envs_per_member " + std::to_string(pio->envs_per_member) +
                                     " is not a positive multiple of 64").c_str());
  if ((int64_t)pio->members * pio->envs_per_member > (int64_t)INT32_MAX)
    return report_error(CS_ERR_ARG, (w + ": members x envs_per_member does not fit a batch").c_str());
  if (!std::isfinite(pio->gamma)) return report_error(CS_ERR_ARG, (w + ": gamma must be finite").c_str());
  if (pio->params_table_dev == nullptr)
    return report_error(CS_ERR_ARG, (w + ": params_table_dev is required").c_str());
  if (pio->returns_dev == nullptr) return report_error(CS_ERR_ARG, (w + ": returns_dev is required").c_str());
  return CS_OK;
}

int check_es_io(const cs_es_io* eio, const char* who, bool gradient) {
  const std::string w(who);
  if (eio == nullptr) return report_error(CS_ERR_ARG, (w + ": null eio").c_str());
  if (eio->struct_size != sizeof(cs_es_io))
    return report_error(CS_ERR_ABI, (w + ": eio->struct_size " + std::to_string(eio->struct_size) + " != " +
                                     std::to_string(sizeof(cs_es_io)) + " (sizeof(cs_es_io))").c_str());
  if (eio->members < 2 || eio->members > CS_ES_MAX_MEMBERS || eio->members % 2 != 0)
    return report_error(CS_ERR_ARG, (w + ": members " + std::to_string(eio->members) + " is not an even number in [2, " +
                                     std::to_string(CS_ES_MAX_MEMBERS) + "]").c_str());
  if (eio->num_params < 1 || eio->num_params > CS_ES_MAX_PARAMS)
    return report_error(CS_ERR_ARG, (w + ": num_params " + std::to_string(eio->num_params) + " is not in [1, " +
                                     std::to_string(CS_ES_MAX_PARAMS) + "]").c_str());
  if (gradient) {
    if (eio->weights_dev == nullptr) return report_error(CS_ERR_ARG, (w + ": weights_dev is required").c_str());
    if (eio->grad_dev == nullptr) return report_error(CS_ERR_ARG, (w + ": grad_dev is required").c_str());
  } else {
    if (!(eio->sigma >= 0.0f) || !std::isfinite(eio->sigma))
      return report_error(CS_ERR_ARG, (w + ": sigma must be finite and >= 0").c_str());
    if (eio->params_dev == nullptr) return report_error(CS_ERR_ARG, (w + ": params_dev is required").c_str());
    if (eio->table_dev == nullptr) return report_error(CS_ERR_ARG, (w + ": table_dev is required").c_str());
  }
  return CS_OK;
}

}  // namespace
}  // namespace cs

extern "C" int cs_rollout_mlp_population(cs_ctx* ctx, const cs_rollout_io* io, const cs_rollout_population_io* pio,
                                         void* stream) {
  const char* who = "cs_rollout_mlp_population";
  if (int rc_ = cs::check_population_io(io, pio, who)) return rc_;
  cs::ContextView v;
  if (int rc_ = cs::enter_context(ctx, who, stream, &v)) return rc_;
  const uint32_t M = (uint32_t)pio->members, E = (uint32_t)pio->envs_per_member;
  if ((uint64_t)M * E != (uint64_t)v.s->n)
    return cs::report_error(CS_ERR_ARG, (std::string(who) + ": members x envs_per_member = " + std::to_string(M) +
                                         " x " + std::to_string(E) + " is not the context's " +
                                         std::to_string(v.s->n) + " envs").c_str());
  const int H = pio->hidden;
  const uint32_t P = cs::mlp_param_count(cs::task_obs_dim(v.task), cs::task_act_dim(v.task), H);
  const cs::PopArgs m{pio->params_table_dev, pio->returns_dev, pio->lengths_dev, pio->end_flags_dev,
                      pio->end_status_dev,   pio->member_returns_dev, pio->gamma, E, P, H};
  hipError_t e = cs::launch_population(v.task, v.mode, *v.c, *v.s, *io, m, (hipStream_t)stream);
  if (e != hipSuccess) return cs::report_hip(e, "cs_rollout_mlp_population: kernel launch");
  if (m.member != nullptr) {
    hipLaunchKernelGGL(cs::member_mean_kernel, dim3(M), dim3(cs::kBlock), 0, (hipStream_t)stream, m.returns, E,
                       m.member);
    e = hipGetLastError();
    if (e != hipSuccess) return cs::report_hip(e, "cs_rollout_mlp_population: member-mean kernel launch");
  }
  return CS_OK;
}

extern "C" int cs_es_perturb(cs_ctx* ctx, const cs_es_io* eio, void* stream) {
  const char* who = "cs_es_perturb";
  if (int rc_ = cs::check_es_io(eio, who, false)) return rc_;
  cs::ContextView v;
  if (int rc_ = cs::enter_context(ctx, who, stream, &v)) return rc_;
  const uint32_t pairs = (uint32_t)eio->members / 2u, P = (uint32_t)eio->num_params;
  hipLaunchKernelGGL(cs::es_perturb_kernel, dim3(pairs, (P + cs::kEsBlock - 1) / cs::kEsBlock), dim3(cs::kEsBlock), 0,
                     (hipStream_t)stream, eio->params_dev, eio->table_dev, P, eio->sigma,
                     cs::es_noise_key(cs::context_seed(ctx)), eio->noise_stream, eio->pair_base);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return cs::report_hip(e, "cs_es_perturb: kernel launch");
  return CS_OK;
}

extern "C" int cs_es_gradient(cs_ctx* ctx, const cs_es_io* eio, void* stream) {
  const char* who = "cs_es_gradient";
  if (int rc_ = cs::check_es_io(eio, who, true)) return rc_;
  cs::ContextView v;
  if (int rc_ = cs::enter_context(ctx, who, stream, &v)) return rc_;
  double* partials = nullptr;
  if (int rc_ = cs::grad_scratch(ctx, cs::kScratchEsGrad, who, stream, cs::kEsScratchBytes, &partials)) return rc_;
  const uint32_t pairs = (uint32_t)eio->members / 2u, P = (uint32_t)eio->num_params;
  const uint32_t chunks = (pairs + CS_ES_PAIR_CHUNK - 1) / CS_ES_PAIR_CHUNK, tiles = (P + cs::kBlock - 1) / cs::kBlock;
  hipLaunchKernelGGL(cs::es_gradient_kernel, dim3(tiles, chunks), dim3(cs::kBlock), 0, (hipStream_t)stream,
                     eio->weights_dev, pairs, P, cs::es_noise_key(cs::context_seed(ctx)), eio->noise_stream,
                     eio->pair_base, partials);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return cs::report_hip(e, "cs_es_gradient: kernel launch");
  hipLaunchKernelGGL(cs::es_gradient_sum_kernel, dim3(tiles), dim3(cs::kBlock), 0, (hipStream_t)stream, partials,
                     chunks, P, eio->grad_dev);
  e = hipGetLastError();
  if (e != hipSuccess) return cs::report_hip(e, "cs_es_gradient: sum kernel launch");
  return CS_OK;
}
