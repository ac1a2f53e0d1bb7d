// copterstep_ppo_grad.hip -- PPO's clipped-surrogate minibatch loss and its gradient on gfx950 (cs_ppo_grad,
// include/copterstep.h): the update half of gym_copter_amd.ppo, over the tapes of cs_rollout_actor_critic and cs_gae.
// DESIGN.md section 18.
//
// The loop replaced: the body of gym_copter_amd/ppo.py's minibatch loop up to and including loss.backward() -- an index
// gather of five tapes, two MLP forwards, the loss, two backwards and the masked reductions, a few dozen torch launches.
//
// The reduction is cs_mlp_param_grad's split-K layout, from the same header (mlp_grad_kit.h: lane = (row slot s, hidden
// unit j), one partial per workgroup, a fixed-order sum kernel), with three additions: a tile's rows are GATHERED through the minibatch's index (lane l fetches sample l's row with
// 8- or 16-byte loads, range-checked in the kernel); the forward runs inside the tile (the outputs are a butterfly over
// the HP lanes of a slot, after which every lane of the slot holds mu, hence dL/dlogp and g_mu); and the advantage's
// mean and deviation come from two small passes over the B advantages whose per-workgroup partials every wavefront of the
// main kernels adds up in the same fixed order.  One template <OBS, A, HP, head>, head = the Gaussian policy or the value
// function, launched once per network into disjoint columns of the partials.  No floating-point atomics.
#include <cmath>
#include <string>

#include "copterstep_jacobian.h"

// the sums are explicit fma chains (the arithmetic include/copterstep.h documents), whatever the compiler would contract
#pragma clang fp contract(off)

#include "mlp_grad_kit.h"

namespace cs {
namespace {

constexpr uint32_t kPrepMaxGroups = 256;         // workgroups of the advantage passes at most
constexpr uint32_t kScalars = 8;                 // per-workgroup scalar columns behind the gradient's
// the scalar columns: sum w Ahat rho', sum w (logp_old - logp), clipped samples, max |rho - 1|, sum w (V - ret)^2
enum { kScSurr = 0, kScKl = 1, kScClip = 2, kScMax = 3, kScValue = 4 };
constexpr int kHeadPolicy = 0, kHeadValue = 1;
// the context's scratch: the partials [kGradMaxGroups][P + Pv + A + kScalars], then the advantage passes' [3][kPrepMaxGroups]
constexpr size_t kPartialDoubles = (size_t)kGradMaxGroups * (kMlpMaxParams + kMlpMaxValueParams + 4 + kScalars);
constexpr size_t kScratchBytes = (kPartialDoubles + 3 * kPrepMaxGroups) * sizeof(double);

struct PpoArgs {
  const float* params;     // this head's network
  const float* log_std;
  const float* obs;
  const float* actions;
  const float* logp;
  const float* adv;
  const float* ret;
  const uint8_t* live;
  const int64_t* index;
  int64_t row_base;
  uint64_t rows, samples;  // R, B
  const double* prep;      // [3][kPrepMaxGroups]: sum w, sum w adv, sum w (adv - m)^2 per workgroup of the passes
  double* partials;
  double clip, vf_coef;
  int hidden;
  uint32_t prep_groups, normalize, tiles_per_group;
  uint32_t stride, offset, ls_offset, scal_offset;  // a partial's length and this head's columns in it
};

// the row of sample s, or -1: past the minibatch's end, or an index outside [0, R) -- such a sample is never read
__device__ __forceinline__ int64_t sample_row(const int64_t* __restrict__ index, const int64_t row_base,
                                              const uint64_t rows, const uint64_t samples, const uint64_t s) {
  if (s >= samples) return -1;
  const int64_t i = index != nullptr ? index[s] : row_base + (int64_t)s;
  return i >= 0 && (uint64_t)i < rows ? i : -1;
}

// sum of col[0..n) over a whole wavefront in a fixed order, the same bits in every lane (a + b = b + a at every level)
__device__ __forceinline__ double wave_sum(const double* __restrict__ col, const uint32_t n, const int lane) {
  double t = 0.0;
  for (uint32_t g = lane; g < n; g += 64) t += col[g];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) t += __shfl_xor(t, off, 64);
  return t;
}

// the advantage passes: PASS 0 writes a workgroup's (sum w, sum w adv), PASS 1 its sum w (adv - m)^2
template <int PASS>
__global__ __launch_bounds__(kGradBlock) void ppo_adv_kernel(const float* __restrict__ adv,
                                                             const uint8_t* __restrict__ live,
                                                             const int64_t* __restrict__ index, const int64_t row_base,
                                                             const uint64_t rows, const uint64_t samples,
                                                             double* __restrict__ prep) {
  __shared__ double red[2][kGradWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t tile_index = blockIdx.x;  // (the workgroup: a strided share of the samples; no state tiles here)
  double mean = 0.0;
  if constexpr (PASS == 1) {
    const double count = wave_sum(prep, gridDim.x, lane);
    mean = wave_sum(prep + kPrepMaxGroups, gridDim.x, lane) / (count > 1.0 ? count : 1.0);
  }
  double t0 = 0.0, t1 = 0.0;
  const uint64_t step = (uint64_t)gridDim.x * kGradBlock;
  for (uint64_t s = (uint64_t)tile_index * kGradBlock + tid; s < samples; s += step) {
    const int64_t i = sample_row(index, row_base, rows, samples, s);
    if (i < 0 || (live != nullptr && live[i] == 0)) continue;
    const double a = (double)adv[i];
    if constexpr (PASS == 0) {
      t0 += 1.0;
      t1 += a;
    } else {
      const double d = a - mean;
      t0 += d * d;
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    t0 += __shfl_xor(t0, off, 64);
    t1 += __shfl_xor(t1, off, 64);
  }
  if (lane == 0) {
    red[0][wave] = t0;
    red[1][wave] = t1;
  }
  __syncthreads();
  if (tid == 0) {
    double s0 = red[0][0], s1 = red[1][0];
#pragma unroll
    for (int w = 1; w < kGradWaves; ++w) {
      s0 += red[0][w];
      s1 += red[1][w];
    }
    if constexpr (PASS == 0) {
      prep[tile_index] = s0;
      prep[kPrepMaxGroups + tile_index] = s1;
    } else {
      prep[2 * kPrepMaxGroups + tile_index] = s0;
    }
  }
}

// a row's OBS floats with the widest loads its stride allows: 16 bytes for OBS = 12, 8 bytes for OBS in {2, 6, 10}
template <int OBS>
__device__ __forceinline__ void load_obs(const float* __restrict__ obs, const uint64_t row, double* o) {
  const float* src = obs + row * OBS;
  if constexpr (OBS % 4 == 0) {
#pragma unroll
    for (int v = 0; v < OBS / 4; ++v) {
      const float4 q = reinterpret_cast<const float4*>(src)[v];
      o[4 * v] = (double)q.x;
      o[4 * v + 1] = (double)q.y;
      o[4 * v + 2] = (double)q.z;
      o[4 * v + 3] = (double)q.w;
    }
  } else {
    static_assert(OBS % 2 == 0, "an even observation width");
#pragma unroll
    for (int v = 0; v < OBS / 2; ++v) {
      const float2 q = reinterpret_cast<const float2*>(src)[v];
      o[2 * v] = (double)q.x;
      o[2 * v + 1] = (double)q.y;
    }
  }
}

// what the rows share: the advantage's normalisation and the Gaussian's constants
template <int A>
struct RowConst {
  double W, mean, den, lo, hi, vf;
  double els[A], lsum, logc;
};

// One row of the policy head: from its extras x = [a[0..A), logp_old, adv, w] and mu, the cotangent g on mu; the
// log_std gradient's terms and the statistics go into sc[0..A) and sc[A + kSc..].  A dead row (w = 0) adds exact zeros.
template <int A>
__device__ __forceinline__ void policy_row(const RowConst<A>& k, const double* x, const double* mu, double* g,
                                           double* sc) {
  const bool on = x[A + 2] != 0.0;
  const double ahat = (x[A + 1] - k.mean) / k.den;
  double z[A], zz = 0.0;
#pragma unroll
  for (int c = 0; c < A; ++c) {
    z[c] = (x[c] - mu[c]) * k.els[c];
    zz += z[c] * z[c];
  }
  const double lp = -0.5 * zz - k.lsum - k.logc;
  const double ratio = exp(lp - x[A]);
  const bool clipped = (ahat > 0.0 && ratio > k.hi) || (ahat < 0.0 && ratio < k.lo);
  const double used = clipped ? fmin(fmax(ratio, k.lo), k.hi) : ratio;
  sc[A + kScSurr] += on ? ahat * used : 0.0;
  sc[A + kScKl] += on ? x[A] - lp : 0.0;
  sc[A + kScClip] += on && clipped ? 1.0 : 0.0;
  sc[A + kScMax] = fmax(sc[A + kScMax], on ? fabs(ratio - 1.0) : 0.0);
  const double dl = on && !clipped ? -(ahat * ratio) / k.W : 0.0;
#pragma unroll
  for (int c = 0; c < A; ++c) {
    g[c] = dl * z[c] * k.els[c];
    sc[c] += dl * (z[c] * z[c] - 1.0);
  }
}

// One row of the value head: x = [ret, w]
template <int A>
__device__ __forceinline__ void value_row(const RowConst<A>& k, const double* x, const double* v, double* g,
                                          double* sc) {
  const bool on = x[1] != 0.0;
  const double d = v[0] - x[0];
  sc[0] += on ? d * d : 0.0;
  g[0] = on ? k.vf * d / k.W : 0.0;
}

// HP: 0 = a linear network (one row per lane), else the hidden width rounded up (8, 16, 32 or 64 lanes per row)
template <int OBS, int A, int HP, int HEAD>
__global__ __launch_bounds__(kGradBlock) void ppo_grad_kernel(const PpoArgs a) {
  constexpr int NOUT = HEAD == kHeadPolicy ? A : 1;  // the network's outputs
  constexpr int LIVE = grad_live(HP), NACC = grad_nacc(OBS, NOUT, HP);
  [[maybe_unused]] constexpr int SLOTS = 64 / LIVE;        // (HP > 0) rows in flight per wavefront
  constexpr int NX = HEAD == kHeadPolicy ? A + 3 : 2;      // a row's extras: [a, logp_old, adv, w] or [ret, w]
  constexpr int NSC = HEAD == kHeadPolicy ? A + 4 : 1;     // scalar accumulators: [g_ls, the four statistics] or [sum d^2]
  static_assert(NSC <= kGradChunk, "the scalars are reduced in one pass");
  constexpr int ROW = OBS + NX;            // float64 values of a staged row
  constexpr int STAGE = HP == 0 ? 0 : kGradWaves * 64 * ROW;
  __shared__ __attribute__((aligned(16))) double smem[STAGE > kGradRed ? STAGE : kGradRed];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t tile_index = blockIdx.x;  // (the workgroup: its share of the sample tiles, its partial; no state tiles here)
  [[maybe_unused]] double* const rd = smem + wave * 64 * ROW;  // the wavefront's tile: [64][ROW] float64
  const int H = a.hidden;
  const float* __restrict__ params = a.params;

  // ---- what the rows share: W, m, sd from the advantage passes' partials, the same bits in every wavefront ----
  RowConst<A> k;
  {
    const double count = wave_sum(a.prep, a.prep_groups, lane);
    k.W = count > 1.0 ? count : 1.0;
    k.mean = 0.0;
    k.den = 1.0;
    if (HEAD == kHeadPolicy && a.normalize != 0) {
      k.mean = wave_sum(a.prep + kPrepMaxGroups, a.prep_groups, lane) / k.W;
      k.den = sqrt(wave_sum(a.prep + 2 * kPrepMaxGroups, a.prep_groups, lane) / k.W) + 1e-8;
    }
    k.lo = 1.0 - a.clip;
    k.hi = 1.0 + a.clip;
    k.vf = a.vf_coef;
    k.lsum = 0.0;
#pragma unroll
    for (int c = 0; c < A; ++c) {
      const double ls = HEAD == kHeadPolicy ? (double)a.log_std[c] : 0.0;
      k.els[c] = HEAD == kHeadPolicy ? exp(-ls) : 1.0;
      k.lsum += ls;
    }
    k.logc = 0.5 * A * 1.8378770664093453;  // ln(2 pi)
  }

  // lane (s, j)'s weights in float64 (mlp_grad_kit.h), and b2 for the forward; its sums
  [[maybe_unused]] const int j = HP == 0 ? 0 : lane & (LIVE - 1), s = HP == 0 ? 0 : lane / LIVE;
  [[maybe_unused]] double w1[OBS], b1, w2[NOUT];
  double b2[NOUT];
  grad_lane_weights<OBS, NOUT, HP>(params, H, j, w1, b1, w2);
#pragma unroll
  for (int c = 0; c < NOUT; ++c) b2[c] = (double)params[HP == 0 ? NOUT * OBS + c : mlp_layout(OBS, NOUT, H).b2 + c];
  double acc[NACC], sc[NSC];
#pragma unroll
  for (int q = 0; q < NACC; ++q) acc[q] = 0.0;
#pragma unroll
  for (int q = 0; q < NSC; ++q) sc[q] = 0.0;

  const uint64_t tiles = (a.samples + 63) / 64;
  const uint64_t first = (uint64_t)tile_index * a.tiles_per_group;
  const uint64_t last = first + a.tiles_per_group < tiles ? first + a.tiles_per_group : tiles;
#pragma clang loop unroll(disable)
  for (uint64_t tile = first + wave; tile < last; tile += kGradWaves) {
    // ---- lane l gathers sample l's row (64-bit offsets: the tapes pass 4 GiB); a sample past the end, out of range or
    // dead is a row of zeros with w = 0 and adds zeros ----
    const int64_t i = sample_row(a.index, a.row_base, a.rows, a.samples, tile * 64 + lane);
    double o[OBS], x[NX];
#pragma unroll
    for (int v = 0; v < OBS; ++v) o[v] = 0.0;
#pragma unroll
    for (int v = 0; v < NX; ++v) x[v] = 0.0;
    if (i >= 0 && (a.live == nullptr || a.live[i] != 0)) {
      load_obs<OBS>(a.obs, (uint64_t)i, o);
      if constexpr (HEAD == kHeadPolicy) {
#pragma unroll
        for (int c = 0; c < A; ++c) x[c] = (double)a.actions[(uint64_t)i * A + c];
        x[A] = (double)a.logp[i];
        x[A + 1] = (double)a.adv[i];
        x[A + 2] = 1.0;
      } else {
        x[0] = (double)a.ret[i];
        x[1] = 1.0;
      }
    }
    if constexpr (HP == 0) {  // lane = row: out[c] an fma chain from the bias in index order
      double out[NOUT], g[NOUT];
#pragma unroll
      for (int c = 0; c < NOUT; ++c) {
        out[c] = b2[c];
#pragma unroll
        for (int v = 0; v < OBS; ++v) out[c] = fma((double)params[c * OBS + v], o[v], out[c]);
      }
      if constexpr (HEAD == kHeadPolicy)
        policy_row<A>(k, x, out, g, sc);
      else
        value_row<A>(k, x, out, g, sc);
#pragma unroll
      for (int c = 0; c < NOUT; ++c) {
#pragma unroll
        for (int v = 0; v < OBS; ++v) acc[c * OBS + v] = fma(g[c], o[v], acc[c * OBS + v]);
        acc[NOUT * OBS + c] += g[c];
      }
    } else {
#pragma unroll
      for (int v = 0; v < OBS; ++v) rd[lane * ROW + v] = o[v];
#pragma unroll
      for (int v = 0; v < NX; ++v) rd[lane * ROW + OBS + v] = x[v];
      wave_sync();
#pragma clang loop unroll(disable)
      for (int it = 0; it < LIVE; ++it) {  // 64 / SLOTS rows per slot
        const double* row = rd + (it * SLOTS + s) * ROW;
        double ro[OBS], rx[NX];
#pragma unroll
        for (int v = 0; v < OBS; ++v) ro[v] = row[v];
#pragma unroll
        for (int v = 0; v < NX; ++v) rx[v] = row[OBS + v];
        double pre = b1;
#pragma unroll
        for (int v = 0; v < OBS; ++v) pre = fma(w1[v], ro[v], pre);
        const double h = tanh(pre);
        // the outputs: the bias plus a butterfly over the slot's HP lanes (idle lanes hold zeros), every lane alike
        double out[NOUT], g[NOUT];
#pragma unroll
        for (int c = 0; c < NOUT; ++c) {
          double t = w2[c] * h;
#pragma unroll
          for (int off = LIVE / 2; off >= 1; off >>= 1) t += __shfl_xor(t, off, 64);
          out[c] = b2[c] + t;
        }
        if constexpr (HEAD == kHeadPolicy)
          policy_row<A>(k, rx, out, g, sc);
        else
          value_row<A>(k, rx, out, g, sc);
        grad_unit_accumulate<OBS, NOUT>(w2, ro, g, h, acc);
      }
      wave_sync();  // (the next tile overwrites these rows)
    }
  }

  // ---- the workgroup's partial, this head's columns of it ----
  double* const red = smem;  // [kGradWaves][kGradChunk][64]
  double* const part = a.partials + (size_t)tile_index * a.stride;
  grad_partial_reduce<OBS, NOUT, HP>(acc, red, part + a.offset, H);
  // ---- the scalars, which every lane of a slot holds alike: lane j = 0 of each slot counts, the same two levels; the
  // largest |rho - 1| is a maximum, not a sum ----
  __syncthreads();
#pragma unroll
  for (int q = 0; q < NSC; ++q) {
    const bool is_max = HEAD == kHeadPolicy && q == A + kScMax;
    double v = sc[q];
#pragma unroll
    for (int off = 32; off >= LIVE; off >>= 1) {
      const double u = __shfl_down(v, off, 64);
      v = is_max ? fmax(v, u) : v + u;
    }
    if (lane == 0) red[(wave * kGradChunk + q) * 64] = v;
  }
  __syncthreads();
  if (tid < NSC) {
    const bool is_max = HEAD == kHeadPolicy && tid == A + kScMax;
    double t = red[tid * 64];
#pragma unroll
    for (int w = 1; w < kGradWaves; ++w) {
      const double u = red[(w * kGradChunk + tid) * 64];
      t = is_max ? fmax(t, u) : t + u;
    }
    if constexpr (HEAD == kHeadPolicy)
      part[tid < A ? a.ls_offset + tid : a.scal_offset + (tid - A)] = t;
    else
      part[a.scal_offset + kScValue] = t;
  }
}

// grad[p] = the sum of column p's partials in a fixed order (mlp_grad_sum_kernel's: four wavefronts take a quarter of the
// workgroups each, in index order, and the quarters are added in order), less ent_coef on log_std's columns; the last
// workgroup does the same for the scalar columns and writes the statistics
__global__ __launch_bounds__(kGradBlock) void ppo_grad_sum_kernel(const double* __restrict__ partials,
                                                                  const uint32_t groups, const uint32_t stride,
                                                                  const uint32_t ngrad, const uint32_t ls_offset,
                                                                  const uint32_t acts, const uint32_t has_critic,
                                                                  const float* __restrict__ log_std,
                                                                  const double* __restrict__ prep,
                                                                  const uint32_t prep_groups, const double vf_coef,
                                                                  const double ent_coef, double* __restrict__ grad,
                                                                  double* __restrict__ stats) {
  __shared__ double quarter[kGradWaves][64];
  const uint32_t tile_index = blockIdx.x;  // (elementwise: 64 columns per workgroup, no state tiles touched)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool scalars = tile_index == gridDim.x - 1;
  const uint32_t p = scalars ? ngrad + lane : tile_index * 64 + lane;
  const bool mine = scalars ? (uint32_t)lane < kScalars && (lane != kScValue || has_critic != 0) && lane <= kScValue
                            : p < ngrad;
  const bool is_max = scalars && lane == kScMax;
  const double count = wave_sum(prep, prep_groups, lane);
  double t = 0.0;
  if (mine) {
    const uint32_t per = (groups + kGradWaves - 1) / kGradWaves;
    const uint32_t g0 = wave * per, g1 = g0 + per < groups ? g0 + per : groups;
#pragma unroll 16
    for (uint32_t g = g0; g < g1; ++g) {
      const double u = partials[(size_t)g * stride + p];
      t = is_max ? fmax(t, u) : t + u;
    }
  }
  quarter[wave][lane] = t;
  __syncthreads();
  if (wave != 0) return;
  double sum = quarter[0][lane];
#pragma unroll
  for (int w = 1; w < kGradWaves; ++w) sum = is_max ? fmax(sum, quarter[w][lane]) : sum + quarter[w][lane];
  if (!scalars) {
    if (p < ngrad) grad[p] = p >= ls_offset ? sum - ent_coef : sum;
    return;
  }
  quarter[0][lane] = sum;
  wave_sync();
  if (lane == 0) {
    const double W = count > 1.0 ? count : 1.0;
    double entropy = 0.0;
    for (uint32_t c = 0; c < acts; ++c) entropy += (double)log_std[c];
    entropy += 0.5 * acts * (1.0 + 1.8378770664093453);
    const double l_pi = -quarter[0][kScSurr] / W, l_v = 0.5 * quarter[0][kScValue] / W;
    stats[0] = count;
    stats[1] = l_pi;
    stats[2] = l_v;
    stats[3] = entropy;
    stats[4] = l_pi + vf_coef * l_v - ent_coef * entropy;
    stats[5] = quarter[0][kScKl] / W;
    stats[6] = quarter[0][kScClip] / W;
    stats[7] = quarter[0][kScMax];
  }
}

template <int OBS, int A, int HEAD>
hipError_t head_launch(const PpoArgs& a, uint32_t groups, hipStream_t stream) {
  return for_grad_width(a.hidden, [&](auto hp) {
    hipLaunchKernelGGL((ppo_grad_kernel<OBS, A, hp(), HEAD>), dim3(groups), dim3(kGradBlock), 0, stream, a);
    return hipGetLastError();
  });
}

template <int OBS, int A>
hipError_t ppo_launch(const cs_ppo_grad_io& io, double* scratch, hipStream_t stream) {
  const uint64_t B = (uint64_t)io.num_samples, R = (uint64_t)io.num_rows;
  const bool critic = io.critic_dev != nullptr;
  const uint32_t P = mlp_param_count(OBS, A, io.hidden), Pv = critic ? mlp_param_count(OBS, 1, io.critic_hidden) : 0u;
  const uint32_t ngrad = P + Pv + A, stride = ngrad + kScalars;
  double* const partials = scratch;
  double* const prep = scratch + kPartialDoubles;
  // the advantage passes: sum w and sum w adv, then (normalize) the centred second moment
  const uint64_t want = (B + kGradBlock - 1) / kGradBlock;
  const uint32_t prep_groups = (uint32_t)(want < kPrepMaxGroups ? want : kPrepMaxGroups);
  hipLaunchKernelGGL(ppo_adv_kernel<0>, dim3(prep_groups), dim3(kGradBlock), 0, stream, io.advantages_dev, io.live_dev,
                     io.index_dev, io.row_base, R, B, prep);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (io.normalize != 0) {
    hipLaunchKernelGGL(ppo_adv_kernel<1>, dim3(prep_groups), dim3(kGradBlock), 0, stream, io.advantages_dev,
                       io.live_dev, io.index_dev, io.row_base, R, B, prep);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  const GradSplit split = grad_split(B);
  const uint32_t groups = split.groups;
  PpoArgs a{};
  a.params = io.actor_dev;
  a.log_std = io.log_std_dev;
  a.obs = io.obs_dev;
  a.actions = io.actions_dev;
  a.logp = io.logp_dev;
  a.adv = io.advantages_dev;
  a.ret = io.returns_dev;
  a.live = io.live_dev;
  a.index = io.index_dev;
  a.row_base = io.row_base;
  a.rows = R;
  a.samples = B;
  a.prep = prep;
  a.partials = partials;
  a.clip = io.clip;
  a.vf_coef = io.vf_coef;
  a.hidden = io.hidden;
  a.prep_groups = prep_groups;
  a.normalize = io.normalize;
  a.tiles_per_group = split.per_group;
  a.stride = stride;
  a.offset = 0;
  a.ls_offset = P + Pv;
  a.scal_offset = ngrad;
  if ((e = head_launch<OBS, A, kHeadPolicy>(a, groups, stream)) != hipSuccess) return e;
  if (critic) {
    a.params = io.critic_dev;
    a.hidden = io.critic_hidden;
    a.offset = P;
    if ((e = head_launch<OBS, A, kHeadValue>(a, groups, stream)) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(ppo_grad_sum_kernel, dim3((ngrad + 63) / 64 + 1), dim3(kGradBlock), 0, stream, partials, groups,
                     stride, ngrad, P + Pv, (uint32_t)A, critic ? 1u : 0u, io.log_std_dev, prep, prep_groups,
                     io.vf_coef, io.ent_coef, io.grad_dev, io.stats_dev);
  return hipGetLastError();
}

hipError_t launch_ppo_grad(int task, const cs_ppo_grad_io& io, double* scratch, hipStream_t stream) {
  return for_task_shape(task, [&](auto obs, auto act) { return ppo_launch<obs(), act()>(io, scratch, stream); });
}

bool misaligned(const void* p, uintptr_t to) { return (reinterpret_cast<uintptr_t>(p) & (to - 1)) != 0; }

// the argument block, checked before the context
int check_ppo_io(const cs_ppo_grad_io* io, const std::string& w) {
  if (io == nullptr) return report_error(CS_ERR_ARG, (w + ": null pio").c_str());
  if (io->struct_size != sizeof(cs_ppo_grad_io))
    return report_error(CS_ERR_ABI, (w + ": pio->struct_size " + std::to_string(io->struct_size) + " != " +
                                     std::to_string(sizeof(cs_ppo_grad_io)) + " (sizeof(cs_ppo_grad_io))").c_str());
  if (int rc_ = check_hidden(w.c_str(), "hidden", io->hidden)) return rc_;
  if (int rc_ = check_hidden(w.c_str(), "critic_hidden", io->critic_hidden)) return rc_;
  if (io->normalize > 1u) return report_error(CS_ERR_ARG, (w + ": normalize must be 0 or 1").c_str());
  if (io->num_rows < 1) return report_error(CS_ERR_ARG, (w + ": num_rows must be >= 1").c_str());
  if (io->num_samples < 1) return report_error(CS_ERR_ARG, (w + ": num_samples must be >= 1").c_str());
  if (!std::isfinite(io->clip) || !(io->clip > 0.0))
    return report_error(CS_ERR_ARG, (w + ": clip must be finite and > 0").c_str());
  if (!std::isfinite(io->vf_coef)) return report_error(CS_ERR_ARG, (w + ": vf_coef must be finite").c_str());
  if (!std::isfinite(io->ent_coef)) return report_error(CS_ERR_ARG, (w + ": ent_coef must be finite").c_str());
  if (io->actor_dev == nullptr) return report_error(CS_ERR_ARG, (w + ": actor_dev is required").c_str());
  if (io->log_std_dev == nullptr) return report_error(CS_ERR_ARG, (w + ": log_std_dev is required").c_str());
  if (io->obs_dev == nullptr) return report_error(CS_ERR_ARG, (w + ": obs_dev is required").c_str());
  if (io->actions_dev == nullptr) return report_error(CS_ERR_ARG, (w + ": actions_dev is required").c_str());
  if (io->logp_dev == nullptr) return report_error(CS_ERR_ARG, (w + ": logp_dev is required").c_str());
  if (io->advantages_dev == nullptr) return report_error(CS_ERR_ARG, (w + ": advantages_dev is required").c_str());
  if (io->critic_dev != nullptr && io->returns_dev == nullptr)
    return report_error(CS_ERR_ARG, (w + ": returns_dev is required with critic_dev").c_str());
  if (io->grad_dev == nullptr) return report_error(CS_ERR_ARG, (w + ": grad_dev is required").c_str());
  if (io->stats_dev == nullptr) return report_error(CS_ERR_ARG, (w + ": stats_dev is required").c_str());
  if (io->index_dev == nullptr && (io->row_base < 0 || io->row_base > io->num_rows - io->num_samples))
    return report_error(CS_ERR_ARG, (w + ": without index_dev, rows row_base .. row_base + num_samples - 1 must lie in "
                                         "[0, num_rows)").c_str());
  if (misaligned(io->obs_dev, 16)) return report_error(CS_ERR_ARG, (w + ": obs_dev must be 16-byte aligned").c_str());
  if (misaligned(io->index_dev, 8) || misaligned(io->grad_dev, 8) || misaligned(io->stats_dev, 8))
    return report_error(CS_ERR_ARG, (w + ": index_dev, grad_dev and stats_dev must be 8-byte aligned").c_str());
  const void* floats[] = {io->actor_dev, io->critic_dev,     io->log_std_dev, io->actions_dev,
                          io->logp_dev,  io->advantages_dev, io->returns_dev};
  for (const void* p : floats)
    if (misaligned(p, 4)) return report_error(CS_ERR_ARG, (w + ": every float32 pointer must be 4-byte aligned").c_str());
  return CS_OK;
}

}  // namespace
}  // namespace cs

extern "C" int cs_ppo_grad(cs_ctx* ctx, const cs_ppo_grad_io* pio, void* stream) {
  const std::string w("cs_ppo_grad");
  if (int rc_ = cs::check_ppo_io(pio, w)) return rc_;
  cs::ContextView v;
  if (int rc_ = cs::enter_context(ctx, w.c_str(), stream, &v)) return rc_;  // (refuses an open served session)
  double* scratch = nullptr;
  if (int rc_ = cs::grad_scratch(ctx, cs::kScratchPpoGrad, w.c_str(), stream, cs::kScratchBytes, &scratch)) return rc_;
  const hipError_t e = cs::launch_ppo_grad(v.task, *pio, scratch, (hipStream_t)stream);
  if (e != hipSuccess) return cs::report_hip(e, (w + ": kernel launch").c_str());
  return CS_OK;
}
