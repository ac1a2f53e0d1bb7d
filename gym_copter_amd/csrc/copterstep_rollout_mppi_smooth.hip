// copterstep_rollout_mppi_smooth.hip -- MPPI with smooth knot noise and a per-env temperature on gfx950
// (cs_rollout_mppi_costs_ex / cs_rollout_mppi_update_ex / cs_rollout_mppi_temperature, include/copterstep.h): the
// kernels of copterstep_rollout_mppi.hip with the blended knot draws of mppi_noise.h as the action source, the update
// with a temperature per env, and the bisection that solves that temperature for a target effective sample size.
// DESIGN.md section 15.
//
// Costs: the white kernel's lane, grid and loop.  The two knot draws of the A components stay in lane-private LDS columns
// and are made again only at the steps where the knot number changes (a uniform branch: the table is the launch's); a
// knot that moves on by one takes over its neighbour's draws, so a hold of h steps costs A Philox calls per h steps.  Update: the
// white kernel's, with the knot pair of step k0 drawn per sample (uniform per workgroup) and lambda read per lane.
// Temperature: one lane per env, float64, 51 passes over the env's cost column.  What the two files' kernels have in
// common word for word -- a step's cost terms, the update's body, the column's finite minimum -- is rollout_mppi.h's.
#include "copterstep_jacobian.h"

// the samples' states must be cs_rollout_states' bit for bit; the cost's float64 arithmetic is not contracted either
#pragma clang fp contract(off)

#include "dev_tile.h"
#include "dev_codec.h"
#include "dev_math.h"
#include "dev_physics.h"
#include "dev_task.h"
#include "jacobian_tangents.h"
#include "rollout_adjoint.h"
#include "rollout_step.h"
#include "mppi_noise.h"
#include "dev_launch.h"
#include "rollout_mppi.h"

namespace cs {
namespace {

// cs_rollout_mppi_ext, checked
struct MppiExt {
  const uint32_t* knot;  // [K] or nullptr: knot k, weights (1, 0)
  const float* weight;   // [K,2]
  const double* lam;     // [N] or nullptr: MppiArgs::lambda
  double target, lam_min, lam_max;
  double* lam_out;
  double* ess_out;
};

// the knot number and the two weights of step k = k0 + 1 (uniform: per-step loads, as the cost's matrices are read)
__device__ __forceinline__ void knot_of_step(const uint32_t* table, const float* weight, uint32_t k0, uint32_t& knot,
                                             float& w0, float& w1) {
  if (table != nullptr) {
    knot = table[k0];
    w0 = weight[2 * (size_t)k0];
    w1 = weight[2 * (size_t)k0 + 1];
  } else {
    knot = k0 + 1u;
    w0 = 1.0f;
    w1 = 0.0f;
  }
}

template <int TASK, int MODE>
__global__ __launch_bounds__(kBlock, 2) void rollout_mppi_smooth_costs_kernel(const DevConst c, const DevState s,
                                                                           const cs_rollout_io io, const MppiArgs m,
                                                                           const uint32_t* knot_table,
                                                                           const float* knot_weight) {
  constexpr int A = task_act_dim(TASK);
  __shared__ __attribute__((aligned(16))) double wts[2 * tri_size(12) + tri_size(A)];  // Q, Q at the last step, R
  // The two knot draws of the A components, a lane-private column each (no barrier: a lane reads what it wrote).  Not in
  // registers: the 2 A values held across the step put the 3D instantiations 120-200 B per lane into scratch (the white
  // kernel stands at 214-253 VGPRs of 256), and the LDS has room: 2 KiB of the 160 KiB at 8 workgroups per CU.
  __shared__ float draws[2 * A * kBlock];
  const int lane = threadIdx.x;
  const uint32_t tile_index = blockIdx.x, p = blockIdx.y;  // tile t -> workgroup t in x; the sample in y
  stage_triangle<12>(m.Q, wts, lane);
  stage_triangle<12>(m.Qf, wts + tri_size(12), lane);
  stage_triangle<A>(m.R, wts + 2 * tri_size(12), lane);
  __syncthreads();
  const uint32_t i = tile_index * kBlock + threadIdx.x;
  const uint32_t n = s.n;
  const bool valid = i < n;
  const uint32_t ii = valid ? i : 0u;  // (padding lanes roll env 0's actions out and store nothing)

  Coef q = uniform_coef(c);
  if (s.veh != nullptr) q = load_coef(s.veh, s.veh_stride, ii);
  // the start point, decoded as rollout_forward decodes it
  using TILE = TileIO<MODE>;
  const TILE tile(s, tile_index, lane);
  Env<MODE> e;
  unpack_env<MODE, TILE>(c, tile.load_group(0), tile.load_group(1), tile.load_group(2), tile.load_group(3), e);
  resolve_episode<MODE>(c, tile, e);
  double px, py, pz;
  rollout_start<TASK, MODE>(c, q, io, tile, i, n, valid, e, px, py, pz);

  const uint32_t gid = c.id_lo + ii;
  const float* abar = io.actions_dev + (size_t)ii * A;
  const size_t astep = (size_t)n * A;
  const double* xr = m.xref + (size_t)ii * 12;
  const size_t xstep = m.xref_steps ? (size_t)n * 12 : 0;
  const int K = io.num_steps;
  double S = 0.0;
  // the draws of knot `held` (slot 0) and of knot held + 1 (slot 1) are in draws[slot][j][lane]; 0 is no knot's number
  uint32_t held = 0u;
#pragma clang loop unroll(disable)
  for (int k = 0; k < K; ++k) {
    // the sample's action: abar + sigma eps~ in float32, one multiply and one add; sample 0 is abar itself
    const float4 ab = load_action_at<TASK>(abar);
    abar += astep;
    const float abv[4] = {ab.x, ab.y, ab.z, ab.w};
    float a[A];
#pragma unroll
    for (int j = 0; j < A; ++j) a[j] = abv[j];
    // sigma and a_ref are read per step, as the table and the cost's matrices are: held across the loop, their 3 A
    // registers and the 2 A of the knot draws spill
    const float* sgp = m.sigma;
    const double* arp = m.aref;
    asm volatile("" : "+s"(sgp), "+s"(arp));
    if (p != 0u) {  // (uniform: the sample is the workgroup's)
      uint32_t knot;
      float w0, w1;
      knot_of_step(knot_table, knot_weight, (uint32_t)k, knot, w0, w1);
      // (the column's address is made opaque per step: the 2 A values would otherwise be promoted to registers)
      float* col = draws + lane;
      asm volatile("" : "+v"(col));
      if (knot != held) {  // (uniform: the table is the launch's)
        // slot 1 moves to slot 0 and knot mk + 1 is drawn into slot 1: once, with mk = knot, where the knot moved on by
        // one -- A Philox calls per hold -- else for mk = knot - 1 and knot (mk = 0 draws knot 1)
#pragma clang loop unroll(disable) vectorize(disable)
        for (uint32_t mk = knot == held + 1u && held != 0u ? knot : knot - 1u; mk <= knot; ++mk) {
#pragma unroll
          for (int j = 0; j < A; ++j) {
            col[j * kBlock] = col[(A + j) * kBlock];
            col[(A + j) * kBlock] = mppi_noise(m.key, gid, m.nonce, mk + 1u, p, (uint32_t)j);
          }
        }
        held = knot;
      }
#pragma unroll
      for (int j = 0; j < A; ++j) {
        const float da = sgp[j] * mppi_knot_blend(w0, col[j * kBlock], w1, col[(A + j) * kBlock]);
        a[j] = abv[j] + da;
      }
    }
    const bool resetting = e.reset_pending;
    double reward;
    bool term, trunc;
    rollout_step<TASK, MODE>(c, q, e, fan_out<A>(a), px, py, pz, reward, term, trunc);
    next_perturbation<MODE>(c, q, tile, i, resetting, e, px, py, pz);
    mppi_step_cost<A>(
        wts, xr, xstep, e.x, a, [&](int j) { return arp != nullptr ? arp[j] : 0.0; }, k == K - 1, m.wr, reward, S);
  }
  if (valid) m.costs[(size_t)p * n + i] = S;  // (64-bit: P x N doubles pass 4 GiB)
}

template <int TASK>
__global__ __launch_bounds__(kBlock) void rollout_mppi_smooth_update_kernel(uint32_t n, uint32_t id_lo,
                                                                            const float* abar_dev, const MppiArgs m,
                                                                            const MppiExt x) {
  constexpr int A = task_act_dim(TASK);
  const uint32_t tile = blockIdx.x, k0 = blockIdx.y;  // tile t -> workgroup t in x; step k0 + 1 in y
  const uint32_t i = tile * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t gid = id_lo + i;
  uint32_t knot;
  float w0, w1;
  knot_of_step(x.knot, x.weight, k0, knot, w0, w1);
  const double lambda = x.lam != nullptr ? x.lam[i] : m.lambda;
  const bool warm = lambda > 0.0 && finite64(lambda);  // (false for a NaN)
  mppi_update_lane<A>(n, i, k0, abar_dev, m, lambda, warm, [&](uint32_t p, uint32_t j) {
    return mppi_noise_smooth(m.key, gid, m.nonce, knot, w0, w1, p, j);
  });
}

// E(lambda) = (sum w)^2 / sum w^2 over the finite costs of a column whose minimum finite cost is beta
__device__ __forceinline__ double effective_size(const double* col, uint32_t n, uint32_t P, double beta, double lambda) {
  double eta = 0.0, eta2 = 0.0;
#pragma clang loop unroll(disable)
  for (uint32_t p = 0; p < P; ++p) {
    const double v = col[(size_t)p * n];
    const double w = finite64(v) ? exp(-(v - beta) / lambda) : 0.0;
    eta += w;
    eta2 += w * w;
  }
  return (eta * eta) / eta2;  // (eta >= 1: the best sample's weight is exp(0))
}

// lambda per env for a target effective sample size: 48 bisections of ln lambda; lane = env, no LDS, float64
__global__ __launch_bounds__(kBlock, 8) void mppi_temperature_kernel(uint32_t n, uint32_t P, const double* costs,
                                                                    const MppiExt x) {
  const uint32_t tile = blockIdx.x;  // tile t -> workgroup t
  const uint32_t i = tile * kBlock + threadIdx.x;
  if (i >= n) return;
  const double* col = costs + i;
  const auto [any, beta] = column_min(col, n, P);
  double lambda = x.lam_max, E = 0.0;
  if (any) {
    E = effective_size(col, n, P, beta, x.lam_max);
    if (!(E < x.target)) {
      const double at_min = effective_size(col, n, P, beta, x.lam_min);
      if (at_min >= x.target) {
        lambda = x.lam_min;
        E = at_min;
      } else {
        double lo = log(x.lam_min), hi = log(x.lam_max);
#pragma clang loop unroll(disable)
        for (int it = 0; it < 48; ++it) {
          const double u = 0.5 * (lo + hi);
          if (effective_size(col, n, P, beta, exp(u)) < x.target)
            lo = u;
          else
            hi = u;
        }
        lambda = exp(hi);
        E = effective_size(col, n, P, beta, lambda);
      }
    }
  }
  x.lam_out[i] = lambda;
  if (x.ess_out != nullptr) x.ess_out[i] = E;
}

template <int TASK, int MODE>
hipError_t mppi_smooth_costs_t(const DevConst& c, const DevState& s, const cs_rollout_io& io, const MppiArgs& m,
                               const MppiExt& x, hipStream_t stream) {
  hipLaunchKernelGGL((rollout_mppi_smooth_costs_kernel<TASK, MODE>), dim3(grid_for(s.n), m.samples), dim3(kBlock), 0,
                     stream, c, s, io, m, x.knot, x.weight);
  return hipGetLastError();
}

template <int TASK, int MODE>
hipError_t mppi_smooth_update_t(const DevConst& c, const DevState& s, const cs_rollout_io& io, const MppiArgs& m,
                                const MppiExt& x, hipStream_t stream) {
  hipLaunchKernelGGL((rollout_mppi_smooth_update_kernel<TASK>), dim3(grid_for(s.n), (uint32_t)io.num_steps),
                     dim3(kBlock), 0, stream, s.n, c.id_lo, io.actions_dev, m, x);
  return hipGetLastError();
}

hipError_t launch_mppi_smooth_costs(int task, int mode, const DevConst& c, const DevState& s, const cs_rollout_io& io,
                                    const MppiArgs& m, const MppiExt& x, hipStream_t stream) {
  CS_DISPATCH(mppi_smooth_costs_t, c, s, io, m, x, stream)
}

hipError_t launch_mppi_smooth_update(int task, int mode, const DevConst& c, const DevState& s, const cs_rollout_io& io,
                                     const MppiArgs& m, const MppiExt& x, hipStream_t stream) {
  CS_DISPATCH(mppi_smooth_update_t, c, s, io, m, x, stream)
}

// the checks of the second block that the three entry points share, made before the context
int check_mppi_ext(const cs_rollout_mppi_ext* ext, const std::string& w) {
  if (ext == nullptr) return report_error(CS_ERR_ARG, (w + ": null ext").c_str());
  if (ext->struct_size != sizeof(cs_rollout_mppi_ext))
    return report_error(CS_ERR_ABI, (w + ": ext->struct_size " + std::to_string(ext->struct_size) + " != " +
                                     std::to_string(sizeof(cs_rollout_mppi_ext)) + " (sizeof(cs_rollout_mppi_ext))").c_str());
  if (ext->reserved_ != 0u) return report_error(CS_ERR_ARG, (w + ": ext->reserved_ must be 0").c_str());
  if ((ext->knot_dev == nullptr) != (ext->knot_weights_dev == nullptr))
    return report_error(CS_ERR_ARG, (w + ": knot_dev and knot_weights_dev go together (both NULL: white noise)").c_str());
  return CS_OK;
}

MppiExt mppi_ext(const cs_rollout_mppi_ext& o) {
  return MppiExt{o.knot_dev, o.knot_weights_dev, o.lam_dev, o.ess_target, o.lam_min, o.lam_max, o.lam_out_dev,
                 o.ess_out_dev};
}

}  // namespace
}  // namespace cs

extern "C" int cs_rollout_mppi_costs_ex(cs_ctx* ctx, const cs_rollout_io* io, const cs_rollout_mppi_io* mio,
                                        const cs_rollout_mppi_ext* ext, void* stream) {
  const char* who = "cs_rollout_mppi_costs_ex";
  if (int rc_ = cs::check_rollout_io(io, who, false)) return rc_;
  if (int rc_ = cs::check_mppi_io(mio, who)) return rc_;
  if (int rc_ = cs::check_mppi_costs_io(mio, who)) return rc_;
  if (int rc_ = cs::check_mppi_ext(ext, who)) return rc_;
  cs::ContextView v;
  if (int rc_ = cs::enter_context(ctx, who, stream, &v)) return rc_;
  const cs::MppiArgs m = cs::mppi_args(ctx, *mio);
  const hipError_t e = cs::launch_mppi_smooth_costs(v.task, v.mode, *v.c, *v.s, *io, m, cs::mppi_ext(*ext),
                                                    (hipStream_t)stream);
  if (e != hipSuccess) return cs::report_hip(e, "cs_rollout_mppi_costs_ex: kernel launch");
  return cs::launch_mppi_best(m, v.s->n, (hipStream_t)stream, who);
}

extern "C" int cs_rollout_mppi_update_ex(cs_ctx* ctx, const cs_rollout_io* io, const cs_rollout_mppi_io* mio,
                                         const cs_rollout_mppi_ext* ext, void* stream) {
  const char* who = "cs_rollout_mppi_update_ex";
  if (int rc_ = cs::check_rollout_io(io, who, false)) return rc_;
  if (int rc_ = cs::check_mppi_io(mio, who)) return rc_;
  if (int rc_ = cs::check_mppi_ext(ext, who)) return rc_;
  if (int rc_ = cs::check_mppi_update_io(io, mio, who, ext->lam_dev == nullptr)) return rc_;
  cs::ContextView v;
  if (int rc_ = cs::enter_context(ctx, who, stream, &v)) return rc_;
  const hipError_t e = cs::launch_mppi_smooth_update(v.task, v.mode, *v.c, *v.s, *io, cs::mppi_args(ctx, *mio),
                                                     cs::mppi_ext(*ext), (hipStream_t)stream);
  if (e != hipSuccess) return cs::report_hip(e, "cs_rollout_mppi_update_ex: kernel launch");
  return CS_OK;
}

extern "C" int cs_rollout_mppi_temperature(cs_ctx* ctx, const cs_rollout_mppi_io* mio, const cs_rollout_mppi_ext* ext,
                                           void* stream) {
  const char* who = "cs_rollout_mppi_temperature";
  if (int rc_ = cs::check_mppi_io(mio, who, false)) return rc_;
  if (int rc_ = cs::check_mppi_ext(ext, who)) return rc_;
  if (!(ext->ess_target >= 1.0) || !std::isfinite(ext->ess_target))
    return cs::report_error(CS_ERR_ARG, "cs_rollout_mppi_temperature: ess_target must be finite and >= 1");
  if (!(ext->lam_min > 0.0) || !(ext->lam_min < ext->lam_max) || !std::isfinite(ext->lam_max))
    return cs::report_error(CS_ERR_ARG, "cs_rollout_mppi_temperature: 0 < lam_min < lam_max, both finite, is required");
  if (ext->lam_out_dev == nullptr)
    return cs::report_error(CS_ERR_ARG, "cs_rollout_mppi_temperature: lam_out_dev is required");
  cs::ContextView v;
  if (int rc_ = cs::enter_context(ctx, who, stream, &v)) return rc_;
  hipLaunchKernelGGL(cs::mppi_temperature_kernel, dim3(cs::grid_for(v.s->n)), dim3(cs::kBlock), 0, (hipStream_t)stream,
                     v.s->n, (uint32_t)mio->num_samples, mio->costs_dev, cs::mppi_ext(*ext));
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return cs::report_hip(e, "cs_rollout_mppi_temperature: kernel launch");
  return CS_OK;
}
