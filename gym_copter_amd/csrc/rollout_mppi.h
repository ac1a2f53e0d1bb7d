// rollout_mppi.h -- what the MPPI translation units share (copterstep_rollout_mppi.hip: the white-noise kernels of
// DESIGN.md section 14; copterstep_rollout_mppi_smooth.hip: the knot-noise kernels and the temperature of section 15):
// the checked argument block, the cost's matrices in the LDS, the motor fan-out, a step's cost terms, the finite minimum
// of a cost column, the weighted update's body (the update rule exists here alone), the arg-min kernel with its launch,
// and the block checks.  Included after the device headers and mppi_noise.h, inside a translation unit that has set
// `#pragma clang fp contract(off)`; not a stand-alone header.
#pragma once

#include <cmath>
#include <string>

namespace cs {
namespace {

// cs_rollout_mppi_io, checked, with the noise key of the context's seed
struct MppiArgs {
  const float* sigma;
  const double* xref;
  const double* aref;
  const double* Q;
  const double* Qf;  // Q at the last step (== Q without a Q_final)
  const double* R;
  double* costs;
  int32_t* best;
  float* out;
  double* ess;
  double* cost_min;
  double lambda, wr;
  uint32_t key, nonce, samples, xref_steps;
};

__device__ __forceinline__ bool finite64(double v) { return fabs(v) <= 1.7976931348623157e308; }

// The cost's matrices in the LDS: the upper triangle of a symmetric D x D matrix, row-major (row i from tri_at(D, i)),
// its diagonal halved, so that 1/2 d^T M d = sum_i d_i (M'_ii d_i + sum_{j > i} M_ij d_j).  Every lane reads the same
// address (a broadcast).  Not through the scalar unit as cs_rollout_lqr's are: the step already holds every SGPR
// (DevConst), and the 78 values' loads, hoisted out of the step loop, spilled 110-250 SGPRs into the vector file.
constexpr int tri_at(int D, int i) { return i * D - i * (i - 1) / 2; }
constexpr int tri_size(int D) { return D * (D + 1) / 2; }

template <int D>
__device__ __forceinline__ void stage_triangle(const double* M, double* dst, int lane) {
#pragma clang loop unroll(disable)
  for (int idx = lane; idx < D * D; idx += kBlock) {
    const int i = idx / D, j = idx - i * D;
    if (j >= i) dst[tri_at(D, i) + (j - i)] = i == j ? 0.5 * M[idx] : M[idx];
  }
}

template <int D>
__device__ __forceinline__ double half_quadratic(const double* tri, const double (&d)[D]) {
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < D; ++i) {
    double t = tri[tri_at(D, i)] * d[i];
#pragma unroll
    for (int j = i + 1; j < D; ++j) t += tri[tri_at(D, i) + (j - i)] * d[j];
    s += d[i] * t;
  }
  return s;
}

// the task's motor fan-out of an action row, as load_action_at()
template <int A>
__device__ __forceinline__ float4 fan_out(const float (&a)[A]) {
  if constexpr (A == 4)
    return make_float4(a[0], a[1], a[2], a[3]);
  else if constexpr (A == 2)
    return make_float4(a[0], a[1], a[1], a[0]);
  else
    return make_float4(a[0], a[0], a[0], a[0]);
}

// One step's cost terms, each added to S on its own: 1/2 dx^T Q dx with dx = x - x_ref (xr: the lane's row, moved on by
// xstep for the next step; Q_final at the last step), 1/2 da^T R da with da = a - a_ref, and -wr reward.  wts: the
// kernel's staged triangles Q, Q at the last step, R.  aref(j): a_ref's component j, read where the kernel keeps it
// (registers in the white kernel, per step through the scalar unit in the knot-noise one), after the x_ref loads as the
// kernels had it: with da made by the caller before them the knot-noise cost kernel ran up to 1.5 % slower at one
// substep (profiles/forward_shared_refactor_ab.txt).
template <int A, class AREF>
__device__ __forceinline__ void mppi_step_cost(const double* wts, const double*& xr, size_t xstep,
                                               const double (&x)[12], const float (&a)[A], AREF aref, bool last,
                                               double wr, double reward, double& S) {
  double dx[12], da[A];
  const double2* xv = reinterpret_cast<const double2*>(xr);
  xr += xstep;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const double2 v = xv[j];
    dx[2 * j] = x[2 * j] - v.x;
    dx[2 * j + 1] = x[2 * j + 1] - v.y;
  }
#pragma unroll
  for (int j = 0; j < A; ++j) da[j] = (double)a[j] - aref(j);
  // (the address is made opaque per step: the 166 loop-invariant reads would otherwise be hoisted into registers)
  const double* w = wts;
  asm volatile("" : "+v"(w));
  S += half_quadratic<12>(last ? w + tri_size(12) : w, dx);
  S += half_quadratic<A>(w + 2 * tri_size(12), da);
  S -= wr * reward;
}

// The finite minimum of a lane's cost column (col = costs + i of [P,N]): any = one of the P costs is finite, beta = the
// least of those
struct ColumnMin {
  bool any;
  double beta;
};

__device__ __forceinline__ ColumnMin column_min(const double* col, uint32_t n, uint32_t P) {
  ColumnMin r{false, 0.0};
#pragma clang loop unroll(disable)
  for (uint32_t p = 0; p < P; ++p) {
    const double v = col[(size_t)p * n];
    if (finite64(v) && (!r.any || v < r.beta)) {
      r.any = true;
      r.beta = v;
    }
  }
  return r;
}

// The weighted update of env i's step k0 + 1 (DESIGN.md sections 14 and 15), the body of both update kernels:
// w_p = exp(-(S_p - beta) / lambda) over the finite costs, abar += sum_p w_p sigma eps_p / sum_p w_p, clipped; the tape
// is copied where no cost is finite or the temperature is not `warm` (finite and > 0).  eps(p, j): the draw of sample
// p >= 1, component j, at this step.  Step 0's lanes store ess and cost_min.
template <int A, class NOISE>
__device__ __forceinline__ void mppi_update_lane(uint32_t n, uint32_t i, uint32_t k0, const float* abar_dev,
                                                 const MppiArgs& m, double lambda, bool warm, NOISE eps) {
  const uint32_t P = m.samples;
  const double* col = m.costs + i;
  const auto [any, beta] = column_min(col, n, P);
  const bool move = any && warm;
  float sig[A];
#pragma unroll
  for (int j = 0; j < A; ++j) sig[j] = m.sigma[j];
  double eta = 0.0, eta2 = 0.0, acc[A];
#pragma unroll
  for (int j = 0; j < A; ++j) acc[j] = 0.0;
  if (move) {
#pragma clang loop unroll(disable)
    for (uint32_t p = 0; p < P; ++p) {
      const double v = col[(size_t)p * n];
      const double w = finite64(v) ? exp(-(v - beta) / lambda) : 0.0;
      eta += w;
      eta2 += w * w;
      if (p != 0u) {  // (sample 0 is the nominal: its perturbation is zero)
#pragma unroll
        for (int j = 0; j < A; ++j) {
          const float da = sig[j] * eps(p, (uint32_t)j);
          acc[j] += w * (double)da;
        }
      }
    }
  }
  const size_t at = ((size_t)k0 * n + i) * A;
  const double inv_eta = 1.0 / eta;  // (eta >= 1 when move: the best sample's weight is exp(0))
#pragma unroll
  for (int j = 0; j < A; ++j) {
    const float ab = abar_dev[at + j];
    m.out[at + j] = move ? clip01((float)((double)ab + inv_eta * acc[j])) : ab;
  }
  if (k0 == 0u) {
    if (m.ess != nullptr) m.ess[i] = move ? (eta * eta) / eta2 : 0.0;
    if (m.cost_min != nullptr) m.cost_min[i] = any ? beta : __builtin_inf();
  }
}

// best[i] = the arg-min over the finite costs of env i, the lowest index on ties, -1 if none is finite (its own loop:
// it tracks the index, with that tie rule)
__global__ __launch_bounds__(kBlock) void mppi_best_kernel(uint32_t n, const MppiArgs m) {
  const uint32_t tile = blockIdx.x;
  const uint32_t i = tile * kBlock + threadIdx.x;
  if (i >= n) return;
  int32_t best = -1;
  double beta = 0.0;
#pragma clang loop unroll(disable)
  for (uint32_t p = 0; p < m.samples; ++p) {
    const double v = m.costs[(size_t)p * n + i];
    if (finite64(v) && (best < 0 || v < beta)) {
      best = (int32_t)p;
      beta = v;
    }
  }
  m.best[i] = best;
}

// the checks of the block that every MPPI entry point makes before the context; `buffers`: sigma_dev is required too
inline int check_mppi_io(const cs_rollout_mppi_io* mio, const std::string& w, bool buffers = true) {
  if (mio == nullptr) return report_error(CS_ERR_ARG, (w + ": null mio").c_str());
  if (mio->struct_size != sizeof(cs_rollout_mppi_io))
    return report_error(CS_ERR_ABI, (w + ": mio->struct_size " + std::to_string(mio->struct_size) + " != " +
                                     std::to_string(sizeof(cs_rollout_mppi_io)) + " (sizeof(cs_rollout_mppi_io))").c_str());
  if (mio->num_samples < 1 || mio->num_samples > CS_MPPI_MAX_SAMPLES)
    return report_error(CS_ERR_ARG, (w + ": num_samples must be in [1, " + std::to_string(CS_MPPI_MAX_SAMPLES) +
                                     "] (the sample index is the launch grid's y)").c_str());
  if (buffers ? mio->sigma_dev == nullptr || mio->costs_dev == nullptr : mio->costs_dev == nullptr)
    return report_error(CS_ERR_ARG, (w + (buffers ? ": sigma_dev and costs_dev are required"
                                                  : ": costs_dev is required")).c_str());
  return CS_OK;
}

// the checks of cs_rollout_mppi_costs(_ex) on its own fields
inline int check_mppi_costs_io(const cs_rollout_mppi_io* mio, const std::string& w) {
  if (mio->x_ref_steps > 1u)
    return report_error(CS_ERR_ARG, (w + ": x_ref_steps must be 0 ([N,12]) or 1 ([K,N,12])").c_str());
  if (mio->x_ref_dev == nullptr || mio->Q_dev == nullptr || mio->R_dev == nullptr)
    return report_error(CS_ERR_ARG, (w + ": x_ref_dev, Q_dev and R_dev are required").c_str());
  if (!(mio->reward_weight >= 0.0) || !std::isfinite(mio->reward_weight))
    return report_error(CS_ERR_ARG, (w + ": reward_weight must be finite and >= 0").c_str());
  return CS_OK;
}

// ... and of cs_rollout_mppi_update(_ex); `scalar_lambda`: mio->lam is the temperature
inline int check_mppi_update_io(const cs_rollout_io* io, const cs_rollout_mppi_io* mio, const std::string& w,
                                bool scalar_lambda = true) {
  if (io->num_steps > CS_MPPI_MAX_SAMPLES)
    return report_error(CS_ERR_ARG, (w + ": num_steps must be <= CS_MPPI_MAX_SAMPLES (the step index is the launch "
                                         "grid's y)").c_str());
  if (scalar_lambda && (!(mio->lam > 0.0) || !std::isfinite(mio->lam)))
    return report_error(CS_ERR_ARG, (w + ": lambda must be finite and > 0").c_str());
  if (mio->actions_out_dev == nullptr) return report_error(CS_ERR_ARG, (w + ": actions_out_dev is required").c_str());
  if (mio->actions_out_dev == io->actions_dev)
    return report_error(CS_ERR_ARG, (w + ": actions_out_dev must not alias io->actions_dev").c_str());
  return CS_OK;
}

inline MppiArgs mppi_args(cs_ctx* ctx, const cs_rollout_mppi_io& o) {
  return MppiArgs{o.sigma_dev, o.x_ref_dev, o.a_ref_dev, o.Q_dev, o.Q_final_dev != nullptr ? o.Q_final_dev : o.Q_dev,
                  o.R_dev, o.costs_dev, o.best_dev, o.actions_out_dev, o.ess_dev, o.cost_min_dev, o.lam,
                  o.reward_weight, mppi_noise_key(context_seed(ctx)), o.noise_stream, (uint32_t)o.num_samples,
                  o.x_ref_steps};
}

// the optional arg-min over the costs a cost entry point `who` has just launched (best_dev NULL: nothing)
inline int launch_mppi_best(const MppiArgs& m, uint32_t n, hipStream_t stream, const std::string& who) {
  if (m.best == nullptr) return CS_OK;
  hipLaunchKernelGGL(mppi_best_kernel, dim3(grid_for(n)), dim3(kBlock), 0, stream, n, m);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return report_hip(e, (who + ": arg-min kernel launch").c_str());
  return CS_OK;
}

}  // namespace
}  // namespace cs
