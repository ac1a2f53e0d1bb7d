// rollout_mppi.h -- what the MPPI translation units share (copterstep_rollout_mppi.hip: the white-noise kernels of
// DESIGN.md section 14; copterstep_rollout_mppi_smooth.hip: the knot-noise kernels and the temperature of section 15):
// the checked argument block, the cost's matrices in the LDS, the motor fan-out, the arg-min kernel and the block
// checks.  Included after the device headers and mppi_noise.h, inside a translation unit that has set
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

// best[i] = the arg-min over the finite costs of env i, the lowest index on ties, -1 if none is finite
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

}  // namespace
}  // namespace cs
