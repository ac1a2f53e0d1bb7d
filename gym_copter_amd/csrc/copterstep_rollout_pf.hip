// copterstep_rollout_pf.hip -- a bootstrap particle filter over the env step on gfx950 (cs_rollout_pf,
// include/copterstep.h): K steps of propagate / weight / estimate / resample per env in one launch, the particles
// resident in the LDS from the first step to the last.  The filter's state is the caller's: nothing of the env state is
// read but the constants and the vehicle table, and nothing is written.  DESIGN.md section 21.
//
// Upstream lines run per particle: those of cs_rollout_states' step (setMotors, the state derivative, step).
//
// One workgroup per env, min(P, 256) lanes; lane t owns the particles t, t + blockDim, .. (P / blockDim <= 4 of them) in
// every per-particle phase, so that a wavefront's LDS accesses are consecutive.  Per step:
//   propagate  the physics of the EKF's mean (clip, motor law, physics_substeps) from the particle's own (x, status),
//              then 12 Philox draws coloured by Lq (pf_noise.h)
//   weight     M scalar innovations per particle, a max and a sum over the workgroup, exp / log
//   integers   wq = rint(e 2^24); S1, S2, the heaviest particle: 64-bit integer reductions -- exact in any order
//   estimate   12 weighted sums, twice (mean, then variance); the 66 off-diagonal sums after the last step only
//   resample   the cumulative wq as a workgroup scan (a lane scans its own run of P / blockDim consecutive particles),
//              the ancestor of a slot by binary search on it, the gather in place one state component at a time behind a
//              barrier (a second particle buffer would not fit beside the first at P = 1 024)
// The LDS holds the particles as 12 rows of P float64 (row j at [j * P]), lw [P], the cumulative wq [P] (64-bit), wq,
// the ancestors and the statuses [P] (32-bit), and 3 KiB of shared constants (Lq or L0, H, r, ln 2 pi r, the z row)
// and reduction partials: 124 P + 3 072 bytes -- 127 KiB at P = 1 024 (one workgroup per CU), 34 KiB at P = 256.
// Every floating-point sum over particles is a lane's own partial in particle order, a butterfly over the wavefront and
// the wavefronts' partials in order: fixed, no atomics.
#include <cmath>
#include <string>

#include "copterstep_jacobian.h"

// the particles must round as the step kernels do: a prior particle is cs_rollout_states' row from the same point plus
// the noise, bit for bit; the noise and the weights are one multiply and one add per term, no fma
#pragma clang fp contract(off)

#include "dev_tile.h"
#include "dev_codec.h"
#include "dev_math.h"
#include "dev_physics.h"
#include "dev_task.h"
#include "jacobian_tangents.h"
#include "rollout_adjoint.h"
#include "rollout_step.h"
#include "rollout_sweep.h"
#include "cov_tile.h"
#include "pf_noise.h"
#include "dev_launch.h"

namespace cs {
namespace {

constexpr int kPfBlock = 256;    // the largest workgroup: one wavefront per SIMD, so the physics keeps its registers
constexpr int kPfPerLane = CS_PF_MAX_PARTICLES / kPfBlock;
constexpr int kPfWaves = kPfBlock / kWave;
// the shared constants and partials behind the per-particle arrays, in float64 words
constexpr int kScrL = 0;                 // Lq (L0 of the env while the Gaussian start is drawn), 144
constexpr int kScrH = 144;               // H, 144
constexpr int kScrR = 288;               // r, 12
constexpr int kScrLn = 300;              // ln(2 pi r), 12
constexpr int kScrZ = 312;               // the step's z row, 12
constexpr int kScrRed = 324;             // reduction partials: 12 values x kPfWaves wavefronts
constexpr int kScrWords = 384;
static_assert(kScrRed + 12 * kPfWaves <= kScrWords, "the partials fit");

size_t pf_lds_bytes(int P) { return (size_t)P * (14 * 8 + 3 * 4) + (size_t)kScrWords * 8; }
static_assert((size_t)CS_PF_MAX_PARTICLES * 124 + kScrWords * 8 <= 160 * 1024, "the LDS of one CU");

struct PfArgs {
  uint32_t key_pf;   // pf_noise_key(seed)
  double neg_ln_p;   // -ln P, taken on the host
};

// NV sums over the workgroup, the same bits in every lane: the wavefront's butterfly (a + b = b + a: both partners hold
// the same value after every round), then the wavefronts' partials in order.  red: 12 x kPfWaves words.
template <int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV], double* red, int tid, int nw) {
#pragma unroll
  for (int j = 0; j < NV; ++j) {
#pragma unroll
    for (int m = kWave / 2; m >= 1; m >>= 1) v[j] = v[j] + __shfl_xor(v[j], m);
  }
  if (nw == 1) return;
  if ((tid & (kWave - 1)) == 0) {
#pragma unroll
    for (int j = 0; j < NV; ++j) red[j * kPfWaves + (tid >> 6)] = v[j];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    double a = red[j * kPfWaves];
    for (int w = 1; w < nw; ++w) a = a + red[j * kPfWaves + w];
    v[j] = a;
  }
  __syncthreads();
}

__device__ __forceinline__ double block_max(double v, double* red, int tid, int nw) {
#pragma unroll
  for (int m = kWave / 2; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m));
  if (nw == 1) return v;
  if ((tid & (kWave - 1)) == 0) red[tid >> 6] = v;
  __syncthreads();
  double a = red[0];
  for (int w = 1; w < nw; ++w) a = fmax(a, red[w]);
  __syncthreads();
  return a;
}

// S1 = sum a, S2 = sum b, top = max c over the workgroup (64-bit integers: exact in any order)
__device__ __forceinline__ void block_int(unsigned long long& a, unsigned long long& b, unsigned long long& c,
                                          unsigned long long* red, int tid, int nw) {
#pragma unroll
  for (int m = kWave / 2; m >= 1; m >>= 1) {
    a += __shfl_xor(a, m);
    b += __shfl_xor(b, m);
    const unsigned long long o = __shfl_xor(c, m);
    c = o > c ? o : c;
  }
  if (nw == 1) return;
  if ((tid & (kWave - 1)) == 0) {
    red[tid >> 6] = a;
    red[kPfWaves + (tid >> 6)] = b;
    red[2 * kPfWaves + (tid >> 6)] = c;
  }
  __syncthreads();
  a = red[0];
  b = red[kPfWaves];
  c = red[2 * kPfWaves];
  for (int w = 1; w < nw; ++w) {
    a += red[w];
    b += red[kPfWaves + w];
    const unsigned long long o = red[2 * kPfWaves + w];
    c = o > c ? o : c;
  }
  __syncthreads();
}

template <int TASK, int MODE, bool GYRO>
__global__ __launch_bounds__(kPfBlock) void rollout_pf_kernel(const DevConst c, const DevState s, const cs_rollout_io io,
                                                              const cs_rollout_pf_io f, const PfArgs pa) {
  constexpr int A = task_act_dim(TASK);
  constexpr bool FULL = MODE == CS_STATE_F64 || kFullTrigInEveryMode;
  extern __shared__ __attribute__((aligned(16))) double pf_lds[];
  const int tid = threadIdx.x;
  const int bd = blockDim.x;
  const int nw = bd >> 6;
  const uint32_t tile_index = blockIdx.x;  // (no arithmetic on it: this kernel's "tile" is one env, and it touches no state tile)
  const uint32_t env = tile_index;
  const uint32_t n = s.n;
  const int P = f.num_particles;
  const int per = P / bd;                // particles per lane, 1 .. kPfPerLane
  const int K = io.num_steps;
  const int M = f.num_meas;
  const uint32_t f32 = f.out_dtype == CS_JAC_F32 ? 1u : 0u;
  const uint32_t g = c.id_lo + env;      // the global env id: the first counter word of every draw

  double* const X = pf_lds;              // row j of the particles at [j * P]
  double* const LW = X + 12 * P;
  unsigned long long* const CW = reinterpret_cast<unsigned long long*>(LW + P);
  double* const scr = LW + 2 * P;
  uint32_t* const WQ = reinterpret_cast<uint32_t*>(scr + kScrWords);
  int* const ANC = reinterpret_cast<int*>(WQ + P);
  int* const ST = ANC + P;
  double* const red = scr + kScrRed;
  unsigned long long* const redu = reinterpret_cast<unsigned long long*>(red);

  Coef q = uniform_coef(c);
  if (s.veh != nullptr) q = load_coef(s.veh, s.veh_stride, env);

  // ---- the shared model: H, r, ln(2 pi r); the start ----
  for (int e = tid; e < M * 12; e += bd) scr[kScrH + e] = f.H_dev[e];
  if (tid < M) {
    const double r = f.r_dev[tid];
    scr[kScrR + tid] = r;
    scr[kScrLn + tid] = log(6.283185307179586476925286766559 * r);
  }
  const size_t pbase = (size_t)env * P;
  if (f.part_in_dev != nullptr) {  // carried: a previous call's part_out / pstatus_out / lw_out
    const double* src = f.part_in_dev + pbase * 12;
    for (int e = tid; e < 12 * P; e += bd) {
      const int p = e / 12, j = e - p * 12;
      X[j * P + p] = src[e];
    }
    for (int p = tid; p < P; p += bd) {
      ST[p] = (int)f.pstatus_in_dev[pbase + p];
      LW[p] = f.lw_in_dev[pbase + p];
    }
  } else {  // Gaussian: xhat_0 + L0 eps(k = 0, p)
    if (f.L0_dev != nullptr) {
      for (int e = tid; e < 144; e += bd) scr[kScrL + e] = f.L0_dev[(size_t)env * 144 + e];
    }
    __syncthreads();
    const int st0 = (int)io.start_status_dev[env];
    double x0[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) x0[j] = io.start_x_dev[(size_t)j * n + env];
#pragma clang loop unroll(disable)
    for (int i = 0; i < per; ++i) {
      const int p = tid + i * bd;
      if (f.L0_dev != nullptr) {
        float eps[12];
#pragma unroll
        for (int j = 0; j < 12; ++j) eps[j] = pf_noise(pa.key_pf, g, f.nonce, 0u, (uint32_t)p, (uint32_t)j);
#pragma unroll
        for (int j = 0; j < 12; ++j) X[j * P + p] = x0[j] + pf_colour(scr + kScrL, 1, j, eps);
      } else {
#pragma unroll
        for (int j = 0; j < 12; ++j) X[j * P + p] = x0[j];
      }
      ST[p] = st0;
      LW[p] = pa.neg_ln_p;
    }
  }
  __syncthreads();
  for (int e = tid; e < 144; e += bd) scr[kScrL + e] = f.Lq_dev[e];
  __syncthreads();

  double loglik = 0.0;
  bool ok = true;

#pragma clang loop unroll(disable)
  for (int k = 0; k < K; ++k) {
    const size_t row = (size_t)k * n + env;            // 64-bit: K x N x P x 12 doubles pass 4 GiB early
    const size_t prow = row * (size_t)P;
    const uint32_t kg = f.first_step + (uint32_t)k;    // the global step index
    const bool last = k == K - 1;

    // ---- the step's wrench (uniform) and its z row ----
    const float4 act = load_action_at<TASK>(io.actions_dev + row * A);
    // (the clip and the motor law as they stood before step_wrench: through it two additions of the sum of squares
    // came out with swapped operands and one A/B row missed by 0.5 %, profiles/filter_shared_refactor_ab.txt)
    const float araw[4] = {act.x, act.y, act.z, act.w};
    float mf[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) mf[j] = clip01(araw[j]);
    Wrench w;
    w.bz = thrust_model(q, mf[0], mf[1], mf[2], mf[3]);
    torque_model(q, mf[0], mf[1], mf[2], mf[3], w);
    if (tid < M) scr[kScrZ + tid] = f.z_dev[row * (size_t)M + tid];

    // ---- propagate: the physics from (x, status), then the noise, whatever the status ----
#pragma clang loop unroll(disable)
    for (int i = 0; i < per; ++i) {
      const int p = tid + i * bd;
      double x[12];
#pragma unroll
      for (int j = 0; j < 12; ++j) x[j] = X[j * P + p];
      int fs = ST[p];
      if (fs != CS_STATUS_LANDED) {
        bool pend = false;
        physics_substeps<FULL, GYRO, false, true>(c, q, w, x, fs, pend, -0.0, -0.0, -0.0);
      }
      float eps[12];
#pragma unroll
      for (int j = 0; j < 12; ++j) eps[j] = pf_noise(pa.key_pf, g, f.nonce, kg, (uint32_t)p, (uint32_t)j);
#pragma unroll
      for (int j = 0; j < 12; ++j) X[j * P + p] = x[j] + pf_colour(scr + kScrL, 1, j, eps);
      ST[p] = fs;
    }
    __syncthreads();  // (the particles and the z row are in the LDS)
    if (f.part_tape_dev != nullptr) {
      double* dst = f.part_tape_dev + prow * 12;
      for (int e = tid; e < 12 * P; e += bd) {
        const int p = e / 12, j = e - p * 12;
        dst[e] = X[j * P + p];
      }
    }
    if (f.pstatus_tape_dev != nullptr) {
      for (int p = tid; p < P; p += bd) f.pstatus_tape_dev[prow + p] = (uint8_t)ST[p];
    }

    // ---- weight: lw' = lw + ll, its maximum ----
    bool present = false;
    double lnr = 0.0;
    for (int m = 0; m < M; ++m) {
      if (scr[kScrZ + m] == scr[kScrZ + m]) {
        present = true;
        lnr = lnr + scr[kScrLn + m];
      }
    }
    double lwp[kPfPerLane];
    double mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < kPfPerLane; ++i) {
      lwp[i] = -INFINITY;
      if (i < per) {
        const int p = tid + i * bd;
        double ll = 0.0;
#pragma clang loop unroll(disable)
        for (int m = 0; m < M; ++m) {
          const double z = scr[kScrZ + m];
          if (z == z) {
            const double* h = scr + kScrH + m * 12;
            double hx = h[0] * X[p];
#pragma unroll
            for (int j = 1; j < 12; ++j) hx = hx + h[j] * X[j * P + p];
            const double nu = z - hx;
            ll = ll - 0.5 * (nu * nu) / scr[kScrR + m];
          }
        }
        double v = LW[p] + ll;
        if (!(fabs(v) < INFINITY)) v = -INFINITY;
        lwp[i] = v;
        mx = fmax(mx, v);
      }
    }
    mx = block_max(mx, red, tid, nw);
    const bool dead = !(mx > -INFINITY);  // no particle has a finite lw'
    if (dead) ok = false;

    // ---- e = exp(lw' - m), eta, the normalised lw; the integer weights ----
    double ep[kPfPerLane];
    double eta[1] = {0.0};
#pragma unroll
    for (int i = 0; i < kPfPerLane; ++i) {
      ep[i] = 0.0;
      if (i < per) {
        ep[i] = dead ? 1.0 : exp(lwp[i] - mx);
        eta[0] = eta[0] + ep[i];
      }
    }
    block_sum<1>(eta, red, tid, nw);
    const double norm = dead ? 0.0 : mx + log(eta[0]);
    if (present && !dead) loglik = loglik + (norm - 0.5 * lnr);
    unsigned long long S1 = 0, S2 = 0, top = 0;
#pragma unroll
    for (int i = 0; i < kPfPerLane; ++i) {
      if (i < per) {
        const int p = tid + i * bd;
        if (dead)
          LW[p] = pa.neg_ln_p;
        else if (present)
          LW[p] = lwp[i] - norm;
        const uint32_t wq = (uint32_t)rint(ep[i] * 16777216.0);
        WQ[p] = wq;
        S1 += wq;
        S2 += (unsigned long long)wq * wq;
        const unsigned long long key = ((unsigned long long)wq << 32) | (uint32_t)(0xFFFFFFFFu - (uint32_t)p);
        top = key > top ? key : top;
      }
    }
    block_int(S1, S2, top, redu, tid, nw);
    __syncthreads();  // (WQ and LW are complete)
    const int best = (int)(0xFFFFFFFFu - (uint32_t)top);
    const double s1d = (double)S1, s2d = (double)S2;
    const double ess = s1d * s1d / s2d;
    const bool resample = s1d * s1d < (f.ess_frac * (double)P) * s2d;
    if (f.lw_tape_dev != nullptr) {
      for (int p = tid; p < P; p += bd) f.lw_tape_dev[prow + p] = LW[p];
    }
    if (f.wq_tape_dev != nullptr) {
      for (int p = tid; p < P; p += bd) f.wq_tape_dev[prow + p] = WQ[p];
    }

    // ---- estimate, before resampling: the weighted mean, then the weighted variance ----
    double xh[12], var[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) xh[j] = 0.0;
#pragma clang loop unroll(disable)
    for (int i = 0; i < per; ++i) {
      const int p = tid + i * bd;
      const uint32_t wq = WQ[p];
      if (wq != 0u) {
        const double wd = (double)wq;
#pragma unroll
        for (int j = 0; j < 12; ++j) xh[j] = xh[j] + wd * X[j * P + p];
      }
    }
    block_sum<12>(xh, red, tid, nw);
#pragma unroll
    for (int j = 0; j < 12; ++j) {
      xh[j] = xh[j] / s1d;
      var[j] = 0.0;
    }
#pragma clang loop unroll(disable)
    for (int i = 0; i < per; ++i) {
      const int p = tid + i * bd;
      const uint32_t wq = WQ[p];
      if (wq != 0u) {
        const double wd = (double)wq;
#pragma unroll
        for (int j = 0; j < 12; ++j) {
          const double d = X[j * P + p] - xh[j];
          var[j] = var[j] + wd * (d * d);
        }
      }
    }
    block_sum<12>(var, red, tid, nw);
#pragma unroll
    for (int j = 0; j < 12; ++j) var[j] = var[j] / s1d;

    if (tid == 0) {
      if (io.x_dev != nullptr) {
#pragma unroll
        for (int j = 0; j < 12; ++j) io.x_dev[row * 12 + j] = xh[j];
      }
      if (f.var_dev != nullptr) {
#pragma unroll
        for (int j = 0; j < 12; ++j) store_out(f.var_dev, row * 12 + j, var[j], f32);
      }
      if (io.status_dev != nullptr) io.status_dev[row] = (uint8_t)ST[best];
      if (f.ess_dev != nullptr) store_out(f.ess_dev, row, ess, f32);
      if (f.resampled_dev != nullptr) f.resampled_dev[row] = resample ? 1 : 0;
      if (f.best_dev != nullptr) f.best_dev[row] = best;
    }

    // ---- after the last step: the full weighted covariance (row a's off-diagonal sums at a time; Lq is dead) ----
    if (last && f.P_dev != nullptr) {
      __syncthreads();
#pragma clang loop unroll(disable)
      for (int a = 0; a < 11; ++a) {
        double cv[12];
#pragma unroll
        for (int b = 0; b < 12; ++b) cv[b] = 0.0;
        double xa = 0.0;
#pragma unroll
        for (int j = 0; j < 12; ++j) xa = j == a ? xh[j] : xa;
#pragma clang loop unroll(disable)
        for (int i = 0; i < per; ++i) {
          const int p = tid + i * bd;
          const uint32_t wq = WQ[p];
          if (wq != 0u) {
            const double wda = (double)wq * (X[a * P + p] - xa);
#pragma unroll
            for (int b = 0; b < 12; ++b) cv[b] = cv[b] + wda * (X[b * P + p] - xh[b]);
          }
        }
        block_sum<12>(cv, red, tid, nw);
        if (tid == 0) {
#pragma unroll
          for (int b = 0; b < 12; ++b) {
            if (b > a) {
              const double v = cv[b] / s1d;
              scr[kScrL + a * 12 + b] = v;
              scr[kScrL + b * 12 + a] = v;
            }
          }
        }
      }
      if (tid == 0) {
#pragma unroll
        for (int j = 0; j < 12; ++j) scr[kScrL + j * 13] = var[j];
      }
      __syncthreads();
      for (int e = tid; e < 144; e += bd) store_out(f.P_dev, (size_t)env * 144 + e, scr[kScrL + e], f32);
    }

    // ---- systematic resampling on the integer weights ----
    if (resample) {
      // the inclusive cumulative wq: a lane scans its run of `per` consecutive particles, the wavefront its lanes, the
      // workgroup its wavefronts
      unsigned long long run = 0;
      for (int i = 0; i < per; ++i) run += WQ[tid * per + i];
      unsigned long long incl = run;
#pragma unroll
      for (int d = 1; d < kWave; d <<= 1) {
        const unsigned long long o = __shfl_up(incl, d);
        if ((tid & (kWave - 1)) >= d) incl += o;
      }
      if (nw > 1) {
        if ((tid & (kWave - 1)) == kWave - 1) redu[tid >> 6] = incl;
        __syncthreads();
        for (int wv = 0; wv < (tid >> 6); ++wv) incl += redu[wv];
      }
      unsigned long long cum = incl - run;
      for (int i = 0; i < per; ++i) {
        cum += WQ[tid * per + i];
        CW[tid * per + i] = cum;
      }
      __syncthreads();
      const unsigned long long u = pf_resample_u(pa.key_pf, g, f.nonce, kg);
      const unsigned long long teeth = (unsigned long long)P << 16;
      int anc[kPfPerLane];
#pragma unroll
      for (int i = 0; i < kPfPerLane; ++i) {
        anc[i] = 0;
        if (i < per) {
          const unsigned long long slot = (unsigned long long)(tid + i * bd);
          const unsigned long long t = ((slot << 16) + u) * S1;
          int lo = 0, hi = P - 1;  // (C[P-1] = S1 passes the test for every slot)
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (CW[mid] * teeth > t)
              hi = mid;
            else
              lo = mid + 1;
          }
          anc[i] = lo;
        }
      }
      // the gather, in place: every lane reads its ancestors' values of one row, then all write
#pragma clang loop unroll(disable)
      for (int j = 0; j < 12; ++j) {
        double v[kPfPerLane];
#pragma unroll
        for (int i = 0; i < kPfPerLane; ++i) v[i] = i < per ? X[j * P + anc[i]] : 0.0;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kPfPerLane; ++i)
          if (i < per) X[j * P + tid + i * bd] = v[i];
      }
      int sv[kPfPerLane];
#pragma unroll
      for (int i = 0; i < kPfPerLane; ++i) sv[i] = i < per ? ST[anc[i]] : 0;
      __syncthreads();
#pragma unroll
      for (int i = 0; i < kPfPerLane; ++i) {
        if (i < per) {
          const int p = tid + i * bd;
          ST[p] = sv[i];
          LW[p] = pa.neg_ln_p;
          ANC[p] = anc[i];
        }
      }
    } else {
      for (int p = tid; p < P; p += bd) ANC[p] = p;
    }
    __syncthreads();  // (the step's posterior particles, statuses, lw and ancestors are in the LDS)
    if (f.anc_tape_dev != nullptr) {
      for (int p = tid; p < P; p += bd) f.anc_tape_dev[prow + p] = ANC[p];
    }
  }

  // ---- the carried state: after step K, post-resample ----
  if (f.part_out_dev != nullptr) {
    double* dst = f.part_out_dev + pbase * 12;
    for (int e = tid; e < 12 * P; e += bd) {
      const int p = e / 12, j = e - p * 12;
      dst[e] = X[j * P + p];
    }
  }
  for (int p = tid; p < P; p += bd) {
    if (f.pstatus_out_dev != nullptr) f.pstatus_out_dev[pbase + p] = (uint8_t)ST[p];
    if (f.lw_out_dev != nullptr) f.lw_out_dev[pbase + p] = LW[p];
  }
  if (tid == 0) {
    if (f.loglik_dev != nullptr) store_out(f.loglik_dev, env, loglik, f32);
    if (f.ok_dev != nullptr) f.ok_dev[env] = ok ? 1 : 0;
  }
}

template <int TASK, int MODE, bool GYRO>
hipError_t pf_launch(const DevConst& c, const DevState& s, const cs_rollout_io& io, const cs_rollout_pf_io& f,
                     const PfArgs& pa, hipStream_t stream) {
  const int P = f.num_particles;
  const size_t lds = pf_lds_bytes(P);
  auto kernel = rollout_pf_kernel<TASK, MODE, GYRO>;
  // (more than 64 KiB of dynamic LDS at P = 1 024: say so to the runtime)
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  const dim3 grid(s.n), block(P < kPfBlock ? P : kPfBlock);
  hipLaunchKernelGGL(kernel, grid, block, lds, stream, c, s, io, f, pa);
  return hipGetLastError();
}

template <int TASK, int MODE>
hipError_t pf_t(const DevConst& c, const DevState& s, const cs_rollout_io& io, const cs_rollout_pf_io& f,
                const PfArgs& pa, hipStream_t stream) {
  if (c.gyro) return pf_launch<TASK, MODE, true>(c, s, io, f, pa, stream);
  return pf_launch<TASK, MODE, false>(c, s, io, f, pa, stream);
}

hipError_t launch_rollout_pf(int task, int mode, const DevConst& c, const DevState& s, const cs_rollout_io& io,
                             const cs_rollout_pf_io& f, const PfArgs& pa, hipStream_t stream) {
  CS_DISPATCH(pf_t, c, s, io, f, pa, stream)
}

}  // namespace
}  // namespace cs

extern "C" int cs_rollout_pf(cs_ctx* ctx, const cs_rollout_io* io, const cs_rollout_pf_io* pio, void* stream) {
  using cs::report_error;
  const char* who = "cs_rollout_pf";
  if (int rc_ = cs::check_rollout_io(io, who, false)) return rc_;
  const bool extra = io->reward_dev != nullptr || io->terminated_dev != nullptr || io->truncated_dev != nullptr ||
                     io->gx_dev != nullptr || io->gr_dev != nullptr || io->g_actions_dev != nullptr ||
                     io->g_x0_dev != nullptr;
  if (int rc_ = cs::check_filter_io(io, who, {"pio", "cs_rollout_pf_io", pio, sizeof(cs_rollout_pf_io)}, nullptr,
                                    extra ? "the reward, flag, cotangent and gradient pointers must be NULL" : nullptr))
    return rc_;
  if (pio->num_meas < 1 || pio->num_meas > CS_EKF_MAX_MEAS)
    return report_error(CS_ERR_ARG, "cs_rollout_pf: num_meas must be 1 .. CS_EKF_MAX_MEAS");
  const int P = pio->num_particles;
  if (P < CS_PF_MIN_PARTICLES || P > CS_PF_MAX_PARTICLES || (P & (P - 1)) != 0)
    return report_error(CS_ERR_ARG,
                        "cs_rollout_pf: num_particles must be a power of two in CS_PF_MIN_PARTICLES .. CS_PF_MAX_PARTICLES");
  if (pio->first_step < 1 || (uint64_t)pio->first_step + (uint64_t)io->num_steps - 1 > 0xFFFFFFFFull)
    return report_error(CS_ERR_ARG, "cs_rollout_pf: first_step must be >= 1 and first_step + num_steps - 1 < 2^32");
  if (!(pio->ess_frac >= 0.0 && pio->ess_frac <= 1.0))
    return report_error(CS_ERR_ARG, "cs_rollout_pf: ess_frac must be in [0, 1]");
  if (pio->H_dev == nullptr || pio->r_dev == nullptr || pio->Lq_dev == nullptr || pio->z_dev == nullptr)
    return report_error(CS_ERR_ARG, "cs_rollout_pf: H_dev, r_dev, Lq_dev and z_dev are required");
  const bool gauss = io->start_x_dev != nullptr;
  const bool any_carried = pio->part_in_dev != nullptr || pio->pstatus_in_dev != nullptr || pio->lw_in_dev != nullptr;
  const bool carried = pio->part_in_dev != nullptr && pio->pstatus_in_dev != nullptr && pio->lw_in_dev != nullptr;
  if (gauss == any_carried || (any_carried && !carried))
    return report_error(CS_ERR_ARG,
                        "cs_rollout_pf: give exactly one start: start_x_dev with start_status_dev (and L0_dev), or all "
                        "of part_in_dev, pstatus_in_dev and lw_in_dev");
  if (carried && pio->L0_dev != nullptr)
    return report_error(CS_ERR_ARG, "cs_rollout_pf: L0_dev belongs to the Gaussian start: NULL with a carried start");
  cs::ContextView v;
  if (int rc_ = cs::enter_filter_context(
          ctx, who, stream, pio->out_dtype,
          {io->start_x_dev, io->x_dev, pio->H_dev, pio->r_dev, pio->Lq_dev, pio->z_dev, pio->L0_dev, pio->part_in_dev,
           pio->lw_in_dev, pio->part_out_dev, pio->lw_out_dev, pio->part_tape_dev, pio->lw_tape_dev},
          {pio->var_dev, pio->ess_dev, pio->P_dev, pio->loglik_dev},
          {io->actions_dev, pio->best_dev, pio->wq_tape_dev, pio->anc_tape_dev}, "actions_dev or a 32-bit array", &v))
    return rc_;
  const cs::PfArgs pa{cs::pf_noise_key(cs::context_seed(ctx)), -std::log((double)P)};
  const hipError_t e = cs::launch_rollout_pf(v.task, v.mode, *v.c, *v.s, *io, *pio, pa, (hipStream_t)stream);
  if (e != hipSuccess) return cs::report_hip(e, "cs_rollout_pf: kernel launch");
  return CS_OK;
}
