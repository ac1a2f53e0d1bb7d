// copterstep_pf_smooth.hip -- a backward-simulation particle smoother (forward filtering, backward simulation) over the
// tapes of cs_rollout_pf on gfx950 (cs_pf_smooth, include/copterstep.h): S trajectories per env drawn backwards through
// the filter's taped particle sets, K backward steps per env in one launch.  Every input is a tape or the caller's:
// nothing of the env state is read but the constants and the vehicle table, and nothing is written.  DESIGN.md section 27.
//
// Upstream lines run per particle: those of cs_rollout_states' step (setMotors, the state derivative, step).
//
// One workgroup per env, min(P, 256) lanes, as cs_rollout_pf.  Per backward step k = K-2 .. 0 (and -1 from a start set):
//   propagate  lane t sends the particles t, t + blockDim, .. of row k through the physics of step k+1 (the filter's own
//              code: clip, motor law, physics_substeps, skipped for a LANDED particle; no noise) and whitens the result,
//              y = Linv mu (pfs_draw.h); y, the status after the step and lw_k go to the LDS
//   paths      each wavefront takes the paths m = wave, wave + nw, ..; within a path a lane owns the run of P / 64
//              consecutive particles lane * run ..: the squared distances to the path's whitened next point, log beta,
//              its maximum (a butterfly), the integer weights, their inclusive scan (shuffles), the draw and the search
//              (a ballot for the lane, the lane's own run for the particle) -- nothing of a path crosses a wavefront, so
//              paths need no workgroup barrier between them
//   estimate   the row's S indices are in the LDS: the mean and the variance of the S drawn particles, a lane's own paths
//              in order, a butterfly over the wavefront and the wavefronts' partials in order: fixed, no atomics
// The LDS holds y as 12 rows of P + 64 float64, lw_k and the statuses at the same slots, Linv, the reduction partials
// and the indices of two rows (this one and the one above): 108 P + 16 656 bytes -- 124 KiB at P = 1 024 (one
// workgroup per CU), 43 KiB at P = 256. A particle p sits at slot p + p / run when run > 1: a lane's run then starts
// run + 1 slots after its neighbour's, an odd number of 8-byte words, so that the 32 lanes of a ds_read_b64 group fall
// on 32 different bank pairs (at a stride of run = 16 words they would share two).
#include <cmath>
#include <string>

#include "copterstep_jacobian.h"

// a propagated particle must round as the filter's did (mu is cs_rollout_states' row from the same point, bit for bit),
// and the whitening, the distances and log beta are one multiply and one add per term, no fma
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
#include "pfs_draw.h"
#include "dev_launch.h"

namespace cs {
namespace {

constexpr int kPfsBlock = 256;  // the largest workgroup: one wavefront per SIMD, so the physics keeps its registers
constexpr int kPfsWaves = kPfsBlock / kWave;
constexpr int kPfsMaxRun = CS_PF_MAX_PARTICLES / kWave;  // particles a lane owns within a path
constexpr int kPfsPad = kWave;                           // slots behind the P particles: one per lane's run
// the shared constants and partials behind the per-particle arrays, in float64 words
constexpr int kScrLinv = 0;    // Linv, 144
constexpr int kScrRed = 144;   // reduction partials: 12 values x kPfsWaves wavefronts
constexpr int kScrWords = 192;
static_assert(kScrRed + 12 * kPfsWaves <= kScrWords, "the partials fit");

constexpr size_t pfs_lds_bytes(int P) {
  return (size_t)(P + kPfsPad) * (13 * 8 + 4) + (size_t)kScrWords * 8 + 2 * (size_t)CS_PFS_MAX_PATHS * 4 + 16;
}
static_assert(pfs_lds_bytes(CS_PF_MAX_PARTICLES) <= 160 * 1024, "the LDS of one CU");

// NV sums over the workgroup, the same bits in every lane (cs_rollout_pf's block_sum): the wavefront's butterfly, then the
// wavefronts' partials in order.  red: 12 x kPfsWaves words.
template <int NV>
__device__ __forceinline__ void pfs_block_sum(double (&v)[NV], double* red, int tid, int nw) {
#pragma unroll
  for (int j = 0; j < NV; ++j) {
#pragma unroll
    for (int m = kWave / 2; m >= 1; m >>= 1) v[j] = v[j] + __shfl_xor(v[j], m);
  }
  if (nw == 1) return;
  if ((tid & (kWave - 1)) == 0) {
#pragma unroll
    for (int j = 0; j < NV; ++j) red[j * kPfsWaves + (tid >> 6)] = v[j];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    double a = red[j * kPfsWaves];
    for (int w = 1; w < nw; ++w) a = a + red[j * kPfsWaves + w];
    v[j] = a;
  }
  __syncthreads();
}

// a lane's run of integer weights within the wavefront's P: its exclusive and inclusive cumulative sums and the total
__device__ __forceinline__ void pfs_scan(const uint32_t (&bw)[kPfsMaxRun], int run, int lane, unsigned long long& excl,
                                         unsigned long long& incl, unsigned long long& s1) {
  unsigned long long own = 0;
#pragma unroll
  for (int i = 0; i < kPfsMaxRun; ++i)
    if (i < run) own += bw[i];
  incl = own;
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const unsigned long long o = __shfl_up(incl, d);
    if (lane >= d) incl += o;
  }
  excl = incl - own;
  s1 = __shfl(incl, kWave - 1);
}

// the smallest p with pfs_draw_passes(C[p], u, S1), the same in every lane: the first lane whose run's end passes, and
// within that lane's run the first particle that does.  P - 1 if none passes (every weight 0: a caller's own wq tape).
__device__ __forceinline__ int pfs_search(const uint32_t (&bw)[kPfsMaxRun], int run, int lane, unsigned long long excl,
                                          unsigned long long incl, unsigned long long s1, unsigned long long u, int P) {
  int cand = -1;
  unsigned long long cum = excl;
#pragma unroll
  for (int i = 0; i < kPfsMaxRun; ++i) {
    if (i < run) {
      cum += bw[i];
      if (cand < 0 && pfs_draw_passes(cum, u, s1)) cand = lane * run + i;
    }
  }
  const unsigned long long hit = __ballot(pfs_draw_passes(incl, u, s1));
  if (hit == 0ull) return P - 1;
  return __shfl(cand, __ffsll(hit) - 1);
}

template <int TASK, int MODE, bool GYRO>
__global__ __launch_bounds__(kPfsBlock) void pf_smooth_kernel(const DevConst c, const DevState s, const cs_rollout_io io,
                                                              const cs_pf_smooth_io f, const uint32_t key_pf) {
  constexpr int A = task_act_dim(TASK);
  constexpr bool FULL = MODE == CS_STATE_F64 || kFullTrigInEveryMode;
  extern __shared__ __attribute__((aligned(16))) double pfs_lds[];
  const int tid = threadIdx.x;
  const int bd = blockDim.x;
  const int nw = bd >> 6;
  const int lane = tid & (kWave - 1);
  const int wave = tid >> 6;
  const uint32_t tile_index = blockIdx.x;  // (no arithmetic on it: this kernel's "tile" is one env, and it touches no state tile)
  const uint32_t env = tile_index;
  const uint32_t n = s.n;
  const int P = f.num_particles;
  const int S = f.num_paths;
  const int per = P / bd;                  // particles a lane propagates, 1 .. 4
  const int run = P >> 6;                  // particles a lane owns within a path, 1 .. kPfsMaxRun
  const int lg = __ffs(run) - 1;
  const int pad = run > 1 ? -1 : 0;        // slot(p) = p + p / run, or p when run is 1
  const int slots = P + kPfsPad;
  const int K = io.num_steps;
  const uint32_t f32 = f.out_dtype == CS_JAC_F32 ? 1u : 0u;
  const uint32_t g = c.id_lo + env;        // the global env id: the first counter word of every draw

  double* const Y = pfs_lds;               // row j of the whitened particles at [j * slots]
  double* const LW = Y + 12 * slots;
  double* const scr = LW + slots;
  int* const SG = reinterpret_cast<int*>(scr + kScrWords);
  int* B_above = SG + slots;               // the indices of the row above, b[k+1, .]
  int* B_here = B_above + CS_PFS_MAX_PATHS;
  int* const flag = B_here + CS_PFS_MAX_PATHS;
  double* const red = scr + kScrRed;

  Coef q = uniform_coef(c);
  if (s.veh != nullptr) q = load_coef(s.veh, s.veh_stride, env);

  for (int e = tid; e < 144; e += bd) scr[kScrLinv + e] = f.Linv_dev[e];
  if (tid == 0) flag[0] = 1;

  // row `row` of the outputs from the S indices B: idx, and the mean and the variance of the drawn particles
  const auto emit_row = [&](size_t row, const int* B) {
    if (f.idx_dev != nullptr) {
      for (int m = tid; m < S; m += bd) f.idx_dev[row * (size_t)S + m] = B[m];
    }
    if (io.x_dev == nullptr && f.var_dev == nullptr) return;
    const double* const part = f.part_tape_dev + row * (size_t)P * 12;
    double xs[12], var[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) xs[j] = 0.0;
    for (int m = tid; m < S; m += bd) {
      const double* src = part + (size_t)B[m] * 12;
#pragma unroll
      for (int j = 0; j < 12; ++j) xs[j] = xs[j] + src[j];
    }
    pfs_block_sum<12>(xs, red, tid, nw);
#pragma unroll
    for (int j = 0; j < 12; ++j) {
      xs[j] = xs[j] / (double)S;
      var[j] = 0.0;
    }
    for (int m = tid; m < S; m += bd) {
      const double* src = part + (size_t)B[m] * 12;
#pragma unroll
      for (int j = 0; j < 12; ++j) {
        const double d = src[j] - xs[j];
        var[j] = var[j] + d * d;
      }
    }
    pfs_block_sum<12>(var, red, tid, nw);
    if (tid == 0) {
      if (io.x_dev != nullptr) {
#pragma unroll
        for (int j = 0; j < 12; ++j) io.x_dev[row * 12 + j] = xs[j];
      }
      if (f.var_dev != nullptr) {
#pragma unroll
        for (int j = 0; j < 12; ++j) store_out(f.var_dev, row * 12 + j, var[j] / (double)S, f32);
      }
    }
  };

  // ---- row K-1: the caller's indices, or S draws from the filter's integer weights ----
  {
    const size_t row = (size_t)(K - 1) * n + env;  // 64-bit: K x N x P x 12 doubles pass 4 GiB early
    const size_t prow = row * (size_t)P;
    if (f.end_idx_dev != nullptr) {
      // (an index is taken mod P: whatever the caller passes, no read leaves the tapes)
      for (int m = tid; m < S; m += bd) B_above[m] = f.end_idx_dev[(size_t)env * S + m] & (P - 1);
    } else {
      uint32_t bw[kPfsMaxRun];
#pragma unroll
      for (int i = 0; i < kPfsMaxRun; ++i) bw[i] = i < run ? f.wq_tape_dev[prow + lane * run + i] : 0u;
      unsigned long long excl, incl, s1;
      pfs_scan(bw, run, lane, excl, incl, s1);
      const uint32_t kg = f.first_step + (uint32_t)(K - 1);
      for (int m = wave; m < S; m += nw) {
        const unsigned long long u = pfs_draw_u(key_pf, g, f.nonce, kg, (uint32_t)m);
        const int idx = pfs_search(bw, run, lane, excl, incl, s1, u, P);
        if (lane == 0) B_above[m] = idx;
        const size_t trow = (row * (size_t)S + m) * (size_t)P + lane * run;
        if (f.logb_tape_dev != nullptr) {
#pragma unroll
          for (int i = 0; i < kPfsMaxRun; ++i)
            if (i < run) f.logb_tape_dev[trow + i] = f.lw_tape_dev[prow + lane * run + i];
        }
        if (f.bwq_tape_dev != nullptr) {
#pragma unroll
          for (int i = 0; i < kPfsMaxRun; ++i)
            if (i < run) f.bwq_tape_dev[trow + i] = (int32_t)bw[i];
        }
      }
    }
    __syncthreads();  // (the row's indices, Linv and the flag are in the LDS)
    emit_row(row, B_above);
  }

  const int k_last = f.part_in_dev != nullptr ? -1 : 0;
#pragma clang loop unroll(disable)
  for (int k = K - 2; k >= k_last; --k) {
    const bool start = k < 0;  // row -1: the caller's start set, under actions[0]
    const size_t row = start ? (size_t)env : (size_t)k * n + env;
    const size_t prow = row * (size_t)P;
    const size_t above = (size_t)(k + 1) * n + env;
    const size_t pabove = above * (size_t)P;
    const double* const part = start ? f.part_in_dev : f.part_tape_dev;
    const uint8_t* const pstatus = start ? f.pstatus_in_dev : f.pstatus_tape_dev;
    const double* const lw = start ? f.lw_in_dev : f.lw_tape_dev;
    const uint32_t kg = f.first_step + (uint32_t)k;  // the global index of the row being drawn (first_step - 1 for row -1)

    // ---- the wrench of step k+1 (uniform), as cs_rollout_pf makes it ----
    const float4 act = load_action_at<TASK>(io.actions_dev + above * A);
    const float araw[4] = {act.x, act.y, act.z, act.w};
    float mf[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) mf[j] = clip01(araw[j]);
    Wrench w;
    w.bz = thrust_model(q, mf[0], mf[1], mf[2], mf[3]);
    torque_model(q, mf[0], mf[1], mf[2], mf[3], w);

    // ---- propagate and whiten: y = Linv mu, the status after the step, lw_k ----
#pragma clang loop unroll(disable)
    for (int i = 0; i < per; ++i) {
      const int p = tid + i * bd;
      const int sl = p + ((p >> lg) & pad);
      const double* src = part + (prow + p) * 12;
      double x[12];
#pragma unroll
      for (int j = 0; j < 12; ++j) x[j] = src[j];
      int fs = (int)pstatus[prow + p];
      if (fs != CS_STATUS_LANDED) {
        bool pend = false;
        physics_substeps<FULL, GYRO, false, true>(c, q, w, x, fs, pend, -0.0, -0.0, -0.0);
      }
#pragma unroll
      for (int r = 0; r < 12; ++r) Y[r * slots + sl] = pfs_whiten(scr + kScrLinv, 1, r, x);
      SG[sl] = fs;
      LW[sl] = lw[prow + p];
    }
    __syncthreads();  // (y, the statuses and lw are in the LDS)

    // ---- the paths of this wavefront ----
    bool dead_any = false;
#pragma clang loop unroll(disable)
    for (int m = wave; m < S; m += nw) {
      const int ba = __builtin_amdgcn_readfirstlane(B_above[m]);
      const double* const xa = f.part_tape_dev + (pabove + ba) * 12;
      const int sa = (int)f.pstatus_tape_dev[pabove + ba];
      double xt[12], yt[12];
#pragma unroll
      for (int j = 0; j < 12; ++j) xt[j] = xa[j];
#pragma unroll
      for (int r = 0; r < 12; ++r) yt[r] = pfs_whiten(scr + kScrLinv, 1, r, xt);

      double lb[kPfsMaxRun];
      double mx = -INFINITY;
      const int sl0 = lane * run + (lane & pad);
#pragma unroll
      for (int i = 0; i < kPfsMaxRun; ++i) {
        lb[i] = -INFINITY;
        if (i < run) {
          const int sl = sl0 + i;
          const double t0 = yt[0] - Y[sl];
          double d2 = t0 * t0;
#pragma unroll
          for (int j = 1; j < 12; ++j) {
            const double t = yt[j] - Y[j * slots + sl];
            d2 = d2 + t * t;
          }
          double v = LW[sl] + (-0.5 * d2);
          if (SG[sl] != sa) v = -INFINITY;  // the status is a deterministic part of the transition
          if (!(fabs(v) < INFINITY)) v = -INFINITY;
          lb[i] = v;
          mx = fmax(mx, v);
        }
      }
#pragma unroll
      for (int d = kWave / 2; d >= 1; d >>= 1) mx = fmax(mx, __shfl_xor(mx, d));
      const bool dead = !(mx > -INFINITY);  // no particle can reach the path's next point
      dead_any = dead_any || dead;

      uint32_t bw[kPfsMaxRun];
#pragma unroll
      for (int i = 0; i < kPfsMaxRun; ++i) {
        bw[i] = 0u;
        if (i < run) bw[i] = (uint32_t)rint((dead ? 1.0 : exp(lb[i] - mx)) * 16777216.0);
      }
      unsigned long long excl, incl, s1;
      pfs_scan(bw, run, lane, excl, incl, s1);
      const unsigned long long u = pfs_draw_u(key_pf, g, f.nonce, kg, (uint32_t)m);
      const int idx = pfs_search(bw, run, lane, excl, incl, s1, u, P);
      if (lane == 0) B_here[m] = idx;

      if (!start) {
        const size_t trow = (row * (size_t)S + m) * (size_t)P + lane * run;
        if (f.logb_tape_dev != nullptr) {
#pragma unroll
          for (int i = 0; i < kPfsMaxRun; ++i)
            if (i < run) f.logb_tape_dev[trow + i] = lb[i];
        }
        if (f.bwq_tape_dev != nullptr) {
#pragma unroll
          for (int i = 0; i < kPfsMaxRun; ++i)
            if (i < run) f.bwq_tape_dev[trow + i] = (int32_t)bw[i];
        }
      }
    }
    if (dead_any && lane == 0) flag[0] = 0;
    __syncthreads();  // (the row's indices are in the LDS; y is dead)

    if (start) {
      if (f.idx0_dev != nullptr) {
        for (int m = tid; m < S; m += bd) f.idx0_dev[(size_t)env * S + m] = B_here[m];
      }
    } else {
      emit_row(row, B_here);
    }
    int* const t = B_above;
    B_above = B_here;
    B_here = t;
  }

  __syncthreads();
  if (tid == 0 && f.ok_dev != nullptr) f.ok_dev[env] = (uint8_t)flag[0];
}

template <int TASK, int MODE, bool GYRO>
hipError_t pfs_launch(const DevConst& c, const DevState& s, const cs_rollout_io& io, const cs_pf_smooth_io& f,
                      uint32_t key_pf, hipStream_t stream) {
  const int P = f.num_particles;
  const size_t lds = pfs_lds_bytes(P);
  auto kernel = pf_smooth_kernel<TASK, MODE, GYRO>;
  // (more than 64 KiB of dynamic LDS at P = 1 024: say so to the runtime)
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  const dim3 grid(s.n), block(P < kPfsBlock ? P : kPfsBlock);
  hipLaunchKernelGGL(kernel, grid, block, lds, stream, c, s, io, f, key_pf);
  return hipGetLastError();
}

template <int TASK, int MODE>
hipError_t pfs_t(const DevConst& c, const DevState& s, const cs_rollout_io& io, const cs_pf_smooth_io& f, uint32_t key_pf,
                 hipStream_t stream) {
  if (c.gyro) return pfs_launch<TASK, MODE, true>(c, s, io, f, key_pf, stream);
  return pfs_launch<TASK, MODE, false>(c, s, io, f, key_pf, stream);
}

hipError_t launch_pf_smooth(int task, int mode, const DevConst& c, const DevState& s, const cs_rollout_io& io,
                            const cs_pf_smooth_io& f, uint32_t key_pf, hipStream_t stream) {
  CS_DISPATCH(pfs_t, c, s, io, f, key_pf, stream)
}

}  // namespace
}  // namespace cs

extern "C" int cs_pf_smooth(cs_ctx* ctx, const cs_rollout_io* io, const cs_pf_smooth_io* sio, void* stream) {
  using cs::report_error;
  const char* who = "cs_pf_smooth";
  if (int rc_ = cs::check_rollout_io(io, who, false)) return rc_;
  const bool extra = io->start_x_dev != nullptr || io->start_status_dev != nullptr || io->reward_dev != nullptr ||
                     io->terminated_dev != nullptr || io->truncated_dev != nullptr || io->status_dev != nullptr ||
                     io->gx_dev != nullptr || io->gr_dev != nullptr || io->g_actions_dev != nullptr ||
                     io->g_x0_dev != nullptr;
  if (int rc_ = cs::check_filter_io(
          io, who, {"sio", "cs_pf_smooth_io", sio, sizeof(cs_pf_smooth_io)}, nullptr,
          extra ? "the start, reward, flag, status, cotangent and gradient pointers must be NULL" : nullptr))
    return rc_;
  const int P = sio->num_particles;
  if (P < CS_PF_MIN_PARTICLES || P > CS_PF_MAX_PARTICLES || (P & (P - 1)) != 0)
    return report_error(CS_ERR_ARG,
                        "cs_pf_smooth: num_particles must be a power of two in CS_PF_MIN_PARTICLES .. CS_PF_MAX_PARTICLES");
  if (sio->num_paths < 1 || sio->num_paths > CS_PFS_MAX_PATHS)
    return report_error(CS_ERR_ARG, "cs_pf_smooth: num_paths must be 1 .. CS_PFS_MAX_PATHS");
  if (sio->first_step < 1 || (uint64_t)sio->first_step + (uint64_t)io->num_steps - 1 > 0xFFFFFFFFull)
    return report_error(CS_ERR_ARG, "cs_pf_smooth: first_step must be >= 1 and first_step + num_steps - 1 < 2^32");
  if (sio->part_tape_dev == nullptr || sio->pstatus_tape_dev == nullptr || sio->lw_tape_dev == nullptr ||
      sio->Linv_dev == nullptr)
    return report_error(CS_ERR_ARG,
                        "cs_pf_smooth: part_tape_dev, pstatus_tape_dev, lw_tape_dev and Linv_dev are required");
  if (sio->end_idx_dev == nullptr && sio->wq_tape_dev == nullptr)
    return report_error(CS_ERR_ARG, "cs_pf_smooth: wq_tape_dev is required without end_idx_dev (row K-1 is drawn from it)");
  const bool any_start = sio->part_in_dev != nullptr || sio->pstatus_in_dev != nullptr || sio->lw_in_dev != nullptr;
  const bool all_start = sio->part_in_dev != nullptr && sio->pstatus_in_dev != nullptr && sio->lw_in_dev != nullptr;
  if (any_start && !all_start)
    return report_error(CS_ERR_ARG,
                        "cs_pf_smooth: the start set is part_in_dev, pstatus_in_dev and lw_in_dev: all three or none");
  if (sio->idx0_dev != nullptr && !all_start)
    return report_error(CS_ERR_ARG, "cs_pf_smooth: idx0_dev needs the start set (part_in_dev, pstatus_in_dev, lw_in_dev)");
  cs::ContextView v;
  if (int rc_ = cs::enter_filter_context(
          ctx, who, stream, sio->out_dtype,
          {io->x_dev, sio->part_tape_dev, sio->lw_tape_dev, sio->Linv_dev, sio->part_in_dev, sio->lw_in_dev,
           sio->logb_tape_dev},
          {sio->var_dev},
          {io->actions_dev, sio->wq_tape_dev, sio->end_idx_dev, sio->idx_dev, sio->idx0_dev, sio->bwq_tape_dev},
          "actions_dev or a 32-bit array", &v))
    return rc_;
  const uint32_t key_pf = cs::pf_noise_key(cs::context_seed(ctx));
  const hipError_t e = cs::launch_pf_smooth(v.task, v.mode, *v.c, *v.s, *io, *sio, key_pf, (hipStream_t)stream);
  if (e != hipSuccess) return cs::report_hip(e, "cs_pf_smooth: kernel launch");
  return CS_OK;
}
