// lqr_step.h -- the Riccati sweep of the iLQR backward passes (cs_rollout_lqr, copterstep_rollout_lqr.hip, and
// cs_ilqr_box_backward, copterstep_ilqr_box.hip): one step of the recursion and the K-step sweep around it, with the
// A x A solve of a step -- d and the gains' columns -- a policy parameter: LqrFreeSolve, the unconstrained Cholesky
// solve, or LqrBoxSolve, the box-constrained programme of boxqp_solve.h.  Everything else -- the tape, the start rules,
// the 25 + A adjoint calls, the S / s update, the outputs and their staging -- is shared.  Device code of those two
// translation units (included there, inside their floating-point-contraction pragma, after rollout_sweep.h and
// cov_tile.h); not a stand-alone header.  DESIGN.md sections 13 and 24.
//
// One lane per env on the tile layout of the step kernels (tile t -> workgroup t).  The backward never forms the step
// Jacobians A, B: every product with them is a call of step_adjoint (rollout_step.h) with no reward cotangent, which
// returns (A^T lambda, B^T lambda) under every branch rule the rollout backward obeys.  Per step, with V = S + Q:
//   1 call   on v                       -> Qx, Qu
//   12 calls on the columns of V        -> W = A^T V and B^T V
//   A calls  on the columns of V B      -> B^T V B
//   12 calls on the columns of V A = W^T -> A^T V A and B^T V A
// All matrices live in lane-private LDS columns (element j of a lane at [j * 64 + lane], as section 11's accumulators):
// the adjoint's primal recompute already needs the whole register file.  302 rows x 512 B = 151 KiB for A = 4: one
// wavefront per CU (profiles/rollout_lqr_resources.txt).  The solve policies work in registers between the sweep's
// synchronisation points and take no LDS.
#pragma once

#include "lqr_solve.h"
#include "boxqp_solve.h"

namespace cs {
namespace {

// what the backward kernel reads and writes beyond cs_rollout_io: cs_rollout_lqr_io, checked
struct LqrArgs {
  const double* q;
  const double* r;
  const double* Q;
  const double* Qf;  // Q at the last step (== Q without a Q_final)
  const double* R;
  double mu;
  void* K;
  void* d;
  void* dV;
  void* S0;
  void* s0;
  uint8_t* ok;
  uint32_t f32;
};

// the lane's LDS rows (row j at [j * kBlock]): the packed upper triangle of S / V / Qxx (column-major: (i, j), i <= j, at
// j (j + 1) / 2 + i), W = A^T V (W[i][c] at i * 12 + c), B^T V then Qux (row a, column c at a * 12 + c), B^T V B, the
// vector s / v / Qx, and Qu.  After the last call of a step W is dead: the gains (row-major per lane, stride 12 A + 1:
// what the wavefront then reads linearly for its stores), G = Quu K + Qux and d are staged in its rows.
constexpr int lqr_rows(int A) { return kEkfSym + 144 + 12 * A + A * A + 12 + A; }
constexpr int kRowW = kEkfSym;
constexpr int kRowBV = kRowW + 144;
constexpr int lqr_row_quu(int A) { return kRowBV + 12 * A; }
constexpr int lqr_row_sv(int A) { return lqr_row_quu(A) + A * A; }
constexpr int lqr_row_qu(int A) { return lqr_row_sv(A) + 12; }
constexpr int kRowG = kRowW + 64;    // (the gain stage takes 12 A + 1 <= 49 rows of W's 144)
constexpr int kRowD = kRowW + 128;   // (A <= 4 doubles per lane: [lane * A + a])
static_assert(lqr_rows(4) * kBlock * sizeof(double) <= 160 * 1024, "the LDS of one CU");

// The solve of a step, a policy of lqr_step: step() takes Quu (full, unregularised), mu, Qu and the step's nominal
// action, factors and leaves d in dd (ok cleared on a bad pivot); gain() turns a column of Qux into the column of K;
// store() writes what the policy reports per (step, env) at `at` = step index x N + env.
//
// the unconstrained solve (cs_rollout_lqr): d = -(Quu + mu I)^-1 Qu, K = -(Quu + mu I)^-1 Qux
template <int A>
struct LqrFreeSolve {
  struct Args {};
  double fac[A * A];
  __device__ __forceinline__ explicit LqrFreeSolve(const Args&) {}
  __device__ __forceinline__ void step(const double (&quu)[A * A], double mu, const double (&qu)[A], const float4&,
                                       bool, double (&dd)[A], bool& ok) {
#pragma unroll
    for (int j = 0; j < A * A; ++j) fac[j] = quu[j];
#pragma unroll
    for (int a = 0; a < A; ++a) fac[a * A + a] = quu[a * A + a] + mu;
    const bool pd = lqr_cholesky<A>(fac);
    ok = ok && pd;
#pragma unroll
    for (int a = 0; a < A; ++a) dd[a] = qu[a];
    lqr_solve<A>(fac, dd);
#pragma unroll
    for (int a = 0; a < A; ++a) dd[a] = -dd[a];
  }
  __device__ __forceinline__ void gain(double (&kk)[A]) const {
    lqr_solve<A>(fac, kk);
#pragma unroll
    for (int a = 0; a < A; ++a) kk[a] = -kk[a];
  }
  __device__ __forceinline__ void store(size_t, bool) const {}
};

// the box-constrained solve (cs_ilqr_box_backward): d minimises 1/2 d^T (Quu + mu I) d + Qu^T d over lo - abar <= d <=
// hi - abar (boxqp_solve.h), the gains' free rows are -(H_ff)^-1 Qux_f and their clamped rows 0.  A resetting step
// (Qux = 0, Quu = R: the env ignores its action) takes the clamped start and no iteration.
template <int A>
struct LqrBoxSolve {
  struct Args {
    const float* lo;
    const float* hi;
    uint8_t* clamped;
    uint8_t* iters;
  };
  Args g;
  BoxQp<A> qp;
  __device__ __forceinline__ explicit LqrBoxSolve(const Args& args) : g(args) {}
  __device__ __forceinline__ void step(const double (&quu)[A * A], double mu, const double (&qu)[A], const float4& act,
                                       bool resetting, double (&dd)[A], bool& ok) {
    double h[A * A], fach[A * A], l[A], u[A];
    const float abar[4] = {act.x, act.y, act.z, act.w};  // (load_action_at's fan-out: the first A are the action)
#pragma unroll
    for (int j = 0; j < A * A; ++j) h[j] = quu[j];
#pragma unroll
    for (int a = 0; a < A; ++a) h[a * A + a] = quu[a * A + a] + mu;
#pragma unroll
    for (int j = 0; j < A * A; ++j) fach[j] = h[j];
    const bool pd = lqr_cholesky<A>(fach);
#pragma unroll
    for (int a = 0; a < A; ++a) {
      l[a] = (double)g.lo[a] - (double)abar[a];
      u[a] = (double)g.hi[a] - (double)abar[a];
    }
    boxqp_solve<A>(h, fach, qu, l, u, resetting ? 0 : kBoxQpIters, qp);
    ok = ok && pd && qp.ok;
#pragma unroll
    for (int a = 0; a < A; ++a) dd[a] = qp.x[a];
  }
  __device__ __forceinline__ void gain(double (&kk)[A]) const { boxqp_gain<A>(qp, kk); }
  __device__ __forceinline__ void store(size_t at, bool valid) const {
    if (valid) {
      if (g.clamped != nullptr) g.clamped[at] = (uint8_t)(qp.lower | (qp.upper << 4));
      if (g.iters != nullptr) g.iters[at] = (uint8_t)qp.iters;
    }
  }
};

// One step of the recursion: on entry the lane's S, s are those after the step (0 beyond the horizon), on exit those
// before it; its gains go out to row `row` (= step index x N) of K_dev, d_dev.  P = the lane's LDS column, wbase = the
// wavefront's W rows (the staging area).  sa: the solve policy's arguments.
template <int TASK, int MODE, bool GYRO, template <int> class SOLVE>
__device__ __forceinline__ void lqr_step(const DevConst& c, const Coef& q, const StepIn& in, double px, double py,
                                         double pz, bool resetting, size_t row, bool last, uint32_t ii,
                                         const RowOut& ro, const LqrArgs& l,
                                         const typename SOLVE<task_act_dim(TASK)>::Args& sa, double* P, double* wbase,
                                         double& dv1, double& dv2, bool& ok) {
  constexpr int A = task_act_dim(TASK);
  constexpr int KW = 12 * A;  // a lane's gain row
  double* const S = P;
  double* const W = P + kRowW * kBlock;
  double* const BV = P + kRowBV * kBlock;
  double* const QUU = P + lqr_row_quu(A) * kBlock;
  double* const SV = P + lqr_row_sv(A) * kBlock;
  double* const QU = P + lqr_row_qu(A) * kBlock;

  // ---- V = S + Q_k (in S's rows), v = s + q_k (in s's) ----
  const double* Qm = last ? l.Qf : l.Q;
#pragma clang loop unroll(disable)
  for (int j = 0; j < 12; ++j) {
#pragma clang loop unroll(disable)
    for (int i = 0; i <= j; ++i) S[(j * (j + 1) / 2 + i) * kBlock] += Qm[i * 12 + j];
  }
  if (l.q != nullptr) {
    const double2* g = reinterpret_cast<const double2*>(l.q + (row + ii) * 12);
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      const double2 v = g[j];
      SV[(2 * j) * kBlock] += v.x;
      SV[(2 * j + 1) * kBlock] += v.y;
    }
  }

  // ---- the 25 + A products with A^T, B^T: one call site, the covector and the results' places picked by the index ----
  constexpr int kEndV = 13, kEndB = 13 + A, kCalls = 25 + A;
#pragma clang loop unroll(disable)
  for (int call = 0; call < kCalls; ++call) {
    double lam[12], ga[4];
    if (call == 0) {
#pragma unroll
      for (int i = 0; i < 12; ++i) lam[i] = SV[i * kBlock];
    } else if (call < kEndV) {  // column call - 1 of V
      const int col = call - 1;
#pragma unroll
      for (int i = 0; i < 12; ++i) lam[i] = S[ekf_sym_at(i, col) * kBlock];
    } else if (call < kEndB) {  // column a of V B = row a of B^T V
      const int a = call - kEndV;
#pragma unroll
      for (int i = 0; i < 12; ++i) lam[i] = BV[(a * 12 + i) * kBlock];
    } else {  // column rr of V A = row rr of W
      const int rr = call - kEndB;
#pragma unroll
      for (int i = 0; i < 12; ++i) lam[i] = W[(rr * 12 + i) * kBlock];
    }
    // (no reward cotangent: prev_none skips the shaping gradients, whose factor would be 0)
    step_adjoint<TASK, MODE, GYRO>(c, q, in, 0.0, px, py, pz, resetting, false, true, nullptr, lam, ga);
    if (call == 0) {  // Qx, Qu = r + B^T v
#pragma unroll
      for (int i = 0; i < 12; ++i) SV[i * kBlock] = lam[i];
#pragma unroll
      for (int a = 0; a < A; ++a) QU[a * kBlock] = l.r != nullptr ? ga[a] + l.r[(row + ii) * A + a] : ga[a];
    } else if (call < kEndV) {
      const int col = call - 1;
#pragma unroll
      for (int i = 0; i < 12; ++i) W[(i * 12 + col) * kBlock] = lam[i];
#pragma unroll
      for (int a = 0; a < A; ++a) BV[(a * 12 + col) * kBlock] = ga[a];
    } else if (call < kEndB) {  // column a of B^T V B
      const int a = call - kEndV;
#pragma unroll
      for (int b = 0; b < A; ++b) QUU[(b * A + a) * kBlock] = ga[b];
    } else {  // column rr of Qxx (its upper part, over V: every column of V has been read) and of Qux (over B^T V)
      const int rr = call - kEndB;
#pragma unroll
      for (int i = 0; i < 12; ++i) {
        if (i <= rr) S[(rr * (rr + 1) / 2 + i) * kBlock] = lam[i];
      }
#pragma unroll
      for (int a = 0; a < A; ++a) BV[(a * 12 + rr) * kBlock] = ga[a];
    }
  }

  // ---- Quu = R + B^T V B (its lower triangle, mirrored), the policy's factor of Quu + mu I, d ----
  double quu[A * A];
#pragma unroll
  for (int a = 0; a < A; ++a) {
#pragma unroll
    for (int b = 0; b <= a; ++b) {
      const double v = l.R[a * A + b] + QUU[(a * A + b) * kBlock];
      quu[a * A + b] = quu[b * A + a] = v;
    }
  }
  double qu[A], dd[A], e[A];
#pragma unroll
  for (int a = 0; a < A; ++a) qu[a] = QU[a * kBlock];
  SOLVE<A> solve(sa);
  solve.step(quu, l.mu, qu, in.act, resetting, dd, ok);
  solve.store(row + ro.i, ro.valid);
#pragma unroll
  for (int a = 0; a < A; ++a) {
    double hd = 0.0;
#pragma unroll
    for (int b = 0; b < A; ++b) hd += quu[a * A + b] * dd[b];
    dv1 += dd[a] * qu[a];
    dv2 += 0.5 * (dd[a] * hd);
    e[a] = hd + qu[a];  // Quu d + Qu
  }

  // ---- K column by column (the policy's gain: -(Quu + mu I)^-1 Qux when nothing is clamped), G = Quu K + Qux; W is
  //      dead, the stage takes its rows ----
  wave_sync();
  double* const kst = wbase + ro.lane * (KW + 1);
  double* const G = P + kRowG * kBlock;
#pragma clang loop unroll(disable)
  for (int j = 0; j < 12; ++j) {
    double rhs[A], kk[A];
#pragma unroll
    for (int a = 0; a < A; ++a) kk[a] = rhs[a] = BV[(a * 12 + j) * kBlock];
    solve.gain(kk);
#pragma unroll
    for (int a = 0; a < A; ++a) kst[a * 12 + j] = kk[a];
#pragma unroll
    for (int a = 0; a < A; ++a) {
      double g = 0.0;
#pragma unroll
      for (int b = 0; b < A; ++b) g += quu[a * A + b] * kk[b];
      G[(a * 12 + j) * kBlock] = g + rhs[a];
    }
  }

  // ---- S <- Qxx + K^T G + Qux^T K (upper triangle), s <- Qx + K^T (Quu d + Qu) + Qux^T d ----
#pragma clang loop unroll(disable)
  for (int j = 0; j < 12; ++j) {
    double kj[A], gj[A];
#pragma unroll
    for (int a = 0; a < A; ++a) {
      kj[a] = kst[a * 12 + j];
      gj[a] = G[(a * 12 + j) * kBlock];
    }
#pragma clang loop unroll(disable)
    for (int i = 0; i <= j; ++i) {
      double acc = S[(j * (j + 1) / 2 + i) * kBlock];
#pragma unroll
      for (int a = 0; a < A; ++a) {
        acc += kst[a * 12 + i] * gj[a];
        acc += BV[(a * 12 + i) * kBlock] * kj[a];
      }
      S[(j * (j + 1) / 2 + i) * kBlock] = acc;
    }
  }
#pragma clang loop unroll(disable)
  for (int i = 0; i < 12; ++i) {
    double acc = SV[i * kBlock];
#pragma unroll
    for (int a = 0; a < A; ++a) {
      acc += kst[a * 12 + i] * e[a];
      acc += BV[(a * 12 + i) * kBlock] * dd[a];
    }
    SV[i * kBlock] = acc;
  }

  // ---- the gains out: a whole wavefront's 64 rows of 12 A values are one contiguous run, read back linearly from the
  //      stage so that every store instruction writes whole lines; a partial wavefront lane by lane ----
  double* const dst = wbase + (kRowD - kRowW) * kBlock;
#pragma unroll
  for (int a = 0; a < A; ++a) dst[ro.lane * A + a] = dd[a];
  wave_sync();
  if (ro.whole) {
    if (l.K != nullptr) {
      const size_t at = (row + ro.env0) * KW;
#pragma clang loop unroll(disable)
      for (int v = 0; v < KW; ++v) {
        const int el = v * kWave + ro.lane;
        const int ln = el / KW, idx = el - ln * KW;
        store_out(l.K, at + el, wbase[ln * (KW + 1) + idx], l.f32);
      }
    }
    if (l.d != nullptr) {
      const size_t at = (row + ro.env0) * A;
#pragma unroll
      for (int v = 0; v < A; ++v) store_out(l.d, at + v * kWave + ro.lane, dst[v * kWave + ro.lane], l.f32);
    }
  } else if (ro.valid) {
    if (l.K != nullptr) {
#pragma clang loop unroll(disable)
      for (int v = 0; v < KW; ++v) store_out(l.K, (row + ro.i) * KW + v, kst[v], l.f32);
    }
    if (l.d != nullptr) {
#pragma unroll
      for (int a = 0; a < A; ++a) store_out(l.d, (row + ro.i) * A + a, dd[a], l.f32);
    }
  }
  wave_sync();  // (the next step's W is written over the stage)
}

// The sweep of a launch over the rollout's tape, k = K .. 1, and its closing stores.  lds: the kernel's lqr_rows(A)
// rows of kBlock doubles.
template <int TASK, int MODE, bool GYRO, template <int> class SOLVE>
__device__ __forceinline__ void lqr_sweep(const DevConst& c, const DevState& s, const cs_rollout_io& io,
                                          const LqrArgs& l, const typename SOLVE<task_act_dim(TASK)>::Args& sa,
                                          double* lds) {
  constexpr int A = task_act_dim(TASK);
  const int lane = threadIdx.x;
  const uint32_t tile_index = blockIdx.x;
  const uint32_t i = tile_index * kBlock + threadIdx.x;
  const uint32_t n = s.n;
  const uint32_t env0 = i - lane;
  const RowOut ro{lane, i, env0, i < n, env0 + (uint32_t)kWave <= n};
  const uint32_t ii = ro.valid ? i : 0u;  // (padding lanes recompute env 0's steps and store nothing)
  const int K = io.num_steps;

  Coef q = uniform_coef(c);
  if (s.veh != nullptr) q = load_coef(s.veh, s.veh_stride, ii);
  double* const P = lds + lane;
  double* const SV = P + lqr_row_sv(A) * kBlock;
#pragma clang loop unroll(disable)
  for (int j = 0; j < kEkfSym; ++j) P[j * kBlock] = 0.0;
#pragma unroll
  for (int j = 0; j < 12; ++j) SV[j * kBlock] = 0.0;
  double dv1 = 0.0, dv2 = 0.0;
  bool ok = true;

  StepIn cur;
  if (K > 1) load_tape_step<TASK>(io, n, ii, K - 1, cur);
#pragma clang loop unroll(disable)
  for (int k = K - 1; k >= 0; --k) {
    StepIn in, nxt;
    double px = -0.0, py = -0.0, pz = -0.0;
    bool resetting = false;
    if (k >= 1) {  // its start is the tape's row k - 1; the earlier step's row is fetched while this one computes
      in = cur;
      nxt = cur;
      if (k >= 2) load_tape_step<TASK>(io, n, ii, k - 1, nxt);
      // the second step of a stored-start lane whose NEXT_STEP reset was pending: the new episode's perturbation enters
      // its first call (rollout_vjp_sweep's peeled step)
      if (k == 1 && io.start_x_dev == nullptr) {
        using TILE = TileIO<MODE>;
        const TILE tile(s, tile_index, lane);
        Env<MODE> e;
        unpack_env<MODE, TILE>(c, tile.load_group(0), tile.load_group(1), tile.load_group(2), tile.load_group(3), e);
        if (e.reset_pending) {
          resolve_episode<MODE>(c, tile, e);
          next_episode<MODE, true>(e);
          pending_perturbation<MODE, true>(c, q, tile, i, e.episode, e.ep_far, true, false, px, py, pz);
        }
      }
    } else {  // the first step: from the start point, decoded as the forward decoded it
      if (io.start_x_dev != nullptr) {
        bool pend;
        double prev_sh;
        explicit_start<TASK, MODE>(c, q, io, i, n, ro.valid, in.x, in.fs, pend, px, py, pz, prev_sh);
      } else {
        using TILE = TileIO<MODE>;
        const TILE tile(s, tile_index, lane);
        Env<MODE> e;
        unpack_env<MODE, TILE>(c, tile.load_group(0), tile.load_group(1), tile.load_group(2), tile.load_group(3), e);
        resolve_episode<MODE>(c, tile, e);
        pending_perturbation<MODE, true>(c, q, tile, i, e.episode, e.ep_far, e.pend, e.expl, px, py, pz);
#pragma unroll
        for (int j = 0; j < 12; ++j) in.x[j] = e.x[j];
        in.fs = e.fs;
        resetting = e.reset_pending;
      }
      in.act = load_action_at<TASK>(io.actions_dev + (size_t)ii * A);
      nxt = in;
    }
    lqr_step<TASK, MODE, GYRO, SOLVE>(c, q, in, px, py, pz, resetting, (size_t)k * n, k == K - 1, ii, ro, l, sa, P,
                                      lds + kRowW * kBlock, dv1, dv2, ok);
    cur = nxt;
  }

  if (ro.valid) {
    if (l.dV != nullptr) {
      store_out(l.dV, (size_t)i * 2, dv1, l.f32);
      store_out(l.dV, (size_t)i * 2 + 1, dv2, l.f32);
    }
    if (l.S0 != nullptr) {
#pragma clang loop unroll(disable)
      for (int a = 0; a < 12; ++a) {
#pragma clang loop unroll(disable)
        for (int b = 0; b < 12; ++b) store_out(l.S0, (size_t)i * 144 + a * 12 + b, P[ekf_sym_at(a, b) * kBlock], l.f32);
      }
    }
    if (l.s0 != nullptr) {
#pragma unroll
      for (int j = 0; j < 12; ++j) store_out(l.s0, (size_t)j * n + i, SV[j * kBlock], l.f32);
    }
    if (l.ok != nullptr) l.ok[i] = ok ? 1 : 0;
  }
}

}  // namespace
}  // namespace cs
