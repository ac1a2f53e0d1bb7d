// cov_tile.h -- what the lane-private covariance kernels share: the filter's and the smoother's step wrench
// (copterstep_rollout_ekf.hip, copterstep_rollout_rts.hip), the typed store (theirs, copterstep_rollout_pf.hip's and
// copterstep_rollout_lqr.hip's), the packed-triangle kit of the kernels that keep a 12 x 12 symmetric matrix per lane in
// LDS columns (element j of a lane at [j * 64 + lane]), and the covariance prediction P- = A P A^T + Q of the filter and
// its smoother; wave_sync() comes with it (wave_sync.h), and so does the launch of a <TASK, MODE, GYRO> kernel
// (CS_GYRO_LAUNCH).  filter_step.h builds the filters' shared step on it.  Device code of those translation units (included there,
// inside their floating-point-contraction pragma, after rollout_sweep.h); not a stand-alone header.  It is no dev_*.h:
// those are the step kernels' sources, whose hash stamps the committed profiles.  DESIGN.md sections 13, 19 and 20.
#pragma once

#include "ekf_update.h"
#include "wave_sync.h"

namespace cs {
namespace {

// the stage of the 12 x 12 stores: a lane's matrix row-major at stride 145 (odd: the lanes' stage writes fall into
// different banks), over W's 144 rows and one row of padding that a kernel keeps behind them
constexpr int kStageStride = 145;
static_assert(kStageStride * kWave <= kStageStride * kBlock, "the stage fits W and its padding row");

// The body of a CS_DISPATCH target (dev_launch.h) whose kernel is a template over <TASK, MODE, GYRO>: one lane per env,
// the instantiation chosen by the configuration's rotor_gyro.  Host code; `c`, `s` and `stream` are the target's own.
#define CS_GYRO_LAUNCH(KERNEL, ...)                                                               \
  do {                                                                                            \
    const dim3 grid(grid_for(s.n)), block(kBlock);                                                \
    if (c.gyro)                                                                                   \
      hipLaunchKernelGGL((KERNEL<TASK, MODE, true>), grid, block, 0, stream, c, s, __VA_ARGS__);  \
    else                                                                                          \
      hipLaunchKernelGGL((KERNEL<TASK, MODE, false>), grid, block, 0, stream, c, s, __VA_ARGS__); \
    return hipGetLastError();                                                                     \
  } while (0)

__device__ __forceinline__ void store_out(void* dst, size_t at, double v, uint32_t f32) {
  if (f32)
    reinterpret_cast<float*>(dst)[at] = (float)v;
  else
    reinterpret_cast<double*>(dst)[at] = v;
}

// The step's wrench under a known action: the motors clipped to [0, 1] (np.clip, task.py:91) through the float64 motor
// law; *clipped (if asked for) says whether the clip changed any of them.
__device__ __forceinline__ Wrench step_wrench(const Coef& q, const float4& act, bool* clipped = nullptr) {
  const float araw[4] = {act.x, act.y, act.z, act.w};
  float mf[4];
  bool any = false;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    mf[j] = clip01(araw[j]);
    any |= !(araw[j] >= 0.f && araw[j] <= 1.f);
  }
  if (clipped != nullptr) *clipped = any;
  Wrench w;
  w.bz = thrust_model(q, mf[0], mf[1], mf[2], mf[3]);
  torque_model(q, mf[0], mf[1], mf[2], mf[3], w);
  return w;
}

// The wavefront's staged matrices (lane l's at stage[l * kStageStride ..], row-major) to rows `at` .. of an [.., N, 144]
// output: a whole wavefront's 64 x 144 values are one contiguous run, read back linearly so that every store instruction
// writes whole lines; a partial wavefront lane by lane.
__device__ __forceinline__ void store_matrix(void* dst, size_t at, const double* stage, const RowOut& ro, uint32_t f32) {
  if (ro.whole) {
    const size_t base = (at + ro.env0) * 144;
#pragma clang loop unroll(disable)
    for (int v = 0; v < 144; ++v) {
      const int el = v * kWave + ro.lane;
      const int ln = el / 144, idx = el - ln * 144;
      store_out(dst, base + el, stage[ln * kStageStride + idx], f32);
    }
  } else if (ro.valid) {
    const size_t base = (at + ro.i) * 144;
    const double* mine = stage + ro.lane * kStageStride;
#pragma clang loop unroll(disable)
    for (int v = 0; v < 144; ++v) store_out(dst, base + v, mine[v], f32);
  }
}

// the upper triangle of a row-major 12 x 12 matrix in global memory -> a packed triangle in the lane's LDS column
// (unrolled: the 78 loads are independent and in flight together; one at a time they would cost 78 L2 latencies a step)
__device__ __forceinline__ void load_triangle(double* T, const double* p) {
#pragma unroll
  for (int a = 0; a < 12; ++a) {
#pragma unroll
    for (int j = a; j < 12; ++j) T[(j * (j + 1) / 2 + a) * kBlock] = p[a * 12 + j];
  }
}

// a packed triangle -> the lane's stage, full and symmetric (the caller syncs the wavefront before the stage is stored)
__device__ __forceinline__ void stage_triangle(double* mine, const double* T) {
#pragma clang loop unroll(disable)
  for (int a = 0; a < 12; ++a) {
#pragma unroll
    for (int b = 0; b < 12; ++b) mine[a * 12 + b] = T[ekf_sym_at(a, b) * kBlock];
  }
}

// The covariance prediction of one step, in place: the packed triangle T (P on entry, P- = A P A^T + Q on exit) and the
// 144 rows W (W = A P on exit, W[i][c] at i * 12 + c), both lane-private LDS columns.  A is the step Jacobian at the
// point x_point[j * x_stride], j < 12, with status fs0 under the wrench w, applied through jacobian_block
// (jacobian_tangents.h) with zero wrench tangents -- the actions are known -- in two passes of 6 blocks of 2 directions:
// the columns of P give W = A P, the rows of W give A W^T = (A P A^T)^T, whose upper triangle is kept.  The point is
// read again for every block: where it lies (LDS, a tape in global memory) is the caller's.  Returns the OR of the
// blocks' branch bits.  The filter and its smoother both call this: the smoother's P- is the filter's prior bit for bit
// because it is the same function of the same arguments.
template <bool FULL, bool GYRO>
__device__ __forceinline__ uint32_t cov_predict(const DevConst& c, const Coef& q, const Wrench& w, int fs0,
                                                const double* x_point, size_t x_stride, double* T, double* W,
                                                const double* Q_dev) {
  uint32_t bits = 0u;
  const Wrench zero{0.0, 0.0, 0.0, 0.0, 0.0};
#pragma clang loop unroll(disable)
  for (int b = 0; b < 12; ++b) {
    const bool second = b >= 6;  // pass 1: columns 2 b', 2 b' + 1 of P -> those of W; pass 2: rows of W -> columns of P-
    const int c0 = (second ? b - 6 : b) * kJacDirs;
    JacPoint pt;
#pragma unroll
    for (int j = 0; j < 12; ++j) pt.x[j] = x_point[j * x_stride];
    pt.fs = fs0;
    pt.active = fs0 != CS_STATUS_LANDED;
    pt.px = pt.py = pt.pz = -0.0;
    double v[kJacDirs][12];
    const Wrench dw[kJacDirs] = {zero, zero};
#pragma unroll
    for (int d = 0; d < kJacDirs; ++d) {
#pragma unroll
      for (int j = 0; j < 12; ++j)
        v[d][j] = second ? W[((c0 + d) * 12 + j) * kBlock] : T[ekf_sym_at(j, c0 + d) * kBlock];
    }
    double xn[12];
    bits |= jacobian_block<FULL, GYRO>(c, q, w, dw, pt, xn, v);
    if (!second) {
#pragma unroll
      for (int d = 0; d < kJacDirs; ++d) {
#pragma unroll
        for (int j = 0; j < 12; ++j) W[(j * 12 + c0 + d) * kBlock] = v[d][j];
      }
    } else {  // column c0 + d of P- above its diagonal (every column of P was read in pass 1), plus Q
#pragma unroll
      for (int d = 0; d < kJacDirs; ++d) {
        const int col = c0 + d;
#pragma unroll
        for (int j = 0; j < 12; ++j) {
          if (j <= col) T[(col * (col + 1) / 2 + j) * kBlock] = v[d][j] + Q_dev[j * 12 + col];
        }
      }
    }
  }
  return bits;
}

}  // namespace
}  // namespace cs
