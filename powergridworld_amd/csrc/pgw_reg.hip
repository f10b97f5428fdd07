// RegControl on the general power flow (include/pgw.h, "RegControl"): the
// per-env Woodbury factor K(t) of the regulators' tap deviation and the
// control pass of OpenDSS's RegControl in STATIC mode.  Replaces what the
// OpenDSS engine does inside the reference's `Solve mode=snap`
// (gridworld/distribution_system/opendss.py:134) for a feeder file with
// RegControl objects (opendss.py:36-39 redirects any DSS file); the rules are
// restated from OpenDSS's published RegControl / SolveSnap documentation in
// oracle/pf_oracle.py (Feeder.solve_regulated), which the tests compare.
//
// Layout (gfx950): the factor is one wave per one or two envs -- lane j owns
// column j of the env's augmented [I + D S | D] (r <= 24 rows, 2r <= 48
// columns; two envs of 32 lanes each when 2r <= 32) in LDS,
// Gauss-Jordan with partial pivoting, the pivot column read into registers
// before the wave updates its columns; the control pass is one lane per env
// (a handful of complex multiply-adds per RegControl; Sample's options --
// PTphase=max / min, a remote regulated bus, Vlimit, inverse time -- are
// per-control branches on uniform settings).  Both are tiny next to
// the power flow itself: K is rebuilt only for the envs whose taps moved.
// The per-env bodies are device functions in pgw_reg.h, shared with the control
// loop that runs inside the general power flow's block (k_pf_regulated).
#include <cmath>

#include "pgw_common.h"
#include "pgw_reg.h"

namespace pgw {

// One block of 64 lanes per EPB envs (reg_factor_env: the per-env body).
template <int EPB>
__global__ void __launch_bounds__(64) k_reg_factor(pgw_reg_params p_, int64_t n, const double* __restrict__ taps,
                                                   const int32_t* __restrict__ active, double* __restrict__ K) {
  const pgw_reg_params& p = PGW_KERNARG0(pgw_reg_params);
  const int lane = threadIdx.x, h = lane / RegFactorShape<EPB>::COLS;
  const int64_t e = (int64_t)blockIdx.x * EPB + h;
  const bool live = e < n && (!active || active[e] != 0);
  if (!__syncthreads_or(live)) return;      // (uniform: every lane of the block takes it)
  __shared__ c2 A[RegFactorShape<EPB>::SCRATCH];
  reg_factor_env<EPB, true>(p, n, e, e < n ? e : 0, live, lane, A, taps, K);
}

__global__ void __launch_bounds__(kBlock) k_reg_control(pgw_reg_params p_, int64_t n, const double* __restrict__ rx,
                                                        const double* __restrict__ rc, double* __restrict__ taps,
                                                        int32_t* __restrict__ active, int32_t* __restrict__ n_changed) {
  const pgw_reg_params& p = PGW_KERNARG0(pgw_reg_params);
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e >= n) return;
  const bool moved = reg_control_env(p, rx, rc, n, e, taps, n, e);
  active[e] = moved ? 1 : 0;
  if (moved && n_changed) atomicAdd(n_changed, 1);
}

int32_t reg_check(const pgw_reg_params* p, const char* who) {
  PGW_REQUIRE(p && p->r_reg >= 1 && p->r_reg <= p->n_reg && p->n_reg <= PGW_PFG_MAX_REG && p->S && p->rho,
              "%s: bad regulator parameters", who);
  PGW_REQUIRE(p->n_phase >= 1 && p->n_phase <= PGW_REG_MAX_PHASES && p->n_ctrl >= 1 &&
                  p->n_ctrl <= PGW_REG_MAX_CTRL, "%s: %d phases / %d controls", who, p->n_phase, p->n_ctrl);
  for (int q = 0; q < p->n_phase; ++q) {
    const pgw_reg_phase& ph = p->phase[q];
    PGW_REQUIRE(ph.a >= 0 && ph.a < p->r_reg && ph.b >= 0 && ph.b < p->r_reg && ph.a != ph.b &&
                    ph.ctrl >= 0 && ph.ctrl < p->n_ctrl && (ph.tap_winding == 1 || ph.tap_winding == 2),
                "%s: regulated phase %d", who, q);
  }
  for (int g = 0; g < p->n_ctrl; ++g) {
    const pgw_reg_ctrl& C = p->ctrl[g];
    PGW_REQUIRE(C.n_mon >= 1 && C.n_mon <= PGW_REG_MAX_MON && C.pick >= PGW_REG_PICK_PHASE &&
                    C.pick <= PGW_REG_PICK_MIN && (C.pick != PGW_REG_PICK_PHASE || C.n_mon == 1) &&
                    (C.winding == 1 || C.winding == 2) && C.ptratio > 0.0 && C.ctprim > 0.0 && C.incr > 0.0 &&
                    C.vbase > 0.0 && C.min_tap <= C.max_tap && C.max_tap_change >= 1 && C.band > 0.0 &&
                    C.vlimit >= 0.0 && C.vlim_node >= -1 && C.vlim_node < p->r_reg,
                "%s: RegControl %d", who, g);
    for (int i = 0; i < C.n_mon; ++i)
      PGW_REQUIRE(C.mon_node[i] >= 0 && C.mon_node[i] < p->r_reg && C.mon_phase[i] >= 0 &&
                      C.mon_phase[i] < p->n_phase && p->phase[C.mon_phase[i]].ctrl == g,
                  "%s: RegControl %d monitored phase %d", who, g, i);
  }
  return PGW_OK;
}

}  // namespace pgw

using namespace pgw;

extern "C" {

int32_t pgw_reg_factor(const pgw_reg_params* p, int64_t n, const double* taps, const int32_t* active,
                       double* Kreg, void* stream) {
  const int32_t rc = reg_check(p, "pgw_reg_factor");
  if (rc) return rc;
  PGW_REQUIRE(taps && Kreg && n >= 0, "pgw_reg_factor: null argument");
  PGW_REQUIRE(2 * p->r_reg <= 64, "pgw_reg_factor: r_reg %d > 32", p->r_reg);
  if (n == 0) return PGW_OK;
  if (2 * p->r_reg <= 32)
    hipLaunchKernelGGL(k_reg_factor<2>, dim3((unsigned)((n + 1) / 2)), dim3(64), 0, (hipStream_t)stream, *p, n,
                       taps, active, Kreg);
  else
    hipLaunchKernelGGL(k_reg_factor<1>, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, *p, n, taps, active,
                       Kreg);
  return check_launch("k_reg_factor");
}

int32_t pgw_reg_control(const pgw_reg_params* p, int64_t n, const double* reg_x, const double* reg_c,
                        double* taps, int32_t* active, int32_t* n_changed, void* stream) {
  const int32_t rc = reg_check(p, "pgw_reg_control");
  if (rc) return rc;
  PGW_REQUIRE(reg_x && reg_c && taps && active && n >= 0, "pgw_reg_control: null argument");
  if (n == 0) return PGW_OK;
  hipLaunchKernelGGL(k_reg_control, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                     (hipStream_t)stream, *p, n, reg_x, reg_c, taps, active, n_changed);
  return check_launch("k_reg_control");
}

}  // extern "C"
