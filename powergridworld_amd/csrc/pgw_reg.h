// RegControl device functions (include/pgw.h, "RegControl"): one env's
// Woodbury factor and one env's control pass.  The stand-alone kernels
// (pgw_reg.hip: k_reg_factor, k_reg_control) and the control loop inside the
// general power flow (pgw_pf_general.hip: k_pf_regulated) both call them, so
// an env gets the same instruction sequence whichever kernel serves it.
#pragma once
#include <cmath>

#include "pgw_common.h"

namespace pgw {

constexpr int kRegMax = PGW_PFG_MAX_REG;

struct c2 {
  double x, y;
};
__device__ __forceinline__ c2 cmul(c2 a, c2 b) { return {a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
__device__ __forceinline__ c2 cadd(c2 a, c2 b) { return {a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ c2 csub(c2 a, c2 b) { return {a.x - b.x, a.y - b.y}; }
__device__ __forceinline__ c2 cscale(c2 a, double s) { return {a.x * s, a.y * s}; }

// The regulated phase's primitive admittance at taps (t1, t2) over (a, b).
__device__ __forceinline__ void reg_yprim(const pgw_reg_phase& ph, double t1, double t2, c2& yaa, c2& yab,
                                          c2& ybb) {
  yaa = cscale({ph.A[0], ph.A[1]}, 1.0 / (t1 * t1));
  yab = cscale({ph.B[0], ph.B[1]}, 1.0 / (t1 * t2));
  ybb = cscale({ph.C[0], ph.C[1]}, 1.0 / (t2 * t2));
}
__device__ __forceinline__ void reg_taps(const pgw_reg_phase& ph, double tap, double& t1, double& t2) {
  t1 = ph.tap_winding == 1 ? tap : ph.tap1;
  t2 = ph.tap_winding == 2 ? tap : ph.tap2;
}

// The ordering between the factor's LDS phases.  BLOCK: the 64 lanes are the
// whole block (k_reg_factor).  Otherwise they are one wave of a larger block
// whose other waves factor other envs (or idle): the wave's own LDS accesses
// complete in program order, so only the compiler has to keep them there.
template <bool BLOCK>
__device__ __forceinline__ void reg_factor_sync() {
  if constexpr (BLOCK) {
    __syncthreads();
  } else {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
}

// EPB envs per 64 lanes (2 when 2 r <= 32: lanes 32 h + j serve the h-th env,
// column j), COLS = 64 / EPB columns per env, RMAX rows.
template <int EPB>
struct RegFactorShape {
  static constexpr int COLS = 64 / EPB;
  static constexpr int RMAX = EPB == 2 ? 16 : kRegMax;
  static constexpr int SCRATCH = EPB * RMAX * COLS;     // c2 per 64 lanes
};

// K(t) of the env this lane's half serves: env e (written where live), taps
// read at env ec (a valid index also where e is not).  lane: 0 .. 63; A: the
// 64 lanes' LDS scratch (RegFactorShape<EPB>::SCRATCH).  Every lane of the 64
// calls it (the sync).
template <int EPB, bool BLOCK>
__device__ __forceinline__ void reg_factor_env(const pgw_reg_params& p, int64_t n, int64_t e, int64_t ec,
                                               bool live, int lane, c2* A, const double* taps, double* K) {
  constexpr int COLS = RegFactorShape<EPB>::COLS;
  constexpr int RMAX = RegFactorShape<EPB>::RMAX;
  const int h = lane / COLS, jl = lane % COLS;
  const int r = p.r_reg;
  c2* Ah = A + h * RMAX * COLS;        // env h: row i, column jl at Ah[i COLS + jl]
  // column jl of [I + D S | D] from the sparse D (a 2 x 2 block per regulated
  // phase over its nodes a, b): (D S)[i][j] = sum over the phases holding i of
  // D[i][a] S[a][j] + D[i][b] S[b][j]
  const c2* S = reinterpret_cast<const c2*>(p.S);
  const int j = jl < r ? jl : jl - r;
  const bool mcol = jl < r;
  c2 col[RMAX];
#pragma unroll
  for (int i = 0; i < RMAX; ++i) col[i] = {(mcol && i == j) ? 1.0 : 0.0, 0.0};
  for (int q = 0; q < p.n_phase; ++q) {
    const pgw_reg_phase& ph = p.phase[q];
    double t1, t2;
    reg_taps(ph, taps[(int64_t)ph.ctrl * n + ec], t1, t2);
    c2 aa, ab, bb, aa0, ab0, bb0;
    reg_yprim(ph, t1, t2, aa, ab, bb);
    reg_yprim(ph, ph.tap1, ph.tap2, aa0, ab0, bb0);
    const c2 daa = csub(aa, aa0), dab = csub(ab, ab0), dbb = csub(bb, bb0);
    const int a = ph.a, b = ph.b;
    c2 ta, tb;                                          // this column's entries of rows a, b
    if (mcol) {
      const c2 sa = S[a * r + j], sb = S[b * r + j];
      ta = cadd(cmul(daa, sa), cmul(dab, sb));
      tb = cadd(cmul(dab, sa), cmul(dbb, sb));
    } else {
      ta = (j == a) ? daa : (j == b ? dab : c2{0.0, 0.0});
      tb = (j == a) ? dab : (j == b ? dbb : c2{0.0, 0.0});
    }
#pragma unroll
    for (int i = 0; i < RMAX; ++i) {
      col[i] = (i == a) ? cadd(col[i], ta) : col[i];
      col[i] = (i == b) ? cadd(col[i], tb) : col[i];
    }
  }
#pragma unroll
  for (int i = 0; i < RMAX; ++i)
    if (i < r) Ah[i * COLS + jl] = (jl < 2 * r) ? col[i] : c2{0.0, 0.0};
  reg_factor_sync<BLOCK>();
  bool singular = false;
  for (int c = 0; c < r; ++c) {
    // pivot: the largest |A[i][c]|, i >= c (every lane of the env finds the same row)
    int pr = c;
    double best = -1.0;
    for (int i = c; i < r; ++i) {
      const c2 v = Ah[i * COLS + c];
      const double a2 = v.x * v.x + v.y * v.y;
      if (a2 > best) {
        best = a2;
        pr = i;
      }
    }
    singular = singular || !(best > 0.0) || !isfinite(best);
    c2 pc[RMAX];                        // the pivot column, rows swapped
#pragma unroll
    for (int i = 0; i < RMAX; ++i) {
      const int src = (i == c) ? pr : (i == pr ? c : i);
      pc[i] = i < r ? Ah[src * COLS + c] : c2{0.0, 0.0};
    }
    const c2 rowc = Ah[pr * COLS + jl], rowp = Ah[c * COLS + jl];
    // the pivot itself, pc[c], read at its place: indexing pc by the loop
    // variable would put the whole column in scratch memory
    const c2 pv = Ah[pr * COLS + c];
    reg_factor_sync<BLOCK>();           // (all reads of column c done)
    // normalise the pivot row, eliminate the others (this lane's column)
    const double inv = 1.0 / (pv.x * pv.x + pv.y * pv.y);
    const c2 f = cmul(rowc, {pv.x * inv, -pv.y * inv});
#pragma unroll
    for (int i = 0; i < RMAX; ++i) {
      if (i < r) {
        c2 v;
        if (i == c) v = f;
        else {
          const c2 old = (i == pr) ? rowp : Ah[i * COLS + jl];
          v = csub(old, cmul(pc[i], f));
        }
        Ah[i * COLS + jl] = v;
      }
    }
    reg_factor_sync<BLOCK>();
  }
  // K: columns r .. 2r - 1 hold (I + D S)^-1 D, complex symmetric (D and S
  // are); its upper triangle is stored (column jj: rows 0 .. jj), half the
  // bytes every solve iteration re-reads
  if (live && jl >= r && jl < 2 * r) {
    const int jj = jl - r;
    for (int i = 0; i <= jj; ++i) {
      const c2 v = Ah[i * COLS + jl];
      const int64_t o = 2 * ((int64_t)(i * r - i * (i - 1) / 2 + (jj - i)) * n + e);
      K[o] = singular ? NAN : v.x;
      K[o + 1] = singular ? NAN : v.y;
    }
  }
}

// V at regulator node j: x_j rho_j - sum_l S_jl c_l (c: the env's corrections,
// in registers).  x of the env at rx[2 (j nx + ex)] (+ 1: imaginary).
__device__ __forceinline__ c2 reg_node_v(const pgw_reg_params& p, int j, const double* __restrict__ rx,
                                         const c2 (&c)[kRegMax], int64_t nx, int64_t ex) {
  const int r = p.r_reg;
  const c2* S = reinterpret_cast<const c2*>(p.S);
  c2 v = cscale({rx[2 * ((int64_t)j * nx + ex)], rx[2 * ((int64_t)j * nx + ex) + 1]}, p.rho[j]);
#pragma unroll
  for (int l = 0; l < kRegMax; ++l)
    if (l < r) v = csub(v, cmul(S[j * r + l], c[l]));
  return v;
}

// One control pass of env e (RegControl.Sample + DoPendingAction, STATIC
// mode): x and c of its accepted solve at rx / rc [2 (j nx + ex)] -- the
// reg_x / reg_c buffers (nx = n, ex = e) or a block's LDS copy (nx = 64, ex =
// lane) -- its taps at taps[g n + e], updated.  True where a tap moved.
__device__ __forceinline__ bool reg_control_env(const pgw_reg_params& p, const double* __restrict__ rx,
                                                const double* __restrict__ rc, int64_t nx, int64_t ex,
                                                double* __restrict__ taps, int64_t n, int64_t e) {
  double want[PGW_REG_MAX_CTRL];
  double dmin = INFINITY;
  c2 c[kRegMax];
#pragma unroll
  for (int l = 0; l < kRegMax; ++l)
    c[l] = l < p.r_reg ? c2{rc[2 * ((int64_t)l * nx + ex)], rc[2 * ((int64_t)l * nx + ex) + 1]} : c2{0.0, 0.0};
  double dl[PGW_REG_MAX_CTRL];                       // each acting control's delay
  for (int g = 0; g < p.n_ctrl; ++g) {
    const pgw_reg_ctrl& C = p.ctrl[g];
    const double tap = taps[(int64_t)g * n + e];
    want[g] = tap;
    dl[g] = INFINITY;
    // RegControl.Sample: the monitored voltage -- the PT phase's, or with
    // PTphase=max / min the phase of largest / smallest |V| (the first on a
    // tie) -- on the 120-V base (V / PTratio)
    int k = 0;
    c2 vk = reg_node_v(p, C.mon_node[0], rx, c, nx, ex);
    double mk = sqrt(vk.x * vk.x + vk.y * vk.y);
    for (int i = 1; i < C.n_mon; ++i) {
      const c2 v = reg_node_v(p, C.mon_node[i], rx, c, nx, ex);
      const double mv = sqrt(v.x * v.x + v.y * v.y);
      if (C.pick == PGW_REG_PICK_MAX ? mv > mk : mv < mk) {
        k = i;
        vk = v;
        mk = mv;
      }
    }
    c2 vc = {vk.x / C.ptratio, vk.y / C.ptratio};
    // Vlimit: the local voltage -- the control voltage before LDC, or with a
    // regulated bus the winding's first phase (V / PTratio)
    double vlocal = 0.0;
    if (C.vlimit > 0.0) {
      if (C.vlim_node >= 0) {
        const c2 vl = reg_node_v(p, C.vlim_node, rx, c, nx, ex);
        vlocal = sqrt((vl.x / C.ptratio) * (vl.x / C.ptratio) + (vl.y / C.ptratio) * (vl.y / C.ptratio));
      } else {
        vlocal = sqrt(vc.x * vc.x + vc.y * vc.y);
      }
    }
    // the line-drop compensation (R + jX) I / CTprim, I the current the
    // controlled phase delivers from the monitored winding into its bus
    if (C.ldc) {
      const pgw_reg_phase& ph = p.phase[C.mon_phase[k]];
      double t1, t2;
      reg_taps(ph, tap, t1, t2);
      c2 yaa, yab, ybb;
      reg_yprim(ph, t1, t2, yaa, yab, ybb);
      const c2 va = reg_node_v(p, ph.a, rx, c, nx, ex), vb = reg_node_v(p, ph.b, rx, c, nx, ex);
      const c2 i_in = C.winding == 2 ? cadd(cmul(yab, va), cmul(ybb, vb)) : cadd(cmul(yaa, va), cmul(yab, vb));
      const c2 i_out = cscale(i_in, -1.0 / C.ctprim);
      vc = csub(vc, cmul({C.r_ldc, C.x_ldc}, i_out));
    }
    const double vact = sqrt(vc.x * vc.x + vc.y * vc.y);
    const double dv = C.vreg - vact;
    const bool over = C.vlimit > 0.0 && vlocal > C.vlimit;
    if (fabs(dv) > C.band * 0.5 || over) {
      // DoPendingAction (STATIC): the needed change (above Vlimit: down to it),
      // truncated to whole taps, at least one, at most max_tap_change, inside
      // [min_tap, max_tap]
      const double need = (over ? C.vlimit - vlocal : dv) / C.vbase;
      double steps = trunc(fabs(need) / C.incr);
      steps = fmin(fmax(steps, 1.0), (double)C.max_tap_change);
      double nt = tap + (need > 0.0 ? steps : -steps) * C.incr;
      nt = fmin(fmax(nt, C.min_tap), C.max_tap);
      if (nt != tap) {
        want[g] = nt;
        dl[g] = C.inverse_time ? C.delay / fmin(10.0, 2.0 * fabs(dv) / C.band) : C.delay;
        dmin = fmin(dmin, dl[g]);
      }
    }
  }
  // ControlQueue.DoNearestActions: only the actions with the smallest delay
  bool moved = false;
  for (int g = 0; g < p.n_ctrl; ++g) {
    const double tap = taps[(int64_t)g * n + e];
    if (want[g] != tap && dl[g] == dmin) {
      taps[(int64_t)g * n + e] = want[g];
      moved = true;
    }
  }
  return moved;
}

// (pgw_reg.hip) the argument checks of the pgw_reg_* entries
int32_t reg_check(const pgw_reg_params* p, const char* who);

}  // namespace pgw
