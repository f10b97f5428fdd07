// The response-table certificate of one interval (distribution_system/
// od_certify.py certify(), restated operation for operation): first-order
// Taylor models of the snap solve's iterates over P in [lo, hi], the band test
// of every element of every iterate, the stopping test of every iteration,
// the FNV signature of the decisions.  One call = one interval = one lane of
// k_pf_od_certify (pgw_pf.hip); host and device so the arithmetic can be
// compared with the Python on a CPU.
//
// Rounding: every multiply and add is separate, as the Python's (contraction
// off in each function below); the matrix products sum j = 0 .. M-1 in order,
// which is not rocBLAS's order -- margins differ from the Python's in the last
// bits, far below the 1e-12 deltas the decisions carry.
#pragma once
#include <math.h>
#include <stdint.h>

#include "pgw.h"

#ifdef __HIPCC__
#define PGW_CERT_HD __host__ __device__ __forceinline__
#else
#define PGW_CERT_HD inline
#endif

// max / min that hand a NaN on, as torch.maximum / torch.minimum do
PGW_CERT_HD double cert_max(double x, double y) { return (x != x || y != y) ? NAN : (x > y ? x : y); }
PGW_CERT_HD double cert_min(double x, double y) { return (x != x || y != y) ? NAN : (x < y ? x : y); }

// |x| of the model (ar + i ai) + (br + i bi) t + R, |R| <= e (od_certify._mag):
// magnitude at t = 0, slope, remainder (inf where |a| <= |b|)
PGW_CERT_HD void cert_mag(double ar, double ai, double br, double bi, double e, double& m0, double& m1,
                          double& rem) {
#pragma clang fp contract(off)
  const double aa = hypot(ar, ai), ba = hypot(br, bi);
  m1 = (ar * br + ai * bi) / (aa > 0.0 ? aa : 1.0);
  const double gap = aa - ba;
  rem = gap > 0.0 ? e + ba * ba / (2.0 * gap) : (double)INFINITY;
  m0 = aa;
}

// Row n of const + Mat x for the models x = (xa, xb, xe)[M] (od_certify._lin)
template <int M>
PGW_CERT_HD void cert_row(const double* __restrict__ mat, const double* __restrict__ mabs,
                          const double* __restrict__ cst, int n, const double* xar, const double* xai,
                          const double* xbr, const double* xbi, const double* xe, double& ar, double& ai,
                          double& br, double& bi, double& e) {
#pragma clang fp contract(off)
  const double* g = mat + 2 * (int64_t)n * M;
  const double* ga = mabs + (int64_t)n * M;
  double sar = 0.0, sai = 0.0, sbr = 0.0, sbi = 0.0, se = 0.0;
#pragma unroll
  for (int j = 0; j < M; ++j) {
    const double gr = g[2 * j], gi = g[2 * j + 1];
    sar += xar[j] * gr - xai[j] * gi;
    sai += xar[j] * gi + xai[j] * gr;
    sbr += xbr[j] * gr - xbi[j] * gi;
    sbi += xbr[j] * gi + xbi[j] * gr;
    se += xe[j] * ga[j];
  }
  ar = cst[2 * n] + sar;
  ai = cst[2 * n + 1] + sai;
  br = sbr;
  bi = sbi;
  e = se;
}

// One interval.  prev: 3 n_nodes doubles of this lane, element q at
// prev[q * stride] (the previous iteration's node magnitude models).
// *ok_out: 1 when every decision is certain; *ret_out: the iteration count,
// negative when stopped by max_iter (or by a failed decision); *sig_out: od_solve's
// SIG hash of the bands and the count.
template <int M>
PGW_CERT_HD void od_certify_lane(const pgw_od_certify_model& a, int h, double lo, double hi,
                                 double* __restrict__ prev, int stride, int32_t* ok_out, int32_t* ret_out,
                                 uint64_t* sig_out) {
#pragma clang fp contract(off)
  const int N = a.n_nodes;
  const double c = 0.5 * (lo + hi), r = 0.5 * (hi - lo);
  const double thr[3] = {a.lo2, a.mn2, a.mx2};
  const double tol_yes = a.tol - a.delta_stop, tol_no = a.tol + a.delta_stop;
  const double* u1b = a.u1b + 2 * (int64_t)h * M;
  const double* J0 = a.J0 + 2 * (int64_t)h * M;
  const double* s0 = a.s0 + 2 * (int64_t)h * M;
  // u_1 and iteration 1's currents: affine in P, no remainder
  double uar[M], uai[M], ubr[M], ubi[M], ue[M];
  double jar[M], jai[M], jbr[M], jbi[M], je[M];
#pragma unroll
  for (int k = 0; k < M; ++k) {
    uar[k] = u1b[2 * k] + c * a.u1P[2 * k];
    uai[k] = u1b[2 * k + 1] + c * a.u1P[2 * k + 1];
    ubr[k] = r * a.u1P[2 * k];
    ubi[k] = r * a.u1P[2 * k + 1];
    ue[k] = 0.0;
    jar[k] = J0[2 * k] + c * a.jP[2 * k];
    jai[k] = J0[2 * k + 1] + c * a.jP[2 * k + 1];
    jbr[k] = r * a.jP[2 * k];
    jbi[k] = r * a.jP[2 * k + 1];
    je[k] = 0.0;
  }
#pragma unroll 1
  for (int n = 0; n < N; ++n) {
    double var, vai, vbr, vbi, ve, p0, p1, pr;
    cert_row<M>(a.G, a.Ga, a.V0, n, jar, jai, jbr, jbi, je, var, vai, vbr, vbi, ve);
    cert_mag(var, vai, vbr, vbi, ve, p0, p1, pr);
    prev[(3 * n + 0) * (int64_t)stride] = p0;
    prev[(3 * n + 1) * (int64_t)stride] = p1;
    prev[(3 * n + 2) * (int64_t)stride] = pr;
  }
  bool ok = true, conv = false;
  int its = 1;
  uint64_t sig = 0xcbf29ce484222325ull;
  const uint64_t prime = 0x100000001b3ull;
  for (int it = 2; it <= a.max_iter; ++it) {
    // ---- the bands of u_{it-1}, g = 1 / clamp(|u|^2) per band, the currents
    uint64_t bands = 0;
    bool certain = true;
#pragma unroll
    for (int k = 0; k < M; ++k) {
      const double ar = uar[k], ai = uai[k], br = ubr[k], bi = ubi[k], e = ue[k];
      // |u|^2 as a real model and its range (od_certify._mag2)
      const double m0 = ar * ar + ai * ai;
      const double m1 = 2.0 * (ar * br + ai * bi);
      const double q2 = br * br + bi * bi;
      const double qmax = m0 + fabs(m1) + q2;
      const double q2s = q2 > 0.0 ? q2 : 1.0;
      const double tv = q2 > 0.0 ? -m1 / (2.0 * q2s) : 0.0;
      const bool inside = q2 > 0.0 && fabs(tv) <= 1.0;
      double qmin = inside ? m0 - m1 * m1 / (4.0 * q2s) : m0 - fabs(m1) + q2;
      qmin = qmin < 0.0 ? 0.0 : qmin;
      double rlo = sqrt(qmin) - e;
      rlo = rlo < 0.0 ? 0.0 : rlo;
      const double mlo = rlo * rlo;
      const double rhi = sqrt(qmax) + e;
      const double mhi = rhi * rhi;
      const double aa = hypot(ar, ai), ba = hypot(br, bi);
      const double em = q2 + 2.0 * (aa + ba) * e + e * e;
      int b = 0;
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const bool above = mlo > thr[q] + a.delta_band, below = mhi < thr[q] - a.delta_band;
        certain &= above | below;
        b += above ? 1 : 0;
      }
      bands |= (uint64_t)b << (2 * k);
      const bool inband = b == 2;
      const double safe = inband ? m0 : 1.0;
      const double g0 = inband ? 1.0 / safe : (b == 1 ? 1.0 / a.mn2 : (b == 3 ? 1.0 / a.mx2 : 1.0));
      const double g1 = inband ? -m1 / (safe * safe) : 0.0;
      const double mlo_s = inband ? mlo : 1.0;
      const double w = fabs(m1) + em;
      const double eg = inband ? em / (safe * safe) + w * w / (safe * safe * mlo_s) : 0.0;
      certain &= (bool)isfinite(eg);
      // y = s g - y0' with s = s_a + s_b t (od_certify._mul_cr)
      const double sar = s0[2 * k] + c * a.fr[k], sai = s0[2 * k + 1] + 0.0, sbr = r * a.fr[k];
      const double sa_abs = hypot(sar, sai), sb_abs = fabs(sbr);
      const double yar = sar * g0 - a.y0[2 * k], yai = sai * g0 - a.y0[2 * k + 1];
      const double ybr = sar * g1 + sbr * g0, ybi = sai * g1 + 0.0;
      const double ye = sb_abs * fabs(g1) + (sa_abs + sb_abs) * eg;
      // J = y u (od_certify._mul_cc)
      jar[k] = yar * ar - yai * ai;
      jai[k] = yar * ai + yai * ar;
      jbr[k] = (yar * br - yai * bi) + (ybr * ar - ybi * ai);
      jbi[k] = (yar * bi + yai * br) + (ybr * ai + ybi * ar);
      const double ya_abs = hypot(yar, yai), yb_abs = hypot(ybr, ybi);
      je[k] = yb_abs * ba + (ya_abs + yb_abs) * e + (aa + ba) * ye + ye * e;
    }
    ok &= certain;
    sig = (sig ^ bands) * prime;
    // ---- the stopping test: every node's | |V_it| - |V_it-1| | against tol
    bool yes = true, no = false;
#pragma unroll 1
    for (int n = 0; n < N; ++n) {
      double var, vai, vbr, vbi, ve, n0, n1, nr;
      cert_row<M>(a.G, a.Ga, a.V0, n, jar, jai, jbr, jbi, je, var, vai, vbr, vbi, ve);
      cert_mag(var, vai, vbr, vbi, ve, n0, n1, nr);
      double* p = prev + 3 * n * (int64_t)stride;
      const double d0 = n0 - p[0], d1 = n1 - p[stride], dr = nr + p[2 * (int64_t)stride];
      const double dlo = d0 - fabs(d1) - dr, dhi = d0 + fabs(d1) + dr;
      const double amax = cert_max(fabs(dlo), fabs(dhi));
      const double amin = (dlo <= 0.0 && dhi >= 0.0) ? 0.0 : cert_min(fabs(dlo), fabs(dhi));
      yes &= amax <= tol_yes;
      no |= amin > tol_no;
      p[0] = n0;
      p[stride] = n1;
      p[2 * (int64_t)stride] = nr;
    }
    if (it < a.min_iter) {
      yes = false;
      no = true;
    }
    ok &= yes | no;
    its = it;
    conv |= yes;
    if (yes || it >= a.max_iter || !ok) break;
    // ---- u_it = u0 + W J
#pragma unroll
    for (int k = 0; k < M; ++k)
      cert_row<M>(a.W, a.Wa, a.u0, k, jar, jai, jbr, jbi, je, uar[k], uai[k], ubr[k], ubi[k], ue[k]);
  }
  const int32_t ret = conv ? its : -its;
  *ok_out = ok ? 1 : 0;
  *ret_out = ret;
  *sig_out = (sig ^ (uint64_t)(uint32_t)ret) * prime;
}
