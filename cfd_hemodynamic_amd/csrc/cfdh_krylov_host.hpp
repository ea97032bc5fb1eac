// The arithmetic of the linear solve that needs no device: the Gram system of the projected guess, the least-squares problem of
// the Arnoldi recurrence, the scale of a Gram-Schmidt pass, the launch-ahead policy and the checks between two cycles.  Plain C++17 without HIP and without the
// context, so that the CPU tests compile it with the host compiler (tests/krylov_host_shim.cpp); gram_solve and gs_scale are also
// called from kernels (cfdh_krylov_vec.hip), which is what keeps the host and the device to ONE copy of each.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#ifdef __HIPCC__
#define CFDH_HD __host__ __device__
#else
#define CFDH_HD
#endif
#ifdef __clang__
#define CFDH_UNROLL _Pragma("unroll")
#else
#define CFDH_UNROLL _Pragma("GCC unroll 8")
#endif

namespace cfdh_krylov {

// c - a b as the compiler in use forms it in a plain loop: one fused operation in device code (hipcc contracts there, and a
// select between the product and the sum must not undo it), a product and a difference on the host
CFDH_HD inline double gram_nmsub(double c, double a, double b) {
#ifdef __HIP_DEVICE_COMPILE__
  return __builtin_fma(-a, b, c);
#else
  return c - a * b;
#endif
}

// The k x k Gram system of the projected guess (k <= 8): y = argmin |b - W y| from the normal equations, by a pivoted Cholesky
// that drops directions which have become numerically dependent -- a pivot whose remaining diagonal is not above 1e-10 of its
// own G_pp, or not above 1e-14 of the largest diagonal entry.  Device layout: hd[8 i + q] = W_q . W_i (i < k), hd[8 k + q] = W_q . b.
// Dropped directions get y = 0.  Rank 0, a non-finite diagonal or a non-finite y: y = 0 and the guess is not used.
//
// K is a template parameter and no array is indexed by a run-time value: every loop has constant bounds, the pivot row and
// column are picked with selects, and a stopped factorisation is a flag instead of a break.  On the device the system then
// lives in registers (one lane, no scratch memory); the operations and their order are those of the plain loops
//   for it < k: p = argmax of the remaining diagonal (first of equals); stop at a dropped pivot; l_pp = sqrt(d_p);
//               t_it = (g_p - sum_{q < it} l_pq t_q) / l_pp                       (forward substitution, row by row)
//               for i not taken: l_i = (G_ip - sum_{q < it} l_iq l_pq) / l_pp, d_i -= l_i^2
//   backward substitution over the taken pivots, last taken first
template <int K>
CFDH_HD inline bool gram_solve_k(const double *hd, double *y, int *rank) {
  double G[K][K], Lc[K][K], dg[K], g[K];
  int piv[K];
  bool taken[K];
  CFDH_UNROLL
  for (int i = 0; i < K; i++) {
    CFDH_UNROLL
    for (int q = 0; q < K; q++) { G[q][i] = hd[i * 8 + q]; Lc[q][i] = 0.0; }
    g[i] = hd[K * 8 + i]; taken[i] = false; piv[i] = -1;
  }
  double dmax0 = 0.0;
  bool ok = true;
  CFDH_UNROLL
  for (int i = 0; i < K; i++) {
    dg[i] = G[i][i];
    if (!std::isfinite(dg[i])) ok = false;
    if (i == 0 || dg[i] > dmax0) dmax0 = dg[i];
  }
  ok = ok && dmax0 > 0.0 && std::isfinite(dmax0);
  // LP: the rows of the factor in pivot order (row `it` is complete when pivot `it` is taken); t: the forward substitution,
  // which needs exactly that row and is done on the spot
  double LP[K][K], t[K], yp[K];
  int r = 0;
  bool go = ok;
  CFDH_UNROLL
  for (int it = 0; it < K; it++) {  // while it runs, r == it
    // the pivot, and with it its diagonal, its right-hand side, column p of G and row p of the factor so far
    int p = -1;
    double dgp = 0.0, gpp = 0.0, gp = 0.0, Gp[K], Lp[K];
    CFDH_UNROLL
    for (int i = 0; i < K; i++) { Gp[i] = 0.0; Lp[i] = 0.0; }
    CFDH_UNROLL
    for (int i = 0; i < K; i++)
      if (!taken[i] && (p < 0 || dg[i] > dgp)) {
        p = i; dgp = dg[i]; gpp = G[i][i]; gp = g[i];
        CFDH_UNROLL
        for (int j = 0; j < K; j++) Gp[j] = G[j][i];
        CFDH_UNROLL
        for (int q = 0; q < it; q++) Lp[q] = Lc[i][q];
      }
    if (p < 0 || !(dgp > 1e-10 * gpp) || !(dgp > 1e-14 * dmax0)) go = false;
    t[it] = 0.0; yp[it] = 0.0;
    CFDH_UNROLL
    for (int q = 0; q < K; q++) LP[it][q] = 0.0;
    if (go) {
      r = it + 1;
      piv[it] = p;
      const double lpp = std::sqrt(dgp);
      CFDH_UNROLL
      for (int q = 0; q < it; q++) LP[it][q] = Lp[q];
      LP[it][it] = lpp;
      double sacc = gp;
      CFDH_UNROLL
      for (int q = 0; q < it; q++) sacc = gram_nmsub(sacc, Lp[q], t[q]);
      t[it] = sacc / lpp;
      CFDH_UNROLL
      for (int i = 0; i < K; i++) {
        if (i == p) taken[i] = true;
        if (taken[i]) continue;
        sacc = Gp[i];
        CFDH_UNROLL
        for (int q = 0; q < it; q++) sacc = gram_nmsub(sacc, Lc[i][q], Lp[q]);
        Lc[i][it] = sacc / lpp;
        dg[i] = gram_nmsub(dg[i], Lc[i][it], Lc[i][it]);
      }
    }
  }
  CFDH_UNROLL
  for (int a = K - 1; a >= 0; a--) {
    if (a < r) {
      double sacc = t[a];
      CFDH_UNROLL
      for (int q = a + 1; q < K; q++) if (q < r) sacc = gram_nmsub(sacc, LP[q][a], yp[q]);
      yp[a] = sacc / LP[a][a];
    }
  }
  double yy[K];
  bool used = ok && r > 0;
  CFDH_UNROLL
  for (int i = 0; i < K; i++) {
    yy[i] = 0.0;
    CFDH_UNROLL
    for (int a = 0; a < K; a++) if (a < r && piv[a] == i) yy[i] = yp[a];
    if (!std::isfinite(yy[i])) used = false;
  }
  CFDH_UNROLL
  for (int i = 0; i < K; i++) y[i] = used ? yy[i] : 0.0;
  *rank = r;
  return used;
}
// the same with k known at run time (host callers); k outside 1 .. 8 has no system to solve: rank 0, not used
CFDH_HD inline bool gram_solve(int k, const double *hd, double *y, int *rank) {
  switch (k) {
    case 1: return gram_solve_k<1>(hd, y, rank);
    case 2: return gram_solve_k<2>(hd, y, rank);
    case 3: return gram_solve_k<3>(hd, y, rank);
    case 4: return gram_solve_k<4>(hd, y, rank);
    case 5: return gram_solve_k<5>(hd, y, rank);
    case 6: return gram_solve_k<6>(hd, y, rank);
    case 7: return gram_solve_k<7>(hd, y, rank);
    case 8: return gram_solve_k<8>(hd, y, rank);
    default: *rank = 0; return false;
  }
}

// Scale of the first Gram-Schmidt pass from the reduced coefficients: s = sqrt(w.w - |h|^2), or, when that difference has
// cancelled (not positive, or above w.w), any positive scale -- the caller re-orthogonalises such a vector.
CFDH_HD inline double gs_scale(double ww, double hh2) {
  const double nrm2 = ww - hh2;
  return (nrm2 > 0.0 && nrm2 <= ww) ? std::sqrt(nrm2) : std::sqrt(ww);
}

// min |beta e_1 - H y| of the Arnoldi recurrence, column by column with Givens rotations (host only: it owns its storage).
// Column j of H sits at H[j (m + 1) ..], already rotated.
struct ArnoldiLsq {
  int m;
  std::vector<double> H, cs, sn, g, y;
  explicit ArnoldiLsq(int m_) : m(m_), H((size_t)(m_ + 1) * m_, 0.0), cs(m_), sn(m_), g(m_ + 1), y(m_) {}
  void start(double beta) {
    std::fill(g.begin(), g.end(), 0.0);
    g[0] = beta;
  }
  // column j = [h_0 .. h_j ; hnorm].  False on breakdown: the new diagonal entry is not positive or not finite.
  bool add_column(int j, const double *h, double hnorm) {
    double *Hj = &H[(size_t)j * (m + 1)];
    for (int i = 0; i <= j; i++) Hj[i] = h[i];
    Hj[j + 1] = hnorm;
    for (int i = 0; i < j; i++) {
      const double t = cs[i] * Hj[i] + sn[i] * Hj[i + 1];
      Hj[i + 1] = -sn[i] * Hj[i] + cs[i] * Hj[i + 1];
      Hj[i] = t;
    }
    const double d = std::hypot(Hj[j], Hj[j + 1]);
    if (!(d > 0) || !std::isfinite(d)) return false;
    cs[j] = Hj[j] / d; sn[j] = Hj[j + 1] / d;
    Hj[j] = d; Hj[j + 1] = 0.0;
    g[j + 1] = -sn[j] * g[j]; g[j] = cs[j] * g[j];
    return true;
  }
  // residual norm of the recurrence after j columns
  double residual(int j) const { return std::fabs(g[j]); }
  // y = H_j^-1 g for the first j columns
  const double *solve(int j) {
    for (int i = j - 1; i >= 0; i--) {
      double s = g[i];
      for (int k = i + 1; k < j; k++) s -= H[(size_t)k * (m + 1) + i] * y[k];
      y[i] = s / H[(size_t)i * (m + 1) + i];
    }
    return y.data();
  }
};

// How far the iterations of a cycle are launched ahead of the host's bookkeeping.  `need` is the number of iterations still
// expected, counted from the last one the host has processed: from the history alone (e_its, the length of the last solve with
// the same Newton index; 0: unknown) before any residual of this cycle is known, afterwards the smaller of the rate-based
// prediction and what the history leaves.
struct LaunchAhead {
  int need = 1;
  double res_hist[4] = {0, 0, 0, 0};
  int nhist = 0;
  int e_its = 0;
  CFDH_HD void start(double beta, int e_its_, int its) {
    e_its = e_its_;
    need = std::max(1, std::min(e_its - its - 2, 3));
    res_hist[0] = beta; res_hist[1] = res_hist[2] = res_hist[3] = 0.0;
    nhist = 1;
  }
  // iterations wanted in flight (one short of the prediction when it is long: the last predicted iteration is confirmed before
  // anything follows it)
  CFDH_HD int in_flight(bool sync_now, int lagmax) const {
    return sync_now ? 1 : std::max(1, std::min(need - (need >= 4 ? 1 : 0), lagmax + 1));
  }
  // the host processes everything launched if that may finish the solve / the cycle, otherwise all but the newest
  CFDH_HD int process_upto(int j, int jl, int maxl, bool sync_now) const {
    return (!sync_now && jl - j > 1 && jl < maxl && need > jl - j) ? jl - 1 : jl;
  }
  // iterations the tolerance is away at the contraction factor of the last (up to three) iterations
  CFDH_HD void observe(double res, double tol, int its) {
    if (nhist < 4) res_hist[nhist++] = res;
    else { res_hist[0] = res_hist[1]; res_hist[1] = res_hist[2]; res_hist[2] = res_hist[3]; res_hist[3] = res; }
    const double rho = std::pow(res / res_hist[0], 1.0 / (nhist - 1));
    int n_rem = (rho > 0.0 && rho < 0.97) ? (int)std::ceil(std::log(tol / res) / std::log(rho)) : (1 << 20);
    if (nhist == 2) n_rem = std::min(n_rem, 3);  // one sample of the rate: a short look ahead only
    need = std::max(1, e_its > 0 ? std::min(n_rem, std::max(e_its - its, 1) + 2) : n_rem);
  }
};

// What the checks between two cycles decide, from the true residual beta formed after a cycle of j_prev columns that started at
// the true residual beta_start and ended with the recurrence estimate est_prev.  Pure: the caller carries out the effects (the
// take-back x -= Z y of a retry, the switches on the context).
//   watchdog  the recurrence lost the true residual (beta > 10 max(est_prev, tol)): the fp32 copy of the basis is the first
//             suspect and is switched off; otherwise long cycles are re-orthogonalised from now on, and the cycle is taken back
//             (retry) when it made the residual worse.  A context that re-orthogonalises already does neither again.
//   stop      attainable accuracy: a second cycle IN A ROW ended converged by the recurrence without halving the true residual,
//             within 10 tol or six orders below |b|.  last_true: the true residual of the last such cycle, -1 after any other.
enum class BetweenFlow { proceed, retry, stop };
enum class BetweenWatchdog { quiet, fp32_off, refine_on };
struct BetweenCycles {
  BetweenFlow flow = BetweenFlow::proceed;
  BetweenWatchdog watchdog = BetweenWatchdog::quiet;
  double last_true = -1.0;
};
inline BetweenCycles between_cycles(int j_prev, double beta, double est_prev, double tol, double bn, double beta_start, double last_true,
                                    bool use32, bool gs_refine_long, bool no_attainable_stop) {
  BetweenCycles d;
  d.last_true = last_true;
  const bool lost = j_prev > 0 && beta > 10.0 * std::max(est_prev, tol);
  if (use32 && lost) {
    d.watchdog = BetweenWatchdog::fp32_off;
  } else if (!gs_refine_long && lost) {
    d.watchdog = BetweenWatchdog::refine_on;
    if (beta > beta_start) { d.flow = BetweenFlow::retry; return d; }
  }
  if (j_prev > 0 && est_prev <= tol && beta > tol && !no_attainable_stop) {
    if (last_true > 0.0 && beta > 0.5 * last_true && (beta <= 10.0 * tol || beta <= 1e-6 * bn)) { d.flow = BetweenFlow::stop; return d; }
    d.last_true = beta;
  } else {
    d.last_true = -1.0;  // a cycle that ended without recurrence convergence (restart): the floor has to be seen twice IN A ROW
  }
  return d;
}

}  // namespace cfdh_krylov
