// The linear solves of a pressure-correction step (cfdh_ipcs.hip): BiCGStab + Jacobi on the scalar or the block A1, flexible PCG
// with one V-cycle of the pressure hierarchy, CG + Jacobi on rho M.  The loops keep their scalars on the device: every dot product
// ends in per-block partial sums that a one-block kernel folds into the scalars; a `done` scalar freezes the kernels of the
// iterations launched ahead of the host's convergence test.  ip_solve is the one place that knows which solve takes which matrix,
// weights, driver and work vectors; the step and the cfdh_ipcs_krylov_solve hook both go through it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "cfdh_internal.hpp"
#include "cfdh_ipcs.hpp"

// ---------------------------------------------------------------- Krylov kernels
// y = A x for D interleaved columns (the matrix is read once), eight lanes per row, grid-stride over the rows, with the dot
// products the iteration needs next.  MODE 0: P0 = y . q ; 1: P0 = y . q, P1 = y . y ; 2: y = q - A x, P0 = y . y, P1 = q . q
// (true residual; not frozen by `done`).  BLK: val holds [nnz][D][D] blocks (row-major) on the interleaved vector, the block A1 of
// ipcs_midpoint; otherwise one scalar matrix for the D columns.
template <int D, int MODE, bool BLK>
__global__ __launch_bounds__(TPB) void ip_spmv_kernel(int n, const int *__restrict__ rowptr, const int *__restrict__ col, const double *__restrict__ val,
                                                     const double *__restrict__ x, double *__restrict__ y, const double *__restrict__ q,
                                                     const double *__restrict__ S, double *__restrict__ P) {
  __shared__ double sh[4];
  if (MODE != 2 && S[IP_DONE] != 0.0) return;
  const int l = threadIdx.x & 7;
  double d0 = 0.0, d1 = 0.0;
  for (int base = blockIdx.x * (TPB / 8); base < n; base += gridDim.x * (TPB / 8)) {
    const int row = base + (threadIdx.x >> 3);
    double a[D];
    for (int d = 0; d < D; d++) a[d] = 0.0;
    if (row < n)
      for (int k = rowptr[row] + l; k < rowptr[row + 1]; k += 8) {
        const int j = col[k];
        if constexpr (BLK) {
          const double *v = val + (size_t)k * D * D;
          double xj[D];
          for (int e = 0; e < D; e++) xj[e] = x[(size_t)D * j + e];
          for (int d = 0; d < D; d++)
            for (int e = 0; e < D; e++) a[d] += v[D * d + e] * xj[e];
        } else {
          const double v = val[k];
          for (int d = 0; d < D; d++) a[d] += v * x[(size_t)D * j + d];
        }
      }
    for (int d = 0; d < D; d++) a[d] = group8_sum(a[d]);
    if (row < n && l == 0)
      for (int d = 0; d < D; d++) {
        const double qv = q[(size_t)D * row + d];
        const double r = MODE == 2 ? qv - a[d] : a[d];
        y[(size_t)D * row + d] = r;
        if (MODE == 2) { d0 += r * r; d1 += qv * qv; }
        else { d0 += r * qv; if (MODE == 1) d1 += r * r; }
      }
  }
  d0 = block_sum(d0, sh);
  if (MODE != 0) d1 = block_sum(d1, sh);
  if (threadIdx.x == 0) { P[blockIdx.x] = d0; if (MODE != 0) P[IP_NB + blockIdx.x] = d1; }
}

// one block: fold the partial sums into the scalars.
// STAGE 0 (init / verification): P0 = |r|^2 of the true residual, P1 = |b|^2 ; first != 0 also sets the tolerance and its = 0
//       1: alpha = rho / P0 (BiCGStab)     2: omega = P0 / P1     3: rho_old = rho, rho = P0, |r|^2 = P1, its++, done?
//       4: rz = P0 (CG start)              5: alpha = rz / P0     6: beta = P0 / rz, rz = P0, |r|^2 = P1, its++, done?
//       7: |r|^2 = P0, its++, done? (flexible PCG, before the cycle)   8: beta = -alpha P1 / rz, rz = P0
template <int STAGE>
__global__ __launch_bounds__(TPB) void ip_scal_kernel(int nb, const double *__restrict__ P, double *__restrict__ S, double rtol, double atol,
                                                     int first, double *__restrict__ mirror) {
  __shared__ double sh[4];
  if (STAGE != 0 && S[IP_DONE] != 0.0) return;
  double a = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < nb; i += TPB) { a += P[i]; b += P[IP_NB + i]; }
  a = block_sum(a, sh);
  b = block_sum(b, sh);
  if (threadIdx.x != 0) return;
  bool check = false;
  if (STAGE == 0) {
    if (first) {
      S[IP_BN2] = b; S[IP_ITS] = 0.0; S[IP_BAD] = 0.0;
      const double t = fmax(rtol * sqrt(b), atol);
      S[IP_TOL2] = t * t;
    }
    S[IP_RN2] = a; S[IP_RHO] = a; S[IP_RHO_OLD] = 1.0; S[IP_ALPHA] = 1.0; S[IP_OMEGA] = 1.0; S[IP_BETA] = 0.0;
    S[IP_DONE] = 0.0;
    check = true;
  } else if (STAGE == 1) {
    const double al = S[IP_RHO] / a;
    S[IP_ALPHA] = al;
    if (!isfinite(al)) { S[IP_BAD] = 1.0; S[IP_DONE] = 1.0; }
  } else if (STAGE == 2) {
    const double om = b > 0.0 ? a / b : 0.0;
    S[IP_OMEGA] = om;
    if (!isfinite(om)) { S[IP_BAD] = 1.0; S[IP_DONE] = 1.0; }
  } else if (STAGE == 3) {
    const double ro = S[IP_RHO];
    S[IP_RHO_OLD] = ro; S[IP_RHO] = a;
    S[IP_BETA] = (a / ro) * (S[IP_ALPHA] / S[IP_OMEGA]);
    S[IP_RN2] = b; S[IP_ITS] += 1.0;
    check = true;
  } else if (STAGE == 4) {
    S[IP_RZ] = a;
  } else if (STAGE == 5) {
    const double al = S[IP_RZ] / a;
    S[IP_ALPHA] = al;
    if (!isfinite(al)) { S[IP_BAD] = 1.0; S[IP_DONE] = 1.0; }
  } else if (STAGE == 6) {
    S[IP_BETA] = a / S[IP_RZ]; S[IP_RZ] = a;
    S[IP_RN2] = b; S[IP_ITS] += 1.0;
    check = true;
  } else if (STAGE == 7) {
    S[IP_RN2] = a; S[IP_ITS] += 1.0;
    check = true;
  } else {
    const double be = -S[IP_ALPHA] * b / S[IP_RZ];
    S[IP_BETA] = be; S[IP_RZ] = a;
    if (!isfinite(be) || !isfinite(a)) { S[IP_BAD] = 1.0; S[IP_DONE] = 1.0; }
  }
  if (check) {
    // a finite |r|^2 within the tolerance is convergence whatever beta is (a BiCGStab solve that lands on the solution has s = 0,
    // t = 0, omega = 0, r = 0 and beta = 0 * inf); above the tolerance a beta that is not finite is a breakdown
    const double rn2 = S[IP_RN2];
    if (!isfinite(rn2)) { S[IP_BAD] = 1.0; S[IP_DONE] = 1.0; }
    else if (rn2 <= S[IP_TOL2]) S[IP_DONE] = 1.0;
    else if (STAGE != 0 && STAGE != 7 && !isfinite(S[IP_BETA])) { S[IP_BAD] = 1.0; S[IP_DONE] = 1.0; }
  }
  // every stage publishes (|r|^2, done, its, bad): a breakdown found between two convergence tests freezes the kernels behind it,
  // so the stage that found it is the last one that can tell the host
  for (int i = 0; i < 4; i++) mirror[i] = S[IP_RN2 + i];
}

// BiCGStab, start / restart: rh = r, p = v = 0
__global__ __launch_bounds__(TPB) void ip_bicg_start_kernel(int n, const double *__restrict__ r, double *__restrict__ rh, double *__restrict__ p, double *__restrict__ v) {
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) { rh[i] = r[i]; p[i] = 0.0; v[i] = 0.0; }
}
// p = r + beta (p - omega v) ; y = dinv p (dinv per node, or per unknown for the block matrix: BLK)
template <int D, bool BLK>
__global__ __launch_bounds__(TPB) void ip_bicg1_kernel(int n, const double *__restrict__ S, const double *__restrict__ r, const double *__restrict__ v,
                                                      const double *__restrict__ dinv, double *__restrict__ p, double *__restrict__ y) {
  if (S[IP_DONE] != 0.0) return;
  const double beta = S[IP_BETA], om = S[IP_OMEGA];
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
    const double pn = r[i] + beta * (p[i] - om * v[i]);
    p[i] = pn;
    y[i] = dinv[BLK ? i : i / D] * pn;
  }
}
// s = r - alpha v ; z = dinv s
template <int D, bool BLK>
__global__ __launch_bounds__(TPB) void ip_bicg2_kernel(int n, const double *__restrict__ S, const double *__restrict__ r, const double *__restrict__ v,
                                                      const double *__restrict__ dinv, double *__restrict__ s, double *__restrict__ z) {
  if (S[IP_DONE] != 0.0) return;
  const double al = S[IP_ALPHA];
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
    const double sn = r[i] - al * v[i];
    s[i] = sn;
    z[i] = dinv[BLK ? i : i / D] * sn;
  }
}
// x += alpha y + omega z ; r = s - omega t ; P0 = rh . r, P1 = r . r
__global__ __launch_bounds__(TPB) void ip_bicg3_kernel(int n, const double *__restrict__ S, const double *__restrict__ y, const double *__restrict__ z,
                                                      const double *__restrict__ s, const double *__restrict__ t, const double *__restrict__ rh,
                                                      double *__restrict__ x, double *__restrict__ r, double *__restrict__ P) {
  __shared__ double sh[4];
  if (S[IP_DONE] != 0.0) return;
  const double al = S[IP_ALPHA], om = S[IP_OMEGA];
  double d0 = 0.0, d1 = 0.0;
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
    x[i] += al * y[i] + om * z[i];
    const double rn = s[i] - om * t[i];
    r[i] = rn;
    d0 += rh[i] * rn; d1 += rn * rn;
  }
  d0 = block_sum(d0, sh);
  d1 = block_sum(d1, sh);
  if (threadIdx.x == 0) { P[blockIdx.x] = d0; P[IP_NB + blockIdx.x] = d1; }
}
// CG start: z = dinv r (JAC) or z given ; p = z ; P0 = r . z
template <int D, bool JAC>
__global__ __launch_bounds__(TPB) void ip_cg_start_kernel(int n, const double *__restrict__ r, const double *__restrict__ dinv, double *__restrict__ z,
                                                         double *__restrict__ p, double *__restrict__ P) {
  __shared__ double sh[4];
  double d0 = 0.0;
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
    double zn;
    if (JAC) { zn = dinv[i / D] * r[i]; z[i] = zn; } else zn = z[i];
    p[i] = zn;
    d0 += r[i] * zn;
  }
  d0 = block_sum(d0, sh);
  if (threadIdx.x == 0) { P[blockIdx.x] = d0; P[IP_NB + blockIdx.x] = 0.0; }
}
// x += alpha p ; r -= alpha q ; JAC: z = dinv r, P0 = r . z, P1 = r . r ; else P0 = r . r
template <int D, bool JAC>
__global__ __launch_bounds__(TPB) void ip_cg_x_kernel(int n, const double *__restrict__ S, const double *__restrict__ p, const double *__restrict__ q,
                                                     const double *__restrict__ dinv, double *__restrict__ x, double *__restrict__ r, double *__restrict__ z,
                                                     double *__restrict__ P) {
  __shared__ double sh[4];
  if (S[IP_DONE] != 0.0) return;
  const double al = S[IP_ALPHA];
  double d0 = 0.0, d1 = 0.0;
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
    x[i] += al * p[i];
    const double rn = r[i] - al * q[i];
    r[i] = rn;
    if (JAC) { const double zn = dinv[i / D] * rn; z[i] = zn; d0 += rn * zn; d1 += rn * rn; }
    else d0 += rn * rn;
  }
  d0 = block_sum(d0, sh);
  d1 = block_sum(d1, sh);
  if (threadIdx.x == 0) { P[blockIdx.x] = d0; P[IP_NB + blockIdx.x] = d1; }
}
// p = z + beta p
__global__ __launch_bounds__(TPB) void ip_cg_p_kernel(int n, const double *__restrict__ S, const double *__restrict__ z, double *__restrict__ p) {
  if (S[IP_DONE] != 0.0) return;
  const double beta = S[IP_BETA];
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) p[i] = z[i] + beta * p[i];
}
// P0 = a . b, P1 = c . b
__global__ __launch_bounds__(TPB) void ip_dot2_kernel(int n, const double *__restrict__ a, const double *__restrict__ c, const double *__restrict__ b,
                                                     double *__restrict__ P) {
  __shared__ double sh[4];
  double d0 = 0.0, d1 = 0.0;
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) { d0 += a[i] * b[i]; d1 += c[i] * b[i]; }
  d0 = block_sum(d0, sh);
  d1 = block_sum(d1, sh);
  if (threadIdx.x == 0) { P[blockIdx.x] = d0; P[IP_NB + blockIdx.x] = d1; }
}
// partial sums of x (P0) ; then x -= mean
__global__ __launch_bounds__(TPB) void ip_sum_kernel(int n, const double *__restrict__ x, double *__restrict__ P) {
  __shared__ double sh[4];
  double d0 = 0.0;
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) d0 += x[i];
  d0 = block_sum(d0, sh);
  if (threadIdx.x == 0) P[blockIdx.x] = d0;
}
__global__ __launch_bounds__(TPB) void ip_submean_kernel(int n, int nb, const double *__restrict__ P, double *__restrict__ x) {
  __shared__ double sh[4];
  double a = 0.0;
  for (int i = threadIdx.x; i < nb; i += TPB) a += P[i];
  a = block_sum(a, sh);
  const double m = a / (double)n;
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) x[i] -= m;
}

// ---- Krylov drivers ------------------------------------------------------------------------------------------------
template <int D, int MODE, bool BLK = false>
static void ip_spmv(cfdh_ctx *c, const IpMat &A, const double *x, double *y, const double *q) {
  IpcsData *I = IP(c);
  IPL(c, (ip_spmv_kernel<D, MODE, BLK>), ip_nb(A.n, TPB / 8), 0, A.n, A.rp, A.col, A.val, x, y, q, (const double *)I->S.p, I->P.p);
}
template <int STAGE>
static void ip_scal(cfdh_ctx *c, int nb, double rtol, double atol, int first) {
  IpcsData *I = IP(c);
  IPL(c, ip_scal_kernel<STAGE>, 1, 0, nb, (const double *)I->P.p, I->S.p, rtol, atol, first, c->h_pinned_dev + HP_IPCS);
}
// mirror: |r|^2, done, its, bad
static int ip_read(cfdh_ctx *c, double m[4]) {
  CHK(ip_sync(c));
  for (int i = 0; i < HP_IPCS_N; i++) m[i] = c->h_pinned[HP_IPCS + i];
  return 0;
}
static int ip_finish(cfdh_ctx *c, int which, const double m[4], bool capped, cfdh_ipcs_stats *st) {
  IpcsData *I = IP(c);
  double S[IP_NS];
  HIPCHK(c, hipMemcpyAsync(S, I->S.p, sizeof S, hipMemcpyDeviceToHost, c->stream));
  CHK(ip_sync(c));
  st->its[which] = (int)S[IP_ITS];
  st->rel_res[which] = S[IP_BN2] > 0 ? std::sqrt(S[IP_RN2] / S[IP_BN2]) : std::sqrt(S[IP_RN2]);
  st->reason[which] = m[3] != 0.0 ? CFDH_KSP_DIVERGED_NANORINF : (capped ? CFDH_KSP_DIVERGED_ITS : CFDH_KSP_CONVERGED_RTOL);
  return 0;
}

// cfdh_ipcs_krylov_solve only: the closing true-residual stage resets the recurrence scalars, so the hook keeps the block as the
// last iteration left it.  A step never takes this copy.
static int ip_snapshot(cfdh_ctx *c) {
  IpcsData *I = IP(c);
  if (!I->snap_on) return 0;
  HIPCHK(c, hipMemcpyAsync(I->snap, I->S.p, sizeof I->snap, hipMemcpyDeviceToHost, c->stream));
  I->snap_set = true;
  return 0;
}

// BiCGStab + Jacobi, A1 x = b on D interleaved columns; x holds the initial guess.  BLK: A.val holds [nnz][D][D] blocks and dinv
// one weight per unknown (ipcs_midpoint); otherwise one scalar matrix for the D columns and one weight per node
template <int D, bool BLK = false>
static int ip_bicgstab(cfdh_ctx *c, IpTol tol, const IpMat &A, const double *dinv, const double *b, double *x, cfdh_ipcs_stats *st) {
  IpcsData *I = IP(c);
  const int n = A.n * D, nbv = ip_nb(n, TPB * 4), nbs = ip_nb(A.n, TPB / 8);
  const double rtol = tol.rtol, atol = tol.atol;
  const int max_it = tol.max_it, batch = 4;
  const double *S = I->S.p;
  double m[4];
  ip_spmv<D, 2, BLK>(c, A, x, I->kr.p, b);
  ip_scal<0>(c, nbs, rtol, atol, 1);
  CHK(ip_read(c, m));
  // `launched` bounds the loop on the host, whatever the device counter says: at most max_it iterations are ever launched
  // (the last batch is cut to what is left), so the solve ends after max_it iterations even if no kernel reports back
  bool capped = false;
  int launched = 0;
  while (m[1] == 0.0) {  // not converged on the true residual: (re)start from it
    if (launched >= max_it) { capped = true; break; }
    IPL(c, ip_bicg_start_kernel, nbv, 0, n, (const double *)I->kr.p, I->krh.p, I->kp.p, I->kv.p);
    while (launched < max_it) {
      const int nbatch = std::min(batch, max_it - launched);
      launched += nbatch;
      for (int k = 0; k < nbatch; k++) {
        IPL(c, (ip_bicg1_kernel<D, BLK>), nbv, 0, n, S, (const double *)I->kr.p, (const double *)I->kv.p, dinv, I->kp.p, I->ky.p);
        ip_spmv<D, 0, BLK>(c, A, I->ky.p, I->kv.p, I->krh.p);
        ip_scal<1>(c, nbs, 0, 0, 0);
        IPL(c, (ip_bicg2_kernel<D, BLK>), nbv, 0, n, S, (const double *)I->kr.p, (const double *)I->kv.p, dinv, I->ks.p, I->kz.p);
        ip_spmv<D, 1, BLK>(c, A, I->kz.p, I->kt.p, I->ks.p);
        ip_scal<2>(c, nbs, 0, 0, 0);
        IPL(c, ip_bicg3_kernel, nbv, 0, n, S, (const double *)I->ky.p, (const double *)I->kz.p, (const double *)I->ks.p, (const double *)I->kt.p,
            (const double *)I->krh.p, x, I->kr.p, I->P.p);
        ip_scal<3>(c, nbv, 0, 0, 0);
      }
      HIPCHK(c, hipGetLastError());
      CHK(ip_read(c, m));
      if (m[1] != 0.0) break;
    }
    if (m[3] != 0.0) break;
    CHK(ip_snapshot(c));
    ip_spmv<D, 2, BLK>(c, A, x, I->kr.p, b);  // the recurrence says converged (or the cap is reached): the true residual decides
    ip_scal<0>(c, nbs, rtol, atol, 0);
    CHK(ip_read(c, m));
  }
  return ip_finish(c, 0, m, capped, st);
}

// CG + Jacobi (JAC) or flexible CG preconditioned by one V-cycle of hLam (single column)
template <int D, bool JAC>
static int ip_cg(cfdh_ctx *c, int which, IpTol tol, const IpMat &A, const double *dinv, const double *b, double *x, double *r, double *z, double *p,
                 double *q, cfdh_ipcs_stats *st) {
  IpcsData *I = IP(c);
  const int n = A.n * D, nbv = ip_nb(n, TPB * 4), nbs = ip_nb(A.n, TPB / 8);
  const double rtol = tol.rtol, atol = tol.atol;
  const int max_it = tol.max_it, batch = JAC ? 4 : 1;
  const double *S = I->S.p;
  double m[4];
  ip_spmv<D, 2>(c, A, x, r, b);
  ip_scal<0>(c, nbs, rtol, atol, 1);
  CHK(ip_read(c, m));
  bool capped = false;
  int launched = 0;  // as in ip_bicgstab
  while (m[1] == 0.0) {
    if (launched >= max_it) { capped = true; break; }
    if (!JAC) CHK(k_amg_vcycle(c, I->hLam, r, z));
    IPL(c, (ip_cg_start_kernel<D, JAC>), nbv, 0, n, (const double *)r, dinv, z, p, I->P.p);
    ip_scal<4>(c, nbv, 0, 0, 0);
    while (launched < max_it) {
      const int nbatch = std::min(batch, max_it - launched);
      launched += nbatch;
      for (int k = 0; k < nbatch; k++) {
        ip_spmv<D, 0>(c, A, p, q, p);
        ip_scal<5>(c, nbs, 0, 0, 0);
        IPL(c, (ip_cg_x_kernel<D, JAC>), nbv, 0, n, S, (const double *)p, (const double *)q, dinv, x, r, z, I->P.p);
        if (JAC) {
          ip_scal<6>(c, nbv, 0, 0, 0);
          IPL(c, ip_cg_p_kernel, nbv, 0, n, S, (const double *)z, p);
        } else {
          ip_scal<7>(c, nbv, 0, 0, 0);
        }
      }
      HIPCHK(c, hipGetLastError());
      CHK(ip_read(c, m));
      if (m[1] != 0.0 || launched >= max_it) break;
      if (!JAC) {  // z = V(r) ; beta = -alpha (q . z) / rz (flexible: the cycle keeps fp32 operators and is not exactly symmetric)
        CHK(k_amg_vcycle(c, I->hLam, r, z));
        IPL(c, ip_dot2_kernel, nbv, 0, n, (const double *)r, (const double *)q, (const double *)z, I->P.p);
        ip_scal<8>(c, nbv, 0, 0, 0);
        IPL(c, ip_cg_p_kernel, nbv, 0, n, S, (const double *)z, p);
      }
    }
    if (m[3] != 0.0) break;
    CHK(ip_snapshot(c));
    ip_spmv<D, 2>(c, A, x, r, b);
    ip_scal<0>(c, nbs, rtol, atol, 0);
    CHK(ip_read(c, m));
  }
  return ip_finish(c, which, m, capped, st);
}

int ip_sub_mean(cfdh_ctx *c, int n, double *x) {
  IpcsData *I = IP(c);
  const int nb = ip_nb(n, TPB * 4);
  IPL(c, ip_sum_kernel, nb, 0, n, (const double *)x, I->P.p);
  IPL(c, ip_submean_kernel, nb, 0, n, nb, (const double *)I->P.p, x);
  HIPCHK(c, hipGetLastError());
  return 0;
}

// Which solve uses what.  Solve 0 works in the velocity-sized kr, krh, kp, kv, ks, kt, ky, kz (ip_bicgstab), solve 1 in the
// pressure-sized pr, pz, pp, pq, solve 2 in the velocity-sized kr, kz, kp, kv.
template <int D>
int ip_solve(cfdh_ctx *c, int which, IpTol tol, const double *b, double *x, cfdh_ipcs_stats *st) {
  IpcsData *I = IP(c);
  if (which == 1)
    return ip_cg<1, false>(c, 1, tol, IpMat{I->nvert, I->rp1.p, I->col1.p, I->Lv.p}, nullptr, b, x, I->pr.p, I->pz.p, I->pp.p, I->pq.p, st);
  if (which == 2)
    return ip_cg<D, true>(c, 2, tol, IpMat{I->nn, I->rp2.p, I->col2.p, I->RMv.p}, I->dinv3.p, b, x, I->kr.p, I->kz.p, I->kp.p, I->kv.p, st);
  if (I->scheme == CFDH_IPCS_MIDPOINT) return ip_bicgstab<D, true>(c, tol, IpMat{I->nn, I->rp2.p, I->col2.p, I->A1B.p}, I->dinvB.p, b, x, st);
  return ip_bicgstab<D>(c, tol, IpMat{I->nn, I->rp2.p, I->col2.p, I->A1v.p}, I->dinv1.p, b, x, st);
}
template int ip_solve<2>(cfdh_ctx *, int, IpTol, const double *, double *, cfdh_ipcs_stats *);
template int ip_solve<3>(cfdh_ctx *, int, IpTol, const double *, double *, cfdh_ipcs_stats *);

// One solve on the caller's b and x0 (cfdh_ipcs_krylov_solve) with the caller's tolerances; b and x live in buffers of the hook's
// own, b1 is kept over the assembly.
int cfdh_ipcs_krylov_solve_impl(cfdh_ctx *c, int which, const double *b, const double *x0, double rtol, double atol, int max_it, double *x,
                                cfdh_ipcs_stats *st, double *scalars) {
  IpcsData *I = IP(c);
  hipStream_t s = c->stream;
  const size_t n1 = (size_t)I->nn * I->D, n = which == 1 ? (size_t)I->nvert : n1;
  memset(st, 0, sizeof *st);
  CHK(ip_prepare(c));
  HIPCHK(c, I->hk_b.alloc(n1)); HIPCHK(c, I->hk_x.alloc(n1));
  const long long launch0 = I->n_launch, sync0 = I->n_sync;
  if (which == 0 && I->scheme == CFDH_IPCS_MIDPOINT) {  // the constant block A1, assembled here only if it is out of date
    CHK(ip_mid_matrix(c));
  } else if (which == 0) {  // A1 of the current state; the assembly also writes b1, which is kept
    const bool was = I->assembled;
    HIPCHK(c, hipMemcpyAsync(I->hk_x.p, I->b1.p, sizeof(double) * n1, hipMemcpyDeviceToDevice, s));
    CHK(ip_assemble_bdf2(c));
    HIPCHK(c, hipMemcpyAsync(I->b1.p, I->hk_x.p, sizeof(double) * n1, hipMemcpyDeviceToDevice, s));
    I->assembled = was;
  }
  HIPCHK(c, hipMemcpyAsync(I->hk_b.p, b, sizeof(double) * n, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(I->hk_x.p, x0, sizeof(double) * n, hipMemcpyHostToDevice, s));
  const IpTol tol{rtol, atol, max_it};
  I->snap_on = true; I->snap_set = false;
  const int rc = I->D == 2 ? ip_solve<2>(c, which, tol, I->hk_b.p, I->hk_x.p, st) : ip_solve<3>(c, which, tol, I->hk_b.p, I->hk_x.p, st);
  I->snap_on = false;
  I->n_launch = launch0; I->n_sync = sync0;
  CHK(rc);
  HIPCHK(c, hipMemcpyAsync(x, I->hk_x.p, sizeof(double) * n, hipMemcpyDeviceToHost, s));
  if (scalars) HIPCHK(c, hipMemcpyAsync(scalars, I->S.p, sizeof(double) * IP_NS, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  if (scalars && I->snap_set)
    for (int k = IP_RHO; k <= IP_BETA; k++) scalars[k] = I->snap[k];
  return 0;
}
