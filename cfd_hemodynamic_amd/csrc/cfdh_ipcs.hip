// Incremental pressure-correction scheme `ipcs_bdf2` on P2/P1 triangles and tetrahedra (include/cfdh.h, "incremental pressure
// correction").  A step is three linear solves, all resident in HBM:
//   1. A1 u* = b1   A1 = rho/dt M + c/2 N(w) + mu/2 K on the P2 node graph, one scalar matrix for the d components,
//                   reassembled every step from w = 1.5 u_prev - 0.5 u_n1; BiCGStab + Jacobi on the interleaved vector
//   2. L phi = b2   P1 stiffness matrix; flexible PCG preconditioned by one V-cycle of the smoothed-aggregation hierarchy
//   3. rho M u = b3 CG + Jacobi
// Assembly needs no run-time quadrature: on an affine simplex N_e[a][b] = |det| sum_k sum_e (sum_d w_k,d Jinv[e][d]) T[a][k][b][e]
// with the reference tensor T = int_ref phi_a phi_k d_e phi_b, computed once on the host with the degree-13 rules of include/.
// Two kernels: one thread per cell forms the 6x2 / 10x3 coefficients |det| (w_k . Jinv_e); then the row's threads sum, for each
// entry of the fixed CSR pattern, the contributions of the cells that hold the node pair in ascending cell order -- row-owner
// layout, no floating-point atomics, a fixed summation order, bitwise reproducible.
// The Krylov loops keep their scalars on the device: every dot product ends in per-block partial sums that a one-block kernel
// folds into the scalars; a `done` scalar freezes the kernels of the iterations launched ahead of the host's convergence test.
// Node numbering is the caller's (no renumbering): vertices [0, nvert), then the edge nodes.
// A second scheme on the same context, `ipcs_midpoint` (cfdh_ipcs_set_scheme): the vector-coupled epsilon form with its ds pair
// and explicit convection.  A1 is then a matrix of [D][D] blocks on the same pattern, constant over a run (assembled when dt, rho,
// mu or the constrained velocity nodes change), the convection is applied matrix-free from cw and T2 into b1, and the pressure
// Dirichlet data of a step are formed on the device from g - p_prev; the Krylov drivers, the pressure and the mass solve are shared.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>

#include "cfdh_internal.hpp"
#include "cfdh_mesh_host.hpp"
#include "cfdh_ipcs.hpp"
#include "cfdh_wave.hpp"
#include "cfdh_quad_tet.h"
#include "cfdh_quad_tri.h"

#define TPB 256
#define IP_NB 2048  // most blocks (= partial sums per dot product) of the reducing kernels

// ---------------------------------------------------------------- assembly
// cw[cell][k][e] = |det| sum_d w_k,d Jinv[e][d],  w = 1.5 u_prev - 0.5 u_n1 at local node k (MID: w = u_prev, the explicit
// convection of ipcs_midpoint);  geo[cell] = (Jinv [D][D], |det|)
template <int D, bool MID = false>
__global__ __launch_bounds__(TPB) void ip_cw_kernel(int nc, const int *__restrict__ cells, const double *__restrict__ geo,
                                                   const double *__restrict__ up, const double *__restrict__ un1, double *__restrict__ cw) {
  constexpr int NL = D == 2 ? 6 : 10;
  const int e = blockIdx.x * TPB + threadIdx.x;
  if (e >= nc) return;
  double J[D * D];
  for (int i = 0; i < D * D; i++) J[i] = geo[(size_t)(D * D + 1) * e + i];
  const double det = geo[(size_t)(D * D + 1) * e + D * D];
  for (int k = 0; k < NL; k++) {
    const int v = cells[(size_t)NL * e + k];
    double w[D];
    for (int d = 0; d < D; d++) w[d] = MID ? up[(size_t)D * v + d] : 1.5 * up[(size_t)D * v + d] - 0.5 * un1[(size_t)D * v + d];
    for (int q = 0; q < D; q++) {
      double a = 0.0;
      for (int d = 0; d < D; d++) a += w[d] * J[D * q + d];
      cw[((size_t)NL * e + k) * D + q] = det * a;
    }
  }
}

// values of A1 on the P2 pattern: unconstrained (Afree) and with the Dirichlet rows / columns treated (A1; diagonal = number of
// objects holding the node).  Eight lanes per row; the entry's element contributions are listed in elist[eptr[k] .. eptr[k+1])
// as cell * NL^2 + a * NL + b, ascending.  T2[a][b][k][e] is staged in LDS.
template <int D>
__global__ __launch_bounds__(TPB) void ip_asm_kernel(int nn, const int *__restrict__ rowptr, const int *__restrict__ col, const int *__restrict__ eptr,
                                                    const int *__restrict__ elist, const double *__restrict__ T2, const double *__restrict__ cw,
                                                    const double *__restrict__ Mv, const double *__restrict__ Kv, double cm, double ck, double cn,
                                                    const unsigned char *__restrict__ flag, const double *__restrict__ cnt,
                                                    double *__restrict__ Afree, double *__restrict__ A1, double *__restrict__ dinv) {
  constexpr int NL = D == 2 ? 6 : 10, NT = NL * D;
  extern __shared__ double sT[];
  for (int i = threadIdx.x; i < NL * NL * NT; i += TPB) sT[i] = T2[i];
  __syncthreads();
  const int gid = blockIdx.x * TPB + threadIdx.x;
  const int row = gid >> 3, l = gid & 7;
  if (row >= nn) return;
  const bool rf = flag[row] != 0;
  for (int k = rowptr[row] + l; k < rowptr[row + 1]; k += 8) {
    double a = 0.0;
    for (int q = eptr[k]; q < eptr[k + 1]; q++) {
      const int code = elist[q], e = code / (NL * NL), ab = code - e * (NL * NL);
      const double *t = sT + ab * NT, *w = cw + (size_t)e * NT;
      double s = 0.0;
#pragma unroll
      for (int j = 0; j < NT; j++) s += w[j] * t[j];
      a += s;
    }
    const double v = cm * Mv[k] + ck * Kv[k] + cn * a;
    const int j = col[k];
    Afree[k] = v;
    const double vc = rf ? (j == row ? cnt[row] : 0.0) : (flag[j] ? 0.0 : v);
    A1[k] = vc;
    if (j == row) dinv[row] = 1.0 / vc;
  }
}

// b1 = 2 rho/dt M u_prev - Afree u_prev - Afree g + B^T p + sf f m1 ; constrained rows: count * value
template <int D>
__global__ __launch_bounds__(TPB) void ip_b1_kernel(int nn, const int *__restrict__ rowptr, const int *__restrict__ col, const double *__restrict__ Mv,
                                                   const double *__restrict__ Afree, double cm2, const double *__restrict__ up,
                                                   const unsigned char *__restrict__ flag, const double *__restrict__ cnt, const double *__restrict__ gval,
                                                   const int *__restrict__ gptr, const int *__restrict__ gcol, const double *__restrict__ BT,
                                                   const double *__restrict__ p, const double *__restrict__ m1, double f0, double f1, double f2,
                                                   double *__restrict__ b) {
  const int gid = blockIdx.x * TPB + threadIdx.x;
  const int row = gid >> 3, l = gid & 7;
  double a[D];
  for (int d = 0; d < D; d++) a[d] = 0.0;
  if (row < nn) {
    for (int k = rowptr[row] + l; k < rowptr[row + 1]; k += 8) {
      const int j = col[k];
      const double af = Afree[k], m = cm2 * Mv[k] - af;
      const bool fj = flag[j] != 0;
      for (int d = 0; d < D; d++) a[d] += m * up[(size_t)D * j + d] - (fj ? af * gval[(size_t)D * j + d] : 0.0);
    }
    for (int k = gptr[row] + l; k < gptr[row + 1]; k += 8) {
      const double pv = p[gcol[k]];
      for (int d = 0; d < D; d++) a[d] += BT[(size_t)D * k + d] * pv;
    }
  }
  for (int d = 0; d < D; d++) a[d] = group8_sum(a[d]);
  if (row < nn && l == 0) {
    const double f[3] = {f0, f1, f2};
    const bool rf = flag[row] != 0;
    for (int d = 0; d < D; d++) b[(size_t)D * row + d] = rf ? cnt[row] * gval[(size_t)D * row + d] : a[d] + f[d] * m1[row];
  }
}

// b2 = -rho/dt sum_d B_d u*_d - lift ; constrained rows: rhsfix
template <int D>
__global__ __launch_bounds__(TPB) void ip_b2_kernel(int nv, const int *__restrict__ bptr, const int *__restrict__ bcol, const double *__restrict__ Bv,
                                                   const double *__restrict__ us, double coef, const unsigned char *__restrict__ pflag,
                                                   const double *__restrict__ lift, const double *__restrict__ rhsfix, double *__restrict__ b) {
  const int gid = blockIdx.x * TPB + threadIdx.x;
  const int row = gid >> 3, l = gid & 7;
  double a = 0.0;
  if (row < nv)
    for (int k = bptr[row] + l; k < bptr[row + 1]; k += 8) {
      const int j = bcol[k];
      for (int d = 0; d < D; d++) a += Bv[(size_t)D * k + d] * us[(size_t)D * j + d];
    }
  a = group8_sum(a);
  if (row < nv && l == 0) b[row] = pflag[row] ? rhsfix[row] : coef * a - lift[row];
}

// b3 = rho M u* - dt G phi
template <int D>
__global__ __launch_bounds__(TPB) void ip_b3_kernel(int nn, const int *__restrict__ rowptr, const int *__restrict__ col, const double *__restrict__ Mv,
                                                   double rho, const double *__restrict__ us, const int *__restrict__ gptr, const int *__restrict__ gcol,
                                                   const double *__restrict__ Gv, double dt, const double *__restrict__ phi, double *__restrict__ b) {
  const int gid = blockIdx.x * TPB + threadIdx.x;
  const int row = gid >> 3, l = gid & 7;
  double a[D];
  for (int d = 0; d < D; d++) a[d] = 0.0;
  if (row < nn) {
    for (int k = rowptr[row] + l; k < rowptr[row + 1]; k += 8) {
      const int j = col[k];
      const double m = rho * Mv[k];
      for (int d = 0; d < D; d++) a[d] += m * us[(size_t)D * j + d];
    }
    for (int k = gptr[row] + l; k < gptr[row + 1]; k += 8) {
      const double pv = dt * phi[gcol[k]];
      for (int d = 0; d < D; d++) a[d] -= Gv[(size_t)D * k + d] * pv;
    }
  }
  for (int d = 0; d < D; d++) a[d] = group8_sum(a[d]);
  if (row < nn && l == 0)
    for (int d = 0; d < D; d++) b[(size_t)D * row + d] = a[d];
}

// ---------------------------------------------------------------- ipcs_midpoint: vector-coupled momentum matrix
// Blocks [nnz][D][D] (row-major alpha, beta) on the P2 pattern: Afree = (cm M + ck K) I + ck ES, ES = E - S the coupling part of the
// epsilon form and its ds term (built on the host, constant); A1 with the Dirichlet treatment (the count on the D diagonal entries of
// a constrained node); dinv [nn][D] the Jacobi weights of the D nn diagonal.  Eight lanes per row.
template <int D>
__global__ __launch_bounds__(TPB) void ip_asm_blk_kernel(int nn, const int *__restrict__ rowptr, const int *__restrict__ col, const double *__restrict__ Mv,
                                                        const double *__restrict__ Kv, const double *__restrict__ ES, double cm, double ck,
                                                        const unsigned char *__restrict__ flag, const double *__restrict__ cnt,
                                                        double *__restrict__ Afree, double *__restrict__ A1, double *__restrict__ dinv) {
  const int gid = blockIdx.x * TPB + threadIdx.x;
  const int row = gid >> 3, l = gid & 7;
  if (row >= nn) return;
  const bool rf = flag[row] != 0;
  for (int k = rowptr[row] + l; k < rowptr[row + 1]; k += 8) {
    const int j = col[k];
    const double s = cm * Mv[k] + ck * Kv[k];
    const bool fj = flag[j] != 0;
    for (int a = 0; a < D; a++)
      for (int b = 0; b < D; b++) {
        const size_t q = ((size_t)k * D + a) * D + b;
        const double v = (a == b ? s : 0.0) + ck * ES[q];
        Afree[q] = v;
        const double vc = rf ? (j == row && a == b ? cnt[row] : 0.0) : (fj ? 0.0 : v);
        A1[q] = vc;
        if (j == row && a == b) dinv[(size_t)D * row + a] = 1.0 / vc;
      }
  }
}

// explicit convection, matrix-free: out[i][alpha] = int phi_i (w . grad) w_alpha = sum over the cells of node i (nlist[nptr[i] ..):
// cell * NL + local node, ascending) of sum_b (sum_{k,e} cw[cell][k][e] T2[a][b][k][e]) w_b,alpha.  No matrix N is written.  Eight
// lanes per row node take its cells in turn; T2 is staged in LDS.
template <int D>
__global__ __launch_bounds__(TPB) void ip_conv_kernel(int nn, const int *__restrict__ nptr, const int *__restrict__ nlist, const int *__restrict__ cells,
                                                     const double *__restrict__ T2, const double *__restrict__ cw, const double *__restrict__ w,
                                                     double *__restrict__ out) {
  constexpr int NL = D == 2 ? 6 : 10, NT = NL * D;
  extern __shared__ double sT[];
  for (int i = threadIdx.x; i < NL * NL * NT; i += TPB) sT[i] = T2[i];
  __syncthreads();
  const int gid = blockIdx.x * TPB + threadIdx.x;
  const int row = gid >> 3, l = gid & 7;
  double a[D];
  for (int d = 0; d < D; d++) a[d] = 0.0;
  if (row < nn)
    for (int q = nptr[row] + l; q < nptr[row + 1]; q += 8) {
      const int code = nlist[q], e = code / NL, la = code - e * NL;
      const double *wc = cw + (size_t)e * NT;
      const int *cv = cells + (size_t)NL * e;
      for (int b = 0; b < NL; b++) {
        const double *t = sT + (la * NL + b) * NT;
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < NT; j++) s += wc[j] * t[j];
        for (int d = 0; d < D; d++) a[d] += s * w[(size_t)D * cv[b] + d];
      }
    }
  for (int d = 0; d < D; d++) a[d] = group8_sum(a[d]);
  if (row < nn && l == 0)
    for (int d = 0; d < D; d++) out[(size_t)D * row + d] = a[d];
}

// b1 of the block form = (2 rho/dt M I - Afree) u_prev - Afree g + (B^T - Pn) p_prev + sf f m1 - cc conv ; constrained rows:
// count * value.  BTP holds B^T - Pn on the gptr / gcol pattern.
template <int D>
__global__ __launch_bounds__(TPB) void ip_b1_blk_kernel(int nn, const int *__restrict__ rowptr, const int *__restrict__ col, const double *__restrict__ Mv,
                                                       const double *__restrict__ Afree, double cm2, const double *__restrict__ up,
                                                       const unsigned char *__restrict__ flag, const double *__restrict__ cnt,
                                                       const double *__restrict__ gval, const int *__restrict__ gptr, const int *__restrict__ gcol,
                                                       const double *__restrict__ BTP, const double *__restrict__ p, const double *__restrict__ m1,
                                                       double f0, double f1, double f2, const double *__restrict__ conv, double cc,
                                                       double *__restrict__ b) {
  const int gid = blockIdx.x * TPB + threadIdx.x;
  const int row = gid >> 3, l = gid & 7;
  double a[D];
  for (int d = 0; d < D; d++) a[d] = 0.0;
  if (row < nn) {
    for (int k = rowptr[row] + l; k < rowptr[row + 1]; k += 8) {
      const int j = col[k];
      const double m = cm2 * Mv[k];
      const bool fj = flag[j] != 0;
      double uj[D], gj[D];
      for (int d = 0; d < D; d++) { uj[d] = up[(size_t)D * j + d]; gj[d] = fj ? gval[(size_t)D * j + d] : 0.0; }
      const double *af = Afree + (size_t)k * D * D;
      for (int d = 0; d < D; d++)
        for (int e = 0; e < D; e++) {
          const double v = af[D * d + e];
          a[d] += ((d == e ? m : 0.0) - v) * uj[e] - (fj ? v * gj[e] : 0.0);
        }
    }
    for (int k = gptr[row] + l; k < gptr[row + 1]; k += 8) {
      const double pv = p[gcol[k]];
      for (int d = 0; d < D; d++) a[d] += BTP[(size_t)D * k + d] * pv;
    }
  }
  for (int d = 0; d < D; d++) a[d] = group8_sum(a[d]);
  if (row < nn && l == 0) {
    const double f[3] = {f0, f1, f2};
    const bool rf = flag[row] != 0;
    for (int d = 0; d < D; d++)
      b[(size_t)D * row + d] = rf ? cnt[row] * gval[(size_t)D * row + d] : a[d] + f[d] * m1[row] - cc * conv[(size_t)D * row + d];
  }
}

// pressure Dirichlet data of one ipcs_midpoint step: the VALUE g goes into p, so phi = p - p_prev takes g - p_prev on the
// constrained vertices.  lift = L_free (g - p_prev) over the constrained columns, rhsfix = count (g - p_prev) (ip_b2_kernel)
__global__ __launch_bounds__(TPB) void ip_plift_kernel(int nv, const int *__restrict__ rowptr, const int *__restrict__ col, const double *__restrict__ Lf,
                                                      const unsigned char *__restrict__ pflag, const double *__restrict__ pcnt,
                                                      const double *__restrict__ pval, const double *__restrict__ pprev, double *__restrict__ lift,
                                                      double *__restrict__ rhsfix) {
  const int gid = blockIdx.x * TPB + threadIdx.x;
  const int row = gid >> 3, l = gid & 7;
  double a = 0.0;
  if (row < nv)
    for (int k = rowptr[row] + l; k < rowptr[row + 1]; k += 8) {
      const int j = col[k];
      if (pflag[j]) a += Lf[k] * (pval[j] - pprev[j]);
    }
  a = group8_sum(a);
  if (row < nv && l == 0) {
    lift[row] = a;
    rhsfix[row] = pflag[row] ? pcnt[row] * (pval[row] - pprev[row]) : 0.0;
  }
}

// ---------------------------------------------------------------- Krylov kernels
// y = A x for D interleaved columns (the matrix is read once), eight lanes per row, grid-stride over the rows, with the dot
// products the iteration needs next.  MODE 0: P0 = y . q ; 1: P0 = y . q, P1 = y . y ; 2: y = q - A x, P0 = y . y, P1 = q . q
// (true residual; not frozen by `done`).
template <int D, int MODE>
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
        const double v = val[k];
        for (int d = 0; d < D; d++) a[d] += v * x[(size_t)D * j + d];
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

// the same three MODEs for a matrix of [nnz][D][D] blocks (row-major) on the interleaved vector: the block A1 of ipcs_midpoint
template <int D, int MODE>
__global__ __launch_bounds__(TPB) void ip_spmv_blk_kernel(int n, const int *__restrict__ rowptr, const int *__restrict__ col, const double *__restrict__ val,
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
        const double *v = val + (size_t)k * D * D;
        double xj[D];
        for (int e = 0; e < D; e++) xj[e] = x[(size_t)D * j + e];
        for (int d = 0; d < D; d++)
          for (int e = 0; e < D; e++) a[d] += v[D * d + e] * xj[e];
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
    const double rn2 = S[IP_RN2];
    if (!isfinite(rn2) || (STAGE != 0 && STAGE != 7 && !isfinite(S[IP_BETA]))) { S[IP_BAD] = 1.0; S[IP_DONE] = 1.0; }
    else if (rn2 <= S[IP_TOL2]) S[IP_DONE] = 1.0;
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
__global__ __launch_bounds__(TPB) void ip_axpy_kernel(int n, double a, const double *__restrict__ x, double *__restrict__ y) {
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) y[i] += a * x[i];
}
// functionals: P0 = x^T A x summed over the D interleaved columns ; eight lanes per row
template <int D>
__global__ __launch_bounds__(TPB) void ip_quad_kernel(int n, const int *__restrict__ rowptr, const int *__restrict__ col, const double *__restrict__ val,
                                                     const double *__restrict__ x, double *__restrict__ P) {
  __shared__ double sh[4];
  const int l = threadIdx.x & 7;
  double d0 = 0.0;
  for (int base = blockIdx.x * (TPB / 8); base < n; base += gridDim.x * (TPB / 8)) {
    const int row = base + (threadIdx.x >> 3);
    if (row < n)
      for (int k = rowptr[row] + l; k < rowptr[row + 1]; k += 8) {
        const int j = col[k];
        const double v = val[k];
        for (int d = 0; d < D; d++) d0 += v * x[(size_t)D * j + d] * x[(size_t)D * row + d];
      }
  }
  d0 = block_sum(d0, sh);
  if (threadIdx.x == 0) P[blockIdx.x] = d0;
}
// P0 = max |x - y| (y may be null; NaN when an entry is NaN)
__global__ __launch_bounds__(TPB) void ip_maxdiff_kernel(int n, const double *__restrict__ x, const double *__restrict__ y, double *__restrict__ P) {
  __shared__ double sh[4];
  double a = 0.0;
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) a = max_nan(a, fabs(y ? x[i] - y[i] : x[i]));
  a = block_max(a, sh);
  if (threadIdx.x == 0) P[blockIdx.x] = a;
}
// drag / lift on the exterior edges of `marker` (gdim 2; the integrand of the P1 path, dfg_1.py:183-202): with n = -FacetNormal,
// t = (n_y, -n_x), u_t = u . t:  F_D = int (mu d_n u_t n_y - p n_x) ds,  F_L = -int (mu d_n u_t n_x + p n_y) ds.  grad u (P2) and p (P1)
// are linear along the edge: two-point Gauss is exact.  One thread per facet, per-facet values into out[] (summed in a fixed order).
__global__ __launch_bounds__(TPB) void ip_draglift_kernel(int nf, const int *__restrict__ fcell, const int *__restrict__ flocal, const int *__restrict__ fmark,
                                                         int marker, int kind, const int *__restrict__ cells, const double *__restrict__ coords,
                                                         const double *__restrict__ geo, const double *__restrict__ u, const double *__restrict__ p,
                                                         double mu, double *__restrict__ out) {
  const int k = blockIdx.x * TPB + threadIdx.x;
  if (k >= nf) return;
  double res = 0.0;
  if (fmark[k] == marker) {
    const int e = fcell[k], f = flocal[k];
    const int *cv = cells + 6 * (size_t)e;
    const double *J = geo + 5 * (size_t)e;   // J[2 q + d] = d xi_q / d x_d ; grad lambda_0 = -(row 0 + row 1)
    double gl[3][2] = {{-(J[0] + J[2]), -(J[1] + J[3])}, {J[0], J[1]}, {J[2], J[3]}};
    const int va = (f + 1) % 3, vb = (f + 2) % 3;
    const double ax = coords[2 * cv[va]], ay = coords[2 * cv[va] + 1], bx = coords[2 * cv[vb]], by = coords[2 * cv[vb] + 1];
    const double len = sqrt((bx - ax) * (bx - ax) + (by - ay) * (by - ay));
    const double gn = sqrt(gl[f][0] * gl[f][0] + gl[f][1] * gl[f][1]);
    const double nx = gl[f][0] / gn, ny = gl[f][1] / gn, tx = ny, ty = -nx;  // n = -FacetNormal
    const int ed[3][2] = {{1, 2}, {0, 2}, {0, 1}};
    for (int g = 0; g < 2; g++) {
      const double s = 0.5 + (g == 0 ? -0.5 : 0.5) / sqrt(3.0);
      double lam[3];
      lam[f] = 0.0; lam[va] = 1.0 - s; lam[vb] = s;
      // d phi_a / d lambda_i at the point, then grad phi_a = sum_i dl[a][i] grad lambda_i
      double dn_ut = 0.0;
      for (int a = 0; a < 6; a++) {
        double dl[3] = {0.0, 0.0, 0.0};
        if (a < 3) dl[a] = 4.0 * lam[a] - 1.0;
        else { dl[ed[a - 3][0]] = 4.0 * lam[ed[a - 3][1]]; dl[ed[a - 3][1]] = 4.0 * lam[ed[a - 3][0]]; }
        const double gx = dl[0] * gl[0][0] + dl[1] * gl[1][0] + dl[2] * gl[2][0], gy = dl[0] * gl[0][1] + dl[1] * gl[1][1] + dl[2] * gl[2][1];
        const double ut = u[2 * (size_t)cv[a]] * tx + u[2 * (size_t)cv[a] + 1] * ty;
        dn_ut += ut * (gx * nx + gy * ny);
      }
      const double pv = lam[0] * p[cv[0]] + lam[1] * p[cv[1]] + lam[2] * p[cv[2]];
      res += 0.5 * len * (kind == 0 ? (mu * dn_ut * ny - pv * nx) : -(mu * dn_ut * nx + pv * ny));
    }
  }
  out[k] = res;
}

// ================================================================ host side
static double ip_now_ms() {
  using namespace std::chrono;
  return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

static const int IP_TRI_EDGES[3][2] = {{1, 2}, {0, 2}, {0, 1}};
static const int IP_TET_EDGES[6][2] = {{2, 3}, {1, 3}, {1, 2}, {0, 3}, {0, 2}, {0, 1}};

// P2 basis and its derivatives with respect to the barycentric coordinates at lam
static void ip_p2(int D, const double *lam, double *phi, double *dl /*[NL][D+1]*/) {
  const int nv = D + 1, ne = D == 2 ? 3 : 6, NL = nv + ne;
  for (int i = 0; i < NL * nv; i++) dl[i] = 0.0;
  for (int i = 0; i < nv; i++) { phi[i] = lam[i] * (2.0 * lam[i] - 1.0); dl[i * nv + i] = 4.0 * lam[i] - 1.0; }
  for (int k = 0; k < ne; k++) {
    const int i = D == 2 ? IP_TRI_EDGES[k][0] : IP_TET_EDGES[k][0], j = D == 2 ? IP_TRI_EDGES[k][1] : IP_TET_EDGES[k][1];
    phi[nv + k] = 4.0 * lam[i] * lam[j];
    dl[(nv + k) * nv + i] = 4.0 * lam[j];
    dl[(nv + k) * nv + j] = 4.0 * lam[i];
  }
}

// reference tensors (volume of the reference simplex 1 / D! included): Mref[a][b] = int phi_a phi_b, Kref[a][b][i][j] = int d_li phi_a d_lj phi_b,
// T2[a][b][k][e] = int phi_a phi_k d_xi_e phi_b, Bref[v][b][i] = int lam_v d_li phi_b, Gref[a] = int phi_a, MPref[v][w] = int lam_v lam_w
struct IpRef {
  int D, NL, NV;
  std::vector<double> M, K, T2, B, G, MP;
};
static void ip_reference(int D, IpRef &R) {
  const int NV = D + 1, NL = D == 2 ? 6 : 10, nq = D == 2 ? CFDH_NQ : CFDH3_NQ;
  R.D = D; R.NL = NL; R.NV = NV;
  R.M.assign(NL * NL, 0.0); R.K.assign((size_t)NL * NL * NV * NV, 0.0); R.T2.assign((size_t)NL * NL * NL * D, 0.0);
  R.B.assign((size_t)NV * NL * NV, 0.0); R.G.assign(NL, 0.0); R.MP.assign(NV * NV, 0.0);
  const double vol = D == 2 ? 0.5 : 1.0 / 6.0;
  std::vector<double> phi(NL), dl((size_t)NL * NV);
  for (int q = 0; q < nq; q++) {
    const double *lam = D == 2 ? CFDH_QL[q] : CFDH3_QL[q];
    const double w = vol * (D == 2 ? CFDH_QW[q] : CFDH3_QW[q]);
    ip_p2(D, lam, phi.data(), dl.data());
    for (int a = 0; a < NL; a++) {
      R.G[a] += w * phi[a];
      for (int b = 0; b < NL; b++) {
        R.M[a * NL + b] += w * phi[a] * phi[b];
        for (int i = 0; i < NV; i++)
          for (int j = 0; j < NV; j++) R.K[(((size_t)a * NL + b) * NV + i) * NV + j] += w * dl[a * NV + i] * dl[b * NV + j];
        for (int k = 0; k < NL; k++)
          for (int e = 0; e < D; e++)
            R.T2[(((size_t)a * NL + b) * NL + k) * D + e] += w * phi[a] * phi[k] * (dl[b * NV + e + 1] - dl[b * NV]);
      }
    }
    for (int v = 0; v < NV; v++) {
      for (int b = 0; b < NL; b++)
        for (int i = 0; i < NV; i++) R.B[((size_t)v * NL + b) * NV + i] += w * lam[v] * dl[b * NV + i];
      for (int x = 0; x < NV; x++) R.MP[v * NV + x] += w * lam[v] * lam[x];
    }
  }
}

// pattern of rows `rc` (per cell, nr local rows) x columns `cc` (per cell, ncl local columns), columns ascending
static void ip_pattern(int nrows, int nc, const int *rc, int nr, const int *cc, int ncl, std::vector<int> &ptr, std::vector<int> &col) {
  std::vector<std::vector<int>> rows(nrows);
  for (int e = 0; e < nc; e++)
    for (int a = 0; a < nr; a++) {
      auto &r = rows[rc[(size_t)nr * e + a]];
      for (int b = 0; b < ncl; b++) r.push_back(cc[(size_t)ncl * e + b]);
    }
  ptr.assign(nrows + 1, 0);
  col.clear();
  for (int i = 0; i < nrows; i++) {
    auto &r = rows[i];
    std::sort(r.begin(), r.end());
    r.erase(std::unique(r.begin(), r.end()), r.end());
    col.insert(col.end(), r.begin(), r.end());
    ptr[i + 1] = (int)col.size();
  }
}
static inline int ip_find(const std::vector<int> &ptr, const std::vector<int> &col, int i, int j) {
  return (int)(std::lower_bound(col.begin() + ptr[i], col.begin() + ptr[i + 1], j) - col.begin());
}

#define IP(c) ((c)->ipcs)

static int ip_sync(cfdh_ctx *c) {
  IP(c)->n_sync++;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}
#define IPL(c, kern, grid, shm, ...)                                                  \
  do {                                                                                \
    hipLaunchKernelGGL(kern, dim3(grid), dim3(TPB), shm, (c)->stream, __VA_ARGS__);   \
    IP(c)->n_launch++;                                                                \
  } while (0)
static inline int ip_grid8(int nrows) { return (int)((8ll * nrows + TPB - 1) / TPB); }
static inline int ip_nb(long long n, int per) {  // blocks of a reducing grid-stride kernel
  long long g = (n + per - 1) / per;
  return (int)(g < 1 ? 1 : (g > IP_NB ? IP_NB : g));
}

int cfdh_ipcs_create(cfdh_ctx *c, int gdim, int64_t nn64, int64_t nvert64, int64_t nc64, const int32_t *cells, const double *coords,
                     int64_t nfac, const int32_t *fcell, const int32_t *flocal, const int32_t *fmarker) {
  const int D = gdim, NL = D == 2 ? 6 : 10, NV = D + 1;
  if (nn64 <= 0 || nvert64 <= 0 || nvert64 > nn64 || nc64 <= 0 || nn64 * D > 2000000000ll || nc64 * NL * NL > 2000000000ll)
    return cfdh_fail(c, CFDH_E_ARG, "cfdh_create_ipcs: bad sizes");
  const int nn = (int)nn64, nvert = (int)nvert64, nc = (int)nc64;
  for (int64_t k = 0; k < (int64_t)NL * nc; k++) {
    const int v = cells[k], a = (int)(k % NL);
    if (v < 0 || v >= nn || (a < NV && v >= nvert) || (a >= NV && v < nvert))
      return cfdh_fail(c, CFDH_E_ARG, "cfdh_create_ipcs: cell node out of range (vertices must be the nodes [0, nvert), edge nodes the rest)");
  }
  cfdh_mesh::Wording W;
  W.facet = "cfdh_create_ipcs: bad exterior facet";
  std::string why;
  if (!cfdh_mesh::check_facets(nfac, fcell, flocal, nc, NV, W, why)) return cfdh_fail(c, CFDH_E_ARG, "%s", why.c_str());
  IpcsData *I = new (std::nothrow) IpcsData();
  if (!I) return cfdh_fail(c, CFDH_E_NOMEM, "out of host memory");
  c->ipcs = I;
  c->dim = D; c->nv = nn; c->nvo = nn; c->ng = 0; c->nc = nc; c->nloc = NL; c->etype = 0; c->gen = false; c->nranks = 1;
  c->nfac = c->nfac_user = (int)nfac;
  I->D = D; I->NL = NL; I->nn = nn; I->nvert = nvert; I->nc = nc;
  I->cells.assign(cells, cells + (size_t)NL * nc);
  I->coords.assign(coords, coords + (size_t)D * nn);
  I->fcell.assign(fcell, fcell + nfac); I->flocal.assign(flocal, flocal + nfac);
  I->fmarker.assign((size_t)nfac, 0);
  if (fmarker) I->fmarker.assign(fmarker, fmarker + nfac);
  hipStream_t s = c->stream;
  // reduction scratch of the shared helpers (AMG set-up uses red_out)
  CHK(cfdh_alloc_reduction(c, false));  // no ev_h in this context
  memset(c->h_pinned, 0, HP_WORDS * sizeof(double));

  IpRef R;
  ip_reference(D, R);
  // geometry: Jinv[q][d] = d xi_q / d x_d = grad lambda_{q+1}, |det|
  std::vector<double> &geo = I->geo;
  geo.assign((size_t)(D * D + 1) * nc, 0.0);
  std::vector<int> c1((size_t)NV * nc);
  for (int e = 0; e < nc; e++) {
    const int *cv = cells + (size_t)NL * e;
    for (int a = 0; a < NV; a++) c1[(size_t)NV * e + a] = cv[a];
    double T[3][3], inv[3][3], det;
    for (int a = 0; a < D; a++)
      for (int i = 0; i < D; i++) T[i][a] = coords[(size_t)D * cv[a + 1] + i] - coords[(size_t)D * cv[0] + i];  // columns x_a - x_0
    if (D == 2) {
      det = T[0][0] * T[1][1] - T[0][1] * T[1][0];
      inv[0][0] = T[1][1] / det; inv[0][1] = -T[0][1] / det; inv[1][0] = -T[1][0] / det; inv[1][1] = T[0][0] / det;
    } else {
      double cf[3][3];
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
          cf[i][j] = T[(i + 1) % 3][(j + 1) % 3] * T[(i + 2) % 3][(j + 2) % 3] - T[(i + 1) % 3][(j + 2) % 3] * T[(i + 2) % 3][(j + 1) % 3];
      det = T[0][0] * cf[0][0] + T[0][1] * cf[0][1] + T[0][2] * cf[0][2];
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) inv[i][j] = cf[j][i] / det;
    }
    if (!(std::fabs(det) > 0)) return cfdh_fail(c, CFDH_E_ARG, "cfdh_create_ipcs: degenerate cell %d", e);
    for (int q = 0; q < D; q++)
      for (int d = 0; d < D; d++) geo[(size_t)(D * D + 1) * e + D * q + d] = inv[q][d];
    geo[(size_t)(D * D + 1) * e + D * D] = std::fabs(det);
  }
  // patterns
  ip_pattern(nn, nc, I->cells.data(), NL, I->cells.data(), NL, I->hM.rowptr, I->hM.col);
  ip_pattern(nvert, nc, c1.data(), NV, c1.data(), NV, I->hL.rowptr, I->hL.col);
  ip_pattern(nn, nc, I->cells.data(), NL, c1.data(), NV, I->gptr, I->gcol);
  ip_pattern(nvert, nc, c1.data(), NV, I->cells.data(), NL, I->bptr, I->bcol);
  const int nnz2 = (int)I->hM.col.size(), nnz1 = (int)I->hL.col.size(), nnzG = (int)I->gcol.size(), nnzB = (int)I->bcol.size();
  I->hM.n = I->hM.m = nn; I->hL.n = I->hL.m = nvert;
  I->hM.val.assign(nnz2, 0.0); I->hK.assign(nnz2, 0.0); I->hL.val.assign(nnz1, 0.0); I->hMp.assign(nnz1, 0.0);
  I->hG.assign((size_t)D * nnzG, 0.0); I->hBT.assign((size_t)D * nnzG, 0.0); I->hB.assign((size_t)D * nnzB, 0.0);
  I->m1.assign(nn, 0.0);
  // constant operators, cells in ascending order (fixed summation order); element lists of the A1 entries
  std::vector<int> ecount(nnz2 + 1, 0), slot((size_t)NL * NL);
  for (int e = 0; e < nc; e++) {
    const int *cv = I->cells.data() + (size_t)NL * e;
    const double *g = geo.data() + (size_t)(D * D + 1) * e;
    const double det = g[D * D];
    double gl[4][3];
    for (int d = 0; d < D; d++) {
      gl[0][d] = 0.0;
      for (int q = 0; q < D; q++) { gl[q + 1][d] = g[D * q + d]; gl[0][d] -= g[D * q + d]; }
    }
    double gg[4][4];
    for (int i = 0; i < NV; i++)
      for (int j = 0; j < NV; j++) { gg[i][j] = 0.0; for (int d = 0; d < D; d++) gg[i][j] += gl[i][d] * gl[j][d]; }
    for (int a = 0; a < NL; a++) {
      I->m1[cv[a]] += det * R.G[a];
      for (int b = 0; b < NL; b++) {
        const int k = ip_find(I->hM.rowptr, I->hM.col, cv[a], cv[b]);
        ecount[k + 1]++;
        I->hM.val[k] += det * R.M[a * NL + b];
        double kv = 0.0;
        for (int i = 0; i < NV; i++)
          for (int j = 0; j < NV; j++) kv += R.K[(((size_t)a * NL + b) * NV + i) * NV + j] * gg[i][j];
        I->hK[k] += det * kv;
      }
      // G_d[a][v] = int phi_a d_d lam_v ; B_d^T[a][v] = int lam_v d_d phi_a
      for (int v = 0; v < NV; v++) {
        const int k = ip_find(I->gptr, I->gcol, cv[a], cv[v]);
        for (int d = 0; d < D; d++) {
          I->hG[(size_t)D * k + d] += det * R.G[a] * gl[v][d];
          double bv = 0.0;
          for (int i = 0; i < NV; i++) bv += R.B[((size_t)v * NL + a) * NV + i] * gl[i][d];
          I->hBT[(size_t)D * k + d] += det * bv;
          const int kb = ip_find(I->bptr, I->bcol, cv[v], cv[a]);
          I->hB[(size_t)D * kb + d] += det * bv;
        }
      }
    }
    const double vol = det * (D == 2 ? 0.5 : 1.0 / 6.0);
    for (int v = 0; v < NV; v++)
      for (int x = 0; x < NV; x++) {
        const int k = ip_find(I->hL.rowptr, I->hL.col, cv[v], cv[x]);
        I->hL.val[k] += vol * gg[v][x];
        I->hMp[k] += det * R.MP[v * NV + x];
      }
  }
  for (int k = 0; k < nnz2; k++) ecount[k + 1] += ecount[k];
  std::vector<int> elist((size_t)ecount[nnz2]), fill(ecount.begin(), ecount.end() - 1);
  for (int e = 0; e < nc; e++) {
    const int *cv = I->cells.data() + (size_t)NL * e;
    for (int a = 0; a < NL; a++)
      for (int b = 0; b < NL; b++) elist[fill[ip_find(I->hM.rowptr, I->hM.col, cv[a], cv[b])]++] = e * NL * NL + a * NL + b;
  }
  // device copies
  HIPCHK(c, I->d_cells.upload(I->cells, s)); HIPCHK(c, I->d_coords.upload(I->coords, s)); HIPCHK(c, I->d_geo.upload(geo, s));
  HIPCHK(c, I->d_T2.upload(R.T2, s));
  HIPCHK(c, I->rp2.upload(I->hM.rowptr, s)); HIPCHK(c, I->col2.upload(I->hM.col, s));
  HIPCHK(c, I->Mv.upload(I->hM.val, s)); HIPCHK(c, I->Kv.upload(I->hK, s));
  HIPCHK(c, I->eptr.upload(ecount, s)); HIPCHK(c, I->elist.upload(elist, s));
  HIPCHK(c, I->d_gptr.upload(I->gptr, s)); HIPCHK(c, I->d_gcol.upload(I->gcol, s));
  HIPCHK(c, I->Gv.upload(I->hG, s)); HIPCHK(c, I->BTv.upload(I->hBT, s));
  HIPCHK(c, I->d_bptr.upload(I->bptr, s)); HIPCHK(c, I->d_bcol.upload(I->bcol, s)); HIPCHK(c, I->Bv.upload(I->hB, s));
  HIPCHK(c, I->d_m1.upload(I->m1, s));
  HIPCHK(c, I->rp1.upload(I->hL.rowptr, s)); HIPCHK(c, I->col1.upload(I->hL.col, s)); HIPCHK(c, I->Mpv.upload(I->hMp, s));
  HIPCHK(c, I->Lv.alloc(nnz1));
  HIPCHK(c, I->Afree.alloc(nnz2)); HIPCHK(c, I->A1v.alloc(nnz2)); HIPCHK(c, I->RMv.alloc(nnz2));
  HIPCHK(c, I->dinv1.alloc(nn)); HIPCHK(c, I->dinv3.alloc(nn));
  HIPCHK(c, I->cw.alloc((size_t)nc * NL * D));
  const size_t n1 = (size_t)nn * D;
  dbuf<double> *uv[] = {&I->u_sol, &I->u_prev, &I->u_n1, &I->us, &I->b1, &I->b3, &I->kr, &I->krh, &I->kp, &I->kv, &I->ks, &I->kt, &I->ky, &I->kz, &I->uval};
  for (auto *b : uv) { HIPCHK(c, b->alloc(n1)); HIPCHK(c, b->zero(s)); }
  dbuf<double> *pv[] = {&I->p_sol, &I->p_prev, &I->phi, &I->b2, &I->pr, &I->pz, &I->pp, &I->pq, &I->lift2, &I->prhs};
  for (auto *b : pv) { HIPCHK(c, b->alloc(nvert)); HIPCHK(c, b->zero(s)); }
  HIPCHK(c, I->ucnt.alloc(nn)); HIPCHK(c, I->ucnt.zero(s));
  HIPCHK(c, I->uflag.alloc(nn)); HIPCHK(c, I->uflag.zero(s));
  HIPCHK(c, I->pflag.alloc(nvert)); HIPCHK(c, I->pflag.zero(s));
  HIPCHK(c, I->S.alloc(IP_NS)); HIPCHK(c, I->S.zero(s));
  HIPCHK(c, I->P.alloc(2 * IP_NB)); HIPCHK(c, I->P.zero(s));
  std::vector<int> wv, wptr, wfac;  // alive until the synchronisation below
  if (nfac > 0) {
    HIPCHK(c, I->d_fcell.upload(I->fcell, s)); HIPCHK(c, I->d_flocal.upload(I->flocal, s)); HIPCHK(c, I->d_fmarker.upload(I->fmarker, s));
    HIPCHK(c, I->fout.alloc((size_t)nfac));
    cfdh_mesh::wall_vertex_facets(NL, NV, nfac, I->fcell.data(), I->flocal.data(), I->cells.data(), nvert, wv, wptr, wfac);
    I->n_wallv = (int)wv.size();
    HIPCHK(c, I->wv_list.upload(wv, s)); HIPCHK(c, I->wv_ptr.upload(wptr, s)); HIPCHK(c, I->wv_fac.upload(wfac, s));
  }
  I->h_uflag.assign(nn, 0); I->h_ucnt.assign(nn, 0.0); I->h_uval.assign(n1, 0.0);
  I->h_pflag.assign(nvert, 0); I->h_pcnt.assign(nvert, 0.0); I->h_pval.assign(nvert, 0.0);
  HIPCHK(c, hipStreamSynchronize(s));
  return 0;
}

void cfdh_ipcs_free(cfdh_ctx *c) {
  if (!c->ipcs) return;
  c->ipcs->hLam.clear();
  delete c->ipcs;
  c->ipcs = nullptr;
}

// ---- Dirichlet data ------------------------------------------------------------------------------------------------
int cfdh_ipcs_clear_dirichlet(cfdh_ctx *c) {
  IpcsData *I = IP(c);
  std::fill(I->h_uflag.begin(), I->h_uflag.end(), 0); std::fill(I->h_ucnt.begin(), I->h_ucnt.end(), 0.0); std::fill(I->h_uval.begin(), I->h_uval.end(), 0.0);
  std::fill(I->h_pflag.begin(), I->h_pflag.end(), 0); std::fill(I->h_pcnt.begin(), I->h_pcnt.end(), 0.0); std::fill(I->h_pval.begin(), I->h_pval.end(), 0.0);
  I->ubc_dirty = I->pbc_dirty = I->pset_dirty = I->uset_dirty = true;
  I->assembled = false;
  return 0;
}
int cfdh_ipcs_add_dirichlet(cfdh_ctx *c, int field, int64_t n, const int32_t *nodes, const double *values, bool update) {
  IpcsData *I = IP(c);
  const int lim = field == 0 ? I->nn : I->nvert, D = I->D;
  for (int64_t k = 0; k < n; k++) {
    if (nodes[k] < 0 || nodes[k] >= lim) return cfdh_fail(c, CFDH_E_ARG, "Dirichlet node %d out of range", (int)nodes[k]);
    if (update && !(field == 0 ? I->h_uflag[nodes[k]] : I->h_pflag[nodes[k]]))
      return cfdh_fail(c, CFDH_E_ARG, "cfdh_update_dirichlet: node %d is not constrained", (int)nodes[k]);
  }
  for (int64_t k = 0; k < n; k++) {
    const int v = nodes[k];
    if (field == 0) {
      if (!update) { I->h_uflag[v] = 1; I->h_ucnt[v] += 1.0; I->uset_dirty = true; }
      for (int d = 0; d < D; d++) I->h_uval[(size_t)D * v + d] = values[(size_t)D * k + d];
    } else {
      if (!update) { I->h_pflag[v] = 1; I->h_pcnt[v] += 1.0; I->pset_dirty = true; }
      I->h_pval[v] = values[k];
    }
  }
  if (field == 0) I->ubc_dirty = true; else I->pbc_dirty = true;
  I->assembled = false;
  return 0;
}

// pressure Laplacian with its Dirichlet rows, the hierarchy, and the constant parts of b2
static int ip_prepare_pressure(cfdh_ctx *c) {
  IpcsData *I = IP(c);
  const int nv = I->nvert;
  hipStream_t s = c->stream;
  if (I->pset_dirty || !I->hLam.valid) {
    CsrHost Lc;
    Lc.n = Lc.m = nv; Lc.rowptr = I->hL.rowptr; Lc.col = I->hL.col; Lc.val = I->hL.val;
    bool any = false;
    for (int i = 0; i < nv; i++) {
      any |= I->h_pflag[i] != 0;
      for (int k = Lc.rowptr[i]; k < Lc.rowptr[i + 1]; k++) {
        const int j = Lc.col[k];
        if (I->h_pflag[i]) Lc.val[k] = j == i ? I->h_pcnt[i] : 0.0;
        else if (I->h_pflag[j]) Lc.val[k] = 0.0;
      }
    }
    I->singular = !any;
    HIPCHK(c, hipMemcpyAsync(I->Lv.p, Lc.val.data(), sizeof(double) * Lc.val.size(), hipMemcpyHostToDevice, s));
    HIPCHK(c, I->pflag.upload(I->h_pflag, s));
    HIPCHK(c, hipStreamSynchronize(s));
    // the hierarchy is built from a matrix without the explicit zeros of the eliminated rows / columns
    CsrHost La;
    La.n = La.m = nv; La.rowptr.assign(nv + 1, 0);
    for (int i = 0; i < nv; i++) {
      for (int k = Lc.rowptr[i]; k < Lc.rowptr[i + 1]; k++) {
        const int j = Lc.col[k];
        if ((I->h_pflag[i] || I->h_pflag[j]) && j != i) continue;
        La.col.push_back(j); La.val.push_back(Lc.val[k]);
      }
      La.rowptr[i + 1] = (int)La.col.size();
    }
    I->hLam.clear();
    int rc = -1;
    if (cfdh_amg_dev_enabled(c)) {
      CsrDev Ld;
      if (cfdh_upload_csr(c, La, Ld, nullptr, CFDH_UP_CSR) == 0) {
        HIPCHK(c, hipStreamSynchronize(s));
        rc = cfdh_amg_setup_dev(c, I->hLam, Ld, I->singular, 1);
      }
      if (rc != 0) {
        if (c->opt.verbose) fprintf(stderr, "[cfdh] device-side AMG set-up gave up (%s): building the pressure hierarchy on the host\n", c->err.c_str());
        c->err.clear(); I->hLam.clear();
      }
    }
    if (rc != 0) CHK(cfdh_amg_setup(c, I->hLam, La, I->singular, 1));
    I->pset_dirty = false;
    I->pbc_dirty = true;
  }
  if (I->pbc_dirty && I->scheme == CFDH_IPCS_MIDPOINT) {  // the lifting depends on p_prev: formed on the device each step (ip_plift_kernel)
    HIPCHK(c, I->pval.upload(I->h_pval, s)); HIPCHK(c, I->pcnt.upload(I->h_pcnt, s));
    HIPCHK(c, hipStreamSynchronize(s));
    I->pbc_dirty = false;
  }
  if (I->pbc_dirty) {
    std::vector<double> lift(nv, 0.0), fix(nv, 0.0);
    for (int i = 0; i < nv; i++) {
      if (I->h_pflag[i]) fix[i] = I->h_pcnt[i] * I->h_pval[i];
      for (int k = I->hL.rowptr[i]; k < I->hL.rowptr[i + 1]; k++) {
        const int j = I->hL.col[k];
        if (I->h_pflag[j]) lift[i] += I->hL.val[k] * I->h_pval[j];
      }
    }
    HIPCHK(c, hipMemcpyAsync(I->lift2.p, lift.data(), sizeof(double) * nv, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(I->prhs.p, fix.data(), sizeof(double) * nv, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipStreamSynchronize(s));
    I->pbc_dirty = false;
  }
  return 0;
}

static int ip_prepare(cfdh_ctx *c) {
  IpcsData *I = IP(c);
  hipStream_t s = c->stream;
  if (!c->params_set) return cfdh_fail(c, CFDH_E_STATE, "cfdh_set_params was not called");
  if (I->ubc_dirty) {
    HIPCHK(c, I->uflag.upload(I->h_uflag, s)); HIPCHK(c, I->ucnt.upload(I->h_ucnt, s)); HIPCHK(c, I->uval.upload(I->h_uval, s));
    HIPCHK(c, hipStreamSynchronize(s));
    I->ubc_dirty = false;
  }
  CHK(ip_prepare_pressure(c));
  if (I->rm_rho != c->rho) {  // rho M and its Jacobi weights
    std::vector<double> rm(I->hM.val.size()), di(I->nn);
    for (size_t k = 0; k < rm.size(); k++) rm[k] = c->rho * I->hM.val[k];
    for (int i = 0; i < I->nn; i++) di[i] = 1.0 / rm[ip_find(I->hM.rowptr, I->hM.col, i, i)];
    HIPCHK(c, hipMemcpyAsync(I->RMv.p, rm.data(), sizeof(double) * rm.size(), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(I->dinv3.p, di.data(), sizeof(double) * di.size(), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipStreamSynchronize(s));
    I->rm_rho = c->rho;
  }
  return 0;
}

template <int D>
static int ip_assemble_t(cfdh_ctx *c) {
  IpcsData *I = IP(c);
  constexpr int NL = D == 2 ? 6 : 10;
  const double conv = I->conv_coeff < 0 ? c->rho : I->conv_coeff, sf = I->force_default ? c->rho : I->force_coeff;
  IPL(c, ip_cw_kernel<D>, (I->nc + TPB - 1) / TPB, 0, I->nc, (const int *)I->d_cells.p, (const double *)I->d_geo.p, (const double *)I->u_prev.p,
      (const double *)I->u_n1.p, I->cw.p);
  IPL(c, ip_asm_kernel<D>, ip_grid8(I->nn), sizeof(double) * NL * NL * NL * D, I->nn, (const int *)I->rp2.p, (const int *)I->col2.p, (const int *)I->eptr.p,
      (const int *)I->elist.p, (const double *)I->d_T2.p, (const double *)I->cw.p, (const double *)I->Mv.p, (const double *)I->Kv.p, c->rho / c->dt,
      0.5 * c->mu, 0.5 * conv, (const unsigned char *)I->uflag.p, (const double *)I->ucnt.p, I->Afree.p, I->A1v.p, I->dinv1.p);
  IPL(c, ip_b1_kernel<D>, ip_grid8(I->nn), 0, I->nn, (const int *)I->rp2.p, (const int *)I->col2.p, (const double *)I->Mv.p, (const double *)I->Afree.p,
      2.0 * c->rho / c->dt, (const double *)I->u_prev.p, (const unsigned char *)I->uflag.p, (const double *)I->ucnt.p, (const double *)I->uval.p,
      (const int *)I->d_gptr.p, (const int *)I->d_gcol.p, (const double *)I->BTv.p, (const double *)I->p_sol.p, (const double *)I->d_m1.p, sf * c->f[0],
      sf * c->f[1], sf * c->f[2], I->b1.p);
  HIPCHK(c, hipGetLastError());
  I->assembled = true;
  I->n_assemblies++;
  return 0;
}

// ---- ipcs_midpoint ---------------------------------------------------------------------------------------------------
// Constant parts of the vector-coupled form, built once on the host (cells, then exterior facets, in ascending order):
//   E(i a, j b) = int d_b phi_i d_a phi_j dx              from 2 mu eps(u) : eps(v) = mu (grad phi_i . grad phi_j delta_ab + d_b phi_i d_a phi_j)
//   S(i a, j b) = int_{dOmega} phi_i d_a phi_j n_b ds     the ds term -mu (nabla_grad(u) n) . v; on the P2 pattern (both nodes in the facet's cell)
//   Pn(i a, k)  = int_{dOmega} phi_i psi_k n_a ds         the ds term p n . v; a sub-pattern of B^T, folded into BTPv = B^T - Pn
// The facet integrands are polynomials of degree 3: three-point Gauss on an edge, the degree-13 triangle rule on a face.  With
// gl_f = grad lambda_f of the vertex opposite the facet, n |facet| = -gl_f |det| / (D - 1)!.
static int ip_mid_build(cfdh_ctx *c) {
  IpcsData *I = IP(c);
  if (I->mid_built) return 0;
  const int D = I->D, NL = I->NL, NV = D + 1, nn = I->nn, nc = I->nc;
  hipStream_t s = c->stream;
  IpRef R;
  ip_reference(D, R);
  const size_t nnz2 = I->hM.col.size(), nnzG = I->gcol.size();
  std::vector<double> E(nnz2 * D * D, 0.0), Sb(nnz2 * D * D, 0.0);
  I->hPn.assign(nnzG * D, 0.0);
  auto grads = [&](int e, double gl[4][3], double &det) {  // grad lambda_0 .. lambda_D and |det| from geo (cfdh_ipcs_create)
    const double *g = I->geo.data() + (size_t)(D * D + 1) * e;
    det = g[D * D];
    for (int d = 0; d < D; d++) {
      gl[0][d] = 0.0;
      for (int q = 0; q < D; q++) { gl[q + 1][d] = g[D * q + d]; gl[0][d] -= g[D * q + d]; }
    }
  };
  for (int e = 0; e < nc; e++) {
    const int *cv = I->cells.data() + (size_t)NL * e;
    double gl[4][3], det;
    grads(e, gl, det);
    for (int a = 0; a < NL; a++)
      for (int b = 0; b < NL; b++) {
        const size_t k = (size_t)ip_find(I->hM.rowptr, I->hM.col, cv[a], cv[b]);
        const double *Kr = R.K.data() + ((size_t)a * NL + b) * NV * NV;
        for (int al = 0; al < D; al++)
          for (int be = 0; be < D; be++) {
            double v = 0.0;
            for (int i = 0; i < NV; i++)
              for (int j = 0; j < NV; j++) v += Kr[i * NV + j] * gl[i][be] * gl[j][al];
            E[(k * D + al) * D + be] += det * v;
          }
      }
  }
  // facet rule: barycentric points on the reference facet, weights summing to 1
  std::vector<double> fl, fw;
  if (D == 2) {
    const double h = 0.5 * std::sqrt(0.6), t[3] = {0.5 - h, 0.5, 0.5 + h}, w[3] = {5.0 / 18.0, 8.0 / 18.0, 5.0 / 18.0};
    for (int q = 0; q < 3; q++) { fl.push_back(1.0 - t[q]); fl.push_back(t[q]); fw.push_back(w[q]); }
  } else {
    for (int q = 0; q < CFDH_NQ; q++) { for (int i = 0; i < 3; i++) fl.push_back(CFDH_QL[q][i]); fw.push_back(CFDH_QW[q]); }
  }
  const double fact = D == 2 ? 1.0 : 0.5;  // 1 / (D - 1)!
  std::vector<double> phi(NL), dl((size_t)NL * NV);
  for (size_t kf = 0; kf < I->fcell.size(); kf++) {
    const int e = I->fcell[kf], f = I->flocal[kf];
    const int *cv = I->cells.data() + (size_t)NL * e;
    double gl[4][3], det;
    grads(e, gl, det);
    for (size_t q = 0; q < fw.size(); q++) {
      double lam[4];
      int m = 0;
      for (int i = 0; i < NV; i++) lam[i] = i == f ? 0.0 : fl[q * D + m++];
      ip_p2(D, lam, phi.data(), dl.data());
      const double w = fw[q] * det * fact;
      for (int a = 0; a < NL; a++) {
        if (phi[a] == 0.0) continue;  // nodes off the facet (their basis functions vanish on it identically)
        for (int b = 0; b < NL; b++) {
          const size_t k = (size_t)ip_find(I->hM.rowptr, I->hM.col, cv[a], cv[b]);
          for (int al = 0; al < D; al++) {
            double g = 0.0;
            for (int i = 0; i < NV; i++) g += dl[b * NV + i] * gl[i][al];
            for (int be = 0; be < D; be++) Sb[(k * D + al) * D + be] -= w * phi[a] * g * gl[f][be];
          }
        }
        for (int v = 0; v < NV; v++) {
          const size_t k = (size_t)ip_find(I->gptr, I->gcol, cv[a], cv[v]);
          for (int al = 0; al < D; al++) I->hPn[k * D + al] -= w * phi[a] * lam[v] * gl[f][al];
        }
      }
    }
  }
  I->hES.resize(E.size());
  for (size_t k = 0; k < E.size(); k++) I->hES[k] = E[k] - Sb[k];
  std::vector<double> btp(I->hBT.size());
  for (size_t k = 0; k < btp.size(); k++) btp[k] = I->hBT[k] - I->hPn[k];
  // the cells of every node, ascending
  std::vector<int> nptr(nn + 1, 0), nlist((size_t)NL * nc);
  for (size_t k = 0; k < nlist.size(); k++) nptr[I->cells[k] + 1]++;
  for (int i = 0; i < nn; i++) nptr[i + 1] += nptr[i];
  std::vector<int> fill(nptr.begin(), nptr.end() - 1);
  for (size_t k = 0; k < nlist.size(); k++) nlist[fill[I->cells[k]]++] = (int)k;  // k = cell * NL + local node
  HIPCHK(c, I->ESv.upload(I->hES, s)); HIPCHK(c, I->BTPv.upload(btp, s));
  HIPCHK(c, I->nptr.upload(nptr, s)); HIPCHK(c, I->nlist.upload(nlist, s));
  HIPCHK(c, I->Lfree.upload(I->hL.val, s));
  HIPCHK(c, I->AfreeB.alloc(nnz2 * D * D)); HIPCHK(c, I->A1B.alloc(nnz2 * D * D));
  HIPCHK(c, I->dinvB.alloc((size_t)nn * D)); HIPCHK(c, I->conv.alloc((size_t)nn * D));
  HIPCHK(c, hipStreamSynchronize(s));
  I->mid_built = true;
  return 0;
}

int cfdh_ipcs_set_scheme_impl(cfdh_ctx *c, int scheme) {
  IpcsData *I = IP(c);
  if (scheme == I->scheme) return 0;
  if (scheme == CFDH_IPCS_MIDPOINT) CHK(ip_mid_build(c));
  I->scheme = scheme;
  I->mid_valid = false; I->assembled = false;
  I->pbc_dirty = true;              // lift2 / prhs hold the other scheme's data
  HIPCHK(c, I->us.zero(c->stream));  // the initial guess of solve 1 belongs to the other scheme's u*
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

// block A1 of ipcs_midpoint: assembled only when dt, rho, mu, the scheme or the constrained velocity nodes / their counts changed
template <int D>
static int ip_mid_matrix(cfdh_ctx *c) {
  IpcsData *I = IP(c);
  bool ok = I->mid_valid && I->mid_key[0] == c->dt && I->mid_key[1] == c->rho && I->mid_key[2] == c->mu;
  if (ok && I->uset_dirty) ok = I->mid_flag == I->h_uflag && I->mid_cnt == I->h_ucnt;
  I->uset_dirty = false;
  if (ok) return 0;
  IPL(c, ip_asm_blk_kernel<D>, ip_grid8(I->nn), 0, I->nn, (const int *)I->rp2.p, (const int *)I->col2.p, (const double *)I->Mv.p, (const double *)I->Kv.p,
      (const double *)I->ESv.p, c->rho / c->dt, 0.5 * c->mu, (const unsigned char *)I->uflag.p, (const double *)I->ucnt.p, I->AfreeB.p, I->A1B.p,
      I->dinvB.p);
  HIPCHK(c, hipGetLastError());
  I->mid_key[0] = c->dt; I->mid_key[1] = c->rho; I->mid_key[2] = c->mu;
  I->mid_flag = I->h_uflag; I->mid_cnt = I->h_ucnt;
  I->mid_valid = true;
  I->n_assemblies++;
  return 0;
}

// A1 (if it is out of date) and b1 of the current state
template <int D>
static int ip_assemble_mid_t(cfdh_ctx *c) {
  IpcsData *I = IP(c);
  constexpr int NL = D == 2 ? 6 : 10;
  const double conv = I->conv_coeff < 0 ? c->rho : I->conv_coeff, sf = I->force_default ? c->rho : I->force_coeff;
  CHK(ip_mid_matrix<D>(c));
  IPL(c, (ip_cw_kernel<D, true>), (I->nc + TPB - 1) / TPB, 0, I->nc, (const int *)I->d_cells.p, (const double *)I->d_geo.p, (const double *)I->u_prev.p,
      (const double *)I->u_prev.p, I->cw.p);
  IPL(c, ip_conv_kernel<D>, ip_grid8(I->nn), sizeof(double) * NL * NL * NL * D, I->nn, (const int *)I->nptr.p, (const int *)I->nlist.p,
      (const int *)I->d_cells.p, (const double *)I->d_T2.p, (const double *)I->cw.p, (const double *)I->u_prev.p, I->conv.p);
  IPL(c, ip_b1_blk_kernel<D>, ip_grid8(I->nn), 0, I->nn, (const int *)I->rp2.p, (const int *)I->col2.p, (const double *)I->Mv.p, (const double *)I->AfreeB.p,
      2.0 * c->rho / c->dt, (const double *)I->u_prev.p, (const unsigned char *)I->uflag.p, (const double *)I->ucnt.p, (const double *)I->uval.p,
      (const int *)I->d_gptr.p, (const int *)I->d_gcol.p, (const double *)I->BTPv.p, (const double *)I->p_prev.p, (const double *)I->d_m1.p, sf * c->f[0],
      sf * c->f[1], sf * c->f[2], (const double *)I->conv.p, conv, I->b1.p);
  HIPCHK(c, hipGetLastError());
  I->assembled = true;
  return 0;
}

int cfdh_ipcs_assemble(cfdh_ctx *c) {
  CHK(ip_prepare(c));
  if (IP(c)->scheme == CFDH_IPCS_MIDPOINT) return IP(c)->D == 2 ? ip_assemble_mid_t<2>(c) : ip_assemble_mid_t<3>(c);
  return IP(c)->D == 2 ? ip_assemble_t<2>(c) : ip_assemble_t<3>(c);
}

// ---- Krylov drivers ------------------------------------------------------------------------------------------------
struct IpMat { int n; const int *rp, *col; const double *val; };

template <int D, int MODE, bool BLK = false>
static void ip_spmv(cfdh_ctx *c, const IpMat &A, const double *x, double *y, const double *q) {
  IpcsData *I = IP(c);
  if (BLK) IPL(c, (ip_spmv_blk_kernel<D, MODE>), ip_nb(A.n, TPB / 8), 0, A.n, A.rp, A.col, A.val, x, y, q, (const double *)I->S.p, I->P.p);
  else IPL(c, (ip_spmv_kernel<D, MODE>), ip_nb(A.n, TPB / 8), 0, A.n, A.rp, A.col, A.val, x, y, q, (const double *)I->S.p, I->P.p);
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
static int ip_bicgstab(cfdh_ctx *c, const IpMat &A, const double *dinv, const double *b, double *x, cfdh_ipcs_stats *st) {
  IpcsData *I = IP(c);
  const int n = A.n * D, nbv = ip_nb(n, TPB * 4), nbs = ip_nb(A.n, TPB / 8);
  const double rtol = I->rtol[0], atol = I->atol;
  const int max_it = I->max_it[0], batch = 4;
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
static int ip_cg(cfdh_ctx *c, int which, const IpMat &A, const double *dinv, const double *b, double *x, double *r, double *z, double *p, double *q,
                 cfdh_ipcs_stats *st) {
  IpcsData *I = IP(c);
  const int n = A.n * D, nbv = ip_nb(n, TPB * 4), nbs = ip_nb(A.n, TPB / 8);
  const double rtol = I->rtol[which], atol = I->atol;
  const int max_it = I->max_it[which], batch = JAC ? 4 : 1;
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

static int ip_sub_mean(cfdh_ctx *c, int n, double *x) {
  IpcsData *I = IP(c);
  const int nb = ip_nb(n, TPB * 4);
  IPL(c, ip_sum_kernel, nb, 0, n, (const double *)x, I->P.p);
  IPL(c, ip_submean_kernel, nb, 0, n, nb, (const double *)I->P.p, x);
  HIPCHK(c, hipGetLastError());
  return 0;
}

template <int D>
static int ip_step_t(cfdh_ctx *c, cfdh_ipcs_stats *st) {
  IpcsData *I = IP(c);
  hipStream_t s = c->stream;
  const int nn = I->nn, nv = I->nvert, n1 = nn * D;
  const double t0 = ip_now_ms();
  I->n_launch = 0; I->n_sync = 0;
  CHK(ip_prepare(c));
  CHK(ip_sync(c));
  const double t1 = ip_now_ms();
  const bool mid = I->scheme == CFDH_IPCS_MIDPOINT;
  CHK(mid ? ip_assemble_mid_t<D>(c) : ip_assemble_t<D>(c));
  CHK(ip_sync(c));
  const double t2 = ip_now_ms();
  // step 1 (initial guess: the previous u*)
  if (mid) {
    const IpMat A1{nn, I->rp2.p, I->col2.p, I->A1B.p};
    CHK((ip_bicgstab<D, true>(c, A1, I->dinvB.p, I->b1.p, I->us.p, st)));
  } else {
    const IpMat A1{nn, I->rp2.p, I->col2.p, I->A1v.p};
    CHK(ip_bicgstab<D>(c, A1, I->dinv1.p, I->b1.p, I->us.p, st));
  }
  const double t3 = ip_now_ms();
  // step 2 (ipcs_midpoint: the pressure Dirichlet value goes into p, so phi takes g - p_prev)
  if (st->reason[0] > 0) {
    if (mid)  // without a pressure object both come out zero
      IPL(c, ip_plift_kernel, ip_grid8(nv), 0, nv, (const int *)I->rp1.p, (const int *)I->col1.p, (const double *)I->Lfree.p,
          (const unsigned char *)I->pflag.p, (const double *)I->pcnt.p, (const double *)I->pval.p, (const double *)I->p_prev.p, I->lift2.p, I->prhs.p);
    IPL(c, ip_b2_kernel<D>, ip_grid8(nv), 0, nv, (const int *)I->d_bptr.p, (const int *)I->d_bcol.p, (const double *)I->Bv.p, (const double *)I->us.p,
        -c->rho / c->dt, (const unsigned char *)I->pflag.p, (const double *)I->lift2.p, (const double *)I->prhs.p, I->b2.p);
    if (I->singular) CHK(ip_sub_mean(c, nv, I->b2.p));
    HIPCHK(c, I->phi.zero(s));
    const IpMat L{nv, I->rp1.p, I->col1.p, I->Lv.p};
    CHK((ip_cg<1, false>(c, 1, L, nullptr, I->b2.p, I->phi.p, I->pr.p, I->pz.p, I->pp.p, I->pq.p, st)));
    if (I->singular) CHK(ip_sub_mean(c, nv, I->phi.p));
    if (mid) HIPCHK(c, hipMemcpyAsync(I->p_sol.p, I->p_prev.p, sizeof(double) * nv, hipMemcpyDeviceToDevice, s));  // p_sol = p_prev + phi
    IPL(c, ip_axpy_kernel, ip_nb(nv, TPB * 4), 0, nv, 1.0, (const double *)I->phi.p, I->p_sol.p);
  }
  const double t4 = ip_now_ms();
  // step 3 (initial guess: the previous u_sol)
  if (st->reason[0] > 0 && st->reason[1] > 0) {
    IPL(c, ip_b3_kernel<D>, ip_grid8(nn), 0, nn, (const int *)I->rp2.p, (const int *)I->col2.p, (const double *)I->Mv.p, c->rho, (const double *)I->us.p,
        (const int *)I->d_gptr.p, (const int *)I->d_gcol.p, (const double *)I->Gv.p, c->dt, (const double *)I->phi.p, I->b3.p);
    const IpMat RM{nn, I->rp2.p, I->col2.p, I->RMv.p};
    CHK((ip_cg<D, true>(c, 2, RM, I->dinv3.p, I->b3.p, I->u_sol.p, I->kr.p, I->kz.p, I->kp.p, I->kv.p, st)));
    // step 4 (ipcs_midpoint has no second history level)
    if (!mid) HIPCHK(c, hipMemcpyAsync(I->u_n1.p, I->u_prev.p, sizeof(double) * n1, hipMemcpyDeviceToDevice, s));
  }
  CHK(ip_sync(c));
  const double t5 = ip_now_ms();
  st->ms_assemble = t2 - t1; st->ms_solve[0] = t3 - t2; st->ms_solve[1] = t4 - t3; st->ms_solve[2] = t5 - t4; st->ms_total = t5 - t0;
  st->launches = (int)I->n_launch; st->host_syncs = (int)I->n_sync;
  return 0;
}

int cfdh_ipcs_step_impl(cfdh_ctx *c, cfdh_ipcs_stats *st) {
  IpcsData *I = IP(c);
  memset(st, 0, sizeof *st);
  CHK(I->D == 2 ? ip_step_t<2>(c, st) : ip_step_t<3>(c, st));
  I->last = *st;
  for (int k = 0; k < 3; k++)
    if (st->reason[k] <= 0) {
      static const char *name[3] = {"tentative velocity (BiCGStab)", "pressure correction (PCG)", "velocity update (CG)"};
      return cfdh_fail(c, CFDH_E_DIVERGED, "ipcs: the %s solve did not converge (reason %d, %d iterations, |r|/|b| = %.3e)", name[k], st->reason[k],
                       st->its[k], st->rel_res[k]);
    }
  return 0;
}

int cfdh_ipcs_apply_pc(cfdh_ctx *c, const double *r, double *z) {
  IpcsData *I = IP(c);
  CHK(ip_prepare(c));
  HIPCHK(c, hipMemcpyAsync(I->pr.p, r, sizeof(double) * I->nvert, hipMemcpyHostToDevice, c->stream));
  CHK(k_amg_vcycle(c, I->hLam, I->pr.p, I->pz.p));
  HIPCHK(c, hipMemcpyAsync(z, I->pz.p, sizeof(double) * I->nvert, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

// One driver on the caller's b and x0 (cfdh_ipcs_krylov_solve): the step's instantiation, matrix, Jacobi weights and work vectors;
// b and x live in buffers of the hook's own, the tolerances of the context are put back, b1 is kept over the assembly.
template <int D>
static int ip_krylov_solve_t(cfdh_ctx *c, int which, cfdh_ipcs_stats *st) {
  IpcsData *I = IP(c);
  if (which == 0 && I->scheme == CFDH_IPCS_MIDPOINT) {
    const IpMat A1{I->nn, I->rp2.p, I->col2.p, I->A1B.p};
    return ip_bicgstab<D, true>(c, A1, I->dinvB.p, I->hk_b.p, I->hk_x.p, st);
  }
  if (which == 0) {
    const IpMat A1{I->nn, I->rp2.p, I->col2.p, I->A1v.p};
    return ip_bicgstab<D>(c, A1, I->dinv1.p, I->hk_b.p, I->hk_x.p, st);
  }
  if (which == 1) {
    const IpMat L{I->nvert, I->rp1.p, I->col1.p, I->Lv.p};
    return ip_cg<1, false>(c, 1, L, nullptr, I->hk_b.p, I->hk_x.p, I->pr.p, I->pz.p, I->pp.p, I->pq.p, st);
  }
  const IpMat RM{I->nn, I->rp2.p, I->col2.p, I->RMv.p};
  return ip_cg<D, true>(c, 2, RM, I->dinv3.p, I->hk_b.p, I->hk_x.p, I->kr.p, I->kz.p, I->kp.p, I->kv.p, st);
}

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
    CHK(I->D == 2 ? ip_mid_matrix<2>(c) : ip_mid_matrix<3>(c));
  } else if (which == 0) {  // A1 of the current state; the assembly also writes b1, which is kept
    const bool was = I->assembled;
    HIPCHK(c, hipMemcpyAsync(I->hk_x.p, I->b1.p, sizeof(double) * n1, hipMemcpyDeviceToDevice, s));
    CHK(I->D == 2 ? ip_assemble_t<2>(c) : ip_assemble_t<3>(c));
    HIPCHK(c, hipMemcpyAsync(I->b1.p, I->hk_x.p, sizeof(double) * n1, hipMemcpyDeviceToDevice, s));
    I->assembled = was;
  }
  HIPCHK(c, hipMemcpyAsync(I->hk_b.p, b, sizeof(double) * n, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(I->hk_x.p, x0, sizeof(double) * n, hipMemcpyHostToDevice, s));
  const double rtol0 = I->rtol[which], atol0 = I->atol;
  const int max0 = I->max_it[which];
  I->rtol[which] = rtol; I->atol = atol; I->max_it[which] = max_it;
  I->snap_on = true; I->snap_set = false;
  const int rc = I->D == 2 ? ip_krylov_solve_t<2>(c, which, st) : ip_krylov_solve_t<3>(c, which, st);
  I->snap_on = false;
  I->rtol[which] = rtol0; I->atol = atol0; I->max_it[which] = max0;
  I->n_launch = launch0; I->n_sync = sync0;
  CHK(rc);
  HIPCHK(c, hipMemcpyAsync(x, I->hk_x.p, sizeof(double) * n, hipMemcpyDeviceToHost, s));
  if (scalars) HIPCHK(c, hipMemcpyAsync(scalars, I->S.p, sizeof(double) * IP_NS, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  if (scalars && I->snap_set)
    for (int k = IP_RHO; k <= IP_BETA; k++) scalars[k] = I->snap[k];
  return 0;
}

// ---- functionals ---------------------------------------------------------------------------------------------------
static int ip_reduce_host(cfdh_ctx *c, int nb, bool is_max, double *out) {
  IpcsData *I = IP(c);
  std::vector<double> h(nb);
  HIPCHK(c, hipMemcpyAsync(h.data(), I->P.p, sizeof(double) * nb, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  double a = 0.0;
  for (int i = 0; i < nb; i++) {
    if (!is_max) a += h[i];
    else if (h[i] > a || h[i] != h[i]) a = h[i];  // a NaN partial stays (std::max would drop it)
  }
  *out = a;
  return 0;
}
int cfdh_ipcs_functional(cfdh_ctx *c, int kind, int marker, double *out) {
  IpcsData *I = IP(c);
  const int D = I->D, nn = I->nn, nv = I->nvert, n1 = nn * D;
  if (kind == 0 || kind == 1) {
    if (D != 2) return cfdh_fail(c, CFDH_E_ARG, "cfdh_functional: drag / lift exist for gdim 2 only");
    const int nf = (int)I->fcell.size();
    *out = 0.0;
    if (nf == 0) return 0;
    if (!c->params_set) return cfdh_fail(c, CFDH_E_STATE, "cfdh_set_params was not called");
    hipLaunchKernelGGL(ip_draglift_kernel, dim3((nf + TPB - 1) / TPB), dim3(TPB), 0, c->stream, nf, (const int *)I->d_fcell.p, (const int *)I->d_flocal.p,
                       (const int *)I->d_fmarker.p, marker, kind, (const int *)I->d_cells.p, (const double *)I->d_coords.p, (const double *)I->d_geo.p,
                       (const double *)I->u_sol.p, (const double *)I->p_sol.p, c->mu, I->fout.p);
    HIPCHK(c, hipGetLastError());
    std::vector<double> h(nf);
    HIPCHK(c, hipMemcpyAsync(h.data(), I->fout.p, sizeof(double) * nf, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    double a = 0.0;
    for (int i = 0; i < nf; i++) a += h[i];
    *out = a;
    return 0;
  }
  if (kind == 2) {
    const int nb = ip_nb(nn, TPB / 8);
    if (D == 2) hipLaunchKernelGGL(ip_quad_kernel<2>, dim3(nb), dim3(TPB), 0, c->stream, nn, (const int *)I->rp2.p, (const int *)I->col2.p, (const double *)I->Mv.p, (const double *)I->u_sol.p, I->P.p);
    else hipLaunchKernelGGL(ip_quad_kernel<3>, dim3(nb), dim3(TPB), 0, c->stream, nn, (const int *)I->rp2.p, (const int *)I->col2.p, (const double *)I->Mv.p, (const double *)I->u_sol.p, I->P.p);
    CHK(ip_reduce_host(c, nb, false, out));
    *out = std::sqrt(std::max(*out, 0.0));
    return 0;
  }
  if (kind == 3) {
    const int nb = ip_nb(nv, TPB / 8);
    hipLaunchKernelGGL(ip_quad_kernel<1>, dim3(nb), dim3(TPB), 0, c->stream, nv, (const int *)I->rp1.p, (const int *)I->col1.p, (const double *)I->Mpv.p, (const double *)I->p_sol.p, I->P.p);
    CHK(ip_reduce_host(c, nb, false, out));
    *out = std::sqrt(std::max(*out, 0.0));
    return 0;
  }
  if (kind >= 4 && kind <= 6) {
    const int nb = ip_nb(n1, TPB * 4);
    const double *x = kind == 5 ? I->u_prev.p : I->u_sol.p, *y = kind == 6 ? I->u_prev.p : nullptr;
    hipLaunchKernelGGL(ip_maxdiff_kernel, dim3(nb), dim3(TPB), 0, c->stream, n1, x, y, I->P.p);
    return ip_reduce_host(c, nb, true, out);
  }
  return cfdh_fail(c, CFDH_E_ARG, "cfdh_functional: kind %d is not available on an IPCS context", kind);
}
