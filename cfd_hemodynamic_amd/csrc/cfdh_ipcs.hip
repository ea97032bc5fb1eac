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
// The three solves are cfdh_ipcs_krylov.hip's (ip_solve); the host arithmetic of the set-up is cfdh_ipcs_host.hpp's, uploaded by
// cfdh_ipcs_setup.cpp.  This file holds the assembly and right-hand-side kernels, the step and the functionals.
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
#include "cfdh_ipcs.hpp"

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

// block A1 of ipcs_midpoint: assembled only when dt, rho, mu, the scheme or the constrained velocity nodes / their counts changed
template <int D>
static int ip_mid_matrix_t(cfdh_ctx *c) {
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
  CHK(ip_mid_matrix_t<D>(c));
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

int ip_assemble_bdf2(cfdh_ctx *c) { return IP(c)->D == 2 ? ip_assemble_t<2>(c) : ip_assemble_t<3>(c); }
int ip_mid_matrix(cfdh_ctx *c) { return IP(c)->D == 2 ? ip_mid_matrix_t<2>(c) : ip_mid_matrix_t<3>(c); }
int cfdh_ipcs_assemble(cfdh_ctx *c) {
  CHK(ip_prepare(c));
  if (IP(c)->scheme == CFDH_IPCS_MIDPOINT) return IP(c)->D == 2 ? ip_assemble_mid_t<2>(c) : ip_assemble_mid_t<3>(c);
  return ip_assemble_bdf2(c);
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
  const auto tol = [I](int which) { return IpTol{I->rtol[which], I->atol, I->max_it[which]}; };
  CHK(mid ? ip_assemble_mid_t<D>(c) : ip_assemble_t<D>(c));
  CHK(ip_sync(c));
  const double t2 = ip_now_ms();
  // step 1 (initial guess: the previous u*)
  CHK(ip_solve<D>(c, 0, tol(0), I->b1.p, I->us.p, st));
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
    CHK(ip_solve<D>(c, 1, tol(1), I->b2.p, I->phi.p, st));
    if (I->singular) CHK(ip_sub_mean(c, nv, I->phi.p));
    if (mid) HIPCHK(c, hipMemcpyAsync(I->p_sol.p, I->p_prev.p, sizeof(double) * nv, hipMemcpyDeviceToDevice, s));  // p_sol = p_prev + phi
    IPL(c, ip_axpy_kernel, ip_nb(nv, TPB * 4), 0, nv, 1.0, (const double *)I->phi.p, I->p_sol.p);
  }
  const double t4 = ip_now_ms();
  // step 3 (initial guess: the previous u_sol)
  if (st->reason[0] > 0 && st->reason[1] > 0) {
    IPL(c, ip_b3_kernel<D>, ip_grid8(nn), 0, nn, (const int *)I->rp2.p, (const int *)I->col2.p, (const double *)I->Mv.p, c->rho, (const double *)I->us.p,
        (const int *)I->d_gptr.p, (const int *)I->d_gcol.p, (const double *)I->Gv.p, c->dt, (const double *)I->phi.p, I->b3.p);
    CHK(ip_solve<D>(c, 2, tol(2), I->b3.p, I->u_sol.p, st));
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
