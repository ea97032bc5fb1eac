// Pressure convection-diffusion (PCD) Schur approximation, pc_type 2 (include/cfdh.h: cfdh_set_schur_pcd).  A restatement of the
// BRM2 variant fenicsx_pctools' PCDPC_vY applies in the reference's stabilized_pcd solver (stabilized_pcd.py:204-276), in this
// library's sign convention (S = A11 - A10 A00^-1 A01 positive):
//   S^-1 r_p ~ mu t + A_p^-1 (K t) ,  t = M_d^-1 r_p ,
//   K = rho N(w) - rho R_in(w) + c_t M   (N_ij = int phi_i w . grad phi_j, R_in,ij = int_{inlet} (w . n) phi_i phi_j, M consistent mass),
//   A_p = the P1 pressure Laplacian with Dirichlet rows on the outlet vertices (bcs_pcd, :215-218) and the pressure-Dirichlet ones.
// Two kernels: the row-owner assembly of K (once per Newton iteration, cfdh_pc_update) and the apply pass that feeds the V-cycle of
// A_p; the combination mu t + y runs in the epilogue of that cycle's last kernel (the Cahouet-Chabard epilogue of cfdh_amg_apply.hip).
#include <algorithm>
#include <cmath>

#include "cfdh_internal.hpp"

#define TPB 256

// K on the vertex graph of the owned rows, in SELL-64 layout (slices of 64 consecutive rows, column-major inside a slice: row r's
// k-th entry at sptr[r / 64] + 64 k + r % 64).  One thread per row walks the row vertex's cells in ascending cell order (the
// incidences of cfdh_pcd_setup) and then the inlet facets that contain it: fixed summation order, no atomics, bitwise reproducible.
// The thread owns its row's entries, so it accumulates them in place (they stay in L2 between the incidences).
//   inc word: cell * 4 + local index of the row vertex; islot: the row positions (8 bits each) of the cell's D + 1 vertices;
//   fac word: cell * 16 + local facet * 4 + local index of the row vertex, fslot as islot.
template <int D>
__global__ __launch_bounds__(TPB) void pcd_k_assemble_kernel(int nvo, const int *__restrict__ sptr, const int *__restrict__ rlen,
                                                             const int *__restrict__ iptr, const int *__restrict__ inc,
                                                             const unsigned *__restrict__ islot, const int *__restrict__ fptr,
                                                             const int *__restrict__ fac, const unsigned *__restrict__ fslot,
                                                             const int *__restrict__ cells, const double *__restrict__ X,
                                                             const double *__restrict__ x, const double *__restrict__ xprev, double th,
                                                             double rho, double ct, const int *__restrict__ scol,
                                                             const double *__restrict__ mdinv, double *__restrict__ K, float *__restrict__ Kf) {
  const int row = blockIdx.x * TPB + threadIdx.x;
  if (row >= nvo) return;
  constexpr int N1 = D + 1;
  const size_t base = (size_t)sptr[row >> 6] + (row & 63);
  const int len = rlen[row];
  for (int k = 0; k < len; k++) K[base + 64 * (size_t)k] = 0.0;
  // vertex coordinates, barycentric gradients and volume of cell e; w = th u + (1 - th) u_prev at its vertices
  auto cell_geom = [&](int e, double g[N1][D], double &vol, double w[N1][D]) {
    int v[N1];
    double P[N1][D];
#pragma unroll
    for (int a = 0; a < N1; a++) {
      v[a] = cells[(size_t)N1 * e + a];
#pragma unroll
      for (int i = 0; i < D; i++) {
        P[a][i] = X[(size_t)D * v[a] + i];
        w[a][i] = th * x[(size_t)D * v[a] + i] + (1.0 - th) * xprev[(size_t)D * v[a] + i];
      }
    }
    if (D == 2) {
      const double j00 = P[1][0] - P[0][0], j01 = P[2][0] - P[0][0], j10 = P[1][1] - P[0][1], j11 = P[2][1] - P[0][1];
      const double det = j00 * j11 - j01 * j10;
      vol = 0.5 * fabs(det);
      // rows of J^-1 = grad lambda_1, grad lambda_2
      g[1][0] = j11 / det; g[1][1] = -j01 / det;
      g[2][0] = -j10 / det; g[2][1] = j00 / det;
    } else {
      double J[3][3];
#pragma unroll
      for (int i = 0; i < 3; i++)
#pragma unroll
        for (int b = 0; b < 3; b++) J[i][b] = P[b + 1][i] - P[0][i];
      const double c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1], c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2], c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
      const double det = J[0][0] * c00 + J[0][1] * c01 + J[0][2] * c02;
      vol = fabs(det) / 6.0;
      // (J^-1)_{b,i} = cof(J)_{i,b} / det: grad lambda_{b+1}
      const double inv = 1.0 / det;
      g[1][0] = c00 * inv; g[2][0] = c01 * inv; g[3][0] = c02 * inv;
      g[1][1] = (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * inv; g[2][1] = (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * inv;
      g[3][1] = (J[0][1] * J[2][0] - J[0][0] * J[2][1]) * inv;
      g[1][2] = (J[0][1] * J[1][2] - J[0][2] * J[1][1]) * inv; g[2][2] = (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * inv;
      g[3][2] = (J[0][0] * J[1][1] - J[0][1] * J[1][0]) * inv;
    }
#pragma unroll
    for (int i = 0; i < D; i++) {
      double s = 0.0;
#pragma unroll
      for (int b = 1; b < N1; b++) s += g[b][i];
      g[0][i] = -s;
    }
  };
  const double cm = 1.0 / ((D + 1) * (D + 2));  // int phi_a phi_c = vol (1 + delta_ac) / ((d + 1)(d + 2))
  for (int q = iptr[row]; q < iptr[row + 1]; q++) {
    const int e = inc[q] >> 2, a = inc[q] & 3;
    const unsigned sl = islot[q];
    double g[N1][D], vol, w[N1][D];
    cell_geom(e, g, vol, w);
    // W = int phi_a w = vol cm (sum_c w_c + w_a)  (selects instead of run-time indices: everything stays in registers)
    double W[D];
#pragma unroll
    for (int i = 0; i < D; i++) {
      double s = 0.0;
#pragma unroll
      for (int c = 0; c < N1; c++) s += (c == a ? 2.0 : 1.0) * w[c][i];
      W[i] = vol * cm * s;
    }
#pragma unroll
    for (int b = 0; b < N1; b++) {
      double nb = 0.0;
#pragma unroll
      for (int i = 0; i < D; i++) nb += W[i] * g[b][i];
      const double v = rho * nb + ct * (vol * cm * (b == a ? 2.0 : 1.0));
      K[base + 64 * (size_t)((sl >> (8 * b)) & 0xffu)] += v;
    }
  }
  // inlet facets: - rho int_f (w . n) phi_a phi_b ds with the facet rules of the backflow term (exact for the cubic integrand):
  // 2-point Gauss on edges, the 6-point degree-3 rule on triangles.  n |f| = -d vol grad(lambda_f), so sigma = w . (n |f|)
  // carries the facet measure and the rule's weights sum to one.
  for (int q = fptr[row]; q < fptr[row + 1]; q++) {
    const int e = fac[q] >> 4, f = (fac[q] >> 2) & 3, a = fac[q] & 3;
    const unsigned sl = fslot[q];
    double g[N1][D], vol, w[N1][D];
    cell_geom(e, g, vol, w);
    double gf[D];
#pragma unroll
    for (int i = 0; i < D; i++) {
      double s = 0.0;
#pragma unroll
      for (int m = 0; m < N1; m++) s += m == f ? g[m][i] : 0.0;
      gf[i] = s;
    }
    // facet vertices j = 0 .. d-1 in increasing local index: m_j = j + (j >= f); sigma and lambda_a there
    double sj[D], aj[D];
#pragma unroll
    for (int j = 0; j < D; j++) {
      double s = 0.0;
#pragma unroll
      for (int m = 0; m < N1; m++)
        if (m == j + (j >= f ? 1 : 0)) {
#pragma unroll
          for (int i = 0; i < D; i++) s += w[m][i] * gf[i];
        }
      sj[j] = -(double)D * vol * s;
      aj[j] = (j + (j >= f ? 1 : 0)) == a ? 1.0 : 0.0;
    }
    double r[D];
#pragma unroll
    for (int j = 0; j < D; j++) r[j] = 0.0;
    if (D == 2) {
      const double gq = 0.28867513459481288;  // 1/(2 sqrt 3)
#pragma unroll
      for (int k = 0; k < 2; k++) {
        const double t = k == 0 ? 0.5 - gq : 0.5 + gq;
        const double l[2] = {1.0 - t, t};
        const double s = l[0] * sj[0] + l[1] * sj[1];
        const double la = aj[0] * l[0] + aj[1] * l[1];
#pragma unroll
        for (int j = 0; j < 2; j++) r[j] += 0.5 * s * la * l[j];
      }
    } else {
      const double A = 0.659027622374092, B = 0.231933368553031, C = 0.109039009072877;
      const double Pq[6][3] = {{A, B, C}, {A, C, B}, {B, A, C}, {B, C, A}, {C, A, B}, {C, B, A}};
#pragma unroll
      for (int k = 0; k < 6; k++) {
        double s = 0.0, la = 0.0;
#pragma unroll
        for (int j = 0; j < D; j++) { s += Pq[k][j] * sj[j]; la += aj[j] * Pq[k][j]; }
#pragma unroll
        for (int j = 0; j < D; j++) r[j] += (1.0 / 6.0) * s * la * Pq[k][j];
      }
    }
#pragma unroll
    for (int j = 0; j < D; j++) K[base + 64 * (size_t)((sl >> (8 * (j + (j >= f ? 1 : 0)))) & 0xffu)] -= rho * r[j];
  }
  // the apply pass streams K M_d^-1 (column j scaled by 1 / m_d,j, rounded to fp32): one gather per entry instead of two
  for (int k = 0; k < len; k++) {
    const size_t p = base + 64 * (size_t)k;
    Kf[p] = (float)(K[p] * mdinv[scol[p]]);
  }
}

// K on the node graph of a degree-1 generic context (rotational form): P1 triangles (ET 0), Q1 parallelograms and parallelepipeds
// (ET 2; node a sits at the reference corner (a & 1, a >> 1 & 1, a >> 2 & 1)).  The contract of pcd_k_assemble_kernel: one owner
// per row, its cells in ascending order and then its inlet facets, in place in the SELL-64 layout, no atomics.  The cells are
// affine, so with w in the element space every integrand is a polynomial of degree <= 3 per direction (<= 2 in total on a
// triangle) and the rules are exact: 2-point Gauss per direction, the 3-point degree-2 rule on the triangle, 2-point Gauss per
// direction on the facets.  Everything is indexed at compile time (the row's local node enters through selects): no scratch.
//   inc word: cell << AB | local node of the row, AB = 2 (gdim 2) or 3 (hexahedra); islot: 8 bits per local node, one word per
//   four nodes; fac word: (cell << AB | facet code) << AB | local node, facet code = the local facet of a triangle, 2 axis + side
//   of the reference face of a Q1 cell (cfdh_pcd_setup); fslot as islot.
template <int ET, int D>
__global__ __launch_bounds__(TPB) void pcd_k_assemble_gen_kernel(int nvo, const int *__restrict__ sptr, const int *__restrict__ rlen,
                                                                 const int *__restrict__ iptr, const int *__restrict__ inc,
                                                                 const unsigned *__restrict__ islot, const int *__restrict__ fptr,
                                                                 const int *__restrict__ fac, const unsigned *__restrict__ fslot,
                                                                 const int *__restrict__ cells, const double *__restrict__ X,
                                                                 const double *__restrict__ x, const double *__restrict__ xprev, double th,
                                                                 double rho, double ct, const int *__restrict__ scol,
                                                                 const double *__restrict__ mdinv, double *__restrict__ K, float *__restrict__ Kf) {
  const int row = blockIdx.x * TPB + threadIdx.x;
  if (row >= nvo) return;
  constexpr int NL = ET == 0 ? 3 : (1 << D);
  constexpr int AB = D == 2 ? 2 : 3, AM = (1 << AB) - 1;
  constexpr int SW = NL > 4 ? 2 : 1;
  const size_t base = (size_t)sptr[row >> 6] + (row & 63);
  const int len = rlen[row];
  for (int k = 0; k < len; k++) K[base + 64 * (size_t)k] = 0.0;
  const double g0 = 0.5 - 0.28867513459481288, g1 = 0.5 + 0.28867513459481288;  // 2-point Gauss on [0, 1]
  // Ji = (d x / d xi)^-1 (rows: grad xi_k), |det|, and w = th u + (1 - th) u_prev at the nodes of cell e
  auto cell_geom = [&](int e, double Ji[D][D], double &adet, double w[NL][D]) {
    double P[NL][D];
#pragma unroll
    for (int a = 0; a < NL; a++) {
      const int v = cells[(size_t)NL * e + a];
#pragma unroll
      for (int i = 0; i < D; i++) {
        P[a][i] = X[(size_t)D * v + i];
        w[a][i] = th * x[(size_t)D * v + i] + (1.0 - th) * xprev[(size_t)D * v + i];
      }
    }
    double J[D][D];  // column k: the edge along reference axis k
#pragma unroll
    for (int i = 0; i < D; i++)
#pragma unroll
      for (int k = 0; k < D; k++) J[i][k] = P[ET == 0 ? k + 1 : (1 << k)][i] - P[0][i];
    if constexpr (D == 2) {
      const double det = J[0][0] * J[1][1] - J[0][1] * J[1][0], inv = 1.0 / det;
      adet = fabs(det);
      Ji[0][0] = J[1][1] * inv; Ji[0][1] = -J[0][1] * inv;
      Ji[1][0] = -J[1][0] * inv; Ji[1][1] = J[0][0] * inv;
    } else {
      const double c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1], c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2], c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
      const double det = J[0][0] * c00 + J[0][1] * c01 + J[0][2] * c02, inv = 1.0 / det;
      adet = fabs(det);
      // (J^-1)_{k,i} = cof(J)_{i,k} / det
      Ji[0][0] = c00 * inv; Ji[1][0] = c01 * inv; Ji[2][0] = c02 * inv;
      Ji[0][1] = (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * inv; Ji[1][1] = (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * inv;
      Ji[2][1] = (J[0][1] * J[2][0] - J[0][0] * J[2][1]) * inv;
      Ji[0][2] = (J[0][1] * J[1][2] - J[0][2] * J[1][1]) * inv; Ji[1][2] = (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * inv;
      Ji[2][2] = (J[0][0] * J[1][1] - J[0][1] * J[1][0]) * inv;
    }
  };
  // at the reference point r: phi_b, the reference gradients, phi of the row's local node a, and wr_k = (grad xi_k) . w
  auto tabulate = [&](const double r[D], int a, const double Ji[D][D], const double w[NL][D], double ph[NL], double dr[NL][D], double &pa,
                      double wr[D]) {
    if (ET == 0) {
      ph[0] = 1.0 - r[0] - r[1]; ph[1] = r[0]; ph[2] = r[1];
      dr[0][0] = -1.0; dr[0][1] = -1.0; dr[1][0] = 1.0; dr[1][1] = 0.0; dr[2][0] = 0.0; dr[2][1] = 1.0;
    } else {
      double l[D][2];
#pragma unroll
      for (int k = 0; k < D; k++) { l[k][0] = 1.0 - r[k]; l[k][1] = r[k]; }
#pragma unroll
      for (int b = 0; b < NL; b++) {
        double p = 1.0;
#pragma unroll
        for (int k = 0; k < D; k++) p *= l[k][(b >> k) & 1];
        ph[b] = p;
#pragma unroll
        for (int k = 0; k < D; k++) {
          double g = ((b >> k) & 1) ? 1.0 : -1.0;
#pragma unroll
          for (int m = 0; m < D; m++) if (m != k) g *= l[m][(b >> m) & 1];
          dr[b][k] = g;
        }
      }
    }
    double wq[D];
    pa = 0.0;
#pragma unroll
    for (int i = 0; i < D; i++) wq[i] = 0.0;
#pragma unroll
    for (int b = 0; b < NL; b++) {
      pa = b == a ? ph[b] : pa;
#pragma unroll
      for (int i = 0; i < D; i++) wq[i] += ph[b] * w[b][i];
    }
#pragma unroll
    for (int k = 0; k < D; k++) {
      double s = 0.0;
#pragma unroll
      for (int i = 0; i < D; i++) s += Ji[k][i] * wq[i];
      wr[k] = s;
    }
  };
  auto scatter = [&](const unsigned *sl, const double acc[NL]) {
    const unsigned lo = sl[0], hi = SW > 1 ? sl[SW - 1] : 0u;
#pragma unroll
    for (int b = 0; b < NL; b++) K[base + 64 * (size_t)(((b < 4 ? lo : hi) >> (8 * (b & 3))) & 0xffu)] += acc[b];
  };
  for (int q = iptr[row]; q < iptr[row + 1]; q++) {
    const int e = inc[q] >> AB, a = inc[q] & AM;
    double Ji[D][D], adet, w[NL][D], acc[NL];
    cell_geom(e, Ji, adet, w);
#pragma unroll
    for (int b = 0; b < NL; b++) acc[b] = 0.0;
    constexpr int NQ = ET == 0 ? 3 : (1 << D);
    for (int k = 0; k < NQ; k++) {
      double r[D], wt;
      if (ET == 0) {
        r[0] = k == 1 ? 2.0 / 3.0 : 1.0 / 6.0; r[1] = k == 2 ? 2.0 / 3.0 : 1.0 / 6.0;
        wt = 1.0 / 6.0;
      } else {
#pragma unroll
        for (int m = 0; m < D; m++) r[m] = ((k >> m) & 1) ? g1 : g0;
        wt = 1.0 / (1 << D);
      }
      double ph[NL], dr[NL][D], pa, wr[D];
      tabulate(r, a, Ji, w, ph, dr, pa, wr);
      const double cn = rho * wt * adet * pa, cm = ct * wt * adet * pa;
#pragma unroll
      for (int b = 0; b < NL; b++) {
        double s = 0.0;
#pragma unroll
        for (int m = 0; m < D; m++) s += wr[m] * dr[b][m];
        acc[b] += cn * s + cm * ph[b];
      }
    }
    scatter(islot + (size_t)SW * q, acc);
  }
  // inlet facets: - rho int_f (w . n) phi_a phi_b ds.  n ds = |det| (grad xi)^T n_ref ds_ref, so w . n ds = |det| (n_ref . wr) ds_ref;
  // n_ref |f_ref| is (1, 1), (-1, 0), (0, -1) on the triangle's facets and -+ e_axis on a Q1 cell's, and the rule's weights sum to one.
  // phi_b vanishes on the facet for the nodes off it: their entries receive zeros.
  for (int q = fptr[row]; q < fptr[row + 1]; q++) {
    const int e = fac[q] >> (2 * AB), f = (fac[q] >> AB) & AM, a = fac[q] & AM;
    double Ji[D][D], adet, w[NL][D], acc[NL];
    cell_geom(e, Ji, adet, w);
#pragma unroll
    for (int b = 0; b < NL; b++) acc[b] = 0.0;
    double nf[D];
    if (ET == 0) { nf[0] = f == 0 ? 1.0 : (f == 1 ? -1.0 : 0.0); nf[1] = f == 0 ? 1.0 : (f == 2 ? -1.0 : 0.0); }
    else {
#pragma unroll
      for (int m = 0; m < D; m++) nf[m] = m == (f >> 1) ? ((f & 1) ? 1.0 : -1.0) : 0.0;
    }
    constexpr int NQF = 1 << (D - 1);
    for (int k = 0; k < NQF; k++) {
      const double t0 = (k & 1) ? g1 : g0, t1 = (k & 2) ? g1 : g0;
      double r[D];
      if (ET == 0) { r[0] = f == 0 ? 1.0 - t0 : (f == 1 ? 0.0 : t0); r[1] = f == 2 ? 0.0 : t0; }
      else {
#pragma unroll
        for (int m = 0; m < D; m++) r[m] = m == (f >> 1) ? (double)(f & 1) : ((m - (m > (f >> 1) ? 1 : 0)) == 0 ? t0 : t1);
      }
      double ph[NL], dr[NL][D], pa, wr[D];
      tabulate(r, a, Ji, w, ph, dr, pa, wr);
      double s = 0.0;
#pragma unroll
      for (int m = 0; m < D; m++) s += nf[m] * wr[m];
      const double cf = rho * (1.0 / NQF) * adet * s * pa;
#pragma unroll
      for (int b = 0; b < NL; b++) acc[b] -= cf * ph[b];
    }
    scatter(fslot + (size_t)SW * q, acc);
  }
  for (int k = 0; k < len; k++) {
    const size_t p = base + 64 * (size_t)k;
    Kf[p] = (float)(K[p] * mdinv[scol[p]]);
  }
}

// One pass in front of the A_p cycle, one lane per row over the fp32 SELL copy of K M_d^-1:
//   t = r / m_d (side output), s = K t = (K M_d^-1) r (0 on the Dirichlet rows of A_p: the cycle's right-hand side),
//   q = the fixed value the cycle's epilogue writes on those rows: r on pressure-Dirichlet rows, mu t on the other outlet rows.
// flag bit 0: Dirichlet row of A_p (pressure-Dirichlet or outlet), bit 1: pressure-Dirichlet row of the Jacobian.
__global__ __launch_bounds__(TPB) void pcd_apply_kernel(int n, const int *__restrict__ sptr, const int *__restrict__ scol,
                                                        const float *__restrict__ Kf, const double *__restrict__ mdinv,
                                                        const unsigned char *__restrict__ flag, const double *__restrict__ r, double mu,
                                                        double *__restrict__ t, double *__restrict__ s, double *__restrict__ q) {
  const int row = blockIdx.x * TPB + threadIdx.x;
  if (row >= n) return;
  const int sl = row >> 6, lane = row & 63;
  const int p0 = sptr[sl], w = (sptr[sl + 1] - p0) >> 6;
  const unsigned fl = flag[row];
  const double ri = r[row], ti = ri * mdinv[row];
  double acc = 0.0;
#pragma unroll 4
  for (int k = 0; k < w; k++) {
    const int p = p0 + k * 64 + lane;
    acc += (double)Kf[p] * r[scol[p]];
  }
  t[row] = ti;
  s[row] = (fl & 1u) ? 0.0 : acc;
  q[row] = (fl & 2u) ? ri : mu * ti;
}

// contexts pc_type 2 exists for: P1 simplices on the closed-form kernels, and the degree-1 cells of the rotational form on the generic
// ones (P1 triangles, Q1 parallelograms / parallelepipeds); one GPU
int cfdh_pcd_supported(cfdh_ctx *c, const char *who) {
  if (c->gen && c->form != CFDH_FORM_ROTATIONAL)
    return cfdh_fail(c, CFDH_E_ARG, "%s: PCD exists for P1 triangles and tetrahedra on the closed-form kernels, and on the generic element kernels in the "
                                    "rotational formulation only (cfdh_set_formulation first)", who);
  if (c->gen && c->etype == 1) return cfdh_fail(c, CFDH_E_ARG, "%s: PCD exists for degree-1 elements only (P1 / Q1), not for P2", who);
  if (c->nranks > 1 || c->nvo != c->nv) return cfdh_fail(c, CFDH_E_ARG, "%s: PCD is not available in partitioned runs", who);
  return 0;
}

// Host side of the operator's data (geometry, markers, node graph): incidences, inlet facets, SELL layout of K, 1 / M_d.
// Closed-form contexts have d + 1 nodes per cell and facet f opposite node f; generic ones nloc nodes and the facet tables of
// cfdh_facet_nodes / cfdh_facet_nodes3 (degree 1 only: cfdh_set_schur_pcd).  The packing of the words follows the kernels:
// ab bits per local node / facet code, 8 bits per slot and one slot word per four nodes.
int cfdh_pcd_setup(cfdh_ctx *c) {
  const int nvo = c->nvo, d = c->dim, n1 = c->gen ? c->nloc : d + 1;
  const int ab = n1 > 4 ? 3 : 2, sw = n1 > 4 ? 2 : 1;
  const bool q1 = c->gen && c->etype == 2;
  // node -> (cell, local) in ascending cell order, with the row positions of the cell's nodes
  std::vector<int> iptr(nvo + 1, 0), inc;
  std::vector<unsigned> islot;
  for (int e = 0; e < c->nc; e++)
    for (int a = 0; a < n1; a++) { const int v = c->h_cells[(size_t)n1 * e + a]; if (v < nvo) iptr[v + 1]++; }
  for (int v = 0; v < nvo; v++) iptr[v + 1] += iptr[v];
  inc.resize(iptr[nvo]); islot.resize((size_t)sw * iptr[nvo]);
  auto slots_of = [&](int v, int e, unsigned *s) {
    const int *nb = &c->h_vcol[c->h_vptr[v]];
    const int deg = c->h_vptr[v + 1] - c->h_vptr[v];
    for (int w = 0; w < sw; w++) s[w] = 0;
    for (int b = 0; b < n1; b++) {
      const int k = (int)(std::lower_bound(nb, nb + deg, c->h_cells[(size_t)n1 * e + b]) - nb);
      s[b >> 2] |= (unsigned)k << (8 * (b & 3));
    }
  };
  {
    std::vector<int> fill(iptr.begin(), iptr.end() - 1);
    for (int e = 0; e < c->nc; e++)
      for (int a = 0; a < n1; a++) {
        const int v = c->h_cells[(size_t)n1 * e + a];
        if (v >= nvo) continue;
        const int q = fill[v]++;
        inc[q] = (e << ab) + a;
        slots_of(v, e, &islot[(size_t)sw * q]);
      }
  }
  // inlet facets per row node (facet order of cfdh_create, the facet's cell then fixes the order)
  std::vector<int> fptr(nvo + 1, 0), fac;
  std::vector<unsigned> fslot;
  std::vector<std::vector<std::pair<int, int>>> rows(nvo);
  for (int k = 0; k < c->nfac; k++) {
    if (c->fac_marker[k] != c->pcd_in) continue;
    const int e = c->fac_cell[k], f = c->fac_local[k];
    int loc[8], nn = 0, code = f;
    if (c->gen) nn = d == 3 ? cfdh_facet_nodes3(c, f, loc) : cfdh_facet_nodes(c, f, loc);
    else for (int a = 0; a < n1; a++) if (a != f) loc[nn++] = a;
    if (q1) {  // the reference face: the axis on which all its nodes agree, and their side of it
      int all = n1 - 1, any = 0;
      for (int q = 0; q < nn; q++) { all &= loc[q]; any |= loc[q]; }
      code = -1;
      for (int ax = 0; ax < d; ax++) {
        if ((all >> ax) & 1) code = 2 * ax + 1;
        else if (!((any >> ax) & 1)) code = 2 * ax;
      }
      if (code < 0) return cfdh_fail(c, CFDH_E_ARG, "cfdh_pcd_setup: local facet %d is no face of the reference cell", f);
    }
    for (int q = 0; q < nn; q++) {
      const int a = loc[q], v = c->h_cells[(size_t)n1 * e + a];
      if (v < nvo) rows[v].push_back({e, (((e << ab) + code) << ab) + a});
    }
  }
  for (int v = 0; v < nvo; v++) {
    std::sort(rows[v].begin(), rows[v].end());
    for (auto &p : rows[v]) {
      fac.push_back(p.second);
      fslot.resize(fslot.size() + sw);
      slots_of(v, p.first, &fslot[fslot.size() - sw]);
    }
    fptr[v + 1] = (int)fac.size();
  }
  // SELL-64 layout of the vertex graph (padding: column = row, value 0)
  const int nsl = (nvo + 63) / 64;
  std::vector<int> sptr(nsl + 1, 0), rlen(nvo);
  for (int s = 0; s < nsl; s++) {
    int wmax = 0;
    for (int r = 64 * s; r < std::min(nvo, 64 * s + 64); r++) wmax = std::max(wmax, c->h_vptr[r + 1] - c->h_vptr[r]);
    sptr[s + 1] = sptr[s] + 64 * wmax;
  }
  std::vector<int> scol((size_t)sptr[nsl]);
  for (int s = 0; s < nsl; s++) {
    const int w = (sptr[s + 1] - sptr[s]) / 64;
    for (int l = 0; l < 64; l++) {
      const int r = 64 * s + l;
      for (int k = 0; k < w; k++) {
        const size_t p = (size_t)sptr[s] + 64 * (size_t)k + l;
        if (r >= nvo) scol[p] = 0;
        else scol[p] = k < c->h_vptr[r + 1] - c->h_vptr[r] ? c->h_vcol[c->h_vptr[r] + k] : r;
      }
    }
  }
  for (int r = 0; r < nvo; r++) rlen[r] = c->h_vptr[r + 1] - c->h_vptr[r];
  // diagonal of the consistent mass: per cell vol * 2 / ((d + 1)(d + 2)) on a simplex, vol / 3^d on an affine Q1 cell (edges along the
  // reference axes: nodes 1, 2, 4)
  std::vector<double> md(nvo, 0.0);
  const double *X = c->h_coords.data();
  for (int e = 0; e < c->nc; e++) {
    const int *v = &c->h_cells[(size_t)n1 * e];
    const int v1 = v[1], v2 = v[2], v3 = d == 3 ? v[q1 ? 4 : 3] : 0;
    double vol;  // simplex: its measure; Q1: |det|
    if (d == 2) {
      vol = 0.5 * std::fabs((X[2 * v1] - X[2 * v[0]]) * (X[2 * v2 + 1] - X[2 * v[0] + 1]) -
                            (X[2 * v1 + 1] - X[2 * v[0] + 1]) * (X[2 * v2] - X[2 * v[0]]));
      if (q1) vol *= 2.0;
    } else {
      const int vb[3] = {v1, v2, v3};
      double J[3][3];
      for (int i = 0; i < 3; i++) for (int b = 0; b < 3; b++) J[i][b] = X[3 * vb[b] + i] - X[3 * v[0] + i];
      vol = std::fabs(J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) + J[0][1] * (J[1][2] * J[2][0] - J[1][0] * J[2][2]) +
                      J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0])) / (q1 ? 1.0 : 6.0);
    }
    const double ma = q1 ? vol / (d == 2 ? 9.0 : 27.0) : vol * 2.0 / ((d + 1) * (d + 2));
    for (int a = 0; a < n1; a++) if (v[a] < nvo) md[v[a]] += ma;
  }
  c->h_pcd_md = md;
  std::vector<double> mdinv(nvo);
  for (int v = 0; v < nvo; v++) mdinv[v] = 1.0 / md[v];
  HIPCHK(c, c->pcd_iptr.upload(iptr, c->stream)); HIPCHK(c, c->pcd_inc.upload(inc, c->stream)); HIPCHK(c, c->pcd_islot.upload(islot, c->stream));
  if (fac.empty()) { fac.push_back(0); fslot.assign(sw, 0u); }  // no inlet facet: a valid (unread) buffer all the same
  HIPCHK(c, c->pcd_fptr.upload(fptr, c->stream)); HIPCHK(c, c->pcd_fac.upload(fac, c->stream)); HIPCHK(c, c->pcd_fslot.upload(fslot, c->stream));
  HIPCHK(c, c->pcd_sptr.upload(sptr, c->stream)); HIPCHK(c, c->pcd_scol.upload(scol, c->stream)); HIPCHK(c, c->pcd_rlen.upload(rlen, c->stream));
  HIPCHK(c, c->pcd_mdinv.upload(mdinv, c->stream));
  HIPCHK(c, c->pcd_K.alloc(std::max((size_t)sptr[nsl], (size_t)1))); HIPCHK(c, c->pcd_K.zero(c->stream));
  HIPCHK(c, c->pcd_Kf.alloc(std::max((size_t)sptr[nsl], (size_t)1))); HIPCHK(c, c->pcd_Kf.zero(c->stream));
  HIPCHK(c, c->pcd_t.alloc(nvo)); HIPCHK(c, c->pcd_q.alloc(nvo));  // (pcd_flag: uploaded with the A_p hierarchy, cfdh_solver.cpp)
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->pcd_ready = true;
  return 0;
}

// K from the iterate xstate (and u_prev), with the time scheme of cfdh_set_time_scheme
int k_pcd_assemble(cfdh_ctx *c, const double *xstate) {
  if (!c->pcd_ready) CHK(cfdh_pcd_setup(c));
  const int nvo = c->nvo;
  c->pcd_ct = c->pcd_time ? c->rho * c->ts_a[0] / (c->ts_theta * c->dt) : 0.0;
  dim3 block(TPB), grid((unsigned)((nvo + TPB - 1) / TPB));
  prof_begin(c, 10);
#define PCD_K_ARGS grid, block, 0, c->stream, nvo, c->pcd_sptr.p, c->pcd_rlen.p, c->pcd_iptr.p, c->pcd_inc.p, c->pcd_islot.p, c->pcd_fptr.p, \
                   c->pcd_fac.p, c->pcd_fslot.p, c->cells.p, c->coords.p, xstate, c->xprev.p, c->ts_theta, c->rho, c->pcd_ct, c->pcd_scol.p, \
                   c->pcd_mdinv.p, c->pcd_K.p, c->pcd_Kf.p
  if (c->gen) {  // degree 1 only (cfdh_set_schur_pcd)
    if (c->etype == 0 && c->dim == 2) hipLaunchKernelGGL((pcd_k_assemble_gen_kernel<0, 2>), PCD_K_ARGS);
    else if (c->etype == 2 && c->dim == 2) hipLaunchKernelGGL((pcd_k_assemble_gen_kernel<2, 2>), PCD_K_ARGS);
    else if (c->etype == 2 && c->dim == 3) hipLaunchKernelGGL((pcd_k_assemble_gen_kernel<2, 3>), PCD_K_ARGS);
    else return cfdh_fail(c, CFDH_E_ARG, "PCD: no K assembly for this element");
  } else if (c->dim == 2)
    hipLaunchKernelGGL(pcd_k_assemble_kernel<2>, PCD_K_ARGS);
  else
    hipLaunchKernelGGL(pcd_k_assemble_kernel<3>, PCD_K_ARGS);
#undef PCD_K_ARGS
  prof_end(c, 10);
  HIPCHK(c, hipGetLastError());
  return 0;
}

// t = r / m_d, s = K t (0 on the Dirichlet rows of A_p), q = the epilogue's fixed values
int k_pcd_apply(cfdh_ctx *c, const double *r, double *s) {
  const int n = c->nvo;
  prof_begin(c, 11);
  hipLaunchKernelGGL(pcd_apply_kernel, dim3((unsigned)((n + TPB - 1) / TPB)), dim3(TPB), 0, c->stream, n, c->pcd_sptr.p, c->pcd_scol.p,
                     c->pcd_Kf.p, c->pcd_mdinv.p, c->pcd_flag.p, r, c->mu, c->pcd_t.p, s, c->pcd_q.p);
  prof_end(c, 11);
  HIPCHK(c, hipGetLastError());
  return 0;
}
