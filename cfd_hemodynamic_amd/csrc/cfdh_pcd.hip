// Pressure convection-diffusion (PCD) Schur approximation, pc_type 2 (include/cfdh.h: cfdh_set_schur_pcd).  A restatement of the
// BRM2 variant fenicsx_pctools' PCDPC_vY applies in the reference's stabilized_pcd solver (stabilized_pcd.py:204-276), in this
// library's sign convention (S = A11 - A10 A00^-1 A01 positive):
//   S^-1 r_p ~ mu t + A_p^-1 (K t) ,  t = M_d^-1 r_p ,
//   K = rho N(w) - rho R_in(w) + c_t M   (N_ij = int phi_i w . grad phi_j, R_in,ij = int_{inlet} (w . n) phi_i phi_j, M consistent mass),
//   A_p = the P1 pressure Laplacian with Dirichlet rows on the outlet vertices (bcs_pcd, :215-218) and the pressure-Dirichlet ones.
// Two kernels: the row-owner assembly of K (once per Newton iteration, cfdh_pc_update) and the apply pass that feeds the V-cycle of
// A_p; the combination mu t + y runs in the epilogue of that cycle's last kernel (the Cahouet-Chabard epilogue of cfdh_kernels.hip).
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

// Host side of the operator's data (geometry, markers, vertex graph): incidences, inlet facets, SELL layout of K, 1 / M_d.
int cfdh_pcd_setup(cfdh_ctx *c) {
  const int nvo = c->nvo, d = c->dim, n1 = d + 1;
  // vertex -> (cell, local) in ascending cell order, with the row positions of the cell's vertices
  std::vector<int> iptr(nvo + 1, 0), inc;
  std::vector<unsigned> islot;
  for (int e = 0; e < c->nc; e++)
    for (int a = 0; a < n1; a++) { const int v = c->h_cells[(size_t)n1 * e + a]; if (v < nvo) iptr[v + 1]++; }
  for (int v = 0; v < nvo; v++) iptr[v + 1] += iptr[v];
  inc.resize(iptr[nvo]); islot.resize(iptr[nvo]);
  auto slots_of = [&](int v, int e) {
    const int *nb = &c->h_vcol[c->h_vptr[v]];
    const int deg = c->h_vptr[v + 1] - c->h_vptr[v];
    unsigned s = 0;
    for (int b = 0; b < n1; b++) {
      const int k = (int)(std::lower_bound(nb, nb + deg, c->h_cells[(size_t)n1 * e + b]) - nb);
      s |= (unsigned)k << (8 * b);
    }
    return s;
  };
  {
    std::vector<int> fill(iptr.begin(), iptr.end() - 1);
    for (int e = 0; e < c->nc; e++)
      for (int a = 0; a < n1; a++) {
        const int v = c->h_cells[(size_t)n1 * e + a];
        if (v >= nvo) continue;
        const int q = fill[v]++;
        inc[q] = 4 * e + a;
        islot[q] = slots_of(v, e);
      }
  }
  // inlet facets per row vertex (facet order of cfdh_create, the facet's cell then fixes the order)
  std::vector<int> fptr(nvo + 1, 0), fac;
  std::vector<unsigned> fslot;
  std::vector<std::vector<std::pair<int, int>>> rows(nvo);
  for (int k = 0; k < c->nfac; k++) {
    if (c->fac_marker[k] != c->pcd_in) continue;
    const int e = c->fac_cell[k], f = c->fac_local[k];
    for (int a = 0; a < n1; a++) {
      if (a == f) continue;
      const int v = c->h_cells[(size_t)n1 * e + a];
      if (v < nvo) rows[v].push_back({e, 16 * e + 4 * f + a});
    }
  }
  for (int v = 0; v < nvo; v++) {
    std::sort(rows[v].begin(), rows[v].end());
    for (auto &p : rows[v]) { fac.push_back(p.second); fslot.push_back(slots_of(v, p.first)); }
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
  // diagonal of the consistent mass: sum over the cells of vol * 2 / ((d + 1)(d + 2))
  std::vector<double> md(nvo, 0.0);
  const double *X = c->h_coords.data();
  for (int e = 0; e < c->nc; e++) {
    const int *v = &c->h_cells[(size_t)n1 * e];
    double vol;
    if (d == 2) {
      vol = 0.5 * std::fabs((X[2 * v[1]] - X[2 * v[0]]) * (X[2 * v[2] + 1] - X[2 * v[0] + 1]) -
                            (X[2 * v[1] + 1] - X[2 * v[0] + 1]) * (X[2 * v[2]] - X[2 * v[0]]));
    } else {
      double J[3][3];
      for (int i = 0; i < 3; i++) for (int b = 0; b < 3; b++) J[i][b] = X[3 * v[b + 1] + i] - X[3 * v[0] + i];
      vol = std::fabs(J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) + J[0][1] * (J[1][2] * J[2][0] - J[1][0] * J[2][2]) +
                      J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0])) / 6.0;
    }
    for (int a = 0; a < n1; a++) if (v[a] < nvo) md[v[a]] += vol * 2.0 / ((d + 1) * (d + 2));
  }
  c->h_pcd_md = md;
  std::vector<double> mdinv(nvo);
  for (int v = 0; v < nvo; v++) mdinv[v] = 1.0 / md[v];
  HIPCHK(c, c->pcd_iptr.upload(iptr, c->stream)); HIPCHK(c, c->pcd_inc.upload(inc, c->stream)); HIPCHK(c, c->pcd_islot.upload(islot, c->stream));
  if (fac.empty()) { fac.push_back(0); fslot.push_back(0); }  // no inlet facet: a valid (unread) buffer all the same
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
  if (c->dim == 2)
    hipLaunchKernelGGL(pcd_k_assemble_kernel<2>, grid, block, 0, c->stream, nvo, c->pcd_sptr.p, c->pcd_rlen.p, c->pcd_iptr.p, c->pcd_inc.p,
                       c->pcd_islot.p, c->pcd_fptr.p, c->pcd_fac.p, c->pcd_fslot.p, c->cells.p, c->coords.p, xstate, c->xprev.p, c->ts_theta,
                       c->rho, c->pcd_ct, c->pcd_scol.p, c->pcd_mdinv.p, c->pcd_K.p, c->pcd_Kf.p);
  else
    hipLaunchKernelGGL(pcd_k_assemble_kernel<3>, grid, block, 0, c->stream, nvo, c->pcd_sptr.p, c->pcd_rlen.p, c->pcd_iptr.p, c->pcd_inc.p,
                       c->pcd_islot.p, c->pcd_fptr.p, c->pcd_fac.p, c->pcd_fslot.p, c->cells.p, c->coords.p, xstate, c->xprev.p, c->ts_theta,
                       c->rho, c->pcd_ct, c->pcd_scol.p, c->pcd_mdinv.p, c->pcd_K.p, c->pcd_Kf.p);
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
