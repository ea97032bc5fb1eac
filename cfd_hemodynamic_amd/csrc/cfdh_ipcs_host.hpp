// Host arithmetic of the pressure-correction context (cfdh_create_ipcs; cfdh_ipcs_setup.cpp): the P2 reference tensors, the four
// sparsity patterns, the cell geometry, the constant operators with their per-entry element lists, the constants of
// ipcs_midpoint, the Dirichlet treatment of the pressure Laplacian, rho M.  Plain C++17 on std::vector without HIP, so that the
// CPU tests compile it with the host compiler (tests/ipcs_host_shim.cpp, tests/ipcs_host_main.cpp).  A step that refuses its
// input returns false and leaves the reason in `msg`; the builder hands it to cfdh_fail(c, CFDH_E_ARG, ...).
// Every loop runs over the cells in ascending order, then over the exterior facets in ascending order: that fixed order of the
// sums makes the arrays reproducible bit for bit.  Node numbering is the caller's: vertices [0, nvert), then the edge nodes.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "cfdh_quad_tet.h"
#include "cfdh_quad_tri.h"

namespace cfdh_ipcs_host {

static const int IP_TRI_EDGES[3][2] = {{1, 2}, {0, 2}, {0, 1}};
static const int IP_TET_EDGES[6][2] = {{2, 3}, {1, 3}, {1, 2}, {0, 3}, {0, 2}, {0, 1}};

// P2 basis and its derivatives with respect to the barycentric coordinates at lam
inline void ip_p2(int D, const double *lam, double *phi, double *dl /*[NL][D+1]*/) {
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

// reference tensors (volume of the reference simplex 1 / D! included): M[a][b] = int phi_a phi_b, K[a][b][i][j] = int d_li phi_a d_lj phi_b,
// T2[a][b][k][e] = int phi_a phi_k d_xi_e phi_b, B[v][b][i] = int lam_v d_li phi_b, G[a] = int phi_a, MP[v][w] = int lam_v lam_w
struct IpRef {
  int D, NL, NV;
  std::vector<double> M, K, T2, B, G, MP;
};
inline void ip_reference(int D, IpRef &R) {
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
inline void ip_pattern(int nrows, int nc, const int *rc, int nr, const int *cc, int ncl, std::vector<int> &ptr, std::vector<int> &col) {
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
inline int ip_find(const std::vector<int> &ptr, const std::vector<int> &col, int i, int j) {
  return (int)(std::lower_bound(col.begin() + ptr[i], col.begin() + ptr[i + 1], j) - col.begin());
}

// ---- refusals of cfdh_create_ipcs: sizes within int32 indexing, vertices in the vertex slots and edge nodes in the edge slots
inline bool ip_check_mesh(int D, int64_t nn, int64_t nvert, int64_t nc, const int32_t *cells, std::string &msg) {
  const int NL = D == 2 ? 6 : 10, NV = D + 1;
  if (nn <= 0 || nvert <= 0 || nvert > nn || nc <= 0 || nn * D > 2000000000ll || nc * NL * NL > 2000000000ll) {
    msg = "cfdh_create_ipcs: bad sizes";
    return false;
  }
  for (int64_t k = 0; k < (int64_t)NL * nc; k++) {
    const int v = cells[k], a = (int)(k % NL);
    if (v < 0 || v >= nn || (a < NV && v >= nvert) || (a >= NV && v < nvert)) {
      msg = "cfdh_create_ipcs: cell node out of range (vertices must be the nodes [0, nvert), edge nodes the rest)";
      return false;
    }
  }
  return true;
}

// geo[cell] = (Jinv [D][D], |det|), Jinv[q][d] = d xi_q / d x_d = grad lambda_{q+1}; refuses a cell without volume
inline bool ip_geometry(int D, int nc, const int32_t *cells, const double *coords, std::vector<double> &geo, std::string &msg) {
  const int NL = D == 2 ? 6 : 10;
  geo.assign((size_t)(D * D + 1) * nc, 0.0);
  for (int e = 0; e < nc; e++) {
    const int *cv = cells + (size_t)NL * e;
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
    if (!(std::fabs(det) > 0)) {
      char buf[64];
      snprintf(buf, sizeof buf, "cfdh_create_ipcs: degenerate cell %d", e);
      msg = buf;
      return false;
    }
    for (int q = 0; q < D; q++)
      for (int d = 0; d < D; d++) geo[(size_t)(D * D + 1) * e + D * q + d] = inv[q][d];
    geo[(size_t)(D * D + 1) * e + D * D] = std::fabs(det);
  }
  return true;
}
// grad lambda_0 .. lambda_D and |det| of cell e from geo
inline void grad_lambda(int D, const double *geo, int e, double gl[4][3], double &det) {
  const double *g = geo + (size_t)(D * D + 1) * e;
  det = g[D * D];
  for (int d = 0; d < D; d++) {
    gl[0][d] = 0.0;
    for (int q = 0; q < D; q++) { gl[q + 1][d] = g[D * q + d]; gl[0][d] -= g[D * q + d]; }
  }
}

// ---- constant operators.  P2 pattern ptr2 / col2 (M, K, A1), P1 pattern ptr1 / col1 (L, Mp), [nn x nvert] gptr / gcol (G_d,
// B_d^T), [nvert x nn] bptr / bcol (B_d); G, BT, B hold [nnz][D] interleaved; m1 = int phi_i.  The element contributions of P2
// entry k are listed in elist[eptr[k] .. eptr[k+1]) as cell * NL^2 + a * NL + b, ascending.
struct IpOps {
  std::vector<int> ptr2, col2, ptr1, col1, gptr, gcol, bptr, bcol, eptr, elist;
  std::vector<double> M, K, L, Mp, G, BT, B, m1;
};
inline void ip_constant_operators(const IpRef &R, int nn, int nvert, int nc, const int *cells, const double *geo, IpOps &O) {
  const int D = R.D, NL = R.NL, NV = R.NV;
  std::vector<int> c1((size_t)NV * nc);
  for (int e = 0; e < nc; e++)
    for (int a = 0; a < NV; a++) c1[(size_t)NV * e + a] = cells[(size_t)NL * e + a];
  ip_pattern(nn, nc, cells, NL, cells, NL, O.ptr2, O.col2);
  ip_pattern(nvert, nc, c1.data(), NV, c1.data(), NV, O.ptr1, O.col1);
  ip_pattern(nn, nc, cells, NL, c1.data(), NV, O.gptr, O.gcol);
  ip_pattern(nvert, nc, c1.data(), NV, cells, NL, O.bptr, O.bcol);
  const int nnz2 = (int)O.col2.size(), nnz1 = (int)O.col1.size(), nnzG = (int)O.gcol.size(), nnzB = (int)O.bcol.size();
  O.M.assign(nnz2, 0.0); O.K.assign(nnz2, 0.0); O.L.assign(nnz1, 0.0); O.Mp.assign(nnz1, 0.0);
  O.G.assign((size_t)D * nnzG, 0.0); O.BT.assign((size_t)D * nnzG, 0.0); O.B.assign((size_t)D * nnzB, 0.0);
  O.m1.assign(nn, 0.0);
  O.eptr.assign(nnz2 + 1, 0);
  for (int e = 0; e < nc; e++) {
    const int *cv = cells + (size_t)NL * e;
    double gl[4][3], det;
    grad_lambda(D, geo, e, gl, det);
    double gg[4][4];
    for (int i = 0; i < NV; i++)
      for (int j = 0; j < NV; j++) { gg[i][j] = 0.0; for (int d = 0; d < D; d++) gg[i][j] += gl[i][d] * gl[j][d]; }
    for (int a = 0; a < NL; a++) {
      O.m1[cv[a]] += det * R.G[a];
      for (int b = 0; b < NL; b++) {
        const int k = ip_find(O.ptr2, O.col2, cv[a], cv[b]);
        O.eptr[k + 1]++;
        O.M[k] += det * R.M[a * NL + b];
        double kv = 0.0;
        for (int i = 0; i < NV; i++)
          for (int j = 0; j < NV; j++) kv += R.K[(((size_t)a * NL + b) * NV + i) * NV + j] * gg[i][j];
        O.K[k] += det * kv;
      }
      // G_d[a][v] = int phi_a d_d lam_v ; B_d^T[a][v] = int lam_v d_d phi_a
      for (int v = 0; v < NV; v++) {
        const int k = ip_find(O.gptr, O.gcol, cv[a], cv[v]);
        for (int d = 0; d < D; d++) {
          O.G[(size_t)D * k + d] += det * R.G[a] * gl[v][d];
          double bv = 0.0;
          for (int i = 0; i < NV; i++) bv += R.B[((size_t)v * NL + a) * NV + i] * gl[i][d];
          O.BT[(size_t)D * k + d] += det * bv;
          const int kb = ip_find(O.bptr, O.bcol, cv[v], cv[a]);
          O.B[(size_t)D * kb + d] += det * bv;
        }
      }
    }
    const double vol = det * (D == 2 ? 0.5 : 1.0 / 6.0);
    for (int v = 0; v < NV; v++)
      for (int x = 0; x < NV; x++) {
        const int k = ip_find(O.ptr1, O.col1, cv[v], cv[x]);
        O.L[k] += vol * gg[v][x];
        O.Mp[k] += det * R.MP[v * NV + x];
      }
  }
  for (int k = 0; k < nnz2; k++) O.eptr[k + 1] += O.eptr[k];
  O.elist.assign((size_t)O.eptr[nnz2], 0);
  std::vector<int> fill(O.eptr.begin(), O.eptr.end() - 1);
  for (int e = 0; e < nc; e++) {
    const int *cv = cells + (size_t)NL * e;
    for (int a = 0; a < NL; a++)
      for (int b = 0; b < NL; b++) O.elist[fill[ip_find(O.ptr2, O.col2, cv[a], cv[b])]++] = e * NL * NL + a * NL + b;
  }
}

// ---- constant parts of the vector-coupled form of ipcs_midpoint:
//   E(i a, j b) = int d_b phi_i d_a phi_j dx              from 2 mu eps(u) : eps(v) = mu (grad phi_i . grad phi_j delta_ab + d_b phi_i d_a phi_j)
//   S(i a, j b) = int_{dOmega} phi_i d_a phi_j n_b ds     the ds term -mu (nabla_grad(u) n) . v; on the P2 pattern (both nodes in the facet's cell)
//   Pn(i a, k)  = int_{dOmega} phi_i psi_k n_a ds         the ds term p n . v; a sub-pattern of B^T
// The facet integrands are polynomials of degree 3: three-point Gauss on an edge, the degree-13 triangle rule on a face.  With
// gl_f = grad lambda_f of the vertex opposite the facet, n |facet| = -gl_f |det| / (D - 1)!.
// ES = E - S as [nnz2][D][D] blocks, Pn and BTP = B^T - Pn as [nnzG][D]; the cells of every node in nlist[nptr[i] .. nptr[i+1])
// as cell * NL + local node, ascending.
struct IpMid {
  std::vector<double> ES, Pn, BTP;
  std::vector<int> nptr, nlist;
};
inline void ip_midpoint_constants(const IpRef &R, const IpOps &O, int nn, int nc, const int *cells, const double *geo, size_t nfac, const int *fcell,
                                  const int *flocal, IpMid &Q) {
  const int D = R.D, NL = R.NL, NV = R.NV;
  const size_t nnz2 = O.col2.size(), nnzG = O.gcol.size();
  std::vector<double> E(nnz2 * D * D, 0.0), Sb(nnz2 * D * D, 0.0);
  Q.Pn.assign(nnzG * D, 0.0);
  for (int e = 0; e < nc; e++) {
    const int *cv = cells + (size_t)NL * e;
    double gl[4][3], det;
    grad_lambda(D, geo, e, gl, det);
    for (int a = 0; a < NL; a++)
      for (int b = 0; b < NL; b++) {
        const size_t k = (size_t)ip_find(O.ptr2, O.col2, cv[a], cv[b]);
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
  for (size_t kf = 0; kf < nfac; kf++) {
    const int e = fcell[kf], f = flocal[kf];
    const int *cv = cells + (size_t)NL * e;
    double gl[4][3], det;
    grad_lambda(D, geo, e, gl, det);
    for (size_t q = 0; q < fw.size(); q++) {
      double lam[4];
      int m = 0;
      for (int i = 0; i < NV; i++) lam[i] = i == f ? 0.0 : fl[q * D + m++];
      ip_p2(D, lam, phi.data(), dl.data());
      const double w = fw[q] * det * fact;
      for (int a = 0; a < NL; a++) {
        if (phi[a] == 0.0) continue;  // nodes off the facet (their basis functions vanish on it identically)
        for (int b = 0; b < NL; b++) {
          const size_t k = (size_t)ip_find(O.ptr2, O.col2, cv[a], cv[b]);
          for (int al = 0; al < D; al++) {
            double g = 0.0;
            for (int i = 0; i < NV; i++) g += dl[b * NV + i] * gl[i][al];
            for (int be = 0; be < D; be++) Sb[(k * D + al) * D + be] -= w * phi[a] * g * gl[f][be];
          }
        }
        for (int v = 0; v < NV; v++) {
          const size_t k = (size_t)ip_find(O.gptr, O.gcol, cv[a], cv[v]);
          for (int al = 0; al < D; al++) Q.Pn[k * D + al] -= w * phi[a] * lam[v] * gl[f][al];
        }
      }
    }
  }
  Q.ES.resize(E.size());
  for (size_t k = 0; k < E.size(); k++) Q.ES[k] = E[k] - Sb[k];
  Q.BTP.resize(O.BT.size());
  for (size_t k = 0; k < Q.BTP.size(); k++) Q.BTP[k] = O.BT[k] - Q.Pn[k];
  Q.nptr.assign(nn + 1, 0);
  Q.nlist.assign((size_t)NL * nc, 0);
  for (size_t k = 0; k < Q.nlist.size(); k++) Q.nptr[cells[k] + 1]++;
  for (int i = 0; i < nn; i++) Q.nptr[i + 1] += Q.nptr[i];
  std::vector<int> fill(Q.nptr.begin(), Q.nptr.end() - 1);
  for (size_t k = 0; k < Q.nlist.size(); k++) Q.nlist[fill[cells[k]]++] = (int)k;  // k = cell * NL + local node
}

// ---- Dirichlet treatment of the pressure Laplacian from the flags and object counts: Lc on the pattern of L (constrained rows
// and columns zero, the count on the diagonal) and the same matrix without the explicit zeros of the eliminated rows / columns
// (aptr, acol, aval: what the AMG set-up is given).  singular: no vertex is constrained.
inline void ip_constrain_laplacian(const IpOps &O, const std::vector<unsigned char> &flag, const std::vector<double> &cnt, std::vector<double> &Lc,
                                   std::vector<int> &aptr, std::vector<int> &acol, std::vector<double> &aval, bool &singular) {
  const int nv = (int)O.ptr1.size() - 1;
  Lc = O.L;
  bool any = false;
  for (int i = 0; i < nv; i++) {
    any |= flag[i] != 0;
    for (int k = O.ptr1[i]; k < O.ptr1[i + 1]; k++) {
      const int j = O.col1[k];
      if (flag[i]) Lc[k] = j == i ? cnt[i] : 0.0;
      else if (flag[j]) Lc[k] = 0.0;
    }
  }
  singular = !any;
  aptr.assign(nv + 1, 0); acol.clear(); aval.clear();
  for (int i = 0; i < nv; i++) {
    for (int k = O.ptr1[i]; k < O.ptr1[i + 1]; k++) {
      const int j = O.col1[k];
      if ((flag[i] || flag[j]) && j != i) continue;
      acol.push_back(j); aval.push_back(Lc[k]);
    }
    aptr[i + 1] = (int)acol.size();
  }
}
// ipcs_bdf2: lift = L_free g over the constrained columns, rhsfix = count * value on the constrained rows
inline void ip_lifting(const IpOps &O, const std::vector<unsigned char> &flag, const std::vector<double> &cnt, const std::vector<double> &val,
                       std::vector<double> &lift, std::vector<double> &fix) {
  const int nv = (int)O.ptr1.size() - 1;
  lift.assign(nv, 0.0); fix.assign(nv, 0.0);
  for (int i = 0; i < nv; i++) {
    if (flag[i]) fix[i] = cnt[i] * val[i];
    for (int k = O.ptr1[i]; k < O.ptr1[i + 1]; k++) {
      const int j = O.col1[k];
      if (flag[j]) lift[i] += O.L[k] * val[j];
    }
  }
}
// rho M and its Jacobi weights
inline void ip_rho_mass(const IpOps &O, double rho, std::vector<double> &rm, std::vector<double> &dinv) {
  const int nn = (int)O.ptr2.size() - 1;
  rm.resize(O.M.size()); dinv.resize(nn);
  for (size_t k = 0; k < rm.size(); k++) rm[k] = rho * O.M[k];
  for (int i = 0; i < nn; i++) dinv[i] = 1.0 / rm[ip_find(O.ptr2, O.col2, i, i)];
}

}  // namespace cfdh_ipcs_host
