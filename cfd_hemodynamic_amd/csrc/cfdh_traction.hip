// Traction boundaries of the convective form on the closed-form P1 kernels (cfdh_set_traction_boundaries, include/cfdh.h):
// the facet terms of stabilized_schur_pressure_backflow.py:191-217, added into F and the blocked A00 values right after the volume
// pass of k_assemble / k3_assemble, on the same stream.  The volume kernels stay as they are (their register budgets are tuned);
// the work here is O(boundary).
//
// One lane owns one destination row (cfdh_traction_host.hpp): it walks the row's (cell, local facet) pairs in their fixed order,
// keeps the residual of the row in registers and adds every column block into its value slot.  Nobody else writes to the row after
// the volume pass, so there are no atomics and two assemblies give the same bits.  A wavefront owns a slice of 64 consecutive rows
// of the list and reads it column-major (consecutive lanes, consecutive words).
//
// Per pair (row vertex a of cell K, facet f opposite vertex f, boundary k), with ubar = theta u + (1 - theta) u_prev, the cell
// constants g_b = grad(lambda_b), n = -g_f / |g_f|, |F| = d |K| |g_f|, W = |F| / d, P = I - n n^T, S = 2 mu eps(ubar) n
// = mu sum_b (g_b (ubar_b . n) + (g_b . n) ubar_b), and oint l_a = W, oint l_a l_b = W (1 + d_ab) / (d + 1):
//   a != f:           + P_k n W
//     tangential:     - (P S) W + (beta mu / h) sum_{b != f} W (1 + d_ab) / (d + 1) P ubar_b
//     otherwise:      - S W
//     backflow:       - beta_k rho sum_q w_q |F| (u_prev . n)_-(x_q) l_a(x_q) ubar(x_q)      (2-point Gauss / 6-point Strang-Fix)
//   tangential, any a: - mu (n (g_a . U) + (g_a . n) U),  U = W sum_{b != f} P ubar_b           (the symmetry term: eps of the test function)
// The Jacobian is theta times the derivative with respect to ubar_b: blocks (a, b) of A00 only.
// Dirichlet treatment as in the volume kernels: constrained rows are left alone, constrained columns are not stored, and their
// unmasked entries lift the residual, F += J[:, k] (g_k - x_k) (modes 1 and 2).
#include "cfdh_internal.hpp"
#include "cfdh_traction_host.hpp"

namespace {

struct TracArgs {
  const double *coords, *x, *un, *bcval, *coef;  // coef: values [CFDH_MAX_PBND], then beta_backflow [CFDH_MAX_PBND]
  const int *cells, *row, *sptr, *pcell, *pmeta, *pslot;
  const unsigned char *bcflag;
  double *A00, *F;
  int nrows;
  unsigned tangential;
  double rho, mu, theta, beta_nitsche;
};

template <int D>
__device__ __forceinline__ void p1_gradients(const double X[D + 1][D], double g[D + 1][D], double &vol, double &h) {
  double r[D][D];  // r[a - 1] = x_a - x_0
#pragma unroll
  for (int a = 1; a <= D; a++)
#pragma unroll
    for (int i = 0; i < D; i++) r[a - 1][i] = X[a][i] - X[0][i];
  if constexpr (D == 2) {
    const double det = r[0][0] * r[1][1] - r[0][1] * r[1][0], id = 1.0 / det;
    g[1][0] = r[1][1] * id; g[1][1] = -r[1][0] * id;
    g[2][0] = -r[0][1] * id; g[2][1] = r[0][0] * id;
    vol = 0.5 * fabs(det);
  } else {
    double c0[3], c1[3], c2[3];  // r1 x r2, r2 x r0, r0 x r1
    c0[0] = r[1][1] * r[2][2] - r[1][2] * r[2][1]; c0[1] = r[1][2] * r[2][0] - r[1][0] * r[2][2]; c0[2] = r[1][0] * r[2][1] - r[1][1] * r[2][0];
    c1[0] = r[2][1] * r[0][2] - r[2][2] * r[0][1]; c1[1] = r[2][2] * r[0][0] - r[2][0] * r[0][2]; c1[2] = r[2][0] * r[0][1] - r[2][1] * r[0][0];
    c2[0] = r[0][1] * r[1][2] - r[0][2] * r[1][1]; c2[1] = r[0][2] * r[1][0] - r[0][0] * r[1][2]; c2[2] = r[0][0] * r[1][1] - r[0][1] * r[1][0];
    const double det = r[0][0] * c0[0] + r[0][1] * c0[1] + r[0][2] * c0[2], id = 1.0 / det;
#pragma unroll
    for (int i = 0; i < 3; i++) { g[1][i] = c0[i] * id; g[2][i] = c1[i] * id; g[3][i] = c2[i] * id; }
    vol = fabs(det) * (1.0 / 6.0);
  }
#pragma unroll
  for (int i = 0; i < D; i++) {
    double s = 0.0;
#pragma unroll
    for (int a = 1; a <= D; a++) s += g[a][i];
    g[0][i] = -s;
  }
  double h2 = 0.0;
#pragma unroll
  for (int a = 0; a <= D; a++)
#pragma unroll
    for (int b = a + 1; b <= D; b++) {
      double s = 0.0;
#pragma unroll
      for (int i = 0; i < D; i++) s += (X[a][i] - X[b][i]) * (X[a][i] - X[b][i]);
      h2 = fmax(h2, s);
    }
  h = sqrt(h2);
}

// MODE as in asm_kernel: 0 residual only, 1 residual + Jacobian, 2 residual with lifting (no Jacobian write)
template <int D, int MODE>
__global__ __launch_bounds__(cfdh_traction::SLICE) void traction_kernel(TracArgs p) {
  constexpr int N1 = D + 1, SL = cfdh_traction::SLICE;
  constexpr bool JAC = MODE != 0, WJ = MODE == 1;
  const int lane = threadIdx.x, s = blockIdx.x;
  const int r = s * SL + lane;
  if (r >= p.nrows) return;
  const int row = p.row[r];
  const int c0 = p.sptr[s], c1 = p.sptr[s + 1];
  const unsigned flr = p.bcflag[row];
  const double th = p.theta, mu = p.mu;
  double Fr[D];
#pragma unroll
  for (int i = 0; i < D; i++) Fr[i] = 0.0;
  for (int c = c0; c < c1; c++) {
    const int e = p.pcell[(size_t)c * SL + lane];
    if (e < 0) continue;
    const int meta = p.pmeta[(size_t)c * SL + lane];
    const int a = meta & 3, f = (meta >> 2) & 3, k = meta >> 4;
    const bool tang = (p.tangential >> k) & 1u;
    const double val = p.coef[k], bfb = p.coef[CFDH_MAX_PBND + k];
    int v[N1];
    double X[N1][D], ub[N1][D], un[N1][D];
#pragma unroll
    for (int b = 0; b < N1; b++) {
      v[b] = p.cells[(size_t)N1 * e + b];
#pragma unroll
      for (int i = 0; i < D; i++) {
        X[b][i] = p.coords[(size_t)D * v[b] + i];
        un[b][i] = p.un[(size_t)D * v[b] + i];
        ub[b][i] = th * p.x[(size_t)D * v[b] + i] + (1.0 - th) * un[b][i];
      }
    }
    double g[N1][D], vol, h;
    p1_gradients<D>(X, g, vol, h);
    double gf[D], ga[D];  // gradients of the facet's and the row's vertex (dynamic local index: select, no register indexing)
#pragma unroll
    for (int i = 0; i < D; i++) {
      gf[i] = 0.0; ga[i] = 0.0;
#pragma unroll
      for (int b = 0; b < N1; b++) { gf[i] = b == f ? g[b][i] : gf[i]; ga[i] = b == a ? g[b][i] : ga[i]; }
    }
    double gl = 0.0;
#pragma unroll
    for (int i = 0; i < D; i++) gl += gf[i] * gf[i];
    gl = sqrt(gl);
    double n[D], P[D][D];
#pragma unroll
    for (int i = 0; i < D; i++) n[i] = -gf[i] / gl;
#pragma unroll
    for (int i = 0; i < D; i++)
#pragma unroll
      for (int j = 0; j < D; j++) P[i][j] = (i == j ? 1.0 : 0.0) - n[i] * n[j];
    const double W = vol * gl;                                   // |F| / d
    const double pen = p.beta_nitsche * mu / h * W / (D + 1.0);  // (beta mu / h) |F| / (d (d + 1))
    double gn[N1], gan = 0.0, Pga[D];
#pragma unroll
    for (int b = 0; b < N1; b++) {
      gn[b] = 0.0;
#pragma unroll
      for (int i = 0; i < D; i++) gn[b] += g[b][i] * n[i];
    }
#pragma unroll
    for (int i = 0; i < D; i++) gan += ga[i] * n[i];
#pragma unroll
    for (int i = 0; i < D; i++) {
      Pga[i] = 0.0;
#pragma unroll
      for (int j = 0; j < D; j++) Pga[i] += P[i][j] * ga[j];
    }
    // backflow weights wbf[b] = sum_q c_q l_a(x_q) l_b(x_q), c_q = beta_k rho (u_prev . n)_-(x_q) w_q |F|; zero off the facet
    double wbf[N1];
#pragma unroll
    for (int b = 0; b < N1; b++) wbf[b] = 0.0;
    if (a != f && bfb > 0.0) {
      double sn[N1];
#pragma unroll
      for (int b = 0; b < N1; b++) {
        sn[b] = 0.0;
#pragma unroll
        for (int i = 0; i < D; i++) sn[b] += un[b][i] * n[i];
      }
      constexpr int NQ = D == 2 ? 2 : 6;
      constexpr double G2 = 0.28867513459481288;  // 1 / (2 sqrt 3)
      constexpr double SA = 0.659027622374092, SB = 0.231933368553031, SC = 0.109039009072877;
      const double Q2[2][2] = {{0.5 + G2, 0.5 - G2}, {0.5 - G2, 0.5 + G2}};
      const double Q3[6][3] = {{SA, SB, SC}, {SA, SC, SB}, {SB, SA, SC}, {SB, SC, SA}, {SC, SA, SB}, {SC, SB, SA}};
#pragma unroll
      for (int q = 0; q < NQ; q++) {
        // barycentrics of the point with respect to the cell: the rule's coordinates on the facet's vertices in increasing local index
        double lam[N1];
#pragma unroll
        for (int b = 0; b < N1; b++) {
          const int m = b - (b > f ? 1 : 0);  // position of b among the facet's vertices
          double l = 0.0;
          if constexpr (D == 2) l = m == 0 ? Q2[q][0] : Q2[q][1];
          else l = m == 0 ? Q3[q][0] : (m == 1 ? Q3[q][1] : Q3[q][2]);
          lam[b] = b == f ? 0.0 : l;
        }
        double sq = 0.0, la = 0.0;
#pragma unroll
        for (int b = 0; b < N1; b++) { sq += lam[b] * sn[b]; la = b == a ? lam[b] : la; }
        const double cq = bfb * p.rho * 0.5 * (sq - fabs(sq)) * (1.0 / NQ) * (D * W);
#pragma unroll
        for (int b = 0; b < N1; b++) wbf[b] += cq * la * lam[b];
      }
    }
    // ---- residual of row (a, :)
    double Fp[D];
#pragma unroll
    for (int i = 0; i < D; i++) Fp[i] = 0.0;
    double UT[D];  // W sum_{b != f} P ubar_b
#pragma unroll
    for (int i = 0; i < D; i++) {
      double sfac = 0.0;
#pragma unroll
      for (int b = 0; b < N1; b++) {
        double t = 0.0;
#pragma unroll
        for (int j = 0; j < D; j++) t += P[i][j] * ub[b][j];
        sfac += b == f ? 0.0 : t;
      }
      UT[i] = W * sfac;
    }
    if (a != f) {
      double S[D];
#pragma unroll
      for (int i = 0; i < D; i++) {
        S[i] = 0.0;
#pragma unroll
        for (int b = 0; b < N1; b++) {
          double ubn = 0.0;
#pragma unroll
          for (int j = 0; j < D; j++) ubn += ub[b][j] * n[j];
          S[i] += mu * (g[b][i] * ubn + gn[b] * ub[b][i]);
        }
      }
#pragma unroll
      for (int i = 0; i < D; i++) {
        double v_ = val * n[i] * W;
        if (tang) {
          double ps = 0.0, up = 0.0;
#pragma unroll
          for (int j = 0; j < D; j++) ps += P[i][j] * S[j];
#pragma unroll
          for (int b = 0; b < N1; b++) {
            double t = 0.0;
#pragma unroll
            for (int j = 0; j < D; j++) t += P[i][j] * ub[b][j];
            up += b == f ? 0.0 : (b == a ? 2.0 : 1.0) * t;
          }
          v_ += -ps * W + pen * up;
        } else {
          v_ -= S[i] * W;
        }
#pragma unroll
        for (int b = 0; b < N1; b++) v_ -= wbf[b] * ub[b][i];
        Fp[i] += v_;
      }
    }
    if (tang) {
      double gu = 0.0;
#pragma unroll
      for (int j = 0; j < D; j++) gu += ga[j] * UT[j];
#pragma unroll
      for (int i = 0; i < D; i++) Fp[i] -= mu * (n[i] * gu + gan * UT[i]);
    }
    // ---- column blocks (a, b), lifting, stores
    if (JAC) {
#pragma unroll
      for (int b = 0; b < N1; b++) {
        const unsigned flb = p.bcflag[v[b]];
        if (!WJ && !flb) continue;  // mode 2 needs the Dirichlet columns only
        double Pgb[D];
#pragma unroll
        for (int i = 0; i < D; i++) {
          Pgb[i] = 0.0;
#pragma unroll
          for (int j = 0; j < D; j++) Pgb[i] += P[i][j] * g[b][j];
        }
        const int slot = p.pslot[((size_t)c * N1 + b) * SL + lane];
#pragma unroll
        for (int i = 0; i < D; i++)
#pragma unroll
          for (int j = 0; j < D; j++) {
            const double dij = i == j ? 1.0 : 0.0;
            double J = 0.0;
            if (a != f) {
              if (tang) {
                J -= W * mu * (Pgb[i] * n[j] + gn[b] * P[i][j]);
                if (b != f) J += pen * (b == a ? 2.0 : 1.0) * P[i][j];
              } else {
                J -= W * mu * (g[b][i] * n[j] + gn[b] * dij);
              }
              J -= wbf[b] * dij;
            }
            if (tang && b != f) J -= mu * W * (n[i] * Pga[j] + gan * P[i][j]);
            J *= th;
            if ((flb >> j) & 1u) {
              Fp[i] += J * (p.bcval[(size_t)N1 * v[b] + j] - p.x[(size_t)D * v[b] + j]);
              continue;
            }
            if (WJ && !((flr >> i) & 1u)) p.A00[(size_t)D * D * slot + D * i + j] += J;
          }
      }
    }
#pragma unroll
    for (int i = 0; i < D; i++) Fr[i] += Fp[i];
  }
#pragma unroll
  for (int i = 0; i < D; i++)
    if (!((flr >> i) & 1u)) p.F[(size_t)D * row + i] += Fr[i];
}

template <int D>
void launch(cfdh_ctx *c, const TracArgs &a, int mode) {
  const dim3 gr(c->tb_nslices), bl(cfdh_traction::SLICE);
  if (mode == 1) hipLaunchKernelGGL((traction_kernel<D, 1>), gr, bl, 0, c->stream, a);
  else if (mode == 2) hipLaunchKernelGGL((traction_kernel<D, 2>), gr, bl, 0, c->stream, a);
  else hipLaunchKernelGGL((traction_kernel<D, 0>), gr, bl, 0, c->stream, a);
}

}  // namespace

// (re)build and upload the work list for the current markers and switches
int cfdh_traction_setup(cfdh_ctx *c) {
  c->tb_ready = false;
  c->tb_nrows = c->tb_nslices = 0;
  if (c->tb_markers.empty()) return 0;
  cfdh_traction::WorkList w;
  std::string why;
  if (!cfdh_traction::build_worklist(c->dim, c->nv, c->nc, c->h_cells.data(), c->nfac, c->fac_cell.data(), c->fac_local.data(), c->fac_marker.data(),
                                     (int)c->tb_markers.size(), c->tb_markers.data(), c->tb_tangential, c->h_vptr.data(), c->h_vcol.data(), w, why))
    return cfdh_fail(c, CFDH_E_ARG, "%s", why.c_str());
  c->tb_nrows = w.nrows; c->tb_nslices = w.nslices;
  if (w.nrows) {
    HIPCHK(c, c->tb_row.upload(w.row, c->stream));
    HIPCHK(c, c->tb_sptr.upload(w.sptr, c->stream));
    HIPCHK(c, c->tb_cell.upload(w.dcell, c->stream));
    HIPCHK(c, c->tb_meta.upload(w.dmeta, c->stream));
    HIPCHK(c, c->tb_slot.upload(w.dslot, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // the host vectors go out of scope
  }
  c->tb_ready = true;
  return 0;
}

// values and backflow coefficients of the boundaries: 2 CFDH_MAX_PBND doubles
int cfdh_traction_upload_coef(cfdh_ctx *c) {
  std::vector<double> h(2 * CFDH_MAX_PBND, 0.0);
  for (size_t k = 0; k < c->tb_markers.size(); k++) { h[k] = c->tb_values[k]; h[CFDH_MAX_PBND + k] = c->tb_backflow[k]; }
  HIPCHK(c, c->tb_coef.upload(h, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

// after the volume pass of k_assemble / k3_assemble, same stream; a context without traction boundaries never gets here
int k_traction(cfdh_ctx *c, const double *xstate, int mode) {
  if (!c->tb_ready) CHK(cfdh_traction_setup(c));
  if (!c->tb_nrows) return 0;
  TracArgs a;
  a.coords = c->coords.p; a.x = xstate; a.un = c->xprev.p; a.bcval = c->bcval.p; a.coef = c->tb_coef.p;
  a.cells = c->cells.p; a.row = c->tb_row.p; a.sptr = c->tb_sptr.p; a.pcell = c->tb_cell.p; a.pmeta = c->tb_meta.p; a.pslot = c->tb_slot.p;
  a.bcflag = c->bcflag.p; a.A00 = c->A00.p; a.F = c->F.p;
  a.nrows = c->tb_nrows; a.tangential = c->tb_tangential;
  a.rho = c->rho; a.mu = c->mu; a.theta = c->ts_theta; a.beta_nitsche = c->tb_beta;
  if (c->dim == 3) launch<3>(c, a, mode);
  else launch<2>(c, a, mode);
  c->n_traction_launches++;
  HIPCHK(c, hipGetLastError());
  return 0;
}
