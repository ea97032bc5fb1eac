// Wall shear stress of the P2/P1 (incremental pressure-correction) context and the cycle-averaged wall shear indices of every
// context kind (include/cfdh.h: cfdh_wall_shear_stress, cfdh_wall_stats_*).
//
// Wall shear stress on P2 velocities (solverBase.py:144-195; the test space is CG1 whatever the velocity degree): with the outward
// unit normal n, T = -mu (grad u + grad u^T) n, Tt = T - (T.n) n and the P1 hat function l_v,
//   shear[v] = sum over the exterior facets f of v of (1/|f|) int_f l_v Tt ds.
// grad u is linear on the facet, so the integrand is quadratic and (1/|f|) int_f l_v Tt = sum_b m_vb Tt(x_b) over the facet's
// vertices b, m_vb = (1 + d_vb) / 6 on an edge and (1 + d_vb) / 12 on a triangle.  At the vertex b of the cell
//   grad u (x_b) = sum_k grad l_k (x) c_k,   c_b = 3 u_b,   c_k = 4 u_edge(b,k) - u_k  (k != b),
// and Tt is linear in grad u, so the weighted sum of the gradients is formed first.  Gather, no atomics: one lane per wall vertex
// walks its exterior facets in ascending facet index and writes its own values -- two calls on one state return the same bytes.
// Every local index below is a compile-time constant after unrolling (the facet's local index enters through selects), so the
// cell's 30 velocities and 12 gradient entries stay in registers.
//
// Indices: per vertex of the wall-shear field S = sum w tau, A = sum w |tau|, M = max |tau|, updated by one pointwise kernel
// (reads dim, reads and writes dim + 2 doubles per vertex); the derived fields are formed on the device before the download.
#include <hip/hip_runtime.h>

#include <cmath>

#include "cfdh_internal.hpp"
#include "cfdh_ipcs.hpp"

#define TPB 256
#define WS_MAX_BLOCKS 2048  // grid-stride above this many blocks

// local node of the edge between the vertices a != b of a P2 cell: triangle 3 + (the vertex opposite), tetrahedron in the Basix
// edge order (2,3) (1,3) (1,2) (0,3) (0,2) (0,1)
template <int D>
__device__ __forceinline__ constexpr int ws_edge_node(int a, int b) {
  const int lo = a < b ? a : b, hi = a < b ? b : a;
  if (D == 2) return 3 + (3 - lo - hi);
  return lo == 0 ? (hi == 3 ? 7 : (hi == 2 ? 8 : 9)) : (lo == 1 ? (hi == 3 ? 5 : 6) : 4);
}

template <int D>
__global__ __launch_bounds__(TPB) void ws_ipcs_wss_kernel(int nw, const int *__restrict__ wv, const int *__restrict__ wptr, const int *__restrict__ wfac,
                                                         const int *__restrict__ fcell, const int *__restrict__ flocal, const int *__restrict__ cells,
                                                         const double *__restrict__ geo, const double *__restrict__ u, double mu,
                                                         double *__restrict__ out) {
  constexpr int NV = D + 1, NL = D == 2 ? 6 : 10;
  const int w = blockIdx.x * TPB + threadIdx.x;
  if (w >= nw) return;
  const int v = wv[w];
  double acc[D];
#pragma unroll
  for (int d = 0; d < D; d++) acc[d] = 0.0;
  for (int q = wptr[w]; q < wptr[w + 1]; q++) {
    const int f = wfac[q], e = fcell[f], fl = flocal[f];
    const int *cv = cells + (size_t)NL * e;
    const double *g = geo + (size_t)(D * D + 1) * e;  // rows grad l_1 .. grad l_D
    double gl[NV][D], U[NL][D];
#pragma unroll
    for (int d = 0; d < D; d++) {
      gl[0][d] = 0.0;
#pragma unroll
      for (int k = 0; k < D; k++) { gl[k + 1][d] = g[D * k + d]; gl[0][d] -= g[D * k + d]; }
    }
    int vid[NV];
#pragma unroll
    for (int a = 0; a < NL; a++) {
      const int node = cv[a];
      if (a < NV) vid[a] = node;
#pragma unroll
      for (int d = 0; d < D; d++) U[a][d] = u[(size_t)D * node + d];
    }
    // outward normal n = -grad l_fl / |grad l_fl|
    double n[D], n2 = 0.0;
#pragma unroll
    for (int d = 0; d < D; d++) {
      double s = gl[0][d];
#pragma unroll
      for (int k = 1; k < NV; k++) s = fl == k ? gl[k][d] : s;
      n[d] = -s;
      n2 += s * s;
    }
    const double rn = 1.0 / sqrt(n2);
#pragma unroll
    for (int d = 0; d < D; d++) n[d] *= rn;
    // G[i][j] = sum_b m_vb d_i u_j (x_b) over the facet's vertices, weights in units of 1/6 (1/12)
    double G[D][D];
#pragma unroll
    for (int i = 0; i < D; i++)
#pragma unroll
      for (int j = 0; j < D; j++) G[i][j] = 0.0;
#pragma unroll
    for (int b = 0; b < NV; b++) {
      const double m = b == fl ? 0.0 : (vid[b] == v ? 2.0 : 1.0);
#pragma unroll
      for (int k = 0; k < NV; k++) {
        const int en = k == b ? b : ws_edge_node<D>(b, k);
#pragma unroll
        for (int j = 0; j < D; j++) {
          const double cj = k == b ? 3.0 * U[b][j] : 4.0 * U[en][j] - U[k][j];
#pragma unroll
          for (int i = 0; i < D; i++) G[i][j] += m * gl[k][i] * cj;
        }
      }
    }
    double T[D], Tn = 0.0;
    const double sc = -mu * (D == 2 ? 1.0 / 6.0 : 1.0 / 12.0);
#pragma unroll
    for (int i = 0; i < D; i++) {
      double s = 0.0;
#pragma unroll
      for (int j = 0; j < D; j++) s += (G[i][j] + G[j][i]) * n[j];
      T[i] = sc * s;
      Tn += T[i] * n[i];
    }
#pragma unroll
    for (int d = 0; d < D; d++) acc[d] += T[d] - Tn * n[d];
  }
#pragma unroll
  for (int d = 0; d < D; d++) out[(size_t)D * v + d] = acc[d];
}

// S += w tau, A += w |tau|, M = max(M, |tau|): pointwise, so the same kernel serves a part of a partitioned run
template <int D>
__global__ __launch_bounds__(TPB) void ws_accumulate_kernel(int n, double w, const double *__restrict__ tau, double *__restrict__ S, double *__restrict__ A,
                                                           double *__restrict__ M) {
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
    double t[D], s2 = 0.0;
#pragma unroll
    for (int d = 0; d < D; d++) { t[d] = tau[(size_t)D * i + d]; s2 += t[d] * t[d]; }
    const double m = sqrt(s2);
#pragma unroll
    for (int d = 0; d < D; d++) S[(size_t)D * i + d] += w * t[d];
    A[i] += w * m;
    M[i] = fmax(M[i], m);
  }
}

// which 0: TAWSS = A / W ; 1: OSI = (1 - |S| / A) / 2 in [0, 1/2], 0 where A == 0 ; 2: RRT = W / |S|, inf where |S| == 0 < A, 0 where
// A == 0 ; 3: S / W ; 4: M
template <int D>
__global__ __launch_bounds__(TPB) void ws_derive_kernel(int n, int which, double W, const double *__restrict__ S, const double *__restrict__ A,
                                                       const double *__restrict__ M, double *__restrict__ out) {
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
    if (which == 3) {
#pragma unroll
      for (int d = 0; d < D; d++) out[(size_t)D * i + d] = S[(size_t)D * i + d] / W;
      continue;
    }
    if (which == 0) { out[i] = A[i] / W; continue; }
    if (which == 4) { out[i] = M[i]; continue; }
    double s2 = 0.0;
#pragma unroll
    for (int d = 0; d < D; d++) s2 += S[(size_t)D * i + d] * S[(size_t)D * i + d];
    const double sn = sqrt(s2), a = A[i];
    double r;
    if (a == 0.0) r = 0.0;
    else if (which == 1) r = fmin(fmax(0.5 * (1.0 - sn / a), 0.0), 0.5);
    else r = sn == 0.0 ? HUGE_VAL : W / sn;
    out[i] = r;
  }
}

static inline int ws_grid(int n) {
  const int g = (n + TPB - 1) / TPB;
  return g < 1 ? 1 : (g > WS_MAX_BLOCKS ? WS_MAX_BLOCKS : g);
}

int k_ipcs_wss(cfdh_ctx *c, double *out) {
  IpcsData *I = c->ipcs;
  const int nw = I->n_wallv;
  if (nw == 0) return 0;
  const dim3 grid((nw + TPB - 1) / TPB), block(TPB);
  if (I->D == 2)
    hipLaunchKernelGGL(ws_ipcs_wss_kernel<2>, grid, block, 0, c->stream, nw, (const int *)I->wv_list.p, (const int *)I->wv_ptr.p, (const int *)I->wv_fac.p,
                       (const int *)I->d_fcell.p, (const int *)I->d_flocal.p, (const int *)I->d_cells.p, (const double *)I->d_geo.p,
                       (const double *)I->u_sol.p, c->mu, out);
  else
    hipLaunchKernelGGL(ws_ipcs_wss_kernel<3>, grid, block, 0, c->stream, nw, (const int *)I->wv_list.p, (const int *)I->wv_ptr.p, (const int *)I->wv_fac.p,
                       (const int *)I->d_fcell.p, (const int *)I->d_flocal.p, (const int *)I->d_cells.p, (const double *)I->d_geo.p,
                       (const double *)I->u_sol.p, c->mu, out);
  HIPCHK(c, hipGetLastError());
  return 0;
}

int k_ws_accumulate(cfdh_ctx *c, int n, double w, const double *tau) {
  if (n == 0) return 0;
  if (c->dim == 2)
    hipLaunchKernelGGL(ws_accumulate_kernel<2>, dim3(ws_grid(n)), dim3(TPB), 0, c->stream, n, w, tau, c->ws_S.p, c->ws_A.p, c->ws_M.p);
  else
    hipLaunchKernelGGL(ws_accumulate_kernel<3>, dim3(ws_grid(n)), dim3(TPB), 0, c->stream, n, w, tau, c->ws_S.p, c->ws_A.p, c->ws_M.p);
  HIPCHK(c, hipGetLastError());
  return 0;
}

int k_ws_derive(cfdh_ctx *c, int n, int which, double *out) {
  if (n == 0) return 0;
  if (c->dim == 2)
    hipLaunchKernelGGL(ws_derive_kernel<2>, dim3(ws_grid(n)), dim3(TPB), 0, c->stream, n, which, c->ws_W, (const double *)c->ws_S.p,
                       (const double *)c->ws_A.p, (const double *)c->ws_M.p, out);
  else
    hipLaunchKernelGGL(ws_derive_kernel<3>, dim3(ws_grid(n)), dim3(TPB), 0, c->stream, n, which, c->ws_W, (const double *)c->ws_S.p,
                       (const double *)c->ws_A.p, (const double *)c->ws_M.p, out);
  HIPCHK(c, hipGetLastError());
  return 0;
}
