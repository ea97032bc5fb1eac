// Passive scalar transport on the closed-form P1 contexts (cfdh_scalar_*, include/cfdh.h): dc/dt + w . grad c - D lap c = s with
// P1, SUPG and a theta-scheme, advected by the velocity the flow step has just computed (u_sol, u_prev: the ends of the step).
// Three parts: the assembly kernel (left-hand values on the vertex graph and the right-hand side in one pass), the BiCGStab +
// Jacobi driver with its kernels (the launch and read-back pattern of ip_bicgstab in cfdh_ipcs_krylov.hip, on kernels of its own
// so that the object code of the pressure-correction drivers stays what their iterate-by-iterate tests pin), the functionals.
//
// Assembly: one lane owns one row of the vertex graph (cfdh_scalar_host.hpp): it zeroes the row's values, walks the row's (cell,
// local index) incidences in ascending cell order, adds every cell's d + 1 entries into their positions of the row and keeps the
// right-hand side of the row in a register.  Nobody else writes to the row: no atomics, a fixed summation order, and two assemblies
// give the same bytes.  A wavefront owns a slice of 64 consecutive rows and reads the list column-major (consecutive lanes,
// consecutive words).  Everything is indexed at compile time (the row's local index enters through selects): no scratch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>

#include "cfdh_internal.hpp"
#include "cfdh_scalar_host.hpp"
#include "cfdh_wave.hpp"

#define SC_NB 1024  // most blocks (= partial sums per dot product) of the reducing kernels

// scalars of the Krylov loop (device array; [SC_RN2, SC_BAD] are mirrored into host-mapped memory): the words SC_RHO .. SC_BAD are
// part of cfdh_scalar_krylov_solve's contract (include/cfdh.h)
enum { SC_NS = CFDH_SCALAR_NSCAL };
struct ScTol { double rtol, atol; int max_it; };

struct ScalarData {
  int n = 0;                         // vertices = rows
  double D = 0, src = 0, theta = 0.5;
  double rtol = 1e-8, atol = 1e-50;
  int max_it = 1000;
  int nslices = 0;
  dbuf<int> sptr, inc;
  dbuf<unsigned> slot;
  dbuf<double> c, cn, A, rhs, dinv, bcval;  // state, iterate of the solve in progress, left-hand values [nnzv], right-hand side, 1 / diag
  dbuf<unsigned char> bcflag;
  dbuf<double> kr, krh, kp, kv, ks, kt, ky, kz;  // BiCGStab work vectors
  dbuf<double> S, P;                 // Krylov scalars, partial sums [2 SC_NB]
  double *h_mirror = nullptr, *h_mirror_dev = nullptr;  // pinned, host-mapped: |r|^2, done, its, bad
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // cfdh_scalar_krylov_solve: right-hand side and iterate of its own, and the scalar block as the last iteration left it
  dbuf<double> hk_b, hk_x;
  double snap[CFDH_SCALAR_NSCAL] = {};
  bool snap_on = false, snap_set = false;
  ~ScalarData() {
    if (h_mirror) (void)hipHostFree(h_mirror);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
  }
};

namespace {

struct ScAsmArgs {
  const int *sptr, *inc, *cells, *vptr, *vcol;
  const unsigned *slot;
  const double *coords, *x, *xprev, *c0, *bcval;
  const unsigned char *bcflag;
  double *A, *rhs, *dinv;
  int n;
  double dt, D, src, theta;
};

template <int D>
__global__ __launch_bounds__(cfdh_scalar::SLICE) void sc_assemble_kernel(ScAsmArgs p) {
  constexpr int N1 = D + 1, SL = cfdh_scalar::SLICE;
  const int lane = threadIdx.x, s = blockIdx.x;
  const int row = s * SL + lane;
  if (row >= p.n) return;
  const int q0 = p.sptr[s], q1 = p.sptr[s + 1];
  const int base = p.vptr[row], len = p.vptr[row + 1] - base;
  const bool dir = p.bcflag[row] != 0;
  int kd = 0;
  for (int k = 0; k < len; k++) {
    const bool diag = p.vcol[base + k] == row;
    kd = diag ? k : kd;
    p.A[base + k] = (dir && diag) ? 1.0 : 0.0;
  }
  if (dir) {  // identity row, the value on the right-hand side
    p.rhs[row] = p.bcval[row];
    p.dinv[row] = 1.0;
    return;
  }
  const double th = p.theta, idt = 1.0 / p.dt;
  double rhs = 0.0;
  for (int q = q0; q < q1; q++) {
    const int w = p.inc[(size_t)q * SL + lane];
    if (w < 0) continue;
    const unsigned sl = p.slot[(size_t)q * SL + lane];
    const int e = w >> 2, a = w & 3;
    double g[N1][D], wv[N1][D], cv[N1], vol, h;
    {
      double X[N1][D];
#pragma unroll
      for (int b = 0; b < N1; b++) {
        const int v = p.cells[(size_t)N1 * e + b];
        cv[b] = p.c0[v];
#pragma unroll
        for (int i = 0; i < D; i++) {
          X[b][i] = p.coords[(size_t)D * v + i];
          wv[b][i] = th * p.x[(size_t)D * v + i] + (1.0 - th) * p.xprev[(size_t)D * v + i];
        }
      }
      double r[D][D];  // r[b - 1] = x_b - x_0
#pragma unroll
      for (int b = 1; b <= D; b++)
#pragma unroll
        for (int i = 0; i < D; i++) r[b - 1][i] = X[b][i] - X[0][i];
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
        double t = 0.0;
#pragma unroll
        for (int b = 1; b <= D; b++) t += g[b][i];
        g[0][i] = -t;
      }
      double h2 = 0.0;
#pragma unroll
      for (int b = 0; b <= D; b++)
#pragma unroll
        for (int b2 = b + 1; b2 <= D; b2++) {
          double t = 0.0;
#pragma unroll
          for (int i = 0; i < D; i++) t += (X[b][i] - X[b2][i]) * (X[b][i] - X[b2][i]);
          h2 = fmax(h2, t);
        }
      h = sqrt(h2);
    }
    // mean velocity, tau_c, the row vertex's gradient and weighted velocity (selects: the local index is a run-time value)
    double wb[D], ws[D], ga[D], wn2 = 0.0;
#pragma unroll
    for (int i = 0; i < D; i++) {
      double t = 0.0, wa = 0.0, gi = 0.0;
#pragma unroll
      for (int b = 0; b < N1; b++) { t += wv[b][i]; wa = b == a ? wv[b][i] : wa; gi = b == a ? g[b][i] : gi; }
      ws[i] = t + wa;              // sum_c w_c + w_a
      wb[i] = t * (1.0 / N1);
      ga[i] = gi;
      wn2 += wb[i] * wb[i];
    }
    const double t0 = 2.0 * idt, t1 = 2.0 * sqrt(wn2) / h, t2 = 4.0 * p.D / (h * h);
    const double tau = 1.0 / sqrt(t0 * t0 + t1 * t1 + t2 * t2);
    double pa = 0.0;
#pragma unroll
    for (int i = 0; i < D; i++) pa += wb[i] * ga[i];
    pa *= tau;
    const double cm = vol * (1.0 / ((D + 1) * (D + 2)));
    const double ms = pa * vol * (1.0 / N1);
#pragma unroll
    for (int b = 0; b < N1; b++) {
      double cab = 0.0, kab = 0.0, wg = 0.0;
#pragma unroll
      for (int i = 0; i < D; i++) { cab += ws[i] * g[b][i]; kab += ga[i] * g[b][i]; wg += wb[i] * g[b][i]; }
      const double mass = (cm * (b == a ? 2.0 : 1.0) + ms) * idt;
      const double sp = cm * cab + p.D * vol * kab + pa * vol * wg;
      p.A[base + ((sl >> (8 * b)) & 0xffu)] += mass + th * sp;
      rhs += (mass - (1.0 - th) * sp) * cv[b];
    }
    rhs += p.src * vol * (1.0 / N1 + pa);
  }
  p.rhs[row] = rhs;
  p.dinv[row] = 1.0 / p.A[base + kd];
}

// ---------------------------------------------------------------- Krylov kernels (one column; cfdh_ipcs_krylov.hip has the pattern)
// y = A x, eight lanes per row, grid-stride over the rows, with the dot products the iteration needs next.
// MODE 0: P0 = y . q ; 1: P0 = y . q, P1 = y . y ; 2: y = q - A x, P0 = y . y, P1 = q . q (true residual; not frozen by `done`)
template <int MODE>
__global__ __launch_bounds__(TPB) void sc_spmv_kernel(int n, const int *__restrict__ rowptr, const int *__restrict__ col, const double *__restrict__ val,
                                                     const double *__restrict__ x, double *__restrict__ y, const double *__restrict__ q,
                                                     const double *__restrict__ S, double *__restrict__ P) {
  __shared__ double sh[4];
  if (MODE != 2 && S[SC_DONE] != 0.0) return;
  const int l = threadIdx.x & 7;
  double d0 = 0.0, d1 = 0.0;
  for (int base = blockIdx.x * (TPB / 8); base < n; base += gridDim.x * (TPB / 8)) {
    const int row = base + (threadIdx.x >> 3);
    double a = 0.0;
    if (row < n)
      for (int k = rowptr[row] + l; k < rowptr[row + 1]; k += 8) a += val[k] * x[col[k]];
    a = group8_sum(a);
    if (row < n && l == 0) {
      const double qv = q[row];
      const double r = MODE == 2 ? qv - a : a;
      y[row] = r;
      if (MODE == 2) { d0 += r * r; d1 += qv * qv; }
      else { d0 += r * qv; if (MODE == 1) d1 += r * r; }
    }
  }
  d0 = block_sum(d0, sh);
  if (MODE != 0) d1 = block_sum(d1, sh);
  if (threadIdx.x == 0) { P[blockIdx.x] = d0; if (MODE != 0) P[SC_NB + blockIdx.x] = d1; }
}

// one block: fold the partial sums into the scalars.
// STAGE 0 (init / verification): P0 = |r|^2 of the true residual, P1 = |b|^2 ; first != 0 also sets the tolerance and its = 0
//       1: alpha = rho / P0     2: omega = P0 / P1     3: rho_old = rho, rho = P0, |r|^2 = P1, its++, done?
template <int STAGE>
__global__ __launch_bounds__(TPB) void sc_scal_kernel(int nb, const double *__restrict__ P, double *__restrict__ S, double rtol, double atol,
                                                     int first, double *__restrict__ mirror) {
  __shared__ double sh[4];
  if (STAGE != 0 && S[SC_DONE] != 0.0) return;
  double a = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < nb; i += TPB) { a += P[i]; if (STAGE != 1) b += P[SC_NB + i]; }
  a = block_sum(a, sh);
  b = block_sum(b, sh);
  if (threadIdx.x != 0) return;
  bool check = false;
  if (STAGE == 0) {
    if (first) {
      S[SC_BN2] = b; S[SC_ITS] = 0.0; S[SC_BAD] = 0.0;
      const double t = fmax(rtol * sqrt(b), atol);
      S[SC_TOL2] = t * t;
    }
    S[SC_RN2] = a; S[SC_RHO] = a; S[SC_RHO_OLD] = 1.0; S[SC_ALPHA] = 1.0; S[SC_OMEGA] = 1.0; S[SC_BETA] = 0.0;
    S[SC_DONE] = 0.0;
    check = true;
  } else if (STAGE == 1) {
    const double al = S[SC_RHO] / a;
    S[SC_ALPHA] = al;
    if (!isfinite(al)) { S[SC_BAD] = 1.0; S[SC_DONE] = 1.0; }
  } else if (STAGE == 2) {
    const double om = b > 0.0 ? a / b : 0.0;
    S[SC_OMEGA] = om;
    if (!isfinite(om)) { S[SC_BAD] = 1.0; S[SC_DONE] = 1.0; }
  } else {
    const double ro = S[SC_RHO];
    S[SC_RHO_OLD] = ro; S[SC_RHO] = a;
    S[SC_BETA] = (a / ro) * (S[SC_ALPHA] / S[SC_OMEGA]);
    S[SC_RN2] = b; S[SC_ITS] += 1.0;
    check = true;
  }
  if (check) {
    // a finite |r|^2 within the tolerance is convergence whatever beta is: a solve that lands on the solution has s = 0, t = 0,
    // omega = 0, r = 0 and beta = 0 * inf; the driver's true residual decides next, as after every stop.  A beta that is not
    // finite above the tolerance is a breakdown (scalar_twin.bicgstab_jacobi takes the two tests in the same order)
    const double rn2 = S[SC_RN2];
    if (!isfinite(rn2)) { S[SC_BAD] = 1.0; S[SC_DONE] = 1.0; }
    else if (rn2 <= S[SC_TOL2]) S[SC_DONE] = 1.0;
    else if (STAGE != 0 && !isfinite(S[SC_BETA])) { S[SC_BAD] = 1.0; S[SC_DONE] = 1.0; }
  }
  // every stage publishes (|r|^2, done, its, bad): a breakdown found between two convergence tests freezes the kernels behind it
  for (int i = 0; i < 4; i++) mirror[i] = S[SC_RN2 + i];
}

// initial guess: c0 with the Dirichlet values imposed
__global__ __launch_bounds__(TPB) void sc_guess_kernel(int n, const double *__restrict__ c0, const unsigned char *__restrict__ flag,
                                                      const double *__restrict__ val, double *__restrict__ x) {
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) x[i] = flag[i] ? val[i] : c0[i];
}
// start / restart: rh = r, p = v = 0
__global__ __launch_bounds__(TPB) void sc_start_kernel(int n, const double *__restrict__ r, double *__restrict__ rh, double *__restrict__ p, double *__restrict__ v) {
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) { rh[i] = r[i]; p[i] = 0.0; v[i] = 0.0; }
}
// p = r + beta (p - omega v) ; y = dinv p
__global__ __launch_bounds__(TPB) void sc_bicg1_kernel(int n, const double *__restrict__ S, const double *__restrict__ r, const double *__restrict__ v,
                                                      const double *__restrict__ dinv, double *__restrict__ p, double *__restrict__ y) {
  if (S[SC_DONE] != 0.0) return;
  const double beta = S[SC_BETA], om = S[SC_OMEGA];
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
    const double pn = r[i] + beta * (p[i] - om * v[i]);
    p[i] = pn;
    y[i] = dinv[i] * pn;
  }
}
// s = r - alpha v ; z = dinv s
__global__ __launch_bounds__(TPB) void sc_bicg2_kernel(int n, const double *__restrict__ S, const double *__restrict__ r, const double *__restrict__ v,
                                                      const double *__restrict__ dinv, double *__restrict__ s, double *__restrict__ z) {
  if (S[SC_DONE] != 0.0) return;
  const double al = S[SC_ALPHA];
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
    const double sn = r[i] - al * v[i];
    s[i] = sn;
    z[i] = dinv[i] * sn;
  }
}
// x += alpha y + omega z ; r = s - omega t ; P0 = rh . r, P1 = r . r
__global__ __launch_bounds__(TPB) void sc_bicg3_kernel(int n, const double *__restrict__ S, const double *__restrict__ y, const double *__restrict__ z,
                                                      const double *__restrict__ s, const double *__restrict__ t, const double *__restrict__ rh,
                                                      double *__restrict__ x, double *__restrict__ r, double *__restrict__ P) {
  __shared__ double sh[4];
  if (S[SC_DONE] != 0.0) return;
  const double al = S[SC_ALPHA], om = S[SC_OMEGA];
  double d0 = 0.0, d1 = 0.0;
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
    x[i] += al * y[i] + om * z[i];
    const double rn = s[i] - om * t[i];
    r[i] = rn;
    d0 += rh[i] * rn; d1 += rn * rn;
  }
  d0 = block_sum(d0, sh);
  d1 = block_sum(d1, sh);
  if (threadIdx.x == 0) { P[blockIdx.x] = d0; P[SC_NB + blockIdx.x] = d1; }
}

// ---------------------------------------------------------------- functionals: block partial sums
// kind 0: int c dx = sum_K |K| mean_a c_a.  partial[block]
template <int D>
__global__ __launch_bounds__(TPB) void sc_integral_kernel(int nc, const int *__restrict__ cells, const double *__restrict__ X, const double *__restrict__ c,
                                                         double *__restrict__ partial) {
  constexpr int N1 = D + 1;
  __shared__ double sh[4];
  double acc = 0.0;
  for (int e = blockIdx.x * TPB + threadIdx.x; e < nc; e += gridDim.x * TPB) {
    double P[N1][D], cs = 0.0;
#pragma unroll
    for (int a = 0; a < N1; a++) {
      const int v = cells[(size_t)N1 * e + a];
      cs += c[v];
#pragma unroll
      for (int i = 0; i < D; i++) P[a][i] = X[(size_t)D * v + i];
    }
    double r[D][D];
#pragma unroll
    for (int a = 1; a <= D; a++)
#pragma unroll
      for (int i = 0; i < D; i++) r[a - 1][i] = P[a][i] - P[0][i];
    double det;
    if constexpr (D == 2) det = r[0][0] * r[1][1] - r[0][1] * r[1][0];
    else det = r[0][0] * (r[1][1] * r[2][2] - r[1][2] * r[2][1]) + r[0][1] * (r[1][2] * r[2][0] - r[1][0] * r[2][2]) + r[0][2] * (r[1][0] * r[2][1] - r[1][1] * r[2][0]);
    acc += fabs(det) * (D == 2 ? 0.5 : 1.0 / 6.0) * cs * (1.0 / N1);
  }
  acc = block_sum(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}
// kind 1: int c (u . n) ds over the exterior facets of `marker`.  c and u are linear on the facet F (opposite local vertex f),
// n |F| = -d |K| grad(lambda_f) and int_F l_a l_b = |F| (1 + d_ab) / (d (d + 1)):
//   sum_{a, b != f} c_a (u_b . n|F|) (1 + d_ab) / (d (d + 1)) = (cs us + sum_a c_a (u_a . n|F|)) / (d (d + 1)), cs, us the sums over the facet
template <int D>
__global__ __launch_bounds__(TPB) void sc_flux_kernel(int nfac, int marker, const int *__restrict__ fcell, const int *__restrict__ flocal,
                                                     const int *__restrict__ fmarker, const int *__restrict__ cells, const double *__restrict__ X,
                                                     const double *__restrict__ u, const double *__restrict__ c, double *__restrict__ partial) {
  constexpr int N1 = D + 1;
  __shared__ double sh[4];
  double acc = 0.0;
  for (int q = blockIdx.x * TPB + threadIdx.x; q < nfac; q += gridDim.x * TPB) {
    if (fmarker[q] != marker) continue;
    const int e = fcell[q], f = flocal[q];
    double P[N1][D], uv[N1][D], cv[N1];
#pragma unroll
    for (int a = 0; a < N1; a++) {
      const int v = cells[(size_t)N1 * e + a];
      cv[a] = c[v];
#pragma unroll
      for (int i = 0; i < D; i++) { P[a][i] = X[(size_t)D * v + i]; uv[a][i] = u[(size_t)D * v + i]; }
    }
    // the outward normal times |F|: perpendicular to the facet, pointing away from the opposite vertex
    double Pf[D], E[D][D];  // opposite vertex; facet vertices in increasing local index
#pragma unroll
    for (int i = 0; i < D; i++) {
      Pf[i] = 0.0;
#pragma unroll
      for (int a = 0; a < N1; a++) Pf[i] = a == f ? P[a][i] : Pf[i];
#pragma unroll
      for (int j = 0; j < D; j++) {
        double t = 0.0;
#pragma unroll
        for (int a = 0; a < N1; a++) t = a == j + (j >= f ? 1 : 0) ? P[a][i] : t;
        E[j][i] = t;
      }
    }
    double nF[D];
    if constexpr (D == 2) {
      nF[0] = E[1][1] - E[0][1]; nF[1] = -(E[1][0] - E[0][0]);
    } else {
      const double a0 = E[1][0] - E[0][0], a1 = E[1][1] - E[0][1], a2 = E[1][2] - E[0][2];
      const double b0 = E[2][0] - E[0][0], b1 = E[2][1] - E[0][1], b2 = E[2][2] - E[0][2];
      nF[0] = 0.5 * (a1 * b2 - a2 * b1); nF[1] = 0.5 * (a2 * b0 - a0 * b2); nF[2] = 0.5 * (a0 * b1 - a1 * b0);
    }
    double sgn = 0.0;
#pragma unroll
    for (int i = 0; i < D; i++) sgn += nF[i] * (E[0][i] - Pf[i]);
    sgn = sgn < 0.0 ? -1.0 : 1.0;
    double cs = 0.0, us = 0.0, cu = 0.0;
#pragma unroll
    for (int a = 0; a < N1; a++) {
      double un = 0.0;
#pragma unroll
      for (int i = 0; i < D; i++) un += uv[a][i] * nF[i];
      const double on = a == f ? 0.0 : 1.0;
      cs += on * cv[a]; us += on * un; cu += on * cv[a] * un;
    }
    acc += sgn * (cs * us + cu) * (1.0 / (D * (D + 1)));
  }
  acc = block_sum(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}
// kinds 2 / 3: per-block minimum and maximum (max_nan keeps a NaN), then one block folds them
__global__ __launch_bounds__(TPB) void sc_minmax_kernel(int n, const double *__restrict__ c, double *__restrict__ partial, int stride) {
  __shared__ double sh[4];
  double lo = -c[0], hi = c[0];
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) { lo = max_nan(lo, -c[i]); hi = max_nan(hi, c[i]); }
  lo = block_max(lo, sh);
  hi = block_max(hi, sh);
  if (threadIdx.x == 0) { partial[blockIdx.x] = lo; partial[stride + blockIdx.x] = hi; }
}
__global__ __launch_bounds__(TPB) void sc_minmax_final_kernel(int nb, int stride, const double *__restrict__ partial, double *__restrict__ out) {
  __shared__ double sh[4];
  double lo = partial[0], hi = partial[stride];
  for (int i = threadIdx.x; i < nb; i += TPB) { lo = max_nan(lo, partial[i]); hi = max_nan(hi, partial[stride + i]); }
  lo = block_max(lo, sh);
  hi = block_max(hi, sh);
  if (threadIdx.x == 0) { out[0] = -lo; out[1] = hi; }
}

inline int sc_nb(long long n, int per) {
  const long long g = (n + per - 1) / per;
  return (int)(g < 1 ? 1 : (g > SC_NB ? SC_NB : g));
}
#define SCL(c, kern, grid, ...) hipLaunchKernelGGL(kern, dim3(grid), dim3(TPB), 0, (c)->stream, __VA_ARGS__)

int sc_need(cfdh_ctx *c, const char *who) {
  if (!c->sc) return cfdh_fail(c, CFDH_E_STATE, "%s: cfdh_scalar_enable was not called", who);
  return 0;
}

// left-hand values, right-hand side and Jacobi weights of the next step at the current state
int sc_assemble(cfdh_ctx *c, bool timed) {
  ScalarData *S = c->sc;
  ScAsmArgs a;
  a.sptr = S->sptr.p; a.inc = S->inc.p; a.slot = S->slot.p; a.cells = c->cells.p; a.vptr = c->vptr.p; a.vcol = c->vcol.p;
  a.coords = c->coords.p; a.x = c->x.p; a.xprev = c->xprev.p; a.c0 = S->c.p; a.bcval = S->bcval.p; a.bcflag = S->bcflag.p;
  a.A = S->A.p; a.rhs = S->rhs.p; a.dinv = S->dinv.p;
  a.n = S->n; a.dt = c->dt; a.D = S->D; a.src = S->src; a.theta = S->theta;
  if (timed) HIPCHK(c, hipEventRecord(S->ev0, c->stream));
  const dim3 gr(S->nslices), bl(cfdh_scalar::SLICE);
  if (c->dim == 3) hipLaunchKernelGGL(sc_assemble_kernel<3>, gr, bl, 0, c->stream, a);
  else hipLaunchKernelGGL(sc_assemble_kernel<2>, gr, bl, 0, c->stream, a);
  if (timed) HIPCHK(c, hipEventRecord(S->ev1, c->stream));
  c->n_scalar_asm++;
  HIPCHK(c, hipGetLastError());
  return 0;
}

template <int MODE>
void sc_spmv(cfdh_ctx *c, const double *x, double *y, const double *q) {
  ScalarData *S = c->sc;
  SCL(c, sc_spmv_kernel<MODE>, sc_nb(S->n, TPB / 8), S->n, (const int *)c->vptr.p, (const int *)c->vcol.p, (const double *)S->A.p, x, y, q,
      (const double *)S->S.p, S->P.p);
}
template <int STAGE>
void sc_scal(cfdh_ctx *c, int nb, double rtol, double atol, int first) {
  ScalarData *S = c->sc;
  SCL(c, sc_scal_kernel<STAGE>, 1, nb, (const double *)S->P.p, S->S.p, rtol, atol, first, S->h_mirror_dev);
}
// mirror: |r|^2, done, its, bad
int sc_read(cfdh_ctx *c, double m[4]) {
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < 4; i++) m[i] = c->sc->h_mirror[i];
  return 0;
}

// cfdh_scalar_krylov_solve only: the closing true-residual stage resets the recurrence scalars, so the hook keeps the block as the
// last iteration left it.  A step never takes this copy.
int sc_snapshot(cfdh_ctx *c) {
  ScalarData *D = c->sc;
  if (!D->snap_on) return 0;
  HIPCHK(c, hipMemcpyAsync(D->snap, D->S.p, sizeof D->snap, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  D->snap_set = true;
  return 0;
}

// BiCGStab + Jacobi on the assembled system; x holds the initial guess (ip_bicgstab's structure)
int sc_bicgstab(cfdh_ctx *c, ScTol tol, const double *b, double *x, cfdh_scalar_stats *st) {
  ScalarData *D = c->sc;
  const int n = D->n, nbv = sc_nb(n, TPB * 4), nbs = sc_nb(n, TPB / 8);
  const double rtol = tol.rtol, atol = tol.atol;
  const int max_it = tol.max_it, batch = 4;
  const double *S = D->S.p;
  double m[4];
  sc_spmv<2>(c, x, D->kr.p, b);
  sc_scal<0>(c, nbs, rtol, atol, 1);
  HIPCHK(c, hipGetLastError());
  CHK(sc_read(c, m));
  // `launched` bounds the loop on the host, whatever the device counter says: at most max_it iterations are ever launched
  bool capped = false;
  int launched = 0;
  while (m[1] == 0.0) {  // not converged on the true residual: (re)start from it
    if (launched >= max_it) { capped = true; break; }
    SCL(c, sc_start_kernel, nbv, n, (const double *)D->kr.p, D->krh.p, D->kp.p, D->kv.p);
    while (launched < max_it) {
      const int nbatch = std::min(batch, max_it - launched);
      launched += nbatch;
      for (int k = 0; k < nbatch; k++) {
        SCL(c, sc_bicg1_kernel, nbv, n, S, (const double *)D->kr.p, (const double *)D->kv.p, (const double *)D->dinv.p, D->kp.p, D->ky.p);
        sc_spmv<0>(c, D->ky.p, D->kv.p, D->krh.p);
        sc_scal<1>(c, nbs, 0, 0, 0);
        SCL(c, sc_bicg2_kernel, nbv, n, S, (const double *)D->kr.p, (const double *)D->kv.p, (const double *)D->dinv.p, D->ks.p, D->kz.p);
        sc_spmv<1>(c, D->kz.p, D->kt.p, D->ks.p);
        sc_scal<2>(c, nbs, 0, 0, 0);
        SCL(c, sc_bicg3_kernel, nbv, n, S, (const double *)D->ky.p, (const double *)D->kz.p, (const double *)D->ks.p, (const double *)D->kt.p,
            (const double *)D->krh.p, x, D->kr.p, D->P.p);
        sc_scal<3>(c, nbv, 0, 0, 0);
      }
      HIPCHK(c, hipGetLastError());
      CHK(sc_read(c, m));
      if (m[1] != 0.0) break;
    }
    if (m[3] != 0.0) break;
    CHK(sc_snapshot(c));
    sc_spmv<2>(c, x, D->kr.p, b);  // the recurrence says converged (or the cap is reached): the true residual decides
    sc_scal<0>(c, nbs, rtol, atol, 0);
    HIPCHK(c, hipGetLastError());
    CHK(sc_read(c, m));
  }
  double h[SC_NS];
  HIPCHK(c, hipMemcpyAsync(h, D->S.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  st->its = (int)h[SC_ITS];
  st->rel_res = h[SC_BN2] > 0 ? std::sqrt(h[SC_RN2] / h[SC_BN2]) : std::sqrt(h[SC_RN2]);
  st->reason = m[3] != 0.0 ? CFDH_KSP_DIVERGED_NANORINF : (capped ? CFDH_KSP_DIVERGED_ITS : CFDH_KSP_CONVERGED_RTOL);
  return 0;
}

}  // namespace

void cfdh_scalar_free(cfdh_ctx *c) {
  delete c->sc;
  c->sc = nullptr;
}

int cfdh_scalar_enable_impl(cfdh_ctx *c, double D, double s, double theta) {
  const char *who = "cfdh_scalar_enable";
  if (c->ipcs) return cfdh_fail(c, CFDH_E_ARG, "%s: not available on an incremental pressure-correction context (cfdh_create_ipcs)", who);
  if (c->gen) return cfdh_fail(c, CFDH_E_ARG, "%s: the scalar lives on the closed-form P1 contexts (cfdh_create), not on the generic element kernels", who);
  if (c->nranks > 1 || c->nvo != c->nv) return cfdh_fail(c, CFDH_E_ARG, "%s: not available in partitioned runs", who);
  std::string why;
  if (!cfdh_scalar::check_params(D, s, theta, why)) return cfdh_fail(c, CFDH_E_ARG, "%s: %s", who, why.c_str());
  if (c->sc) {  // new parameters, c kept
    c->sc->D = D; c->sc->src = s; c->sc->theta = theta;
    return 0;
  }
  cfdh_scalar::WorkList w;
  if (!cfdh_scalar::build_worklist(c->dim, c->nv, c->nc, c->h_cells.data(), c->h_vptr.data(), c->h_vcol.data(), w, why))
    return cfdh_fail(c, CFDH_E_ARG, "%s: %s", who, why.c_str());
  ScalarData *S = new (std::nothrow) ScalarData();
  if (!S) return cfdh_fail(c, CFDH_E_NOMEM, "out of host memory");
  c->sc = S;
  int rc = [&]() -> int {
    S->n = c->nv; S->D = D; S->src = s; S->theta = theta;
    S->nslices = w.nslices;
    const size_t n = (size_t)c->nv;
    HIPCHK(c, S->sptr.upload(w.sptr, c->stream));
    HIPCHK(c, S->inc.upload(w.dinc, c->stream));
    HIPCHK(c, S->slot.upload(w.dslot, c->stream));
    for (dbuf<double> *b : {&S->c, &S->cn, &S->rhs, &S->dinv, &S->bcval, &S->kr, &S->krh, &S->kp, &S->kv, &S->ks, &S->kt, &S->ky, &S->kz}) {
      HIPCHK(c, b->alloc(n));
      HIPCHK(c, b->zero(c->stream));
    }
    HIPCHK(c, S->A.alloc((size_t)c->nnzv));
    HIPCHK(c, S->A.zero(c->stream));
    HIPCHK(c, S->bcflag.alloc(n));
    HIPCHK(c, S->bcflag.zero(c->stream));
    HIPCHK(c, S->S.alloc(SC_NS));
    HIPCHK(c, S->S.zero(c->stream));
    HIPCHK(c, S->P.alloc(2 * SC_NB));
    HIPCHK(c, S->P.zero(c->stream));
    HIPCHK(c, hipHostMalloc((void **)&S->h_mirror, 4 * sizeof(double)));
    HIPCHK(c, hipHostGetDevicePointer((void **)&S->h_mirror_dev, S->h_mirror, 0));
    HIPCHK(c, hipEventCreate(&S->ev0));
    HIPCHK(c, hipEventCreate(&S->ev1));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // the host vectors go out of scope
    return 0;
  }();
  if (rc) cfdh_scalar_free(c);
  return rc;
}

int cfdh_scalar_set_dirichlet_impl(cfdh_ctx *c, int64_t n, const int32_t *nodes, const double *values) {
  CHK(sc_need(c, "cfdh_scalar_set_dirichlet"));
  std::string why;
  if (!cfdh_scalar::check_dirichlet(n, c->nv, nodes, values, why)) return cfdh_fail(c, CFDH_E_ARG, "cfdh_scalar_set_dirichlet: %s", why.c_str());
  ScalarData *S = c->sc;
  std::vector<unsigned char> flag((size_t)c->nv, 0);
  std::vector<double> val((size_t)c->nv, 0.0);
  for (int64_t k = 0; k < n; k++) { const int r = c->perm[nodes[k]]; flag[r] = 1; val[r] = values[k]; }
  HIPCHK(c, S->bcflag.upload(flag, c->stream));
  HIPCHK(c, S->bcval.upload(val, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

// set != NULL: upload c; get != NULL: download it (caller's numbering)
int cfdh_scalar_state_impl(cfdh_ctx *c, const double *set, double *get) {
  CHK(sc_need(c, set ? "cfdh_scalar_set_state" : "cfdh_scalar_get_state"));
  ScalarData *S = c->sc;
  const int n = S->n;
  std::vector<double> h((size_t)n);
  if (set) {
    for (int v = 0; v < n; v++)
      if (!cfdh_scalar::finite(set[v])) return cfdh_fail(c, CFDH_E_ARG, "cfdh_scalar_set_state: entry %d is not finite", v);
    for (int v = 0; v < n; v++) h[c->perm[v]] = set[v];
    HIPCHK(c, hipMemcpyAsync(S->c.p, h.data(), sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  if (get) {
    HIPCHK(c, hipMemcpyAsync(h.data(), S->c.p, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int v = 0; v < n; v++) get[v] = h[c->perm[v]];
  }
  return 0;
}

int cfdh_scalar_set_tolerances_impl(cfdh_ctx *c, double rtol, double atol, int max_it) {
  CHK(sc_need(c, "cfdh_scalar_set_tolerances"));
  if (!(rtol >= 0.0 && rtol < 1.0) || !(atol >= 0.0) || max_it < 1)
    return cfdh_fail(c, CFDH_E_ARG, "cfdh_scalar_set_tolerances: need 0 <= rtol < 1, atol >= 0, max_it >= 1");
  c->sc->rtol = rtol; c->sc->atol = atol; c->sc->max_it = max_it;
  return 0;
}

static int sc_ready(cfdh_ctx *c, const char *who) {
  CHK(sc_need(c, who));
  if (!c->params_set || !c->state_set) return cfdh_fail(c, CFDH_E_STATE, "%s: parameters (cfdh_set_params) and a state are needed", who);
  return 0;
}

int cfdh_scalar_step_impl(cfdh_ctx *c, cfdh_scalar_stats *stats) {
  cfdh_scalar_stats st;
  memset(&st, 0, sizeof st);
  if (stats) *stats = st;
  CHK(sc_ready(c, "cfdh_scalar_step"));
  ScalarData *S = c->sc;
  const auto t0 = std::chrono::steady_clock::now();
  CHK(sc_assemble(c, true));
  SCL(c, sc_guess_kernel, sc_nb(S->n, TPB * 4), S->n, (const double *)S->c.p, (const unsigned char *)S->bcflag.p, (const double *)S->bcval.p, S->cn.p);
  CHK(sc_bicgstab(c, ScTol{S->rtol, S->atol, S->max_it}, S->rhs.p, S->cn.p, &st));
  const bool ok = st.reason > 0;
  if (ok) {
    HIPCHK(c, hipMemcpyAsync(S->c.p, S->cn.p, sizeof(double) * S->n, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->n_scalar_steps++;
  }
  float ms = 0.f;
  HIPCHK(c, hipEventElapsedTime(&ms, S->ev0, S->ev1));
  st.ms_assemble = ms;
  st.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (stats) *stats = st;
  if (!ok)
    return cfdh_fail(c, CFDH_E_DIVERGED, "cfdh_scalar_step: BiCGStab did not converge (reason %d, %d iterations, |r| / |b| = %.3e); c is unchanged", st.reason,
                     st.its, st.rel_res);
  return 0;
}

int cfdh_scalar_get_operator_impl(cfdh_ctx *c, int64_t *nnz, int32_t *rowptr, int32_t *col, double *vals, double *rhs) {
  CHK(sc_need(c, "cfdh_scalar_get_operator"));
  *nnz = c->nnzv;
  if (!rowptr && !col && !vals && !rhs) return 0;
  if (!rowptr || !col || !vals || !rhs) return cfdh_fail(c, CFDH_E_ARG, "cfdh_scalar_get_operator: pass all of rowptr/col/vals/rhs or none");
  CHK(sc_ready(c, "cfdh_scalar_get_operator"));
  ScalarData *S = c->sc;
  CHK(sc_assemble(c, false));
  std::vector<double> A((size_t)c->nnzv), b((size_t)S->n);
  HIPCHK(c, hipMemcpyAsync(A.data(), S->A.p, sizeof(double) * A.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(b.data(), S->rhs.p, sizeof(double) * b.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  int64_t pos = 0;
  std::vector<std::pair<int, int>> ord;
  for (int vu = 0; vu < S->n; vu++) {
    const int r = c->perm[vu];
    ord.clear();
    for (int k = c->h_vptr[r]; k < c->h_vptr[r + 1]; k++) ord.push_back({c->iperm[c->h_vcol[k]], k});
    std::sort(ord.begin(), ord.end());
    rowptr[vu] = (int32_t)pos;
    for (auto &e : ord) { col[pos] = e.first; vals[pos] = A[e.second]; pos++; }
    rhs[vu] = b[r];
  }
  rowptr[S->n] = (int32_t)pos;
  return 0;
}

// One solve on the caller's b and x0 (cfdh_scalar_krylov_solve) with the caller's tolerances; b and x live in buffers of the hook's
// own, the assembly counter (cfdh_info 97) is put back.
int cfdh_scalar_krylov_solve_impl(cfdh_ctx *c, const double *b, const double *x0, double rtol, double atol, int max_it, double *x,
                                  cfdh_scalar_stats *st, double *scalars, double *p) {
  const char *who = "cfdh_scalar_krylov_solve";
  CHK(sc_ready(c, who));
  ScalarData *S = c->sc;
  hipStream_t s = c->stream;
  const int n = S->n;
  for (int v = 0; v < n; v++)
    if (!cfdh_scalar::finite(b[v]) || !cfdh_scalar::finite(x0[v])) return cfdh_fail(c, CFDH_E_ARG, "%s: entry %d of b or x0 is not finite", who, v);
  memset(st, 0, sizeof *st);
  HIPCHK(c, S->hk_b.alloc((size_t)n)); HIPCHK(c, S->hk_x.alloc((size_t)n));
  const long long asm0 = c->n_scalar_asm;
  CHK(sc_assemble(c, false));
  c->n_scalar_asm = asm0;
  std::vector<double> hb((size_t)n), hx((size_t)n);
  for (int v = 0; v < n; v++) { hb[c->perm[v]] = b[v]; hx[c->perm[v]] = x0[v]; }
  HIPCHK(c, hipMemcpyAsync(S->hk_b.p, hb.data(), sizeof(double) * n, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(S->hk_x.p, hx.data(), sizeof(double) * n, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipStreamSynchronize(s));
  S->snap_on = true; S->snap_set = false;
  const int rc = sc_bicgstab(c, ScTol{rtol, atol, max_it}, S->hk_b.p, S->hk_x.p, st);
  S->snap_on = false;
  CHK(rc);
  double h[SC_NS];
  HIPCHK(c, hipMemcpyAsync(hx.data(), S->hk_x.p, sizeof(double) * n, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(h, S->S.p, sizeof h, hipMemcpyDeviceToHost, s));
  if (p) HIPCHK(c, hipMemcpyAsync(hb.data(), S->kp.p, sizeof(double) * n, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  for (int v = 0; v < n; v++) x[v] = hx[c->perm[v]];
  if (p) for (int v = 0; v < n; v++) p[v] = hb[c->perm[v]];
  if (scalars) {
    for (int k = 0; k < SC_NS; k++) scalars[k] = h[k];
    if (S->snap_set)
      for (int k = SC_RHO; k <= SC_BETA; k++) scalars[k] = S->snap[k];
  }
  return 0;
}

int cfdh_scalar_get_order_impl(cfdh_ctx *c, int32_t *row) {
  CHK(sc_need(c, "cfdh_scalar_get_order"));
  for (int v = 0; v < c->sc->n; v++) row[v] = c->perm[v];
  return 0;
}

int cfdh_scalar_functional_impl(cfdh_ctx *c, int kind, int marker, double *out) {
  CHK(sc_need(c, "cfdh_scalar_functional"));
  ScalarData *S = c->sc;
  const int nb = 256;
  if (kind == 0 || kind == 1) {
    if (kind == 1 && !c->state_set) return cfdh_fail(c, CFDH_E_STATE, "cfdh_scalar_functional: kind 1 needs a state");
    if (kind == 0) {
      if (c->dim == 3) SCL(c, sc_integral_kernel<3>, nb, c->nc, (const int *)c->cells.p, (const double *)c->coords.p, (const double *)S->c.p, c->red_partial.p);
      else SCL(c, sc_integral_kernel<2>, nb, c->nc, (const int *)c->cells.p, (const double *)c->coords.p, (const double *)S->c.p, c->red_partial.p);
    } else {
      if (c->dim == 3)
        SCL(c, sc_flux_kernel<3>, nb, c->nfac, marker, (const int *)c->d_fac_cell.p, (const int *)c->d_fac_local.p, (const int *)c->d_fac_marker.p,
            (const int *)c->cells.p, (const double *)c->coords.p, (const double *)c->x.p, (const double *)S->c.p, c->red_partial.p);
      else
        SCL(c, sc_flux_kernel<2>, nb, c->nfac, marker, (const int *)c->d_fac_cell.p, (const int *)c->d_fac_local.p, (const int *)c->d_fac_marker.p,
            (const int *)c->cells.p, (const double *)c->coords.p, (const double *)c->x.p, (const double *)S->c.p, c->red_partial.p);
    }
    HIPCHK(c, hipGetLastError());
    ScalarRead h;
    CHK(scalars_finish(c, c->red_out.p + RO_RESULT, 1, 0, nb, &h));
    return scalars_read(c, h, out);
  }
  if (kind == 2 || kind == 3) {
    SCL(c, sc_minmax_kernel, nb, S->n, (const double *)S->c.p, c->red_partial.p, nb);
    SCL(c, sc_minmax_final_kernel, 1, nb, nb, (const double *)c->red_partial.p, c->red_out.p + RO_RESULT);
    HIPCHK(c, hipGetLastError());
    double v[2];
    CHK(scalars_read(c, ScalarRead{c->red_out.p + RO_RESULT, 2, false}, v));
    *out = v[kind - 2];
    return 0;
  }
  return cfdh_fail(c, CFDH_E_ARG, "cfdh_scalar_functional: unknown kind %d (0: integral, 1: flux through a marker, 2: min, 3: max)", kind);
}
