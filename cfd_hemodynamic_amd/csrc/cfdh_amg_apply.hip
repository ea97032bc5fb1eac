// One application of the preconditioner's algebraic multigrid on gfx950 (CDNA4, wave64): the kernels that apply a hierarchy
// (the hierarchies are BUILT in cfdh_setup.cpp on the host and in cfdh_amg_dev.hip on the device).
//
//  * scalar CSR / SELL-64 operators on one, two or three interleaved right-hand sides (double, double2, d3)
//  * level smoothers: Chebyshev steps, damped-Jacobi pre- / post-sweeps, dense coarsest solve
//  * the cycles: fused V(1,1) Jacobi cycle on composite operators (one kernel per level and direction, SELL-64 / fp32 on the
//    fine levels, dense coarse solve folded into the level above), the sweep-by-sweep Jacobi cycle, the Chebyshev cycle, and
//    the distributed finest level of a partitioned run (k_dl0_down / k_dl0_up); k_amg_vcycle picks one
//  * the other steps of a preconditioner application: Cahouet-Chabard scaling / combination, global scatter / gather,
//    packing of the extended velocity right-hand side
//
// SELL-64 or CSR: the size rules are cfdh_sweep_sell / cfdh_cheb2_sell (cfdh_internal.hpp); a kernel gets the SELL arrays only
// when the rule says so AND the operator has them (CsrDev::has_sell*), CSR otherwise.  AmgLevel::fine / sell of the fused
// cycle are set by the builds together with the copies they select.  Where the SELL-64 operators of an up-sweep (or H's Chebyshev
// matrix) have head copies (CsrDev::head_w > 0), the sweep takes the head kernel, which needs no pointer for the head's entries.
//
// HBM-bound gather work, fixed summation order everywhere (bitwise reproducible).
#include <hip/hip_runtime.h>

#include "cfdh_internal.hpp"
#include "cfdh_wave.hpp"

// ---------------------------------------------------------------- scalar CSR operators (AMG levels)
// All level kernels are templated on the vector element T: double (one right-hand side) or
// double2 (two right-hand sides sharing one scalar operator: the two velocity components).
// three right-hand sides sharing one scalar operator: the velocity components of a tetrahedral mesh
struct d3 { double x, y, z; };
__device__ __forceinline__ d3 vzero(const d3 *) { return d3{0.0, 0.0, 0.0}; }
__device__ __forceinline__ d3 vfma(double a, d3 x, d3 acc) { return d3{acc.x + a * x.x, acc.y + a * x.y, acc.z + a * x.z}; }
__device__ __forceinline__ d3 vsub(d3 a, d3 b) { return d3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ d3 vadd(d3 a, d3 b) { return d3{a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ d3 vscale(double a, d3 x) { return d3{a * x.x, a * x.y, a * x.z}; }
__device__ __forceinline__ d3 g8(d3 v) { return d3{group8_sum(v.x), group8_sum(v.y), group8_sum(v.z)}; }
__device__ __forceinline__ d3 wsum(d3 v) { return d3{wave_sum(v.x), wave_sum(v.y), wave_sum(v.z)}; }
__device__ __forceinline__ double vzero(const double *) { return 0.0; }
__device__ __forceinline__ double2 vzero(const double2 *) { return make_double2(0.0, 0.0); }
__device__ __forceinline__ double vfma(double a, double x, double acc) { return acc + a * x; }
__device__ __forceinline__ double2 vfma(double a, double2 x, double2 acc) { return make_double2(acc.x + a * x.x, acc.y + a * x.y); }
__device__ __forceinline__ double vsub(double a, double b) { return a - b; }
__device__ __forceinline__ double2 vsub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ double vadd(double a, double b) { return a + b; }
__device__ __forceinline__ double2 vadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double vscale(double a, double x) { return a * x; }
__device__ __forceinline__ double2 vscale(double a, double2 x) { return make_double2(a * x.x, a * x.y); }
__device__ __forceinline__ double g8(double v) { return group8_sum(v); }
__device__ __forceinline__ double2 g8(double2 v) { return make_double2(group8_sum(v.x), group8_sum(v.y)); }
__device__ __forceinline__ double wsum(double v) { return wave_sum(v); }
__device__ __forceinline__ double2 wsum(double2 v) { return make_double2(wave_sum(v.x), wave_sum(v.y)); }

// One row of a SELL-64 matrix times x, latency-oriented: at ~1 M DOF a sweep is one wave of work per SIMD lane group and
// 85 % of a wave's life is spent waiting on memory (SQ_WAIT_ANY / SQ_WAVE_CYCLES, profiles/r02_pmc_sq_tcc.json), in a
// chain  columns -> gathers -> next columns ...  With all column/value loads of the row issued first, then all gathers,
// the chain is three round trips whatever the row length.  The slice width is wave-uniform: the guards are scalar branches.
template <int MAXW, typename T>
__device__ __forceinline__ T sell_row_dot(const int *__restrict__ sp, const int *__restrict__ sc, const float *__restrict__ sv,
                                          const T *__restrict__ x, int sl, int lane, T a) {
  sl = __builtin_amdgcn_readfirstlane(sl);  // wave-uniform: slice pointers and width live in scalar registers
  const int p0 = sp[sl], w = (sp[sl + 1] - p0) >> 6;
  int cidx[MAXW];
  float cval[MAXW];
#pragma unroll
  for (int k = 0; k < MAXW; k++)
    if (k < w) { const int p = p0 + k * 64 + lane; cidx[k] = NTLOAD(sc + p); cval[k] = NTLOAD(sv + p); }
  T g[MAXW];
#pragma unroll
  for (int k = 0; k < MAXW; k++)
    if (k < w) g[k] = x[cidx[k]];
#pragma unroll
  for (int k = 0; k < MAXW; k++)
    if (k < w) a = vfma((double)cval[k], g[k], a);
  for (int k = MAXW; k < w; k++) { const int p = p0 + k * 64 + lane; a = vfma((double)sv[p], x[sc[p]], a); }
  return a;
}

// ---- head copies of SELL-64 operators (CsrDev::hcol / hvalf / hlen): the pointer trip taken out of that chain.  The first head_w
// entries of a slice sit at an address computed from the slice index, so columns and values are requested at once, together with the
// width and the pointer; only the tail of a wider slice waits for the pointer.  Same entries, same lane -> entry mapping, same
// guards k < width, same order of additions as the pointer kernels: bit-identical results (tests/test_gpu_amg_head.py).
__device__ __forceinline__ int head_slice_len(const unsigned short *__restrict__ hlen, int sl) {
  const unsigned wd = ((const unsigned *)hlen)[sl >> 1];  // sl is wave-uniform: one scalar load
  return (int)((wd >> ((sl & 1) * 16)) & 0xffffu);
}
// sell_row_dot through the head (wh <= MAXW entries per row)
template <int MAXW, typename T>
__device__ __forceinline__ T sell_row_dot_head(const int *__restrict__ sp, const int *__restrict__ sc, const float *__restrict__ sv,
                                               const int *__restrict__ hc, const float *__restrict__ hv,
                                               const unsigned short *__restrict__ hlen, int wh, const T *__restrict__ x, int sl, int lane, T a) {
  static_assert(MAXW <= 10, "ten named entries");
  sl = __builtin_amdgcn_readfirstlane(sl);
  // named scalars, not arrays: an entry is written in one of two places (head or tail), and the compiler keeps such an array as
  // ONE register tuple that it copies -- and therefore waits for -- after the first load
#define RDH_ALL(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9)
#define RDH_DECL(k) int c##k = 0; float v##k = 0.0f;
#define RDH_HEAD(k) if (k < MAXW && k < wh) { c##k = NTLOAD(hc + h0 + k * 64); v##k = NTLOAD(hv + h0 + k * 64); }
#define RDH_TAIL(k) if (k < MAXW && k >= wh && k < w) { const int p = p0 + k * 64 + lane; c##k = NTLOAD(sc + p); v##k = NTLOAD(sv + p); }
#define RDH_DECL_G(k) T g##k = vzero((const T *)nullptr);
#define RDH_GATHER(k) if (k < MAXW && k < w) g##k = x[c##k];
#define RDH_FMA(k) if (k < MAXW && k < w) a = vfma((double)v##k, g##k, a);
  RDH_ALL(RDH_DECL)
  const size_t h0 = (size_t)sl * wh * 64 + lane;
  RDH_ALL(RDH_HEAD)
  const int w = head_slice_len(hlen, sl), p0 = sp[sl];
  RDH_ALL(RDH_TAIL)
  RDH_ALL(RDH_DECL_G)
  RDH_ALL(RDH_GATHER)
  RDH_ALL(RDH_FMA)
#undef RDH_ALL
#undef RDH_DECL
#undef RDH_HEAD
#undef RDH_TAIL
#undef RDH_DECL_G
#undef RDH_GATHER
#undef RDH_FMA
  for (int k = MAXW; k < w; k++) { const int p = p0 + k * 64 + lane; a = vfma((double)sv[p], x[sc[p]], a); }
  return a;
}

// MODE 0: y = A x; 1: y = b - A x; 2: y += A x; 3: y = b + A x
template <int MODE, typename T>
__global__ __launch_bounds__(TPB) void csr_spmv_kernel(int n, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                       const double *__restrict__ val, const T *__restrict__ x,
                                                       T *__restrict__ y, const T *__restrict__ b) {
  const int gid = blockIdx.x * TPB + threadIdx.x;
  const int row = gid >> 3, l = gid & 7;
  T a = vzero((const T *)nullptr);
  if (row < n) {
    const int ks = rowptr[row], ke = rowptr[row + 1];
    for (int k = ks + l; k < ke; k += 8) a = vfma(val[k], x[col[k]], a);
  }
  a = g8(a);
  if (row < n && l == 0) {
    if (MODE == 0) y[row] = a;
    else if (MODE == 1) y[row] = vsub(b[row], a);
    else if (MODE == 2) y[row] = vadd(y[row], a);
    else y[row] = vadd(b[row], a);
  }
}

template <typename T>
static int csr_spmv_t(cfdh_ctx *c, const CsrDev &A, const T *x, T *y, int mode, const T *b) {
  const long long nthreads = 8ll * A.n;
  dim3 grid((unsigned)((nthreads + TPB - 1) / TPB)), block(TPB);
  if (mode == 0) hipLaunchKernelGGL((csr_spmv_kernel<0, T>), grid, block, 0, c->stream, A.n, A.rowptr.p, A.col.p, A.val.p, x, y, b);
  else if (mode == 1) hipLaunchKernelGGL((csr_spmv_kernel<1, T>), grid, block, 0, c->stream, A.n, A.rowptr.p, A.col.p, A.val.p, x, y, b);
  else if (mode == 2) hipLaunchKernelGGL((csr_spmv_kernel<2, T>), grid, block, 0, c->stream, A.n, A.rowptr.p, A.col.p, A.val.p, x, y, b);
  else hipLaunchKernelGGL((csr_spmv_kernel<3, T>), grid, block, 0, c->stream, A.n, A.rowptr.p, A.col.p, A.val.p, x, y, b);
  HIPCHK(c, hipGetLastError());
  return 0;
}
int k_csr_spmv(cfdh_ctx *c, const CsrDev &A, const double *x, double *y, int mode, const double *b) {
  return csr_spmv_t<double>(c, A, x, y, mode, b);
}
// the same scalar matrix applied to ncol interleaved right-hand sides (velocity components through the scalar proxy)
int k_csr_spmv_ncol(cfdh_ctx *c, const CsrDev &A, const double *x, double *y, int mode, const double *b, int ncol) {
  if (ncol == 2) return csr_spmv_t<double2>(c, A, (const double2 *)x, (double2 *)y, mode, (const double2 *)b);
  if (ncol == 3) return csr_spmv_t<d3>(c, A, (const d3 *)x, (d3 *)y, mode, (const d3 *)b);
  return csr_spmv_t<double>(c, A, x, y, mode, b);
}

// One Chebyshev step on a scalar CSR level (single right-hand side):
//   r_out = r_in - A d_old ; d_new = c1 d_old + c2 D^-1 r_out ; x (+)= ...
// MODE 0: x += d_new.
// MODE 1: first step of a zero-guess smoothing fused with its initialisation: d_old = D^-1 r_in / theta
//         is formed on the fly while gathering (never stored), x = d_old + d_new.
// MODE 2: first step after csr_resid_init_kernel (which left d_old = D^-1 r / theta unapplied): x += d_old + d_new.
// LAST: r_out / d_new are not needed any more and are not written.
template <int MODE, bool LAST>
__global__ __launch_bounds__(TPB) void cheb_csr_step_kernel(int n, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                            const double *__restrict__ val, const double *__restrict__ dinv,
                                                            const double *__restrict__ rin, double *__restrict__ rout,
                                                            const double *__restrict__ dold, double *__restrict__ dnew,
                                                            double *__restrict__ x, double c1, double c2, double itheta) {
  const int gid = blockIdx.x * TPB + threadIdx.x;
  const int row = gid >> 3, l = gid & 7;
  double a = 0;
  if (row < n) {
    const int ks = rowptr[row], ke = rowptr[row + 1];
    for (int k = ks + l; k < ke; k += 8) {
      const int j = col[k];
      a += val[k] * (MODE == 1 ? dinv[j] * rin[j] * itheta : dold[j]);
    }
  }
  a = group8_sum(a);
  if (row < n && l == 0) {
    const double di = dinv[row], ri = rin[row];
    const double dd = (MODE == 1) ? di * ri * itheta : dold[row];
    const double r = ri - a;
    const double dn = c1 * dd + c2 * di * r;
    if (!LAST) { rout[row] = r; dnew[row] = dn; }
    if (MODE == 0) x[row] += dn;
    else if (MODE == 1) x[row] = dd + dn;
    else x[row] += dd + dn;
  }
}

// r = b - A x ; d0 = D^-1 r / theta   (residual of a non-zero guess fused with the Chebyshev initialisation)
__global__ __launch_bounds__(TPB) void csr_resid_init_kernel(int n, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                             const double *__restrict__ val, const double *__restrict__ dinv,
                                                             const double *__restrict__ b, const double *__restrict__ x,
                                                             double *__restrict__ r, double *__restrict__ d0, double itheta) {
  const int gid = blockIdx.x * TPB + threadIdx.x;
  const int row = gid >> 3, l = gid & 7;
  double a = 0;
  if (row < n) {
    const int ks = rowptr[row], ke = rowptr[row + 1];
    for (int k = ks + l; k < ke; k += 8) a += val[k] * x[col[k]];
  }
  a = group8_sum(a);
  if (row < n && l == 0) {
    const double rr = b[row] - a;
    r[row] = rr;
    d0[row] = dinv[row] * rr * itheta;
  }
}

// Chebyshev smoothing with the level operator (ncol = 1): zero_guess ? x = S b : x <- x + S (b - A x)
static int level_cheb(cfdh_ctx *c, AmgLevel *L, const double *b, double *x, bool zero_guess, int deg, bool prof) {
  const int n = L->n;
  const double theta = 0.5 * (L->lmax + L->lmin), delta = 0.5 * (L->lmax - L->lmin), sigma = theta / delta;
  double rho = 1.0 / sigma;
  double *dold = L->d0.p, *dnew = L->d1.p, *r = L->r.p;
  const double *rin = b;
  const double itheta = 1.0 / theta;
  const long long nthreads = 8ll * n;
  dim3 grid((unsigned)((nthreads + TPB - 1) / TPB)), block(TPB);
  const int *rp = L->A.rowptr.p, *cl = L->A.col.p;
  const double *vl = L->A.val.p, *di = L->dinv.p;
  if (deg == 1) {  // plain damped Jacobi
    if (!zero_guess) { CHK(k_csr_spmv(c, L->A, x, r, 1, b)); rin = r; }
    return k_cheb_init(c, n, di, rin, dold, x, itheta, zero_guess ? 0 : 1, nullptr);
  }
  if (!zero_guess) {
    hipLaunchKernelGGL(csr_resid_init_kernel, grid, block, 0, c->stream, n, rp, cl, vl, di, b, x, r, dold, itheta);
    rin = r;
  }
  for (int k = 1; k < deg; k++) {
    const double rho_new = 1.0 / (2.0 * sigma - rho);
    const double c1 = rho_new * rho, c2 = 2.0 * rho_new / delta;
    const bool last = (k == deg - 1);
    const int mode = (k == 1) ? (zero_guess ? 1 : 2) : 0;
    if (prof) prof_begin(c, 4);
#define LAUNCH_STEP(M, LST) hipLaunchKernelGGL((cheb_csr_step_kernel<M, LST>), grid, block, 0, c->stream, n, rp, cl, vl, di, rin, r, dold, dnew, x, c1, c2, itheta)
    if (mode == 1) { if (last) LAUNCH_STEP(1, true); else LAUNCH_STEP(1, false); }
    else if (mode == 2) { if (last) LAUNCH_STEP(2, true); else LAUNCH_STEP(2, false); }
    else { if (last) LAUNCH_STEP(0, true); else LAUNCH_STEP(0, false); }
#undef LAUNCH_STEP
    if (prof) prof_end(c, 4);
    rin = r;
    std::swap(dold, dnew);
    rho = rho_new;
  }
  HIPCHK(c, hipGetLastError());
  return 0;
}
int k_level_smooth(cfdh_ctx *c, AmgLevel *L, const double *b, double *x, int degree) { return level_cheb(c, L, b, x, true, degree, false); }

// Two Chebyshev steps from a zero guess on a SELL-64 level in ONE pass over the matrix, with the
// Cahouet-Chabard scaling fused:  d = w D^-1 b ; r = b - A d ; x = d + (c1 d + c2 D^-1 r) ; y = ml .* x.
// (svalw carries the column weights w D^-1, as in the Jacobi pre-sweep.)
// HEAD: the matrix through its head copy (hcol, hval, hlen, wh: CsrDev::hcol ...)
template <bool HEAD>
__global__ __launch_bounds__(TPB) void sell_cheb2_scale_kernel(int n, const int *__restrict__ sptr, const int *__restrict__ scol,
                                                               const float *__restrict__ svalw, const int *__restrict__ hcol,
                                                               const float *__restrict__ hval, const unsigned short *__restrict__ hlen, int wh,
                                                               const double *__restrict__ wdinv,
                                                               const double *__restrict__ dinv, const double *__restrict__ b,
                                                               double *__restrict__ x, const double *__restrict__ ml,
                                                               double *__restrict__ y, double c1, double c2) {
  const int row = blockIdx.x * TPB + threadIdx.x;
  if (row >= n) return;
  const int sl = row >> 6, lane = row & 63;
  const double a = HEAD ? sell_row_dot_head<10, double>(sptr, scol, svalw, hcol, hval, hlen, wh, b, sl, lane, 0.0)
                        : sell_row_dot<10, double>(sptr, scol, svalw, b, sl, lane, 0.0);
  const double bi = b[row];
  const double dd = wdinv[row] * bi;
  const double xv = dd + (c1 * dd + c2 * dinv[row] * (bi - a));
  x[row] = xv;
  y[row] = ml[row] * xv;
}
// x = Cheb2(H) b and y = ml .* x; false when the level does not qualify (the caller takes the generic path)
bool k_cc_cheb2_scale(cfdh_ctx *c, AmgLevel *L, const double *b, double *x, const double *ml, double *y) {
  const int n = L->n;
  if (!(cfdh_cheb2_sell(L->A.nnz, n) && L->A.has_sell_weighted())) return false;
  const double theta = 0.5 * (L->lmax + L->lmin), delta = 0.5 * (L->lmax - L->lmin), sigma = theta / delta;
  const double rho = 1.0 / sigma, rho_new = 1.0 / (2.0 * sigma - rho);
  const double c1 = rho_new * rho, c2 = 2.0 * rho_new / delta;
  const CsrDev &A = L->A;
  if (A.head_w > 0)
    hipLaunchKernelGGL(sell_cheb2_scale_kernel<true>, dim3((n + TPB - 1) / TPB), dim3(TPB), 0, c->stream, n, A.sptr.p, A.scol.p, A.svalw.p,
                       A.hcol.p, A.hvalf.p, A.hlen.p, A.head_w, L->wdinv.p, L->dinv.p, b, x, ml, y, c1, c2);
  else
    hipLaunchKernelGGL(sell_cheb2_scale_kernel<false>, dim3((n + TPB - 1) / TPB), dim3(TPB), 0, c->stream, n, A.sptr.p, A.scol.p, A.svalw.p,
                       (const int *)nullptr, (const float *)nullptr, (const unsigned short *)nullptr, 0, L->wdinv.p, L->dinv.p, b, x, ml, y, c1, c2);
  return hipGetLastError() == hipSuccess;
}

// y = Minv b for the dense coarsest inverse: one wave per row
template <typename T>
__global__ __launch_bounds__(64) void dense_mv_kernel(int n, const double *__restrict__ Minv, const T *__restrict__ b,
                                                      T *__restrict__ y) {
  const int row = blockIdx.x, l = threadIdx.x;
  T a = vzero((const T *)nullptr);
  for (int k = l; k < n; k += 64) a = vfma(Minv[(size_t)row * n + k], b[k], a);
  a = wsum(a);
  if (l == 0) y[row] = a;
}

// damped-Jacobi V-cycle building blocks: each touches the level matrix once.  A row whose only entry is
// its diagonal (Dirichlet row, isolated unknown) is solved exactly (weight 1 instead of 1/theta).
//   pre : xa = w D^-1 b (formed while gathering) ; r = b - A xa
//   post: x_out = x_in + w D^-1 (b - A x_in)
template <typename T>
__global__ __launch_bounds__(TPB) void jacobi_pre_kernel(int n, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                         const double *__restrict__ val, const double *__restrict__ wdinv,
                                                         const T *__restrict__ b, T *__restrict__ xa, T *__restrict__ r) {
  const int gid = blockIdx.x * TPB + threadIdx.x;
  const int row = gid >> 3, l = gid & 7;
  T a = vzero((const T *)nullptr);
  if (row < n) {
    const int ks = rowptr[row], ke = rowptr[row + 1];
    for (int k = ks + l; k < ke; k += 8) {
      const int j = col[k];
      a = vfma(val[k] * wdinv[j], b[j], a);
    }
  }
  a = g8(a);
  if (row < n && l == 0) {
    const T bi = b[row];
    xa[row] = vscale(wdinv[row], bi);
    r[row] = vsub(bi, a);
  }
}
template <typename T>
__global__ __launch_bounds__(TPB) void jacobi_post_kernel(int n, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                          const double *__restrict__ val, const double *__restrict__ wdinv,
                                                          const T *__restrict__ b, const T *__restrict__ xin,
                                                          T *__restrict__ xout) {
  const int gid = blockIdx.x * TPB + threadIdx.x;
  const int row = gid >> 3, l = gid & 7;
  T a = vzero((const T *)nullptr);
  if (row < n) {
    const int ks = rowptr[row], ke = rowptr[row + 1];
    for (int k = ks + l; k < ke; k += 8) a = vfma(val[k], xin[col[k]], a);
  }
  a = g8(a);
  if (row < n && l == 0) {
    xout[row] = vadd(xin[row], vscale(wdinv[row], vsub(b[row], a)));
  }
}

// ---- SELL-64 variants: one lane per row, fully coalesced matrix stream, no cross-lane reduction
template <int MODE, typename T>
__global__ __launch_bounds__(TPB) void sell_spmv_kernel(int n, const int *__restrict__ sptr, const int *__restrict__ scol,
                                                        const float *__restrict__ sval, const T *__restrict__ x,
                                                        T *__restrict__ y, const T *__restrict__ b) {
  const int row = blockIdx.x * TPB + threadIdx.x;
  if (row >= n) return;
  const int sl = row >> 6, lane = row & 63;
  const int p0 = sptr[sl], w = (sptr[sl + 1] - p0) >> 6;
  T a = vzero((const T *)nullptr);
#pragma unroll 4
  for (int k = 0; k < w; k++) {
    const int p = p0 + k * 64 + lane;
    a = vfma((double)sval[p], x[scol[p]], a);
  }
  if (MODE == 0) y[row] = a;
  else if (MODE == 1) y[row] = vsub(b[row], a);
  else if (MODE == 2) y[row] = vadd(y[row], a);
  else y[row] = vadd(b[row], a);
}
template <typename T>
__global__ __launch_bounds__(TPB) void sell_jacobi_pre_kernel(int n, const int *__restrict__ sptr, const int *__restrict__ scol,
                                                              const float *__restrict__ svalw, const double *__restrict__ wdinv,
                                                              const T *__restrict__ b, T *__restrict__ xa, T *__restrict__ r) {
  const int row = blockIdx.x * TPB + threadIdx.x;
  if (row >= n) return;
  const int sl = row >> 6, lane = row & 63;
  const int p0 = sptr[sl], w = (sptr[sl + 1] - p0) >> 6;
  T a = vzero((const T *)nullptr);
#pragma unroll 4
  for (int k = 0; k < w; k++) {
    const int p = p0 + k * 64 + lane;
    a = vfma((double)svalw[p], b[scol[p]], a);   // A (w D^-1 b): the column weight is folded into svalw
  }
  const T bi = b[row];
  xa[row] = vscale(wdinv[row], bi);
  r[row] = vsub(bi, a);
}
template <typename T>
__global__ __launch_bounds__(TPB) void sell_jacobi_post_kernel(int n, const int *__restrict__ sptr, const int *__restrict__ scol,
                                                               const float *__restrict__ sval, const double *__restrict__ wdinv,
                                                               const T *__restrict__ b, const T *__restrict__ xin,
                                                               T *__restrict__ xout) {
  const int row = blockIdx.x * TPB + threadIdx.x;
  if (row >= n) return;
  const int sl = row >> 6, lane = row & 63;
  const int p0 = sptr[sl], w = (sptr[sl + 1] - p0) >> 6;
  T a = vzero((const T *)nullptr);
#pragma unroll 4
  for (int k = 0; k < w; k++) {
    const int p = p0 + k * 64 + lane;
    a = vfma((double)sval[p], xin[scol[p]], a);
  }
  xout[row] = vadd(xin[row], vscale(wdinv[row], vsub(b[row], a)));
}

// The three sweeps of a level on n rows, each through SELL-64 (one lane per row) when the size rule asked for it (`sell`) and
// the operator has the copy, through CSR (8 lanes per row) otherwise.
//   pre : xa = W b ; r = b - A xa
template <typename T>
static void launch_jacobi_pre(cfdh_ctx *c, const CsrDev &A, bool sell, int n, const double *wdinv, const T *b, T *xa, T *r) {
  dim3 block(TPB), gridS((unsigned)((n + TPB - 1) / TPB)), gridC((unsigned)((8ll * n + TPB - 1) / TPB));
  if (cfdh_pre_takes_sell(A, sell))
    hipLaunchKernelGGL((sell_jacobi_pre_kernel<T>), gridS, block, 0, c->stream, n, A.sptr.p, A.scol.p, A.svalw.p, wdinv, b, xa, r);
  else
    hipLaunchKernelGGL((jacobi_pre_kernel<T>), gridC, block, 0, c->stream, n, A.rowptr.p, A.col.p, A.val.p, wdinv, b, xa, r);
}
//   post: x = x1 + W (b - A x1)
template <typename T>
static void launch_jacobi_post(cfdh_ctx *c, const CsrDev &A, bool sell, int n, const double *wdinv, const T *b, const T *x1, T *x) {
  dim3 block(TPB), gridS((unsigned)((n + TPB - 1) / TPB)), gridC((unsigned)((8ll * n + TPB - 1) / TPB));
  if (cfdh_post_takes_sell(A, sell))
    hipLaunchKernelGGL((sell_jacobi_post_kernel<T>), gridS, block, 0, c->stream, n, A.sptr.p, A.scol.p, A.sval.p, wdinv, b, x1, x);
  else
    hipLaunchKernelGGL((jacobi_post_kernel<T>), gridC, block, 0, c->stream, n, A.rowptr.p, A.col.p, A.val.p, wdinv, b, x1, x);
}
//   y = b + P x  (n = rows of P)
template <typename T>
static void launch_prolong_add(cfdh_ctx *c, const CsrDev &P, bool sell, int n, const T *x, T *y, const T *b) {
  dim3 block(TPB), gridS((unsigned)((n + TPB - 1) / TPB)), gridC((unsigned)((8ll * n + TPB - 1) / TPB));
  if (cfdh_prolong_takes_sell(P, sell))
    hipLaunchKernelGGL((sell_spmv_kernel<3, T>), gridS, block, 0, c->stream, n, P.sptr.p, P.scol.p, P.sval.p, x, y, b);
  else
    hipLaunchKernelGGL((csr_spmv_kernel<3, T>), gridC, block, 0, c->stream, n, P.rowptr.p, P.col.p, P.val.p, x, y, b);
}

template <typename T>
static int amg_cycle_jacobi(cfdh_ctx *c, AmgHier &H, size_t lev, const T *b, T *x, int prof) {
  AmgLevel *L = H.lev[lev];
  if (lev + 1 == H.lev.size()) {
    if (H.coarse_n > 0) {
      hipLaunchKernelGGL((dense_mv_kernel<T>), dim3(H.coarse_n), dim3(64), 0, c->stream, H.coarse_n, H.coarse_inv.p, b, x);
    } else {
      // near-diagonal coarsest level (coarsening stalled, cfdh_amg_setup): two damped-Jacobi sweeps
      const int n = L->n;
      T *xa = (T *)L->d0.p, *r = (T *)L->r.p;
      launch_jacobi_pre<T>(c, L->A, false, n, L->wdinv.p, b, xa, r);
      launch_jacobi_post<T>(c, L->A, false, n, L->wdinv.p, b, (const T *)xa, x);
    }
    HIPCHK(c, hipGetLastError());
    return 0;
  }
  AmgLevel *N = H.lev[lev + 1];
  const int n = L->n;
  const bool sell = cfdh_sweep_sell(L->A.nnz, n);  // A and P alike
  T *xa = (T *)L->d0.p, *x1 = (T *)L->d1.p, *r = (T *)L->r.p;
  if (prof && lev == 0) prof_begin(c, prof);
  launch_jacobi_pre<T>(c, L->A, sell, n, L->wdinv.p, b, xa, r);
  if (prof && lev == 0) prof_end(c, prof);
  CHK(csr_spmv_t<T>(c, L->R, r, (T *)N->b.p, 0, (const T *)nullptr));   // b_c = R r
  CHK(amg_cycle_jacobi<T>(c, H, lev + 1, (const T *)N->b.p, (T *)N->x.p, prof));
  launch_prolong_add<T>(c, L->P, sell, n, (const T *)N->x.p, x1, (const T *)xa);  // x1 = xa + P x_c
  HIPCHK(c, hipGetLastError());
  if (prof && lev == 0) prof_begin(c, prof);
  launch_jacobi_post<T>(c, L->A, sell, n, L->wdinv.p, b, (const T *)x1, x);
  if (prof && lev == 0) prof_end(c, prof);
  HIPCHK(c, hipGetLastError());
  return 0;
}

// ---- fused V(1,1) Jacobi cycle: one kernel per level and direction on precomputed composite operators
// (AmgLevel::G / Sb / Sc / D, built in cfdh_amg_setup).  Same linear map as amg_cycle_jacobi.
template <int LPR>
__device__ __forceinline__ double lpr_sum(double v) {
  v = group8_sum(v);
  if (LPR >= 16) v += dpp_shuffle<0x140>(v);  // row_mirror: sums of 16
  if (LPR >= 32) v += __shfl_xor(v, 16);
  if (LPR >= 64) v += __shfl_xor(v, 32);
  return v;
}
template <int LPR> __device__ __forceinline__ double lsum(double v) { return lpr_sum<LPR>(v); }
template <int LPR> __device__ __forceinline__ double2 lsum(double2 v) { return make_double2(lpr_sum<LPR>(v.x), lpr_sum<LPR>(v.y)); }
template <int LPR> __device__ __forceinline__ d3 lsum(d3 v) { return d3{lpr_sum<LPR>(v.x), lpr_sum<LPR>(v.y), lpr_sum<LPR>(v.z)}; }

__device__ __forceinline__ double epi_apply(double acc, int row, double alpha, double beta, const double *zH, const double *r, const unsigned char *pbc) {
  return (pbc[row] & 1) ? r[row] : alpha * acc + beta * zH[row];
}
__device__ __forceinline__ double2 epi_apply(double2 acc, int, double, double, const double *, const double *, const unsigned char *) { return acc; }
__device__ __forceinline__ double epi_value(double acc, unsigned flag, double alpha, double beta, double zh, double r) { return (flag & 1u) ? r : alpha * acc + beta * zh; }
__device__ __forceinline__ double2 epi_value(double2 acc, unsigned, double, double, double, double) { return acc; }
__device__ __forceinline__ d3 epi_apply(d3 acc, int, double, double, const double *, const double *, const unsigned char *) { return acc; }
__device__ __forceinline__ d3 epi_value(d3 acc, unsigned, double, double, double, double) { return acc; }

// y = G x, LPR lanes per row (rows of the coarse level: tens to hundreds of entries)
template <int LPR, typename VT, typename T>
__global__ __launch_bounds__(TPB) void fused_down_kernel(int n, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                         const VT *__restrict__ val, const T *__restrict__ x, T *__restrict__ y) {
  const int gid = blockIdx.x * TPB + threadIdx.x;
  const int row = gid / LPR, l = gid % LPR;
  T a = vzero((const T *)nullptr);
  if (row < n) {
    const int ks = rowptr[row], ke = rowptr[row + 1];
    // up to four entries per lane with all loads in flight together, then the gathers (see sell_row_dot).  The loads are
    // unconditional, a lane past the end of its row re-reading the row's last entry (the same cache line as its neighbours'), and
    // only the sums are guarded: with the loads under k < ke the compiler kept cidx / cval as register tuples, copied them after
    // the first pair of loads and so waited for that pair before it requested the other three -- a fourth dependent round trip.
    if (ks < ke) {
      int cidx[4];
      VT cval[4];
#pragma unroll
      for (int q = 0; q < 4; q++) { const int k = min(ks + l + q * LPR, ke - 1); cidx[q] = col[k]; cval[q] = val[k]; }
      T g[4];
#pragma unroll
      for (int q = 0; q < 4; q++) g[q] = x[cidx[q]];
#pragma unroll
      for (int q = 0; q < 4; q++) { const T t = vfma((double)cval[q], g[q], a); if (ks + l + q * LPR < ke) a = t; }
    }
    for (int k = ks + l + 4 * LPR; k < ke; k += LPR) a = vfma((double)val[k], x[col[k]], a);
  }
  a = lsum<LPR>(a);
  if (row < n && l == 0) y[row] = a;
}
// x = Sb b + Sc xc  (Sc may be absent: smoothing-only coarsest level), 8 lanes per row over CSR
template <typename T>
__global__ __launch_bounds__(TPB) void fused_up_csr_kernel(int n, const int *__restrict__ rpB, const int *__restrict__ clB,
                                                           const double *__restrict__ vlB, const T *__restrict__ b,
                                                           const int *__restrict__ rpC, const int *__restrict__ clC,
                                                           const double *__restrict__ vlC, const T *__restrict__ xc,
                                                           T *__restrict__ x, double ea, double eb, const double *__restrict__ ezH,
                                                           const double *__restrict__ er, const unsigned char *__restrict__ epbc) {
  const int gid = blockIdx.x * TPB + threadIdx.x;
  const int row = gid >> 3, l = gid & 7;
  T a = vzero((const T *)nullptr);
  if (row < n) {
    // two entries of each matrix per lane requested together, then their gathers (rows of 10-30 entries on the coarse levels:
    // the plain loops make two to four dependent round trips per matrix)
    const int kb = rpB[row] + l, keB = rpB[row + 1];
    int kc = 0, keC = 0;
    if (rpC) { kc = rpC[row] + l; keC = rpC[row + 1]; }
    int cb[2], cc[2];
    double vb[2], vc[2];
#pragma unroll
    for (int q = 0; q < 2; q++) {
      if (kb + 8 * q < keB) { cb[q] = clB[kb + 8 * q]; vb[q] = vlB[kb + 8 * q]; }
      if (kc + 8 * q < keC) { cc[q] = clC[kc + 8 * q]; vc[q] = vlC[kc + 8 * q]; }
    }
    T gb[2], gc[2];
#pragma unroll
    for (int q = 0; q < 2; q++) {
      if (kb + 8 * q < keB) gb[q] = b[cb[q]];
      if (kc + 8 * q < keC) gc[q] = xc[cc[q]];
    }
#pragma unroll
    for (int q = 0; q < 2; q++) {
      if (kb + 8 * q < keB) a = vfma(vb[q], gb[q], a);
      if (kc + 8 * q < keC) a = vfma(vc[q], gc[q], a);
    }
    for (int k = kb + 16; k < keB; k += 8) a = vfma(vlB[k], b[clB[k]], a);
    for (int k = kc + 16; k < keC; k += 8) a = vfma(vlC[k], xc[clC[k]], a);
  }
  a = g8(a);
  if (row < n && l == 0) x[row] = epbc ? epi_apply(a, row, ea, eb, ezH, er, epbc) : a;
}
// the same on SELL-64 (fp32 values), one lane per row.  WIDE: rows longer than one chunk of preloaded entries (tetrahedra)
template <typename T, bool WIDE>
__global__ __launch_bounds__(TPB) void fused_up_sell_kernel(int n, const int *__restrict__ spB, const int *__restrict__ scB,
                                                            const float *__restrict__ svB, const T *__restrict__ b,
                                                            const int *__restrict__ spC, const int *__restrict__ scC,
                                                            const float *__restrict__ svC, const T *__restrict__ xc,
                                                            T *__restrict__ x, double ea, double eb, const double *__restrict__ ezH,
                                                            const double *__restrict__ er, const unsigned char *__restrict__ epbc) {
  const int row = blockIdx.x * TPB + threadIdx.x;
  if (row >= n) return;
  const int sl = __builtin_amdgcn_readfirstlane(row >> 6), lane = row & 63;
  T a = vzero((const T *)nullptr);
  // operands of the epilogue: requested now, so that they arrive together with the matrix data
  double e_zh = 0.0, e_r = 0.0;
  unsigned e_f = 0;
  if (epbc) { e_f = epbc[row]; e_zh = ezH[row]; e_r = er[row]; }
  // both matrices together: slice pointers, then ALL column/value loads of a chunk of the row, then ALL its gathers (three
  // dependent round trips; the straightforward loops make about ten).  Triangle meshes need one chunk (rows of <= 10
  // entries), the 15- to 25-entry rows of tetrahedral meshes two or three.
  constexpr int MW = sizeof(T) > 8 ? 8 : 10;
  const int pB = spB[sl], wB = (spB[sl + 1] - pB) >> 6;
  int pC = 0, wC = 0;
  if (spC) { pC = spC[sl]; wC = (spC[sl + 1] - pC) >> 6; }
  const int wmax = wB > wC ? wB : wC;
  for (int k0 = 0; k0 < (WIDE ? wmax : 1); k0 += MW) {
    int cB[MW], cC[MW];
    float vB[MW], vC[MW];
#pragma unroll
    for (int k = 0; k < MW; k++) if (k0 + k < wB) { const int p = pB + (k0 + k) * 64 + lane; cB[k] = NTLOAD(scB + p); vB[k] = NTLOAD(svB + p); }
#pragma unroll
    for (int k = 0; k < MW; k++) if (k0 + k < wC) { const int p = pC + (k0 + k) * 64 + lane; cC[k] = NTLOAD(scC + p); vC[k] = NTLOAD(svC + p); }
    T gB[MW], gC[MW];
#pragma unroll
    for (int k = 0; k < MW; k++) if (k0 + k < wB) gB[k] = b[cB[k]];
#pragma unroll
    for (int k = 0; k < MW; k++) if (k0 + k < wC) gC[k] = xc[cC[k]];
#pragma unroll
    for (int k = 0; k < MW; k++) if (k0 + k < wB) a = vfma((double)vB[k], gB[k], a);
#pragma unroll
    for (int k = 0; k < MW; k++) if (k0 + k < wC) a = vfma((double)vC[k], gC[k], a);
  }
  if (!WIDE) {  // rows beyond the chunk (none on triangle meshes)
    for (int k = MW; k < wB; k++) { const int p = pB + k * 64 + lane; a = vfma((double)svB[p], b[scB[p]], a); }
    for (int k = MW; k < wC; k++) { const int p = pC + k * 64 + lane; a = vfma((double)svC[p], xc[scC[p]], a); }
  }
  x[row] = epbc ? epi_value(a, e_f, ea, eb, e_zh, e_r) : a;
}
// The same through the head copies of Sb and Sc (whB, whC <= MW entries per row; whC = 0 and spC = nullptr: no Sc).  The first chunk
// is requested from the slice index alone; the operands of the epilogue are requested behind it, so that nothing stands between
// the kernel's entry and the matrix stream.  Chunks beyond the first (WIDE) and rows beyond the chunk go through the pointers.
template <typename T, bool WIDE>
__global__ __launch_bounds__(TPB) void fused_up_sell_head_kernel(int n, const int *__restrict__ spB, const int *__restrict__ scB,
                                                                 const float *__restrict__ svB, const int *__restrict__ hcB,
                                                                 const float *__restrict__ hvB, const unsigned short *__restrict__ hlB, int whB,
                                                                 const T *__restrict__ b, const int *__restrict__ spC,
                                                                 const int *__restrict__ scC, const float *__restrict__ svC,
                                                                 const int *__restrict__ hcC, const float *__restrict__ hvC,
                                                                 const unsigned short *__restrict__ hlC, int whC, const T *__restrict__ xc,
                                                                 T *__restrict__ x, double ea, double eb, const double *__restrict__ ezH,
                                                                 const double *__restrict__ er, const unsigned char *__restrict__ epbc) {
  const int row = blockIdx.x * TPB + threadIdx.x;
  if (row >= n) return;
  const int sl = __builtin_amdgcn_readfirstlane(row >> 6), lane = row & 63;
  T a = vzero((const T *)nullptr);
  constexpr int MW = sizeof(T) > 8 ? 8 : 10;
  // The first chunk lives in named scalars, not arrays: an entry is written in one of two places (head or tail), and the
  // compiler keeps such an array as ONE register tuple that it copies -- and therefore waits for -- after the first load.
#define UPH_ALL(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9)
#define UPH_DECL(k) int cB##k = 0, cC##k = 0; float vB##k = 0.0f, vC##k = 0.0f;
#define UPH_HEAD_B(k) if (k < MW && k < whB) { cB##k = NTLOAD(hcB + hB0 + k * 64); vB##k = NTLOAD(hvB + hB0 + k * 64); }
#define UPH_HEAD_C(k) if (k < MW && k < whC) { cC##k = NTLOAD(hcC + hC0 + k * 64); vC##k = NTLOAD(hvC + hC0 + k * 64); }
#define UPH_TAIL_B(k) if (k < MW && k >= whB && k < wB) { const int p = pB + k * 64 + lane; cB##k = NTLOAD(scB + p); vB##k = NTLOAD(svB + p); }
#define UPH_TAIL_C(k) if (k < MW && k >= whC && k < wC) { const int p = pC + k * 64 + lane; cC##k = NTLOAD(scC + p); vC##k = NTLOAD(svC + p); }
#define UPH_DECL_G(k) T gB##k = vzero((const T *)nullptr), gC##k = vzero((const T *)nullptr);
#define UPH_GATHER_B(k) if (k < MW && k < wB) gB##k = b[cB##k];
#define UPH_GATHER_C(k) if (k < MW && k < wC) gC##k = xc[cC##k];
#define UPH_FMA_B(k) if (k < MW && k < wB) a = vfma((double)vB##k, gB##k, a);
#define UPH_FMA_C(k) if (k < MW && k < wC) a = vfma((double)vC##k, gC##k, a);
  UPH_ALL(UPH_DECL)
  const size_t hB0 = (size_t)sl * whB * 64 + lane, hC0 = (size_t)sl * whC * 64 + lane;
  UPH_ALL(UPH_HEAD_B)
  UPH_ALL(UPH_HEAD_C)
  // lengths and pointers: scalar loads, in flight together with the head (and before the epilogue's operands, whose flag the
  // compiler waits for where it is requested)
  const int wB = head_slice_len(hlB, sl), pB = spB[sl];
  int pC = 0, wC = 0;
  if (spC) { wC = head_slice_len(hlC, sl); pC = spC[sl]; }
  double e_zh = 0.0, e_r = 0.0;
  unsigned e_f = 0;
  if (epbc) { e_f = epbc[row]; e_zh = ezH[row]; e_r = er[row]; }
  // the tail inside the first chunk (slices wider than the head)
  UPH_ALL(UPH_TAIL_B)
  UPH_ALL(UPH_TAIL_C)
  {
    UPH_ALL(UPH_DECL_G)
    UPH_ALL(UPH_GATHER_B)
    UPH_ALL(UPH_GATHER_C)
    UPH_ALL(UPH_FMA_B)
    UPH_ALL(UPH_FMA_C)
  }
#undef UPH_ALL
#undef UPH_DECL
#undef UPH_HEAD_B
#undef UPH_HEAD_C
#undef UPH_TAIL_B
#undef UPH_TAIL_C
#undef UPH_DECL_G
#undef UPH_GATHER_B
#undef UPH_GATHER_C
#undef UPH_FMA_B
#undef UPH_FMA_C
  if (WIDE) {
    const int wmax = wB > wC ? wB : wC;
    int cB[MW], cC[MW];
    float vB[MW], vC[MW];
    for (int k0 = MW; k0 < wmax; k0 += MW) {
#pragma unroll
      for (int k = 0; k < MW; k++) if (k0 + k < wB) { const int p = pB + (k0 + k) * 64 + lane; cB[k] = NTLOAD(scB + p); vB[k] = NTLOAD(svB + p); }
#pragma unroll
      for (int k = 0; k < MW; k++) if (k0 + k < wC) { const int p = pC + (k0 + k) * 64 + lane; cC[k] = NTLOAD(scC + p); vC[k] = NTLOAD(svC + p); }
      T gB[MW], gC[MW];
#pragma unroll
      for (int k = 0; k < MW; k++) if (k0 + k < wB) gB[k] = b[cB[k]];
#pragma unroll
      for (int k = 0; k < MW; k++) if (k0 + k < wC) gC[k] = xc[cC[k]];
#pragma unroll
      for (int k = 0; k < MW; k++) if (k0 + k < wB) a = vfma((double)vB[k], gB[k], a);
#pragma unroll
      for (int k = 0; k < MW; k++) if (k0 + k < wC) a = vfma((double)vC[k], gC[k], a);
    }
  } else {
    for (int k = MW; k < wB; k++) { const int p = pB + k * 64 + lane; a = vfma((double)svB[p], b[scB[p]], a); }
    for (int k = MW; k < wC; k++) { const int p = pC + k * 64 + lane; a = vfma((double)svC[p], xc[scC[p]], a); }
  }
  x[row] = epbc ? epi_value(a, e_f, ea, eb, e_zh, e_r) : a;
}
// x = Sb b + D bc with the dense folded coarse correction D [n][nc] (fp32), one wave per row
template <typename T>
__global__ __launch_bounds__(TPB) void fused_up_dense_kernel(int n, const int *__restrict__ rpB, const int *__restrict__ clB,
                                                             const double *__restrict__ vlB, const T *__restrict__ b,
                                                             const float *__restrict__ D, int nc, const T *__restrict__ bc,
                                                             T *__restrict__ x) {
  const int gid = blockIdx.x * TPB + threadIdx.x;
  const int row = gid >> 6, l = gid & 63;
  T a = vzero((const T *)nullptr);
  if (row < n) {
    for (int k = rpB[row] + l, ke = rpB[row + 1]; k < ke; k += 64) a = vfma(vlB[k], b[clB[k]], a);
    const float *Dr = D + (size_t)row * nc;
    // the whole row in flight at once when it fits 12 steps (coarsest levels of <= 768 unknowns), remainder in a loop
    float dv[12];
    T bv[12];
#pragma unroll
    for (int q = 0; q < 12; q++) { const int j = l + 64 * q; if (j < nc) { dv[q] = Dr[j]; bv[q] = bc[j]; } }
#pragma unroll
    for (int q = 0; q < 12; q++) { const int j = l + 64 * q; if (j < nc) a = vfma((double)dv[q], bv[q], a); }
    for (int j = l + 768; j < nc; j += 64) a = vfma((double)Dr[j], bc[j], a);
  }
  a = wsum(a);
  if (row < n && l == 0) x[row] = a;
}

// x = Sb b (+ Sc xc) on nrow rows over SELL-64: through the head copies when every operator involved has one, the pointers otherwise
template <typename T, bool WIDE>
static void launch_up_sell(cfdh_ctx *c, int nrow, const CsrDev &Sb, const T *b, const CsrDev *Sc, const T *xc, T *x, double ea, double eb,
                           const double *ezH, const double *er, const unsigned char *epbc) {
  constexpr int MW = sizeof(T) > 8 ? 8 : 10;
  const dim3 grid((unsigned)((nrow + TPB - 1) / TPB)), block(TPB);
  const int *spC = Sc ? Sc->sptr.p : nullptr, *scC = Sc ? Sc->scol.p : nullptr;
  const float *svC = Sc ? Sc->sval.p : nullptr;
  const auto has_head = [](const CsrDev &M) { return M.head_w > 0 && M.head_w <= MW; };
  if (has_head(Sb) && (!Sc || has_head(*Sc)))
    hipLaunchKernelGGL((fused_up_sell_head_kernel<T, WIDE>), grid, block, 0, c->stream, nrow, Sb.sptr.p, Sb.scol.p, Sb.sval.p, Sb.hcol.p,
                       Sb.hvalf.p, Sb.hlen.p, Sb.head_w, b, spC, scC, svC, Sc ? Sc->hcol.p : (const int *)nullptr,
                       Sc ? Sc->hvalf.p : (const float *)nullptr, Sc ? Sc->hlen.p : (const unsigned short *)nullptr, Sc ? Sc->head_w : 0, xc,
                       x, ea, eb, ezH, er, epbc);
  else
    hipLaunchKernelGGL((fused_up_sell_kernel<T, WIDE>), grid, block, 0, c->stream, nrow, Sb.sptr.p, Sb.scol.p, Sb.sval.p, b, spC, scC, svC, xc,
                       x, ea, eb, ezH, er, epbc);
}

template <typename VT, typename T>
static void launch_down(cfdh_ctx *c, const CsrDev &G, const VT *val, const T *x, T *y) {
  const int lpr = cfdh_down_lpr(G);  // 2-4 entries per lane, loaded together
  dim3 block(TPB), grid((unsigned)(((long long)G.n * lpr + TPB - 1) / TPB));
  if (lpr == 64) hipLaunchKernelGGL((fused_down_kernel<64, VT, T>), grid, block, 0, c->stream, G.n, G.rowptr.p, G.col.p, val, x, y);
  else if (lpr == 32) hipLaunchKernelGGL((fused_down_kernel<32, VT, T>), grid, block, 0, c->stream, G.n, G.rowptr.p, G.col.p, val, x, y);
  else if (lpr == 16) hipLaunchKernelGGL((fused_down_kernel<16, VT, T>), grid, block, 0, c->stream, G.n, G.rowptr.p, G.col.p, val, x, y);
  else hipLaunchKernelGGL((fused_down_kernel<8, VT, T>), grid, block, 0, c->stream, G.n, G.rowptr.p, G.col.p, val, x, y);
}

template <typename T>
// l0 > 0: the cycle of the levels l0 .. (the replicated levels of a partitioned run below its distributed finest pressure level);
// b / x are then level l0's vectors
static int amg_cycle_fused(cfdh_ctx *c, AmgHier &H, const T *b, T *x, int prof, int l0 = 0) {
  const int nl = (int)H.lev.size();
  // down: right-hand sides of all coarse levels.  (Merging the coarse levels' down-sweeps into one launch through the
  // products G_2 G_1, ... was measured and dropped: the products fill in -- 1.1 M entries for a 713-row level -- and the one
  // launch costs more than the two it replaces.)
  for (int l = l0; l + 1 < nl; l++) {
    AmgLevel *L = H.lev[l], *N = H.lev[l + 1];
    const T *src = l == l0 ? b : (const T *)L->b.p;
    if (prof && l == 0) prof_begin(c, prof + 4);
    if (L->fine) launch_down<float, T>(c, L->G, L->G.valf.p, src, (T *)N->b.p);
    else launch_down<double, T>(c, L->G, L->G.val.p, src, (T *)N->b.p);
    if (prof && l == 0) prof_end(c, prof + 4);
  }
  // coarsest level (or the level above it when the dense solve is folded into its up-sweep)
  int l = nl - 1;
  {
    AmgLevel *L = H.lev[l];
    const T *bl = l == l0 ? b : (const T *)L->b.p;
    T *xl = l == l0 ? x : (T *)L->x.p;
    if (nl - 2 >= l0 && H.lev[nl - 2]->Dn > 0) {
      AmgLevel *U = H.lev[nl - 2];
      const T *bu = nl - 2 == l0 ? b : (const T *)U->b.p;
      T *xu = nl - 2 == l0 ? x : (T *)U->x.p;
      // (a two-level hierarchy: this IS the finest up-sweep -- owned rows only where the caller keeps just those)
      const int un = (nl - 2 == 0 && c->up0_rows > 0 && c->up0_rows < U->n) ? c->up0_rows : U->n;
      hipLaunchKernelGGL((fused_up_dense_kernel<T>), dim3((unsigned)((64ll * un + TPB - 1) / TPB)), dim3(TPB), 0, c->stream, un,
                         U->Sb.rowptr.p, U->Sb.col.p, U->Sb.val.p, bu, U->D.p, U->Dn, bl, xu);
      l = nl - 3;
    } else {
      if (H.coarse_n > 0)
        hipLaunchKernelGGL((dense_mv_kernel<T>), dim3(H.coarse_n), dim3(64), 0, c->stream, H.coarse_n, H.coarse_inv.p, bl, xl);
      else if (L->sell)
        launch_up_sell<T, true>(c, L->n, L->Sb, bl, nullptr, (const T *)nullptr, xl, 0.0, 0.0, nullptr, nullptr, nullptr);
      else
        hipLaunchKernelGGL((fused_up_csr_kernel<T>), dim3((unsigned)((8ll * L->n + TPB - 1) / TPB)), dim3(TPB), 0, c->stream, L->n,
                           L->Sb.rowptr.p, L->Sb.col.p, L->Sb.val.p, bl, (const int *)nullptr, (const int *)nullptr,
                           (const double *)nullptr, (const T *)nullptr, xl, 0.0, 0.0, (const double *)nullptr, (const double *)nullptr,
                           (const unsigned char *)nullptr);
      l = nl - 2;
    }
  }
  // up
  for (; l >= l0; l--) {
    AmgLevel *L = H.lev[l], *N = H.lev[l + 1];
    const T *bl = l == l0 ? b : (const T *)L->b.p;
    T *xl = l == l0 ? x : (T *)L->x.p;
    // Cahouet-Chabard combination in the epilogue of the last kernel of the (single right-hand side) pressure cycle
    const bool epi = l == 0 && c->epi.on && sizeof(T) == sizeof(double);
    const double ea = epi ? c->epi.alpha : 0.0, eb = epi ? c->epi.beta : 0.0;
    const double *ezH = epi ? c->epi.zH : nullptr, *er = epi ? c->epi.r : nullptr;
    const unsigned char *epbc = epi ? c->epi.pbc : nullptr;
    if (epi) { xl = (T *)c->epi.out; c->epi.done = true; }
    // overlapping velocity cycle of a partitioned run: only the owned rows (the first ones) of the finest level's result are kept
    const int nrow = (l == 0 && c->up0_rows > 0 && c->up0_rows < L->n) ? c->up0_rows : L->n;
    if (prof && l == 0) prof_begin(c, prof);
    // a few longer rows (irregular vertices of a triangle mesh) go through the tail loop of the one-chunk kernel; the chunked
    // kernel is for meshes whose typical row exceeds a chunk (tetrahedra)
    if (L->sell && L->Sb.sell_maxw <= 14 && L->Sc.sell_maxw <= 14)
      launch_up_sell<T, false>(c, nrow, L->Sb, bl, &L->Sc, (const T *)N->x.p, xl, ea, eb, ezH, er, epbc);
    else if (L->sell)
      launch_up_sell<T, true>(c, nrow, L->Sb, bl, &L->Sc, (const T *)N->x.p, xl, ea, eb, ezH, er, epbc);
    else
      hipLaunchKernelGGL((fused_up_csr_kernel<T>), dim3((unsigned)((8ll * nrow + TPB - 1) / TPB)), dim3(TPB), 0, c->stream, nrow,
                         L->Sb.rowptr.p, L->Sb.col.p, L->Sb.val.p, bl, L->Sc.rowptr.p, L->Sc.col.p, L->Sc.val.p, (const T *)N->x.p, xl,
                         ea, eb, ezH, er, epbc);
    if (prof && l == 0) prof_end(c, prof);
  }
  HIPCHK(c, hipGetLastError());
  return 0;
}

// V-cycle with Chebyshev smoothing of degree >= 2 (single right-hand side)
static int amg_cycle_cheb(cfdh_ctx *c, AmgHier &H, size_t lev, const double *b, double *x, bool prof) {
  AmgLevel *L = H.lev[lev];
  if (lev + 1 == H.lev.size()) {
    if (H.coarse_n > 0) {
      hipLaunchKernelGGL((dense_mv_kernel<double>), dim3(H.coarse_n), dim3(64), 0, c->stream, H.coarse_n, H.coarse_inv.p, b, x);
      HIPCHK(c, hipGetLastError());
      return 0;
    }
    return level_cheb(c, L, b, x, true, c->opt.amg_smooth_degree > 2 ? c->opt.amg_smooth_degree : 2, false);  // near-diagonal coarsest level: smoothing only
  }
  AmgLevel *N = H.lev[lev + 1];
  const int deg = c->opt.amg_smooth_degree;
  CHK(level_cheb(c, L, b, x, true, deg, prof && lev == 0));
  CHK(k_csr_spmv(c, L->A, x, L->r.p, 1, b));     // r = b - A x
  CHK(k_csr_spmv(c, L->R, L->r.p, N->b.p, 0, nullptr));  // b_c = R r
  CHK(amg_cycle_cheb(c, H, lev + 1, N->b.p, N->x.p, prof));
  CHK(k_csr_spmv(c, L->P, N->x.p, x, 2, nullptr));  // x += P x_c
  CHK(level_cheb(c, L, b, x, false, deg, prof && lev == 0));
  return 0;
}

// ---- distributed finest level of the replicated pressure hierarchy (cfdh_ctx::DistL0)
// b_loc = pressure slot of a halo-layout vector on owned + ghost vertices; xa = w D^-1 b on all of them
__global__ __launch_bounds__(TPB) void dl0_pack_kernel(int nvo, int nv, int dim, const double *__restrict__ vec, const double *__restrict__ wdinv,
                                                       double *__restrict__ b, double *__restrict__ xa, int ghosts) {
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i >= nv) return;
  // pressure slot: owned at dim nvo + i, ghost record (u..., p) of dim + 1 doubles behind the owned part
  // ghosts == 0: the ghost layer of the right-hand side was not exchanged -- the pre-smoothed iterate is taken as zero there
  const double v = i < nvo ? vec[(size_t)dim * nvo + i] : (ghosts ? vec[((size_t)dim + 1) * nvo + ((size_t)dim + 1) * (size_t)(i - nvo) + dim] : 0.0);
  b[i] = v;
  xa[i] = wdinv[i] * v;
}
// pre-smoothing on the owned rows and the owned part of the coarse right-hand side: lev[1].b = P_owned^T (b - A xa)
int k_dl0_down(cfdh_ctx *c, const double *halo_vec) {
  cfdh_ctx::DistL0 &d = c->dl0;
  AmgLevel *N = c->hLg.lev[1];
  const int nvo = c->nvo, nv = c->nv;
  // without the exchange of the right-hand side's ghost layer the producer (the H solve) has written the owned part of d.b itself;
  // the ghost parts of d.b and d.xa stay zero
  if (d.ghost_rhs) hipLaunchKernelGGL(dl0_pack_kernel, dim3((nv + TPB - 1) / TPB), dim3(TPB), 0, c->stream, nvo, nv, c->dim, halo_vec, d.wdinv.p, d.b.p, d.xa.p, 1);
  // short regular rows: SELL-64 (as the replicated level 0 would use)
  launch_jacobi_pre<double>(c, d.A, cfdh_dl0_rule_A(c), nvo, d.wdinv.p, (const double *)d.b.p, d.xa.p, d.r.p);
  HIPCHK(c, hipGetLastError());
  return csr_spmv_t<double>(c, d.PT, d.r.p, N->b.p, 0, (const double *)nullptr);
}
// replicated coarse cycle from level 1, prolongation to owned + ghost rows, post-smoothing of the owned rows -> out
int k_dl0_up(cfdh_ctx *c, double *out) {
  cfdh_ctx::DistL0 &d = c->dl0;
  AmgLevel *N = c->hLg.lev[1];
  const int nvo = c->nvo, nv = c->nv;
  // the replicated levels: composite-operator cycle from level 1 (6 launches for four coarse levels instead of 13 sweeps)
  if (cfdh_dl0_coarse_fused(c)) CHK(amg_cycle_fused<double>(c, c->hLg, (const double *)N->b.p, N->x.p, 0, 1));
  else CHK(amg_cycle_jacobi<double>(c, c->hLg, 1, (const double *)N->b.p, N->x.p, 0));
  launch_prolong_add<double>(c, d.P, cfdh_dl0_rule_P(c), nv, (const double *)N->x.p, d.x1.p, (const double *)d.xa.p);  // x1 = xa + P x_c
  HIPCHK(c, hipGetLastError());
  launch_jacobi_post<double>(c, d.A, cfdh_dl0_rule_A(c), nvo, d.wdinv.p, (const double *)d.b.p, (const double *)d.x1.p, out);
  HIPCHK(c, hipGetLastError());
  return 0;
}

// x = V(H) b; for ncol == 2 b and x hold interleaved pairs
int k_amg_vcycle(cfdh_ctx *c, AmgHier &H, const double *b, double *x) {
  if (!H.valid || H.lev.empty()) return cfdh_fail(c, CFDH_E_STATE, "AMG hierarchy not built");
  const bool prof = (&H == &c->hS) || (&H == &c->hL) || (&H == &c->hLg);
  if (H.ncol == 3) {
    if (H.fused && c->opt.amg_smooth_degree == 1 && H.lev.size() >= 2) return amg_cycle_fused<d3>(c, H, (const d3 *)b, (d3 *)x, 5);
    return amg_cycle_jacobi<d3>(c, H, 0, (const d3 *)b, (d3 *)x, 5);
  }
  if (H.fused && c->opt.amg_smooth_degree == 1 && H.lev.size() >= 2) {
    if (H.ncol == 2) return amg_cycle_fused<double2>(c, H, (const double2 *)b, (double2 *)x, 5);
    return amg_cycle_fused<double>(c, H, b, x, prof ? 4 : 0);
  }
  if (H.ncol == 2) return amg_cycle_jacobi<double2>(c, H, 0, (const double2 *)b, (double2 *)x, 5);
  if (c->opt.amg_smooth_degree == 1) return amg_cycle_jacobi<double>(c, H, 0, b, x, prof ? 4 : 0);
  return amg_cycle_cheb(c, H, 0, b, x, prof);
}

// Cahouet-Chabard combination: y = M_l z (0 on Dirichlet rows) ; out = alpha t + beta z, out = r on Dirichlet rows
__global__ __launch_bounds__(TPB) void cc_scale_kernel(int n, const double *__restrict__ ml, const double *__restrict__ z, double *__restrict__ y) {
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i < n) y[i] = ml[i] * z[i];
}
__global__ __launch_bounds__(TPB) void cc_combine_kernel(int n, double alpha, double beta, const double *__restrict__ t,
                                                         const double *__restrict__ z, const double *__restrict__ r,
                                                         const unsigned char *__restrict__ pbc, double *__restrict__ out, double *__restrict__ out2) {
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i < n) {
    const double v = (pbc[i] & 1) ? r[i] : alpha * t[i] + beta * z[i];
    out[i] = v;
    if (out2) out2[i] = v;  // partitioned run: z_p also into the pressure slot of the halo scratch vector
  }
}
__global__ __launch_bounds__(TPB) void scatter_global_kernel(int n, const int *__restrict__ l2g, const double *__restrict__ loc, double *__restrict__ glob) {
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i < n) glob[l2g[i]] = loc[i];
}
__global__ __launch_bounds__(TPB) void gather_global_kernel(int n, const int *__restrict__ l2g, const double *__restrict__ glob, double *__restrict__ loc) {
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i < n) loc[i] = glob[l2g[i]];
}
// velocity part of a halo-layout vector ([u owned | p owned | (ux,uy,p) per ghost]) as nv contiguous pairs
__global__ __launch_bounds__(TPB) void ext_pack_kernel(int nvo, int nv, const double *__restrict__ vec, double2 *__restrict__ out) {
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i >= nv) return;
  if (i < nvo) out[i] = make_double2(vec[2 * (size_t)i], vec[2 * (size_t)i + 1]);
  else {
    const double *t = vec + 3 * (size_t)nvo + 3 * (size_t)(i - nvo);
    out[i] = make_double2(t[0], t[1]);
  }
}
__global__ __launch_bounds__(TPB) void ext_pack3_kernel(int nvo, int nv, const double *__restrict__ vec, double *__restrict__ out) {
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i >= nv) return;
  const double *t = i < nvo ? vec + 3 * (size_t)i : vec + 4 * (size_t)i;  // ghost record (ux, uy, uz, p) at 4 nvo + 4 (i - nvo)
  out[3 * (size_t)i] = t[0]; out[3 * (size_t)i + 1] = t[1]; out[3 * (size_t)i + 2] = t[2];
}
int k_ext_pack(cfdh_ctx *c, const double *vec, double *out) {
  if (c->dim == 3) {
    hipLaunchKernelGGL(ext_pack3_kernel, dim3((c->nv + TPB - 1) / TPB), dim3(TPB), 0, c->stream, c->nvo, c->nv, vec, out);
    HIPCHK(c, hipGetLastError());
    return 0;
  }
  hipLaunchKernelGGL(ext_pack_kernel, dim3((c->nv + TPB - 1) / TPB), dim3(TPB), 0, c->stream, c->nvo, c->nv, vec, (double2 *)out);
  HIPCHK(c, hipGetLastError());
  return 0;
}
int k_scatter_global(cfdh_ctx *c, int n, const int *l2g, const double *loc, double *glob) {
  hipLaunchKernelGGL(scatter_global_kernel, dim3((n + TPB - 1) / TPB), dim3(TPB), 0, c->stream, n, l2g, loc, glob);
  HIPCHK(c, hipGetLastError());
  return 0;
}
int k_gather_global(cfdh_ctx *c, int n, const int *l2g, const double *glob, double *loc) {
  hipLaunchKernelGGL(gather_global_kernel, dim3((n + TPB - 1) / TPB), dim3(TPB), 0, c->stream, n, l2g, glob, loc);
  HIPCHK(c, hipGetLastError());
  return 0;
}
int k_cc_scale(cfdh_ctx *c, int n, const double *ml, const double *z, double *y) {
  hipLaunchKernelGGL(cc_scale_kernel, dim3((n + TPB - 1) / TPB), dim3(TPB), 0, c->stream, n, ml, z, y);
  HIPCHK(c, hipGetLastError());
  return 0;
}
int k_cc_combine(cfdh_ctx *c, int n, double alpha, double beta, const double *t, const double *z, const double *r,
                 const unsigned char *pbc, double *out, double *out2) {
  hipLaunchKernelGGL(cc_combine_kernel, dim3((n + TPB - 1) / TPB), dim3(TPB), 0, c->stream, n, alpha, beta, t, z, r, pbc, out, out2);
  HIPCHK(c, hipGetLastError());
  return 0;
}
