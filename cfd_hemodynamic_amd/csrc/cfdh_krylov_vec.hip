// Vector kernels of FGMRES and of a linear solve's prologue / epilogue on gfx950 (CDNA4, wave64): every v_* wrapper.
//
//  * axpy family, pointwise product, scaled copies, mean removal
//  * dot products and norms (partial sums and read-backs: the protocol of cfdh_reduce.hip)
//  * Gram-Schmidt building blocks: fused multi-dot, update + normalisation, against the fp64 basis or its fp32 copy
//  * lean solve path (cfdh_solver.cpp): Gram system of the projected guess and its solve on the device, x = U y / r = b - W y,
//    kept linear combination, three norms with one read-back
//
// The host arithmetic shared with the solver (gs_scale, gram_solve) is cfdh_krylov_host.hpp.  The lean wrappers that launch a
// block-SpMV kernel (k_resid_norm, k_spmv_full_kept, k_spmv_a01_keep) stay with that kernel in cfdh_kernels.hip.
// HBM-bound streams; every sum has a fixed order (bitwise reproducible).  Tested one by one: tests/test_gpu_krylov_vec.py.
#include <hip/hip_runtime.h>

#include <cmath>

#include "cfdh_internal.hpp"
#include "cfdh_krylov_host.hpp"
#include "cfdh_wave.hpp"

// ---------------------------------------------------------------- vector kernels
__global__ __launch_bounds__(TPB) void axpy_kernel(int n, double a, const double *__restrict__ x, double *__restrict__ y) {
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) y[i] += a * x[i];
}
__global__ __launch_bounds__(TPB) void waxpy_kernel(int n, double a, const double *__restrict__ x, const double *__restrict__ y,
                                                    double *__restrict__ w) {
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) w[i] = y[i] + a * x[i];
}
__global__ __launch_bounds__(TPB) void scale_kernel(int n, double a, double *__restrict__ x) {
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) x[i] *= a;
}

__global__ __launch_bounds__(TPB) void pmult_kernel(int n, const double *__restrict__ a, const double *__restrict__ b, double *__restrict__ o) {
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) o[i] = a[i] * b[i];
}
int v_pointwise_mult(cfdh_ctx *c, int n, const double *a, const double *b, double *out) {
  hipLaunchKernelGGL(pmult_kernel, dim3(vgrid(n)), dim3(TPB), 0, c->stream, n, a, b, out);
  HIPCHK(c, hipGetLastError());
  return 0;
}
int v_copy(cfdh_ctx *c, int n, const double *x, double *y) {
  HIPCHK(c, hipMemcpyAsync(y, x, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, c->stream));
  return 0;
}
int v_zero(cfdh_ctx *c, int n, double *y) {
  HIPCHK(c, hipMemsetAsync(y, 0, sizeof(double) * (size_t)n, c->stream));
  return 0;
}
int v_axpy(cfdh_ctx *c, int n, double a, const double *x, double *y) {
  hipLaunchKernelGGL(axpy_kernel, dim3(vgrid(n)), dim3(TPB), 0, c->stream, n, a, x, y);
  HIPCHK(c, hipGetLastError());
  return 0;
}
int v_waxpy(cfdh_ctx *c, int n, double a, const double *x, const double *y, double *w) {
  hipLaunchKernelGGL(waxpy_kernel, dim3(vgrid(n)), dim3(TPB), 0, c->stream, n, a, x, y, w);
  HIPCHK(c, hipGetLastError());
  return 0;
}
int v_scale(cfdh_ctx *c, int n, double a, double *x) {
  hipLaunchKernelGGL(scale_kernel, dim3(vgrid(n)), dim3(TPB), 0, c->stream, n, a, x);
  HIPCHK(c, hipGetLastError());
  return 0;
}

// ---- reductions (protocol and kernels: cfdh_reduce.hip)
static int reduce_dev(cfdh_ctx *c, int op, int n, const double *x, const double *y, double *out_dev, ScalarRead *h) {
  const int nb = red_grid(c, n);
  CHK(red_partials_launch(c, op, nb, n, x, y, c->red_partial.p));
  return scalars_finish(c, out_dev, 1, op, nb, h);
}

int v_dot(cfdh_ctx *c, int n, const double *x, const double *y, double *out_host) {
  ScalarRead h;
  CHK(reduce_dev(c, 0, n, x, y, c->red_out.p, &h));
  return scalars_read(c, h, out_host);
}
int v_norm2(cfdh_ctx *c, int n, const double *x, double *out_host) {
  CHK(v_dot(c, n, x, x, out_host));
  *out_host = sqrt(*out_host);
  return 0;
}
// |x| and |y| with one read-back (one host synchronisation instead of two)
int v_norm2_pair(cfdh_ctx *c, int n, const double *x, const double *y, double *nx, double *ny) {
  const int nb = red_grid(c, n);
  if ((size_t)2 * nb > c->red_partial.n) return cfdh_fail(c, CFDH_E_STATE, "reduction workspace too small");
  CHK(red_partials_launch(c, 0, nb, n, x, x, c->red_partial.p));
  CHK(red_partials_launch(c, 0, nb, n, y, y, c->red_partial.p + nb));
  ScalarRead h;
  CHK(scalars_finish(c, c->red_out.p, 2, 0, nb, &h));
  double v[2];
  CHK(scalars_read(c, h, v));
  *nx = sqrt(v[0]); *ny = sqrt(v[1]);
  return 0;
}
int v_norminf_diff(cfdh_ctx *c, int n, const double *x, const double *y, double *out_host) {
  ScalarRead h;
  CHK(reduce_dev(c, 1, n, x, y, c->red_out.p, &h));
  return scalars_read(c, h, out_host);
}

__global__ __launch_bounds__(TPB) void sub_scalar_kernel(int n, double *__restrict__ p, const double *__restrict__ s, double scale) {
  const double m = s[0] * scale;
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) p[i] -= m;
}
// p -= mean(p) over all ranks (constant-pressure null vector, stabilized_schur.py:282-293,319)
int v_sub_mean(cfdh_ctx *c, int n, double *p) {
  const int nb = red_grid(c, n);
  double *acc = c->red_out.p + RO_MEAN;  // [sum, count]
  CHK(red_partials_launch(c, 2, nb, n, p, nullptr, c->red_partial.p));
  CHK(red_final(c, 0, 1, nb, nb, c->red_partial.p, acc, nullptr));
  double scale = 1.0 / n;
  if (c->nranks > 1) {
    CHK(comm_allreduce_dev(c, acc, 1, 0));
    // global number of pressure dofs: constant, reduced once when the communicator is attached (global_counts)
    if (n != c->nvo || !(c->nvo_global > 0)) return cfdh_fail(c, CFDH_E_STATE, "v_sub_mean: global count unknown");
    scale = 1.0 / c->nvo_global;
  }
  hipLaunchKernelGGL(sub_scalar_kernel, dim3(vgrid(n)), dim3(TPB), 0, c->stream, n, p, acc, scale);
  HIPCHK(c, hipGetLastError());
  return 0;
}

// ---- Gram-Schmidt building blocks: h_i = V_i . w for i < nvec (V column-major, leading dim ld)
#define MD_G 8     // vectors reduced together: one pass over the w chunk feeds 8 dot products
#define MD_NB 1024 // blocks: 4 per CU, each owning a contiguous chunk (w stays L1/L2 resident across groups)
__global__ __launch_bounds__(TPB) void multidot_kernel(int n, const double *__restrict__ V, size_t ld, int nvec,
                                                       const double *__restrict__ w, double *__restrict__ partial, int nblk,
                                                       int with_ww) {
  __shared__ double sh[4][MD_G];
  const int nout = nvec + with_ww;
  const int per = (((n + nblk - 1) / nblk) + 1) & ~1;
  const int lo = blockIdx.x * per, hi = min(n, lo + per);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int g0 = 0; g0 < nout; g0 += MD_G) {
    const double *ptr[MD_G];
    double acc[MD_G];
#pragma unroll
    for (int q = 0; q < MD_G; q++) {
      const int v = g0 + q;
      ptr[q] = (v < nvec) ? V + (size_t)v * ld : w;  // v == nvec: w.w ; v > nvec: dummy (discarded)
      acc[q] = 0.0;
    }
    // two consecutive entries per lane (16-B loads; lo and the leading dimension are even), odd tail by the last lane
    const int hi2 = hi > lo ? lo + ((hi - lo) & ~1) : hi;  // blocks past the end of a short vector own nothing
    for (int i = lo + 2 * threadIdx.x; i < hi2; i += 2 * TPB) {
      const double2 wi = *(const double2 *)(w + i);
#pragma unroll
      for (int q = 0; q < MD_G; q++) {
        const double2 vi = *(const double2 *)(ptr[q] + i);
        acc[q] += vi.x * wi.x + vi.y * wi.y;
      }
    }
    if (hi2 < hi && threadIdx.x == 0) {
      const double wi = w[hi2];
#pragma unroll
      for (int q = 0; q < MD_G; q++) acc[q] += ptr[q][hi2] * wi;
    }
#pragma unroll
    for (int q = 0; q < MD_G; q++) {
      const double r = wave_sum(acc[q]);
      if (lane == 0) sh[wv][q] = r;
    }
    __syncthreads();
    if (threadIdx.x < MD_G && g0 + (int)threadIdx.x < nout)
      partial[(size_t)(g0 + threadIdx.x) * nblk + blockIdx.x] =
          (sh[0][threadIdx.x] + sh[1][threadIdx.x]) + (sh[2][threadIdx.x] + sh[3][threadIdx.x]);
    __syncthreads();
  }
}
// Gram system of the projected initial guess in ONE pass over the K + 1 vectors: out slot (i, q) = W_q . W_i for i < K and
// W_q . b for i = K, laid out as out[8 i + q] (the unused slots of the 8-wide rows are written as zeros).
template <int K>
__global__ __launch_bounds__(TPB) void gram_kernel(int n, const double *__restrict__ W, size_t ld, const double *__restrict__ b,
                                                   double *__restrict__ partial, int nblk) {
  constexpr int NP = K * (K + 1) / 2 + K;
  __shared__ double sh[4][NP];
  const int per = (((n + nblk - 1) / nblk) + 1) & ~1;
  const int lo = blockIdx.x * per, hi = min(n, lo + per);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  double acc[NP];
#pragma unroll
  for (int t = 0; t < NP; t++) acc[t] = 0.0;
  for (int i = lo + threadIdx.x; i < hi; i += TPB) {
    double x[K];
#pragma unroll
    for (int q = 0; q < K; q++) x[q] = W[(size_t)q * ld + i];
    const double bi = b[i];
    int t = 0;
#pragma unroll
    for (int q = 0; q < K; q++) {
#pragma unroll
      for (int r = q; r < K; r++) acc[t++] += x[q] * x[r];
    }
#pragma unroll
    for (int q = 0; q < K; q++) acc[t++] += x[q] * bi;
  }
#pragma unroll
  for (int t = 0; t < NP; t++) {
    const double r = wave_sum(acc[t]);
    if (lane == 0) sh[wv][t] = r;
  }
  __syncthreads();
  // scatter into the 8-wide slot layout (symmetric entries twice)
  if (threadIdx.x < 8 * (K + 1)) {
    const int i = threadIdx.x >> 3, q = threadIdx.x & 7;
    double v = 0.0;
    if (q < K) {
      int t;
      if (i < K) { const int lo_ = min(i, q), hi_ = max(i, q); t = lo_ * K - lo_ * (lo_ - 1) / 2 + (hi_ - lo_); }
      else t = K * (K + 1) / 2 + q;
      v = (sh[0][t] + sh[1][t]) + (sh[2][t] + sh[3][t]);
    }
    partial[(size_t)threadIdx.x * nblk + blockIdx.x] = v;
  }
}
// out_dev[8 i + q] as above, NOT reduced over the ranks (the caller does that once)
int v_gram(cfdh_ctx *c, int n, const double *W, int ld, int k, const double *b, double *out_dev) {
  const int nb = MD_NB, nout = 8 * (k + 1);
  if (k < 2 || k > 4 || (size_t)nout * nb > c->red_partial.n) {
    for (int i = 0; i <= k; i++) CHK(v_multidot(c, n, W, ld, k, i < k ? W + (size_t)i * ld : b, out_dev + (size_t)i * 8, false, nullptr, false));
    return 0;
  }
  if (k == 2) hipLaunchKernelGGL((gram_kernel<2>), dim3(nb), dim3(TPB), 0, c->stream, n, W, (size_t)ld, b, c->red_partial.p, nb);
  else if (k == 3) hipLaunchKernelGGL((gram_kernel<3>), dim3(nb), dim3(TPB), 0, c->stream, n, W, (size_t)ld, b, c->red_partial.p, nb);
  else hipLaunchKernelGGL((gram_kernel<4>), dim3(nb), dim3(TPB), 0, c->stream, n, W, (size_t)ld, b, c->red_partial.p, nb);
  HIPCHK(c, hipGetLastError());
  return red_final(c, 0, nout, nb, nb, c->red_partial.p, out_dev, nullptr);
}
// (A "last block does the final reduction" variant was measured and dropped: the device-scope release fence every
// block needs before taking its ticket writes the XCD's L2 back -- 133 us per launch against 17 + 4 us for two kernels.)
// h_dev[0..nvec) = V^T w (and h_dev[nvec] = w.w when with_ww), reduced over all ranks
int v_multidot(cfdh_ctx *c, int n, const double *V, int ld, int nvec, const double *w, double *h_dev, bool with_ww, double *mirror, bool reduce_ranks) {
  const int nb = MD_NB, nout = nvec + (with_ww ? 1 : 0);
  if ((size_t)nout * nb > c->red_partial.n) return cfdh_fail(c, CFDH_E_STATE, "multidot workspace too small");
  hipLaunchKernelGGL(multidot_kernel, dim3(nb), dim3(TPB), 0, c->stream, n, V, (size_t)ld, nvec, w, c->red_partial.p, nb,
                     with_ww ? 1 : 0);
  // single rank: the h values also land in host-mapped memory (`mirror`: device view of a slot of the FGMRES read-back ring)
  // straight from the kernel
  HIPCHK(c, hipGetLastError());
  CHK(red_final(c, 0, nout, nb, nb, c->red_partial.p, h_dev, (mirror && c->nranks <= 1) ? mirror : nullptr));
  if (!reduce_ranks) return 0;  // the caller reduces several results over the ranks at once
  CHK(comm_allreduce_dev(c, h_dev, nout, 0));
  // partitioned: publish the REDUCED coefficients the same way (behind the all-reduce)
  if (mirror && c->nranks > 1) CHK(red_publish(c, nout, h_dev, mirror));
  return 0;
}
__global__ __launch_bounds__(TPB) void scale_to_kernel(int n, double a, const double *__restrict__ x, double *__restrict__ y) {
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) y[i] = a * x[i];
}
int v_scale_to(cfdh_ctx *c, int n, double a, const double *x, double *y) {
  hipLaunchKernelGGL(scale_to_kernel, dim3(vgrid(n)), dim3(TPB), 0, c->stream, n, a, x, y);
  HIPCHK(c, hipGetLastError());
  return 0;
}
// w -= sum_i h_i V_i
__global__ __launch_bounds__(TPB) void multiaxpy_kernel(int n, const double *__restrict__ V, size_t ld, int nvec,
                                                        const double *__restrict__ h, double *__restrict__ w, double sign) {
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
    double a0 = w[i], a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int v = 0;
    for (; v + 4 <= nvec; v += 4) {  // four independent streams in flight
      const double x0 = V[(size_t)v * ld + i], x1 = V[(size_t)(v + 1) * ld + i], x2 = V[(size_t)(v + 2) * ld + i],
                   x3 = V[(size_t)(v + 3) * ld + i];
      a0 += sign * h[v] * x0; a1 += sign * h[v + 1] * x1; a2 += sign * h[v + 2] * x2; a3 += sign * h[v + 3] * x3;
    }
    for (; v < nvec; v++) a0 += sign * h[v] * V[(size_t)v * ld + i];
    w[i] = (a0 + a1) + (a2 + a3);
  }
}
int v_multiaxpy(cfdh_ctx *c, int n, const double *V, int ld, int nvec, const double *h_dev, double *w) {
  hipLaunchKernelGGL(multiaxpy_kernel, dim3(vgrid(n)), dim3(TPB), 0, c->stream, n, V, (size_t)ld, nvec, h_dev, w, -1.0);
  HIPCHK(c, hipGetLastError());
  return 0;
}
__global__ __launch_bounds__(TPB) void gs_update_normalize_kernel(int n, const double *__restrict__ V, size_t ld, int nvec,
                                                                 const double *__restrict__ h, const double *__restrict__ w,
                                                                 double *__restrict__ vn, double *__restrict__ s_out) {
  const double ww = h[nvec];
  double hh2 = 0.0;
  for (int v = 0; v < nvec; v++) hh2 += h[v] * h[v];
  const double s = cfdh_krylov::gs_scale(ww, hh2);  // cancellation: any positive scale, the caller re-orthogonalises
  const double inv = s > 0.0 ? 1.0 / s : 0.0;
  if (blockIdx.x == 0 && threadIdx.x == 0) *s_out = s;
  // two consecutive entries per lane (16-B loads: ld is even and all vectors are 16-B aligned); same summation order per entry
  const int n2 = n & ~1;
  for (int i = 2 * (blockIdx.x * TPB + threadIdx.x); i < n2; i += 2 * gridDim.x * TPB) {
    const double2 wi = *(const double2 *)(w + i);
    double a0 = wi.x, a1 = 0.0, a2 = 0.0, a3 = 0.0, b0 = wi.y, b1 = 0.0, b2 = 0.0, b3 = 0.0;
    int v = 0;
    for (; v + 4 <= nvec; v += 4) {
      const double2 x0 = *(const double2 *)(V + (size_t)v * ld + i), x1 = *(const double2 *)(V + (size_t)(v + 1) * ld + i),
                    x2 = *(const double2 *)(V + (size_t)(v + 2) * ld + i), x3 = *(const double2 *)(V + (size_t)(v + 3) * ld + i);
      a0 -= h[v] * x0.x; a1 -= h[v + 1] * x1.x; a2 -= h[v + 2] * x2.x; a3 -= h[v + 3] * x3.x;
      b0 -= h[v] * x0.y; b1 -= h[v + 1] * x1.y; b2 -= h[v + 2] * x2.y; b3 -= h[v + 3] * x3.y;
    }
    for (; v < nvec; v++) { const double2 xv = *(const double2 *)(V + (size_t)v * ld + i); a0 -= h[v] * xv.x; b0 -= h[v] * xv.y; }
    *(double2 *)(vn + i) = make_double2(((a0 + a1) + (a2 + a3)) * inv, ((b0 + b1) + (b2 + b3)) * inv);
  }
  if (n2 < n && blockIdx.x == 0 && threadIdx.x == 0) {
    double a0 = w[n2];
    for (int v = 0; v < nvec; v++) a0 -= h[v] * V[(size_t)v * ld + n2];
    vn[n2] = a0 * inv;
  }
}
int v_gs_update_normalize(cfdh_ctx *c, int n, const double *V, int ld, int nvec, const double *h_dev, const double *w, double *vn, double *s_dev) {
  hipLaunchKernelGGL(gs_update_normalize_kernel, dim3(vgrid(n)), dim3(TPB), 0, c->stream, n, V, (size_t)ld, nvec, h_dev, w, vn, s_dev);
  HIPCHK(c, hipGetLastError());
  return 0;
}
__global__ void sqrt_kernel(double *s);
// ---- Gram-Schmidt against an fp32 COPY of the basis (long Krylov cycles: the two passes over V are 40 % of an iteration at
// depth 25; the fp64 vectors stay where the preconditioner reads them).  The norm of the new vector is measured, not inferred
// from w.w - |h|^2 (that identity needs an orthonormal basis to round-off, which rounded columns are not).
__global__ __launch_bounds__(TPB) void multidot32_kernel(int n, const float *__restrict__ V, size_t ld, int nvec,
                                                         const double *__restrict__ w, double *__restrict__ partial, int nblk) {
  __shared__ double sh[4][MD_G + 1];
  const int per = (((n + nblk - 1) / nblk) + 3) & ~3;  // chunks of whole float4 / 2 x double2 groups
  const int lo = blockIdx.x * per, hi = min(n, lo + per);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int hi4 = hi > lo ? lo + ((hi - lo) & ~3) : hi;
  for (int g0 = 0; g0 < nvec; g0 += MD_G) {
    const float *ptr[MD_G];
    double acc[MD_G], aww = 0.0;
#pragma unroll
    for (int q = 0; q < MD_G; q++) { ptr[q] = V + (size_t)min(g0 + q, nvec - 1) * ld; acc[q] = 0.0; }  // past the end: a dummy, discarded
    // four consecutive entries per lane: one 16-B load per fp32 column, two for w
    for (int i = lo + 4 * threadIdx.x; i < hi4; i += 4 * TPB) {
      const double2 w0 = *(const double2 *)(w + i), w1 = *(const double2 *)(w + i + 2);
      if (g0 == 0) aww += (w0.x * w0.x + w0.y * w0.y) + (w1.x * w1.x + w1.y * w1.y);
#pragma unroll
      for (int q = 0; q < MD_G; q++) {
        const float4 vi = *(const float4 *)(ptr[q] + i);
        acc[q] += ((double)vi.x * w0.x + (double)vi.y * w0.y) + ((double)vi.z * w1.x + (double)vi.w * w1.y);
      }
    }
    if (threadIdx.x == 0)
      for (int i = hi4; i < hi; i++) {
        const double wi = w[i];
        if (g0 == 0) aww += wi * wi;
#pragma unroll
        for (int q = 0; q < MD_G; q++) acc[q] += (double)ptr[q][i] * wi;
      }
#pragma unroll
    for (int q = 0; q < MD_G; q++) {
      const double r = wave_sum(acc[q]);
      if (lane == 0) sh[wv][q] = r;
    }
    if (g0 == 0) { const double r = wave_sum(aww); if (lane == 0) sh[wv][MD_G] = r; }
    __syncthreads();
    if (threadIdx.x < MD_G && g0 + (int)threadIdx.x < nvec)
      partial[(size_t)(g0 + threadIdx.x) * nblk + blockIdx.x] =
          (sh[0][threadIdx.x] + sh[1][threadIdx.x]) + (sh[2][threadIdx.x] + sh[3][threadIdx.x]);
    if (g0 == 0 && threadIdx.x == MD_G)
      partial[(size_t)nvec * nblk + blockIdx.x] = (sh[0][MD_G] + sh[1][MD_G]) + (sh[2][MD_G] + sh[3][MD_G]);
    __syncthreads();
  }
}
// h_dev[0..nvec) = V32^T w, h_dev[nvec] = w.w (reduced over the ranks, mirrored like v_multidot)
int v_multidot32(cfdh_ctx *c, int n, const float *V, int ld, int nvec, const double *w, double *h_dev, double *mirror) {
  const int nb = MD_NB, nout = nvec + 1;
  if ((size_t)nout * nb > c->red_partial.n) return cfdh_fail(c, CFDH_E_STATE, "multidot workspace too small");
  hipLaunchKernelGGL(multidot32_kernel, dim3(nb), dim3(TPB), 0, c->stream, n, V, (size_t)ld, nvec, w, c->red_partial.p, nb);
  HIPCHK(c, hipGetLastError());
  CHK(red_final(c, 0, nout, nb, nb, c->red_partial.p, h_dev, c->nranks <= 1 ? mirror : nullptr));
  CHK(comm_allreduce_dev(c, h_dev, nout, 0));
  if (c->nranks > 1) CHK(red_publish(c, nout, h_dev, mirror));
  return 0;
}
// vn = w - V32 h (not normalised) and the block partials of |vn|^2
__global__ __launch_bounds__(TPB) void gs_update32_kernel(int n, const float *__restrict__ V, size_t ld, int nvec, const double *__restrict__ h,
                                                          const double *__restrict__ w, double *__restrict__ vn, double *__restrict__ partial) {
  __shared__ double sh[4];
  double ss = 0.0;
  const int n2 = n & ~1;
  for (int i = 2 * (blockIdx.x * TPB + threadIdx.x); i < n2; i += 2 * gridDim.x * TPB) {
    const double2 wi = *(const double2 *)(w + i);
    double a0 = wi.x, a1 = 0.0, b0 = wi.y, b1 = 0.0;
    int v = 0;
    for (; v + 2 <= nvec; v += 2) {
      const float2 x0 = *(const float2 *)(V + (size_t)v * ld + i), x1 = *(const float2 *)(V + (size_t)(v + 1) * ld + i);
      a0 -= h[v] * (double)x0.x; a1 -= h[v + 1] * (double)x1.x;
      b0 -= h[v] * (double)x0.y; b1 -= h[v + 1] * (double)x1.y;
    }
    for (; v < nvec; v++) { const float2 xv = *(const float2 *)(V + (size_t)v * ld + i); a0 -= h[v] * (double)xv.x; b0 -= h[v] * (double)xv.y; }
    const double r0 = a0 + a1, r1 = b0 + b1;
    *(double2 *)(vn + i) = make_double2(r0, r1);
    ss += r0 * r0 + r1 * r1;
  }
  if (n2 < n && blockIdx.x == 0 && threadIdx.x == 0) {
    double a0 = w[n2];
    for (int v = 0; v < nvec; v++) a0 -= h[v] * (double)V[(size_t)v * ld + n2];
    vn[n2] = a0;
    ss += a0 * a0;
  }
  ss = block_sum(ss, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = ss;
}
// vn /= s (s on the device) and its fp32 copy
__global__ __launch_bounds__(TPB) void scale_store32_kernel(int n, double *__restrict__ vn, const double *__restrict__ s, float *__restrict__ v32) {
  const double inv = s[0] > 0.0 ? 1.0 / s[0] : 0.0;
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) { const double x = vn[i] * inv; vn[i] = x; v32[i] = (float)x; }
}
__global__ __launch_bounds__(TPB) void store32_kernel(int n, const double *__restrict__ v, float *__restrict__ v32) {
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) v32[i] = (float)v[i];
}
int v_store32(cfdh_ctx *c, int n, const double *v, float *v32) {
  hipLaunchKernelGGL(store32_kernel, dim3(vgrid(n)), dim3(TPB), 0, c->stream, n, v, v32);
  HIPCHK(c, hipGetLastError());
  return 0;
}
// vn = (w - V32 h) / |w - V32 h| with its fp32 copy in v32n; s_dev[0] = that norm (reduced over the ranks), mirrored to
// the host-mapped word `mirror` for the host
int v_gs_update32(cfdh_ctx *c, int n, const float *V, int ld, int nvec, const double *h_dev, const double *w, double *vn, float *v32n,
                  double *s_dev, double *mirror) {
  const int nb = red_grid(c, n);
  double *part = c->red_partial.p + (size_t)(MD_NB) * 8;  // behind the first multi-dot groups (the stream serialises the users)
  hipLaunchKernelGGL(gs_update32_kernel, dim3(nb), dim3(TPB), 0, c->stream, n, V, (size_t)ld, nvec, h_dev, w, vn, part);
  if (c->nranks <= 1) {  // square root and host-mapped copy in the reduction kernel itself
    CHK(red_final(c, 2, 1, nb, nb, part, s_dev, mirror));
  } else {
    CHK(red_final(c, 0, 1, nb, nb, part, s_dev, nullptr));
    CHK(comm_allreduce_dev(c, s_dev, 1, 0));
    hipLaunchKernelGGL(sqrt_kernel, dim3(1), dim3(1), 0, c->stream, s_dev);
    CHK(red_publish(c, 1, s_dev, mirror));
  }
  hipLaunchKernelGGL(scale_store32_kernel, dim3(vgrid(n)), dim3(TPB), 0, c->stream, n, vn, (const double *)s_dev, v32n);
  HIPCHK(c, hipGetLastError());
  return 0;
}
int v_lincomb(cfdh_ctx *c, int n, const double *Z, int ld, int nvec, const double *y_dev, double *x) {
  hipLaunchKernelGGL(multiaxpy_kernel, dim3(vgrid(n)), dim3(TPB), 0, c->stream, n, Z, (size_t)ld, nvec, y_dev, x, 1.0);
  HIPCHK(c, hipGetLastError());
  return 0;
}

// ---- lean solve path: prologue and epilogue of a linear solve with one read-back each (cfdh_solver.cpp) ----------------------
// (the mirror words of the prologue: DESIGN.md, "Scalar reductions and read-backs")
// The K x K Gram system of the projected guess (K <= 8), solved by one lane: cfdh_krylov::gram_solve_k<K>, the function behind the
// gram_solve the general path calls on the host.  With K a template parameter the system stays in registers (the one kernel for
// all k worked out of scratch memory and took 22 us).
template <int K>
__global__ __launch_bounds__(64) void gram_solve_kernel(const double *__restrict__ hd, double *__restrict__ y, double *__restrict__ info) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  // the whole system requested at once, through vector loads (K (K + 1) doubles; as scalars they would crowd the scalar registers)
  double h[8 * K + K], yy[K];
#pragma unroll
  for (int i = 0; i <= K; i++)
#pragma unroll
    for (int q = 0; q < K; q++) h[8 * i + q] = NTLOAD(hd + 8 * i + q);
  int r = 0;
  const bool used = cfdh_krylov::gram_solve_k<K>(h, yy, &r);
#pragma unroll
  for (int i = 0; i < K; i++) { y[i] = yy[i]; info[3 + i] = yy[i]; }
  info[1] = used ? 1.0 : 0.0;
  info[2] = (double)r;
}
template <int K>
static void launch_gram_solve(cfdh_ctx *c, const double *hd, double *y, double *info) {
  hipLaunchKernelGGL(gram_solve_kernel<K>, dim3(1), dim3(64), 0, c->stream, hd, y, info);
}
// x = U y, r = b - W y and the block partials of |r|^2 in one pass over U, W and b.  Entry by entry the arithmetic of
// multiaxpy_kernel (on a zeroed x, and on a copy of b), block by block the partial sums of reduce_partial_kernel<0>.
__global__ __launch_bounds__(TPB) void guess_combine_kernel(int n, const double *__restrict__ U, const double *__restrict__ W, size_t ld,
                                                            int nvec, const double *__restrict__ y, const double *__restrict__ b,
                                                            double *__restrict__ x, double *__restrict__ r, double *__restrict__ partial) {
  __shared__ double sh[4];
  double ss = 0.0;
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, c0 = b[i], c1 = 0.0, c2 = 0.0, c3 = 0.0;
    int v = 0;
    for (; v + 4 <= nvec; v += 4) {
      const double y0 = y[v], y1 = y[v + 1], y2 = y[v + 2], y3 = y[v + 3];
      const double u0 = U[(size_t)v * ld + i], u1 = U[(size_t)(v + 1) * ld + i], u2 = U[(size_t)(v + 2) * ld + i], u3 = U[(size_t)(v + 3) * ld + i];
      const double w0 = W[(size_t)v * ld + i], w1 = W[(size_t)(v + 1) * ld + i], w2 = W[(size_t)(v + 2) * ld + i], w3 = W[(size_t)(v + 3) * ld + i];
      a0 += y0 * u0; a1 += y1 * u1; a2 += y2 * u2; a3 += y3 * u3;
      c0 -= y0 * w0; c1 -= y1 * w1; c2 -= y2 * w2; c3 -= y3 * w3;
    }
    for (; v < nvec; v++) { a0 += y[v] * U[(size_t)v * ld + i]; c0 -= y[v] * W[(size_t)v * ld + i]; }
    const double ri = (c0 + c1) + (c2 + c3);
    x[i] = (a0 + a1) + (a2 + a3);
    r[i] = ri;
    ss += ri * ri;
  }
  ss = block_sum(ss, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = ss;
}
// x *= 1 / sqrt(s2[0]) with the squared norm read on the device (0 when it is not positive)
__global__ __launch_bounds__(TPB) void scale_inv_sqrt_kernel(int n, double *__restrict__ x, const double *__restrict__ s2) {
  const double beta = sqrt(s2[0]);
  const double a = beta > 0.0 ? 1.0 / beta : 0.0;
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) x[i] *= a;
}
// x += sum_i y_i Z_i as v_lincomb, and the result stored a second time in x2 (the kept copy of a converged solve)
__global__ __launch_bounds__(TPB) void lincomb_keep_kernel(int n, const double *__restrict__ V, size_t ld, int nvec,
                                                           const double *__restrict__ h, double *__restrict__ w, double *__restrict__ w2) {
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
    double a0 = w[i], a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int v = 0;
    for (; v + 4 <= nvec; v += 4) {
      const double x0 = V[(size_t)v * ld + i], x1 = V[(size_t)(v + 1) * ld + i], x2 = V[(size_t)(v + 2) * ld + i],
                   x3 = V[(size_t)(v + 3) * ld + i];
      a0 += h[v] * x0; a1 += h[v + 1] * x1; a2 += h[v + 2] * x2; a3 += h[v + 3] * x3;
    }
    for (; v < nvec; v++) a0 += h[v] * V[(size_t)v * ld + i];
    const double o = (a0 + a1) + (a2 + a3);
    w[i] = o;
    w2[i] = o;
  }
}
// block partials of a.a, b.b and c.c in one pass (each sum in the order of reduce_partial_kernel<0>)
__global__ __launch_bounds__(TPB) void norm3_partial_kernel(int n, const double *__restrict__ a, const double *__restrict__ b,
                                                            const double *__restrict__ cc, double *__restrict__ partial) {
  __shared__ double sh[4];
  double s0 = 0, s1 = 0, s2 = 0;
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
    const double ai = a[i], bi = b[i], ci = cc[i];
    s0 += ai * ai; s1 += bi * bi; s2 += ci * ci;
  }
  s0 = block_sum(s0, sh);
  s1 = block_sum(s1, sh);
  s2 = block_sum(s2, sh);
  if (threadIdx.x == 0) { partial[blockIdx.x] = s0; partial[gridDim.x + blockIdx.x] = s1; partial[2 * gridDim.x + blockIdx.x] = s2; }
}
// Prologue of a solve with k kept vectors, hd = Gram system from v_gram: y on the device (ky), x = U y, r = b - W y, |r|^2 and the
// "used" flag in the host-mapped words.  Nothing is read back here.
int v_guess_combine(cfdh_ctx *c, int n, const double *U, const double *W, int ld, int k, const double *hd, const double *b, double *x, double *r) {
  if (k < 1 || k > 8) return cfdh_fail(c, CFDH_E_STATE, "projected guess: %d kept vectors", k);
  const int nb = red_grid(c, n);
  double *mir = scalars_mirror(c);
  switch (k) {
    case 1: launch_gram_solve<1>(c, hd, c->ky.p, mir); break;
    case 2: launch_gram_solve<2>(c, hd, c->ky.p, mir); break;
    case 3: launch_gram_solve<3>(c, hd, c->ky.p, mir); break;
    case 4: launch_gram_solve<4>(c, hd, c->ky.p, mir); break;
    case 5: launch_gram_solve<5>(c, hd, c->ky.p, mir); break;
    case 6: launch_gram_solve<6>(c, hd, c->ky.p, mir); break;
    case 7: launch_gram_solve<7>(c, hd, c->ky.p, mir); break;
    default: launch_gram_solve<8>(c, hd, c->ky.p, mir); break;
  }
  hipLaunchKernelGGL(guess_combine_kernel, dim3(nb), dim3(TPB), 0, c->stream, n, U, W, (size_t)ld, k, (const double *)c->ky.p, b, x, r, c->red_partial.p);
  HIPCHK(c, hipGetLastError());
  return red_final(c, 0, 1, nb, nb, c->red_partial.p, c->red_out.p + RO_LEAN_S2, mir);
}
// the one read-back of the prologue: |r0|, whether the guess is used, the rank and the coefficients
int v_guess_read(cfdh_ctx *c, int k, double *beta, bool *used, int *rank, double *y) {
  double m[3 + 8];
  CHK(scalars_read(c, scalars_mirrored(3 + k), m));
  *beta = sqrt(m[0]);
  *used = m[1] != 0.0;
  *rank = (int)m[2];
  for (int i = 0; i < k; i++) y[i] = m[3 + i];
  return 0;
}
// x /= the norm the last lean prologue / epilogue left on the device
int v_scale_inv_lean(cfdh_ctx *c, int n, double *x) {
  hipLaunchKernelGGL(scale_inv_sqrt_kernel, dim3(vgrid(n)), dim3(TPB), 0, c->stream, n, x, (const double *)(c->red_out.p + RO_LEAN_S2));
  HIPCHK(c, hipGetLastError());
  return 0;
}
int v_lincomb_keep(cfdh_ctx *c, int n, const double *Z, int ld, int nvec, const double *y_dev, double *x, double *x2) {
  hipLaunchKernelGGL(lincomb_keep_kernel, dim3(vgrid(n)), dim3(TPB), 0, c->stream, n, Z, (size_t)ld, nvec, y_dev, x, x2);
  HIPCHK(c, hipGetLastError());
  return 0;
}
// |a|, |b|, |cc| with one pass and one read-back (one rank)
int v_norm2_triple(cfdh_ctx *c, int n, const double *a, const double *b, const double *cc, double *out) {
  const int nb = red_grid(c, n);
  if ((size_t)3 * nb > c->red_partial.n) return cfdh_fail(c, CFDH_E_STATE, "reduction workspace too small");
  hipLaunchKernelGGL(norm3_partial_kernel, dim3(nb), dim3(TPB), 0, c->stream, n, a, b, cc, c->red_partial.p);
  HIPCHK(c, hipGetLastError());
  CHK(red_final(c, 0, 3, nb, nb, c->red_partial.p, c->red_out.p, scalars_mirror(c)));
  CHK(scalars_read(c, scalars_mirrored(3), out));
  for (int i = 0; i < 3; i++) out[i] = sqrt(out[i]);
  return 0;
}
__global__ void sqrt_kernel(double *s) { s[0] = sqrt(s[0]); }
int v_norm_to_dev(cfdh_ctx *c, int n, const double *w, double *out_dev) {
  CHK(reduce_dev(c, 0, n, w, w, out_dev, nullptr));  // stays on the device
  hipLaunchKernelGGL(sqrt_kernel, dim3(1), dim3(1), 0, c->stream, out_dev);
  HIPCHK(c, hipGetLastError());
  return 0;
}
// the same without the reduction over the ranks: norms of rank-local operators (hierarchy set-up of a partitioned run)
int v_norm_to_dev_local(cfdh_ctx *c, int n, const double *w, double *out_dev) {
  const int nb = red_grid(c, n);
  CHK(red_partials_launch(c, 0, nb, n, w, w, c->red_partial.p));
  CHK(red_final(c, 0, 1, nb, nb, c->red_partial.p, out_dev, nullptr));
  hipLaunchKernelGGL(sqrt_kernel, dim3(1), dim3(1), 0, c->stream, out_dev);
  HIPCHK(c, hipGetLastError());
  return 0;
}
__global__ __launch_bounds__(TPB) void scale_inv_dev_kernel(int n, const double *__restrict__ w, const double *__restrict__ nrm,
                                                            double *__restrict__ v) {
  const double s = nrm[0] != 0.0 ? 1.0 / nrm[0] : 0.0;
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) v[i] = w[i] * s;
}
int v_scale_inv_dev(cfdh_ctx *c, int n, const double *w, const double *nrm_dev, double *v) {
  hipLaunchKernelGGL(scale_inv_dev_kernel, dim3(vgrid(n)), dim3(TPB), 0, c->stream, n, w, nrm_dev, v);
  HIPCHK(c, hipGetLastError());
  return 0;
}
