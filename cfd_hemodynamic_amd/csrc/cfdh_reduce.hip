// Scalar reductions and their read-backs ("Scalar reductions and read-backs"): per-block partials in red_partial ->
// one final block per value -> all-reduce over the ranks -> the host reads the result, from host-mapped words a kernel wrote
// or through a small copy.  The protocol only: what is reduced (Krylov vectors, functionals, null-space test) is launched by
// the files that own those kernels.  The scratch words are named in cfdh_scratch.hpp.
#include <hip/hip_runtime.h>

#include "cfdh_internal.hpp"
#include "cfdh_wave.hpp"

#define TPB 256

int vgrid(int n) { int g = (n + TPB * 4 - 1) / (TPB * 4); return g < 1 ? 1 : (g > 2048 ? 2048 : g); }
int red_grid(const cfdh_ctx *c, int n) { const int g = vgrid(n); return g > c->red_blocks ? c->red_blocks : g; }

// ---- reductions: per-block partials (fixed order) -> one final block; deterministic
// OP 0: sum x*y, 1: max |x - y| (y may be null; NaN when an entry is NaN)
template <int OP>
__global__ __launch_bounds__(TPB) void reduce_partial_kernel(int n, const double *__restrict__ x, const double *__restrict__ y,
                                                             double *__restrict__ partial) {
  __shared__ double sh[4];
  double a = 0;
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
    if (OP == 0) a += x[i] * y[i];
    else a = max_nan(a, fabs(y ? x[i] - y[i] : x[i]));
  }
  a = (OP == 0) ? block_sum(a, sh) : block_max(a, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = a;
}
// out[v] = reduce(partial[v*stride .. +nblk)), one block per v; OP 2: sqrt of the sum
template <int OP>
__global__ __launch_bounds__(TPB) void reduce_final_kernel(int nblk, int stride, const double *__restrict__ partial,
                                                           double *__restrict__ out, double *__restrict__ mirror = nullptr) {
  __shared__ double sh[4];
  const double *pp = partial + (size_t)blockIdx.x * stride;
  double a = 0;
  for (int i = threadIdx.x; i < nblk; i += TPB) a = (OP == 1) ? max_nan(a, pp[i]) : a + pp[i];
  a = (OP == 1) ? block_max(a, sh) : block_sum(a, sh);
  if (threadIdx.x == 0) {
    const double v = (OP == 2) ? sqrt(a) : a;
    out[blockIdx.x] = v;
    if (mirror) mirror[blockIdx.x] = v;  // host-mapped copy: the host reads it after an event, no copy kernel
  }
}
__global__ __launch_bounds__(TPB) void mirror_copy_kernel(int n, const double *__restrict__ src, double *__restrict__ dst) {
  for (int i = threadIdx.x; i < n; i += TPB) dst[i] = src[i];
}
__global__ __launch_bounds__(TPB) void sum_partial_kernel(int n, const double *__restrict__ x, double *__restrict__ partial) {
  __shared__ double sh[4];
  double a = 0;
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) a += x[i];
  a = block_sum(a, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = a;
}

// ---- launches
int red_partials_launch(cfdh_ctx *c, int op, int nb, int n, const double *x, const double *y, double *partial) {
  if (op == 0) hipLaunchKernelGGL(reduce_partial_kernel<0>, dim3(nb), dim3(TPB), 0, c->stream, n, x, y, partial);
  else if (op == 1) hipLaunchKernelGGL(reduce_partial_kernel<1>, dim3(nb), dim3(TPB), 0, c->stream, n, x, y, partial);
  else hipLaunchKernelGGL(sum_partial_kernel, dim3(nb), dim3(TPB), 0, c->stream, n, x, partial);
  HIPCHK(c, hipGetLastError());
  return 0;
}
int red_final(cfdh_ctx *c, int op, int nval, int nblk, int stride, const double *partial, double *out, double *mirror) {
  if (op == 0) hipLaunchKernelGGL(reduce_final_kernel<0>, dim3(nval), dim3(TPB), 0, c->stream, nblk, stride, partial, out, mirror);
  else if (op == 1) hipLaunchKernelGGL(reduce_final_kernel<1>, dim3(nval), dim3(TPB), 0, c->stream, nblk, stride, partial, out, mirror);
  else hipLaunchKernelGGL(reduce_final_kernel<2>, dim3(nval), dim3(TPB), 0, c->stream, nblk, stride, partial, out, mirror);
  HIPCHK(c, hipGetLastError());
  return 0;
}
int red_publish(cfdh_ctx *c, int n, const double *src, double *mirror) {
  hipLaunchKernelGGL(mirror_copy_kernel, dim3(1), dim3(TPB), 0, c->stream, n, src, mirror);
  HIPCHK(c, hipGetLastError());
  return 0;
}

// ---- reduce and read
// One rank: the final reduction kernel also stores its results into the host-mapped mirror words, so reading them back costs
// a stream synchronisation instead of a copy kernel (~11 us each).  Partitioned: the REDUCED values are published to the same
// words by a one-block kernel behind the collective.
int scalars_finish(cfdh_ctx *c, double *dev, int n, int op, int nblk, ScalarRead *h) {
  const bool mirrored = n <= SCALARS_MIRROR_MAX;
  CHK(red_final(c, op, n, nblk, nblk, c->red_partial.p, dev, (mirrored && c->nranks <= 1) ? scalars_mirror(c) : nullptr));
  CHK(comm_allreduce_dev(c, dev, n, op));
  if (mirrored && c->nranks > 1) CHK(red_publish(c, n, dev, scalars_mirror(c)));
  if (h) *h = ScalarRead{dev, n, mirrored};
  return 0;
}
int scalars_read(cfdh_ctx *c, const ScalarRead &h, double *host, bool counted) {
  const double *words = c->h_pinned + (h.mirrored ? HP_MIRROR : HP_COPY);
  if ((size_t)h.n > (size_t)(h.mirrored ? HP_MIRROR_N : HP_COPY_N)) return cfdh_fail(c, CFDH_E_STATE, "read-back of %d scalars does not fit the pinned words", h.n);
  if (!h.mirrored) HIPCHK(c, hipMemcpyAsync(c->h_pinned + HP_COPY, h.dev, sizeof(double) * h.n, hipMemcpyDeviceToHost, c->stream));
  if (counted) c->n_host_sync++;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < h.n; i++) host[i] = words[i];
  return 0;
}
