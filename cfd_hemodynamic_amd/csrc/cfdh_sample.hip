// Point sampler of the closed-form P1 contexts (cfdh_sample_*, include/cfdh.h): the value of (u, p) at probe points, along lines and
// on regular voxel grids, from the u_sol that sits in HBM between cfdh_solve_step and cfdh_advance.
//
// Location, once per sample set.  Point x belongs to the cell of the lowest caller's index among the cells in which every
// barycentric coordinate of x is >= -tol.  sm_locate_kernel (one lane per point) finds the bin of its point in the uniform bin grid
// of cfdh_sample_host.hpp and scans that bin's list, which is in ascending caller's index, until the first cell that holds the
// point; it stores the cell and the d + 1 coordinates.  A point outside the bounding box takes no trip.  The walk of the particle
// tracker is of no use here: it needs a seed cell near every point and ends at the first wall, and most nodes of a grid over a
// vascular tree are outside the lumen.
//
// Sampling.  sm_sample_kernel (one lane per point) reads the cell, its vertex ids and the stored coordinates, gathers u and p at
// the d + 1 vertices and writes (u [d], p), or adds the weighted row to the mean accumulators.  Gather only, no atomics: two calls
// return the same bytes.  Every local index is a compile-time constant after unrolling (template <int D>).
#include <hip/hip_runtime.h>

#include <cmath>
#include <new>

#include "cfdh_internal.hpp"
#include "cfdh_sample_host.hpp"
#include "cfdh_wave.hpp"

struct SampleGrid {
  double origin[3], spacing[3];
  long long dims[3];
};

struct SampleData {
  // the search structure, kept while tol stays the same
  cfdh_sample::BinGrid bg;
  double bins_tol = -1.0;
  dbuf<int> bptr, blist;
  // the set
  size_t n = 0;
  long long nlocated = 0;
  dbuf<double> x, lam;  // [n][d], [n][d + 1] in the stored cell's vertex order
  dbuf<int> cell;       // stored cell, -1: none
  dbuf<int> count;      // per-block counts of the located points
  dbuf<double> rows;    // [n][d + 1]: cfdh_sample_now and cfdh_sample_mean_get before their download
  // series
  size_t cap = 0, nrec = 0;
  dbuf<double> series;  // [cap][n][d + 1]
  std::vector<double> t;
  // means: allocated by the first reset
  bool means = false;
  dbuf<double> sU, sP, sU2;  // sum w u [n][d], sum w p, sum w |u|^2
  double W = 0.0;
  long long count_acc = 0;
};

namespace {

constexpr int SM_COUNT_BLOCKS = 1024;
constexpr unsigned long long SM_SERIES_MAX_BYTES = 1ull << 40;  // cfdh_sample_series_enable refuses a larger buffer

// lambda of x in stored cell e by the cofactor formulas of fl_cell (cfdh_flow.hip): E[k] = x_{k+1} - x_0, g[k] = det grad lambda_{k+1}.
// true when the cell is not degenerate and every lambda >= -tol (or x is one of its vertices).
template <int D>
__device__ __forceinline__ bool sm_bary(const int *__restrict__ cells, const double *__restrict__ coords, int e, const double (&x)[D], double tol,
                                        double (&lam)[D + 1]) {
  double X[D + 1][D];
#pragma unroll
  for (int a = 0; a <= D; a++) {
    const int v = cells[(size_t)(D + 1) * e + a];
#pragma unroll
    for (int i = 0; i < D; i++) X[a][i] = coords[(size_t)D * v + i];
  }
  double E[D][D], g[D][D], det;
#pragma unroll
  for (int k = 0; k < D; k++)
#pragma unroll
    for (int i = 0; i < D; i++) E[k][i] = X[k + 1][i] - X[0][i];
  if constexpr (D == 2) {
    det = E[0][0] * E[1][1] - E[0][1] * E[1][0];
    g[0][0] = E[1][1]; g[0][1] = -E[1][0];
    g[1][0] = -E[0][1]; g[1][1] = E[0][0];
  } else {
#pragma unroll
    for (int k = 0; k < D; k++) {
      const int p = (k + 1) % D, q = (k + 2) % D;
      g[k][0] = E[p][1] * E[q][2] - E[p][2] * E[q][1];
      g[k][1] = E[p][2] * E[q][0] - E[p][0] * E[q][2];
      g[k][2] = E[p][0] * E[q][1] - E[p][1] * E[q][0];
    }
    det = E[0][0] * g[0][0] + E[0][1] * g[0][1] + E[0][2] * g[0][2];
  }
  if (det == 0.0) return false;
  // a point that is a vertex of the cell, bit for bit, lies in it with the unit row: a probe on a mesh vertex returns the nodal value
#pragma unroll
  for (int a = 0; a <= D; a++) {
    bool same = true;
#pragma unroll
    for (int i = 0; i < D; i++) same = same && x[i] == X[a][i];
    if (same) {
#pragma unroll
      for (int b = 0; b <= D; b++) lam[b] = b == a ? 1.0 : 0.0;
      return true;
    }
  }
  const double rdet = 1.0 / det;
  double sum = 0.0, mn;
#pragma unroll
  for (int k = 0; k < D; k++) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < D; i++) s += g[k][i] * (x[i] - X[0][i]);
    lam[k + 1] = s * rdet;
    sum += lam[k + 1];
  }
  lam[0] = 1.0 - sum;
  mn = lam[0];
#pragma unroll
  for (int k = 1; k <= D; k++) mn = fmin(mn, lam[k]);
  return mn >= -tol;  // false for a NaN
}

// grid != 0: point i is node (i0, i1, i2) of the grid, i = i0 + dims[0] (i1 + dims[1] i2), at fma(index, spacing, origin); it is
// stored in xs for the read-back.  Otherwise xs holds the points.
template <int D>
__global__ __launch_bounds__(TPB) void sm_locate_kernel(size_t n, int grid, SampleGrid sg, cfdh_sample::BinGrid bg, const int *__restrict__ bptr,
                                                       const int *__restrict__ blist, const int *__restrict__ cells, const double *__restrict__ coords,
                                                       double tol, double *__restrict__ xs, int *__restrict__ cell, double *__restrict__ lam) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  double x[D];
  if (grid) {
    long long idx[3];
    idx[0] = (long long)(i % (size_t)sg.dims[0]);
    const size_t r = i / (size_t)sg.dims[0];
    idx[1] = (long long)(r % (size_t)sg.dims[1]);
    idx[2] = (long long)(r / (size_t)sg.dims[1]);
#pragma unroll
    for (int a = 0; a < D; a++) {
      x[a] = fma((double)idx[a], sg.spacing[a], sg.origin[a]);
      xs[(size_t)D * i + a] = x[a];
    }
  } else {
#pragma unroll
    for (int a = 0; a < D; a++) x[a] = xs[(size_t)D * i + a];
  }
  int found = -1;
  double l[D + 1], keep[D + 1];
#pragma unroll
  for (int a = 0; a <= D; a++) keep[a] = 0.0;
  const long long b = cfdh_sample::point_bin(bg, x);
  if (b >= 0) {
    const int k1 = bptr[b + 1];
    for (int k = bptr[b]; k < k1; k++) {
      const int e = blist[k];
      if (sm_bary<D>(cells, coords, e, x, tol, l)) {
        found = e;
#pragma unroll
        for (int a = 0; a <= D; a++) keep[a] = l[a];
        break;
      }
    }
  }
  cell[i] = found;
#pragma unroll
  for (int a = 0; a <= D; a++) lam[(size_t)(D + 1) * i + a] = keep[a];
}

// partial[block] = located points of the block's share, in a fixed order
__global__ __launch_bounds__(TPB) void sm_count_kernel(size_t n, const int *__restrict__ cell, int *__restrict__ partial) {
  __shared__ double sh[4];
  double a = 0.0;
  for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (size_t)gridDim.x * TPB) a += cell[i] >= 0 ? 1.0 : 0.0;
  const double s = block_sum(a, sh);  // whole numbers below 2^53: exact
  if (threadIdx.x == 0) partial[blockIdx.x] = (int)s;
}

// u [nv][D] and p [nv] are the two parts of the state.  ACC: the weighted row goes to the accumulators instead of out.
template <int D, bool ACC>
__global__ __launch_bounds__(TPB) void sm_sample_kernel(size_t n, const int *__restrict__ cell, const double *__restrict__ lam,
                                                       const int *__restrict__ cells, const double *__restrict__ u, const double *__restrict__ p, double w,
                                                       double *__restrict__ out, double *__restrict__ sU, double *__restrict__ sP,
                                                       double *__restrict__ sU2) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const int e = cell[i];
  double row[D + 1];
#pragma unroll
  for (int j = 0; j <= D; j++) row[j] = 0.0;
  if (e >= 0) {
#pragma unroll
    for (int a = 0; a <= D; a++) {
      const int v = cells[(size_t)(D + 1) * e + a];
      const double la = lam[(size_t)(D + 1) * i + a];
#pragma unroll
      for (int j = 0; j < D; j++) row[j] += la * u[(size_t)D * v + j];
      row[D] += la * p[v];
    }
  }
  if constexpr (ACC) {
    if (e < 0) return;  // the accumulators of an unlocated point stay 0
    double u2 = 0.0;
#pragma unroll
    for (int j = 0; j < D; j++) {
      u2 += row[j] * row[j];
      sU[(size_t)D * i + j] += w * row[j];
    }
    sP[i] += w * row[D];
    sU2[i] += w * u2;
  } else {
#pragma unroll
    for (int j = 0; j <= D; j++) out[(size_t)(D + 1) * i + j] = row[j];
  }
}

// which 0: sU / W [n][D] ; 1: sP / W ; 2: max(0, (sU2 / W - |sU / W|^2) / 2)
template <int D>
__global__ __launch_bounds__(TPB) void sm_mean_kernel(size_t n, int which, double W, const double *__restrict__ sU, const double *__restrict__ sP,
                                                     const double *__restrict__ sU2, double *__restrict__ out) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  if (which == 0) {
#pragma unroll
    for (int j = 0; j < D; j++) out[(size_t)D * i + j] = sU[(size_t)D * i + j] / W;
  } else if (which == 1) {
    out[i] = sP[i] / W;
  } else {
    double m2 = 0.0;
#pragma unroll
    for (int j = 0; j < D; j++) { const double m = sU[(size_t)D * i + j] / W; m2 += m * m; }
    out[i] = fmax(0.0, 0.5 * (sU2[i] / W - m2));
  }
}

// the contexts that carry the sampler; everything else is refused before any device work
int sm_supported(cfdh_ctx *c, const char *who) {
  if (c->ipcs) return cfdh_fail(c, CFDH_E_ARG, "%s: not available on an incremental pressure-correction context (cfdh_create_ipcs)", who);
  if (c->gen) return cfdh_fail(c, CFDH_E_ARG, "%s: the sampler lives on the closed-form P1 contexts (cfdh_create), not on the generic element kernels", who);
  if (c->nranks > 1 || c->nvo != c->nv) return cfdh_fail(c, CFDH_E_ARG, "%s: not available in partitioned runs", who);
  return 0;
}

// device events around kernel k (0: locate, 1: sample), read by cfdh_info 115 / 116
int sm_time_begin(cfdh_ctx *c, int k) {
  for (int i = 2 * k; i < 2 * k + 2; i++)
    if (!c->sm_ev[i]) HIPCHK(c, hipEventCreate(&c->sm_ev[i]));
  HIPCHK(c, hipEventRecord(c->sm_ev[2 * k], c->stream));
  return 0;
}
int sm_time_end(cfdh_ctx *c, int k) {
  HIPCHK(c, hipEventRecord(c->sm_ev[2 * k + 1], c->stream));
  c->sm_timed[k] = true;
  return 0;
}

dim3 sm_blocks(size_t n) { return dim3((unsigned)((n + TPB - 1) / TPB)); }

// SampleData and the bins for this tol
int sm_need(cfdh_ctx *c, double tol) {
  if (c->sm && c->sm->bins_tol == tol) return 0;
  const int D = c->dim;
  std::vector<int> visit((size_t)c->nc, 0);
  for (int e = 0; e < c->nc; e++) {
    const int k = c->cell_user[e];
    if (k < 0 || k >= c->nc) return cfdh_fail(c, CFDH_E_STATE, "sampler: the context does not hold every cell of the mesh");
    visit[k] = e;
  }
  if (c->cell_flipped.size() != (size_t)c->nc) return cfdh_fail(c, CFDH_E_STATE, "sampler: the context does not know the orientation of its cells");
  cfdh_sample::Bins B;
  std::string why;
  if (!cfdh_sample::build_bins(D, c->nv, c->nc, c->h_coords.data(), c->h_cells.data(), visit.data(), tol, B, why))
    return cfdh_fail(c, CFDH_E_ARG, "%s", why.c_str());
  if (!c->sm) {
    c->sm = new (std::nothrow) SampleData();
    if (!c->sm) return cfdh_fail(c, CFDH_E_NOMEM, "out of host memory");
  }
  SampleData *S = c->sm;
  S->bins_tol = -1.0;
  HIPCHK(c, S->bptr.upload(B.ptr, c->stream));
  HIPCHK(c, S->blist.upload(B.list, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));  // the host vectors go out of scope
  S->bg = B.g;
  S->bins_tol = tol;
  c->sm_bin_doublings = B.doublings;
  c->sm_bin_total = B.total;
  c->sm_bin_maxlen = B.maxlen;
  return 0;
}

// series and means go with the set they belong to
void sm_drop_derived(SampleData *S) {
  S->series.release();
  S->cap = S->nrec = 0;
  S->t.clear();
  S->sU.release(); S->sP.release(); S->sU2.release();
  S->means = false;
  S->W = 0.0;
  S->count_acc = 0;
  S->rows.release();
}

// buffers of n points, the locate launch and the count of the located points.  In grid mode xs is written by the kernel.
int sm_locate(cfdh_ctx *c, size_t n, const SampleGrid *sg, const double *x, double tol) {
  const int D = c->dim;
  CHK(sm_need(c, tol));
  SampleData *S = c->sm;
  sm_drop_derived(S);
  S->n = 0;
  S->nlocated = 0;
  HIPCHK(c, S->x.alloc(n * D));
  HIPCHK(c, S->lam.alloc(n * (D + 1)));
  HIPCHK(c, S->cell.alloc(n));
  HIPCHK(c, S->count.alloc(SM_COUNT_BLOCKS));
  if (x) HIPCHK(c, hipMemcpyAsync(S->x.p, x, sizeof(double) * n * D, hipMemcpyHostToDevice, c->stream));
  SampleGrid g = {};
  if (sg) g = *sg;
  CHK(sm_time_begin(c, 0));
  if (D == 3)
    hipLaunchKernelGGL(sm_locate_kernel<3>, sm_blocks(n), dim3(TPB), 0, c->stream, n, sg ? 1 : 0, g, S->bg, (const int *)S->bptr.p, (const int *)S->blist.p,
                       (const int *)c->cells.p, (const double *)c->coords.p, tol, S->x.p, S->cell.p, S->lam.p);
  else
    hipLaunchKernelGGL(sm_locate_kernel<2>, sm_blocks(n), dim3(TPB), 0, c->stream, n, sg ? 1 : 0, g, S->bg, (const int *)S->bptr.p, (const int *)S->blist.p,
                       (const int *)c->cells.p, (const double *)c->coords.p, tol, S->x.p, S->cell.p, S->lam.p);
  HIPCHK(c, hipGetLastError());
  CHK(sm_time_end(c, 0));
  const int nb = (int)std::min<size_t>((n + TPB - 1) / TPB, SM_COUNT_BLOCKS);
  hipLaunchKernelGGL(sm_count_kernel, dim3(nb), dim3(TPB), 0, c->stream, n, (const int *)S->cell.p, S->count.p);
  HIPCHK(c, hipGetLastError());
  std::vector<int> part((size_t)nb);
  HIPCHK(c, hipMemcpyAsync(part.data(), S->count.p, sizeof(int) * nb, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));  // also: the caller's x has been read
  for (int v : part) S->nlocated += v;
  S->n = n;
  return 0;
}

void sm_remove_set(cfdh_ctx *c) {
  delete c->sm;
  c->sm = nullptr;
}

// one launch of the sample kernel on the current state
int sm_launch(cfdh_ctx *c, double *out, bool acc, double w) {
  SampleData *S = c->sm;
  const int D = c->dim;
  const double *u = c->x.p, *p = c->x.p + (size_t)D * c->nv;
  CHK(sm_time_begin(c, 1));
#define SM_LAUNCH(DD, ACC)                                                                                                                       \
  hipLaunchKernelGGL((sm_sample_kernel<DD, ACC>), sm_blocks(S->n), dim3(TPB), 0, c->stream, S->n, (const int *)S->cell.p, (const double *)S->lam.p, \
                     (const int *)c->cells.p, u, p, w, out, S->sU.p, S->sP.p, S->sU2.p)
  if (D == 3) { if (acc) SM_LAUNCH(3, true); else SM_LAUNCH(3, false); }
  else { if (acc) SM_LAUNCH(2, true); else SM_LAUNCH(2, false); }
#undef SM_LAUNCH
  HIPCHK(c, hipGetLastError());
  CHK(sm_time_end(c, 1));
  c->n_sample_launches++;
  return 0;
}

int sm_download(cfdh_ctx *c, void *host, const void *dev, size_t bytes) {
  if (bytes == 0) return 0;
  HIPCHK(c, hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

}  // namespace

void cfdh_sample_free(cfdh_ctx *c) { sm_remove_set(c); }

// cfdh_destroy: the buffers and the timing events
void cfdh_sample_destroy(cfdh_ctx *c) {
  sm_remove_set(c);
  for (hipEvent_t &e : c->sm_ev) {
    if (e) (void)hipEventDestroy(e);
    e = nullptr;
  }
  c->sm_timed[0] = c->sm_timed[1] = false;
}

static int sm_check_tol(cfdh_ctx *c, const char *who, double tol) {
  if (!cfdh_sample::finite(tol) || tol < 0.0 || tol > cfdh_sample::TOL_MAX) return cfdh_fail(c, CFDH_E_ARG, "%s: tol must be finite and lie in [0, 1e-3]", who);
  return 0;
}

int cfdh_sample_set_points_impl(cfdh_ctx *c, int64_t n, const double *x, double tol) {
  const char *who = "cfdh_sample_set_points";
  CHK(sm_supported(c, who));
  if (n < 0 || n > 0x7fffffffll) return cfdh_fail(c, CFDH_E_ARG, "%s: n must lie in [0, 2^31 - 1]", who);
  CHK(sm_check_tol(c, who, tol));
  if (n == 0) { sm_remove_set(c); return 0; }
  if (!x) return cfdh_fail(c, CFDH_E_ARG, "%s: x is NULL", who);
  for (size_t k = 0; k < (size_t)n * c->dim; k++)
    if (!cfdh_sample::finite(x[k])) return cfdh_fail(c, CFDH_E_ARG, "%s: coordinate %d of point %lld is not finite", who, (int)(k % c->dim), (long long)(k / c->dim));
  const int rc = sm_locate(c, (size_t)n, nullptr, x, tol);
  if (rc) sm_remove_set(c);
  return rc;
}

int cfdh_sample_set_grid_impl(cfdh_ctx *c, const double *origin, const double *spacing, const int64_t *dims, double tol) {
  const char *who = "cfdh_sample_set_grid";
  CHK(sm_supported(c, who));
  if (!origin || !spacing || !dims) return cfdh_fail(c, CFDH_E_ARG, "%s: origin, spacing or dims is NULL", who);
  SampleGrid g = {};
  long long n = 1;
  for (int a = 0; a < 3; a++) {
    g.origin[a] = 0.0; g.spacing[a] = 1.0; g.dims[a] = 1;
    if (dims[a] < 1) return cfdh_fail(c, CFDH_E_ARG, "%s: dims[%d] = %lld is below 1", who, a, (long long)dims[a]);
    if (a >= c->dim) {
      if (dims[a] != 1) return cfdh_fail(c, CFDH_E_ARG, "%s: dims[2] must be 1 in 2-D", who);
      continue;
    }
    if (!cfdh_sample::finite(origin[a]) || !cfdh_sample::finite(spacing[a])) return cfdh_fail(c, CFDH_E_ARG, "%s: origin[%d] or spacing[%d] is not finite", who, a, a);
    if (!(spacing[a] > 0.0)) return cfdh_fail(c, CFDH_E_ARG, "%s: spacing[%d] must be positive", who, a);
    if (dims[a] > 0x7fffffffll || (n *= dims[a]) > 0x7fffffffll) return cfdh_fail(c, CFDH_E_ARG, "%s: the grid has more than 2^31 - 1 nodes", who);
    g.origin[a] = origin[a]; g.spacing[a] = spacing[a]; g.dims[a] = dims[a];
  }
  CHK(sm_check_tol(c, who, tol));
  const int rc = sm_locate(c, (size_t)n, &g, nullptr, tol);
  if (rc) sm_remove_set(c);
  return rc;
}

int cfdh_sample_get_location_impl(cfdh_ctx *c, int64_t *n, int32_t *cell, double *lambda, double *x) {
  const char *who = "cfdh_sample_get_location";
  CHK(sm_supported(c, who));
  if (!n) return cfdh_fail(c, CFDH_E_ARG, "%s: n is NULL", who);
  SampleData *S = c->sm;
  *n = S ? (int64_t)S->n : 0;
  if (!S || S->n == 0) return 0;
  const int n1 = c->dim + 1;
  if (x) CHK(sm_download(c, x, S->x.p, sizeof(double) * S->n * c->dim));
  if (!cell && !lambda) return 0;
  std::vector<int> st(S->n);
  CHK(sm_download(c, st.data(), S->cell.p, sizeof(int) * S->n));
  if (lambda) {
    CHK(sm_download(c, lambda, S->lam.p, sizeof(double) * S->n * n1));
    // the context swapped the last two vertices of the cells the caller gave in negative orientation
    for (size_t i = 0; i < S->n; i++)
      if (st[i] >= 0 && c->cell_flipped[st[i]]) std::swap(lambda[n1 * i + n1 - 2], lambda[n1 * i + n1 - 1]);
  }
  if (cell)
    for (size_t i = 0; i < S->n; i++) cell[i] = st[i] >= 0 ? c->cell_user[st[i]] : -1;
  return 0;
}

// the checks every sampling call shares: a set and a state
static int sm_ready(cfdh_ctx *c, const char *who) {
  if (!c->sm || c->sm->n == 0) return cfdh_fail(c, CFDH_E_STATE, "%s: no sample set (cfdh_sample_set_points or cfdh_sample_set_grid)", who);
  return 0;
}

int cfdh_sample_now_impl(cfdh_ctx *c, int64_t *n, double *out) {
  const char *who = "cfdh_sample_now";
  CHK(sm_supported(c, who));
  if (!n) return cfdh_fail(c, CFDH_E_ARG, "%s: n is NULL", who);
  CHK(sm_ready(c, who));
  SampleData *S = c->sm;
  *n = (int64_t)S->n;
  if (!out) return 0;
  if (!c->state_set) return cfdh_fail(c, CFDH_E_STATE, "%s: a state is needed (cfdh_set_state or a solved step)", who);
  const size_t m = S->n * (c->dim + 1);
  HIPCHK(c, S->rows.alloc(m));
  CHK(sm_launch(c, S->rows.p, false, 0.0));
  return sm_download(c, out, S->rows.p, sizeof(double) * m);
}

int cfdh_sample_series_enable_impl(cfdh_ctx *c, int64_t rows) {
  const char *who = "cfdh_sample_series_enable";
  CHK(sm_supported(c, who));
  if (rows < 0 || rows > 0x7fffffffll) return cfdh_fail(c, CFDH_E_ARG, "%s: rows must lie in [0, 2^31 - 1]", who);
  CHK(sm_ready(c, who));
  SampleData *S = c->sm;
  S->series.release();
  S->cap = S->nrec = 0;
  S->t.clear();
  if (rows == 0) return 0;
  // rows and n are below 2^31 each: their product fits 64 bits, the byte count need not
  const unsigned long long blocks = (unsigned long long)rows * S->n, per = 8ull * (c->dim + 1);
  if (blocks > SM_SERIES_MAX_BYTES / per)
    return cfdh_fail(c, CFDH_E_ARG, "%s: %lld row blocks of %lld points are more than 2^40 bytes", who, (long long)rows, (long long)S->n);
  HIPCHK(c, S->series.alloc((size_t)blocks * (c->dim + 1)));
  S->cap = (size_t)rows;
  S->t.reserve(S->cap);
  return 0;
}

int cfdh_sample_record_impl(cfdh_ctx *c, double t) {
  const char *who = "cfdh_sample_record";
  CHK(sm_supported(c, who));
  CHK(sm_ready(c, who));
  SampleData *S = c->sm;
  if (S->cap == 0) return cfdh_fail(c, CFDH_E_STATE, "%s: cfdh_sample_series_enable was not called", who);
  if (!c->state_set) return cfdh_fail(c, CFDH_E_STATE, "%s: a state is needed (cfdh_set_state or a solved step)", who);
  if (S->nrec == S->cap)
    return cfdh_fail(c, CFDH_E_STATE, "%s: the series buffer holds its %lld row blocks; empty it with cfdh_sample_series_get(ctx, &rows, t, out)", who, (long long)S->cap);
  CHK(sm_launch(c, S->series.p + S->nrec * S->n * (c->dim + 1), false, 0.0));
  S->t.push_back(t);
  S->nrec++;
  return 0;
}

int cfdh_sample_series_get_impl(cfdh_ctx *c, int64_t *rows, double *t, double *out) {
  const char *who = "cfdh_sample_series_get";
  CHK(sm_supported(c, who));
  if (!rows) return cfdh_fail(c, CFDH_E_ARG, "%s: rows is NULL", who);
  CHK(sm_ready(c, who));
  SampleData *S = c->sm;
  if (S->cap == 0) return cfdh_fail(c, CFDH_E_STATE, "%s: cfdh_sample_series_enable was not called", who);
  *rows = (int64_t)S->nrec;
  if (!out) return 0;
  CHK(sm_download(c, out, S->series.p, sizeof(double) * S->nrec * S->n * (c->dim + 1)));
  if (t)
    for (size_t k = 0; k < S->nrec; k++) t[k] = S->t[k];
  S->nrec = 0;
  S->t.clear();
  return 0;
}

int cfdh_sample_mean_reset_impl(cfdh_ctx *c) {
  const char *who = "cfdh_sample_mean_reset";
  CHK(sm_supported(c, who));
  CHK(sm_ready(c, who));
  SampleData *S = c->sm;
  HIPCHK(c, S->sU.alloc(S->n * c->dim));
  HIPCHK(c, S->sP.alloc(S->n));
  HIPCHK(c, S->sU2.alloc(S->n));
  for (dbuf<double> *b : {&S->sU, &S->sP, &S->sU2}) HIPCHK(c, b->zero(c->stream));
  S->W = 0.0;
  S->count_acc = 0;
  S->means = true;
  return 0;
}

int cfdh_sample_mean_accumulate_impl(cfdh_ctx *c, double weight) {
  const char *who = "cfdh_sample_mean_accumulate";
  CHK(sm_supported(c, who));
  if (!cfdh_sample::finite(weight) || !(weight > 0.0)) return cfdh_fail(c, CFDH_E_ARG, "%s: the weight must be finite and > 0", who);
  if (!c->sm || !c->sm->means) return cfdh_fail(c, CFDH_E_STATE, "%s: cfdh_sample_mean_reset was not called", who);
  if (!c->state_set) return cfdh_fail(c, CFDH_E_STATE, "%s: a state is needed (cfdh_set_state or a solved step)", who);
  SampleData *S = c->sm;
  CHK(sm_launch(c, nullptr, true, weight));
  S->W += weight;
  S->count_acc++;
  return 0;
}

int cfdh_sample_mean_get_impl(cfdh_ctx *c, int which, int64_t *n, double *out) {
  const char *who = "cfdh_sample_mean_get";
  CHK(sm_supported(c, who));
  if (!n) return cfdh_fail(c, CFDH_E_ARG, "%s: n is NULL", who);
  if (which < 0 || which > 3) return cfdh_fail(c, CFDH_E_ARG, "%s: unknown field %d (0 mean velocity, 1 mean pressure, 2 fluctuation energy, 3 {W, count})", who, which);
  if (!c->sm || !c->sm->means) return cfdh_fail(c, CFDH_E_STATE, "%s: cfdh_sample_mean_reset was not called", who);
  SampleData *S = c->sm;
  if (which == 3) {
    *n = 2;
    if (out) { out[0] = S->W; out[1] = (double)S->count_acc; }
    return 0;
  }
  if (!(S->W > 0.0)) return cfdh_fail(c, CFDH_E_STATE, "%s: nothing accumulated since the last reset", who);
  const size_t m = S->n * (which == 0 ? (size_t)c->dim : 1);
  *n = (int64_t)m;
  if (!out) return 0;
  HIPCHK(c, S->rows.alloc(S->n * (c->dim + 1)));
  if (c->dim == 3)
    hipLaunchKernelGGL(sm_mean_kernel<3>, sm_blocks(S->n), dim3(TPB), 0, c->stream, S->n, which, S->W, (const double *)S->sU.p, (const double *)S->sP.p,
                       (const double *)S->sU2.p, S->rows.p);
  else
    hipLaunchKernelGGL(sm_mean_kernel<2>, sm_blocks(S->n), dim3(TPB), 0, c->stream, S->n, which, S->W, (const double *)S->sU.p, (const double *)S->sP.p,
                       (const double *)S->sU2.p, S->rows.p);
  HIPCHK(c, hipGetLastError());
  return sm_download(c, out, S->rows.p, sizeof(double) * m);
}

int64_t cfdh_sample_info(const cfdh_ctx *c, int what) {
  switch (what) {
    case 111: return c->sm ? (int64_t)c->sm->n : 0;
    case 112: return c->sm ? c->sm->nlocated : 0;
    case 113: return c->n_sample_launches;
    case 114: return c->sm ? (int64_t)c->sm->nrec : 0;
    case 115: case 116: {  // nanoseconds of the last locate / sample kernel
      const int k = what - 115;
      float ms = 0.f;
      if (!c->sm_timed[k] || hipEventSynchronize(c->sm_ev[2 * k + 1]) != hipSuccess || hipEventElapsedTime(&ms, c->sm_ev[2 * k], c->sm_ev[2 * k + 1]) != hipSuccess)
        return 0;
      return (int64_t)((double)ms * 1e6);
    }
    case 117: return c->sm_bin_doublings;  // the bin grid built last: doublings of the edge, total and longest list
    case 118: return c->sm_bin_total;
    case 119: return c->sm_bin_maxlen;
    default: return 0;
  }
}
