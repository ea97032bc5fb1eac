// Volumetric flow diagnostics of the closed-form P1 contexts (cfdh_flow_*, include/cfdh.h): vorticity, Q-criterion, shear rate,
// viscous dissipation, helicity, the energy integrals and the pulsatile window averages of the velocity that sits in HBM between
// cfdh_solve_step and cfdh_advance.  A P1 velocity has one constant gradient G_c per cell; the vertex value is the volume-weighted
// mean of the cells around the vertex.
//
// Two passes.  The cell pass (one lane per cell) reads the cell's d + 1 vertex ids, coordinates and velocities and writes the row
// (|c|, G_c) of d d + 1 doubles; the vertex pass (one lane per vertex) runs over the cells of its vertex in a fixed order through the
// sliced inverted index of cfdh_flow_host.hpp, forms G_v = sum |c| G_c / sum |c| in registers and ends in the pointwise formula that
// was asked for.  Gather only, no atomics: two calls on one state return the same bytes.  DESIGN.md section 9 counts the bytes and
// the dependent memory trips behind the two choices made here (geometry recomputed, not cached; two passes, not one).
//
// Every local index is a compile-time constant after unrolling (template <int D>), so G, the cell's velocities and the sums stay
// in registers.
#include <hip/hip_runtime.h>

#include <cmath>
#include <new>

#include "cfdh_flow_host.hpp"
#include "cfdh_internal.hpp"
#include "cfdh_wave.hpp"

struct FlowData {
  int nslices = 0;
  dbuf<int> sptr, dinc;    // the inverted index (cfdh_flow::CellIndex)
  dbuf<double> contrib;    // [nc][d d + 1]: |c|, G_c row-major
  dbuf<double> out;        // [nv][d d]: the field of cfdh_flow_field / cfdh_flow_stats_get before its download
  // window averages (cfdh_flow_stats_*): allocated by the first reset
  bool stats = false;
  dbuf<double> sU, sU2, sPhi, sGam, sMax;  // sum w u [nv][d], sum w |u|^2, sum w phi, sum w gamma, max gamma
  double W = 0.0;
  long long count = 0;
};

namespace {

template <int D>
struct FlowPoint {
  double w[3], ss, ww;  // vorticity (2-D: w[2] only), S:S, W:W
};

template <int D>
__device__ __forceinline__ FlowPoint<D> fl_point(const double (&G)[D][D]) {
  FlowPoint<D> q;
  q.w[0] = q.w[1] = 0.0;
  if constexpr (D == 3) { q.w[0] = G[2][1] - G[1][2]; q.w[1] = G[0][2] - G[2][0]; }
  q.w[2] = G[1][0] - G[0][1];
  q.ss = 0.0; q.ww = 0.0;
#pragma unroll
  for (int i = 0; i < D; i++)
#pragma unroll
    for (int j = 0; j < D; j++) {
      const double s = 0.5 * (G[i][j] + G[j][i]), a = 0.5 * (G[i][j] - G[j][i]);
      q.ss += s * s;
      q.ww += a * a;
    }
  return q;
}

// |c|, G_c and the corner velocities of cell e.  A degenerate cell (det == 0) contributes nothing.
template <int D>
__device__ __forceinline__ void fl_cell(const int *__restrict__ cells, const double *__restrict__ coords, const double *__restrict__ u, int e,
                                        double &vol, double (&G)[D][D], double (&U)[D + 1][D]) {
  double X[D + 1][D];
#pragma unroll
  for (int a = 0; a <= D; a++) {
    const int v = cells[(size_t)(D + 1) * e + a];
#pragma unroll
    for (int i = 0; i < D; i++) { X[a][i] = coords[(size_t)D * v + i]; U[a][i] = u[(size_t)D * v + i]; }
  }
  double E[D][D], g[D][D], det;  // E[k] = x_{k+1} - x_0 ; g[k] = grad lambda_{k+1} times det
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
  vol = fabs(det) * (D == 2 ? 0.5 : 1.0 / 6.0);
  const double rdet = det != 0.0 ? 1.0 / det : 0.0;
#pragma unroll
  for (int i = 0; i < D; i++)
#pragma unroll
    for (int j = 0; j < D; j++) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < D; k++) s += (U[k + 1][i] - U[0][i]) * g[k][j];
      G[i][j] = s * rdet;
    }
}

template <int D>
__global__ __launch_bounds__(TPB) void fl_cell_kernel(int nc, const int *__restrict__ cells, const double *__restrict__ coords, const double *__restrict__ u,
                                                     double *__restrict__ contrib) {
  const int e = blockIdx.x * TPB + threadIdx.x;
  if (e >= nc) return;
  double vol, G[D][D], U[D + 1][D];
  fl_cell<D>(cells, coords, u, e, vol, G, U);
  double *row = contrib + (size_t)(D * D + 1) * e;
  row[0] = vol;
#pragma unroll
  for (int i = 0; i < D; i++)
#pragma unroll
    for (int j = 0; j < D; j++) row[1 + D * i + j] = G[i][j];
}

// G_v of vertex v (< nv): the cells of the vertex in the order of the index.  A vertex of no cell has G_v = 0.
template <int D>
__device__ __forceinline__ void fl_recover(int v, const int *__restrict__ sptr, const int *__restrict__ dinc, const double *__restrict__ contrib,
                                           double (&G)[D][D]) {
  const int s = v >> 6, lane = v & 63;
  double den = 0.0;
#pragma unroll
  for (int i = 0; i < D; i++)
#pragma unroll
    for (int j = 0; j < D; j++) G[i][j] = 0.0;
  const int k1 = sptr[s + 1];
  for (int k = sptr[s]; k < k1; k++) {
    const int e = dinc[(size_t)k * cfdh_flow::SLICE + lane];
    if (e < 0) continue;
    const double *row = contrib + (size_t)(D * D + 1) * e;
    const double vol = row[0];
    den += vol;
#pragma unroll
    for (int i = 0; i < D; i++)
#pragma unroll
      for (int j = 0; j < D; j++) G[i][j] += vol * row[1 + D * i + j];
  }
  const double r = den > 0.0 ? 1.0 / den : 0.0;
#pragma unroll
  for (int i = 0; i < D; i++)
#pragma unroll
    for (int j = 0; j < D; j++) G[i][j] *= r;
}

template <int D>
__global__ __launch_bounds__(TPB) void fl_field_kernel(int nv, int which, double mu, const int *__restrict__ sptr, const int *__restrict__ dinc,
                                                      const double *__restrict__ contrib, const double *__restrict__ u, double *__restrict__ out) {
  const int v = blockIdx.x * TPB + threadIdx.x;
  if (v >= nv) return;
  double G[D][D];
  fl_recover<D>(v, sptr, dinc, contrib, G);
  if (which == 0) {
#pragma unroll
    for (int i = 0; i < D; i++)
#pragma unroll
      for (int j = 0; j < D; j++) out[(size_t)(D * D) * v + D * i + j] = G[i][j];
    return;
  }
  const FlowPoint<D> q = fl_point<D>(G);
  if (which == 1) {
    if constexpr (D == 2) out[v] = q.w[2];
    else { out[(size_t)3 * v] = q.w[0]; out[(size_t)3 * v + 1] = q.w[1]; out[(size_t)3 * v + 2] = q.w[2]; }
  } else if (which == 2) {
    out[v] = 0.5 * (q.ww - q.ss);
  } else if (which == 3) {
    out[v] = sqrt(2.0 * q.ss);
  } else if (which == 4) {
    out[v] = 2.0 * mu * q.ss;
  } else if constexpr (D == 3) {  // 5: helicity density, 6: local normalised helicity
    double h = 0.0, u2 = 0.0, w2 = 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++) {
      const double ui = u[(size_t)D * v + i];
      h += ui * q.w[i]; u2 += ui * ui; w2 += q.w[i] * q.w[i];
    }
    if (which == 5) out[v] = h;
    else {
      const double nu = sqrt(u2), nw = sqrt(w2);
      out[v] = (nu == 0.0 || nw == 0.0) ? 0.0 : h / (nu * nw);
    }
  }
}

// one trip over the d + 4 accumulators of a vertex
template <int D>
__global__ __launch_bounds__(TPB) void fl_accumulate_kernel(int nv, double w, double mu, const int *__restrict__ sptr, const int *__restrict__ dinc,
                                                           const double *__restrict__ contrib, const double *__restrict__ u, double *__restrict__ sU,
                                                           double *__restrict__ sU2, double *__restrict__ sPhi, double *__restrict__ sGam,
                                                           double *__restrict__ sMax) {
  const int v = blockIdx.x * TPB + threadIdx.x;
  if (v >= nv) return;
  double G[D][D];
  fl_recover<D>(v, sptr, dinc, contrib, G);
  const FlowPoint<D> q = fl_point<D>(G);
  double u2 = 0.0;
#pragma unroll
  for (int i = 0; i < D; i++) {
    const double ui = u[(size_t)D * v + i];
    u2 += ui * ui;
    sU[(size_t)D * v + i] += w * ui;
  }
  const double gam = sqrt(2.0 * q.ss);
  sU2[v] += w * u2;
  sPhi[v] += w * (2.0 * mu * q.ss);
  sGam[v] += w * gam;
  sMax[v] = fmax(sMax[v], gam);
}

// which 0: sU / W ; 1: max(0, (sU2 / W - |sU / W|^2) / 2) ; 2: sPhi / W ; 3: sGam / W ; 4: sMax
template <int D>
__global__ __launch_bounds__(TPB) void fl_derive_kernel(int nv, int which, double W, const double *__restrict__ sU, const double *__restrict__ sU2,
                                                       const double *__restrict__ sPhi, const double *__restrict__ sGam, const double *__restrict__ sMax,
                                                       double *__restrict__ out) {
  const int v = blockIdx.x * TPB + threadIdx.x;
  if (v >= nv) return;
  if (which == 0) {
#pragma unroll
    for (int i = 0; i < D; i++) out[(size_t)D * v + i] = sU[(size_t)D * v + i] / W;
  } else if (which == 1) {
    double m2 = 0.0;
#pragma unroll
    for (int i = 0; i < D; i++) { const double m = sU[(size_t)D * v + i] / W; m2 += m * m; }
    out[v] = fmax(0.0, 0.5 * (sU2[v] / W - m2));
  } else if (which == 2) {
    out[v] = sPhi[v] / W;
  } else if (which == 3) {
    out[v] = sGam[v] / W;
  } else {
    out[v] = sMax[v];
  }
}

// the 8 cell-exact integrals: partial[k nb + block], summed per block in a fixed order
template <int D>
__global__ __launch_bounds__(TPB) void fl_integrals_kernel(int nc, double rho, double mu, const int *__restrict__ cells, const double *__restrict__ coords,
                                                          const double *__restrict__ u, double *__restrict__ partial) {
  __shared__ double sh[4];
  double a[8];
#pragma unroll
  for (int k = 0; k < 8; k++) a[k] = 0.0;
  for (int e = blockIdx.x * TPB + threadIdx.x; e < nc; e += gridDim.x * TPB) {
    double vol, G[D][D], U[D + 1][D];
    fl_cell<D>(cells, coords, u, e, vol, G, U);
    const FlowPoint<D> q = fl_point<D>(G);
    double sq = 0.0, sm2 = 0.0, hel = 0.0, tr = 0.0;
#pragma unroll
    for (int i = 0; i < D; i++) {
      double sm = 0.0;
#pragma unroll
      for (int b = 0; b <= D; b++) { sq += U[b][i] * U[b][i]; sm += U[b][i]; }
      sm2 += sm * sm;
      if constexpr (D == 3) hel += sm * q.w[i];
      tr += G[i][i];
    }
    double w2 = q.w[2] * q.w[2];
    if constexpr (D == 3) w2 += q.w[0] * q.w[0] + q.w[1] * q.w[1];
    a[0] += vol;
    a[1] += 0.5 * rho * vol * (sq + sm2) * (1.0 / ((D + 1) * (D + 2)));
    a[2] += 0.5 * vol * w2;
    a[3] += vol * (2.0 * mu * q.ss);
    a[4] += vol * hel * (1.0 / (D + 1));
    a[5] += vol * tr;
    a[6] += vol * (0.5 * (q.ww - q.ss));
    a[7] += vol * tr * tr;
  }
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const double s = block_sum(a[k], sh);
    if (threadIdx.x == 0) partial[(size_t)k * gridDim.x + blockIdx.x] = s;
  }
}

// the contexts that carry the diagnostics; everything else is refused before any device work
int fl_supported(cfdh_ctx *c, const char *who) {
  if (c->ipcs) return cfdh_fail(c, CFDH_E_ARG, "%s: not available on an incremental pressure-correction context (cfdh_create_ipcs)", who);
  if (c->gen) return cfdh_fail(c, CFDH_E_ARG, "%s: the flow diagnostics live on the closed-form P1 contexts (cfdh_create), not on the generic element kernels", who);
  if (c->nranks > 1 || c->nvo != c->nv) return cfdh_fail(c, CFDH_E_ARG, "%s: not available in partitioned runs", who);
  return 0;
}

// device events around kernel k (0: the cell pass, 1: the vertex, accumulate or integral kernel behind it), read by cfdh_info 109 / 110
int fl_time_begin(cfdh_ctx *c, int k) {
  for (int i = 2 * k; i < 2 * k + 2; i++)
    if (!c->fl_ev[i]) HIPCHK(c, hipEventCreate(&c->fl_ev[i]));
  HIPCHK(c, hipEventRecord(c->fl_ev[2 * k], c->stream));
  return 0;
}
int fl_time_end(cfdh_ctx *c, int k) {
  HIPCHK(c, hipEventRecord(c->fl_ev[2 * k + 1], c->stream));
  c->fl_timed[k] = true;
  return 0;
}

// index, contribution rows and output field: allocated by the first call that needs them
int fl_need(cfdh_ctx *c) {
  if (c->fl) return 0;
  const int D = c->dim;
  std::vector<int> visit((size_t)c->nc, 0);
  for (int e = 0; e < c->nc; e++) {
    const int k = c->cell_user[e];
    if (k < 0 || k >= c->nc) return cfdh_fail(c, CFDH_E_STATE, "flow diagnostics: the context does not hold every cell of the mesh");
    visit[k] = e;
  }
  cfdh_flow::CellIndex ix;
  std::string why;
  if (!cfdh_flow::build_index(D, c->nv, c->nc, c->h_cells.data(), visit.data(), ix, why)) return cfdh_fail(c, CFDH_E_ARG, "%s", why.c_str());
  FlowData *F = new (std::nothrow) FlowData();
  if (!F) return cfdh_fail(c, CFDH_E_NOMEM, "out of host memory");
  c->fl = F;
  int rc = [&]() -> int {
    F->nslices = ix.nslices;
    HIPCHK(c, F->sptr.upload(ix.sptr, c->stream));
    HIPCHK(c, F->dinc.upload(ix.dinc, c->stream));
    HIPCHK(c, F->contrib.alloc((size_t)c->nc * (D * D + 1)));
    HIPCHK(c, F->out.alloc((size_t)c->nv * (D * D)));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // the host vectors go out of scope
    return 0;
  }();
  if (rc) cfdh_flow_free(c);
  return rc;
}

int fl_cell_pass(cfdh_ctx *c) {
  FlowData *F = c->fl;
  if (c->nc == 0) return 0;
  const dim3 gr((c->nc + TPB - 1) / TPB), bl(TPB);
  CHK(fl_time_begin(c, 0));
  if (c->dim == 3)
    hipLaunchKernelGGL(fl_cell_kernel<3>, gr, bl, 0, c->stream, c->nc, (const int *)c->cells.p, (const double *)c->coords.p, (const double *)c->x.p, F->contrib.p);
  else
    hipLaunchKernelGGL(fl_cell_kernel<2>, gr, bl, 0, c->stream, c->nc, (const int *)c->cells.p, (const double *)c->coords.p, (const double *)c->x.p, F->contrib.p);
  HIPCHK(c, hipGetLastError());
  CHK(fl_time_end(c, 0));
  c->n_flow_cell_passes++;
  return 0;
}

// out [nv][width] in the caller's vertex numbering from the device field in the context's
int fl_download(cfdh_ctx *c, const double *dev, size_t width, double *out) {
  std::vector<double> h(width * (size_t)c->nv);
  if (h.empty()) return 0;
  HIPCHK(c, hipMemcpyAsync(h.data(), dev, sizeof(double) * h.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int k = 0; k < c->nv; k++) {
    const size_t v = (size_t)c->iperm[k];
    for (size_t i = 0; i < width; i++) out[width * v + i] = h[width * (size_t)k + i];
  }
  return 0;
}

}  // namespace

void cfdh_flow_free(cfdh_ctx *c) {
  delete c->fl;
  c->fl = nullptr;
}

// cfdh_destroy: the buffers and the timing events (the events belong to the context, not to FlowData: cfdh_flow_integrals
// records them without allocating a buffer)
void cfdh_flow_destroy(cfdh_ctx *c) {
  cfdh_flow_free(c);
  for (hipEvent_t &e : c->fl_ev) {
    if (e) (void)hipEventDestroy(e);
    e = nullptr;
  }
  c->fl_timed[0] = c->fl_timed[1] = false;
}

int cfdh_flow_field_impl(cfdh_ctx *c, int which, int64_t *n, double *out) {
  const char *who = "cfdh_flow_field";
  CHK(fl_supported(c, who));
  const int D = c->dim, width = cfdh_flow::field_width(D, which);
  if (width == 0) {
    if (D == 2 && (which == 5 || which == 6)) return cfdh_fail(c, CFDH_E_ARG, "%s: helicity and LNH (which %d) exist in 3-D only", who, which);
    return cfdh_fail(c, CFDH_E_ARG, "%s: unknown field %d (0 gradient, 1 vorticity, 2 Q, 3 shear rate, 4 dissipation, 5 helicity, 6 LNH)", who, which);
  }
  if (!n) return cfdh_fail(c, CFDH_E_ARG, "%s: n is NULL", who);
  *n = (int64_t)width * c->nv;
  if (!out) return 0;
  if (!c->state_set) return cfdh_fail(c, CFDH_E_STATE, "%s: a state is needed (cfdh_set_state or a solved step)", who);
  if (which == 4 && !c->params_set) return cfdh_fail(c, CFDH_E_STATE, "%s: the dissipation needs mu of cfdh_set_params", who);
  CHK(fl_need(c));
  FlowData *F = c->fl;
  if (c->nv == 0) return 0;
  CHK(fl_cell_pass(c));
  const dim3 gr((c->nv + TPB - 1) / TPB), bl(TPB);
  CHK(fl_time_begin(c, 1));
  if (D == 3)
    hipLaunchKernelGGL(fl_field_kernel<3>, gr, bl, 0, c->stream, c->nv, which, c->mu, (const int *)F->sptr.p, (const int *)F->dinc.p,
                       (const double *)F->contrib.p, (const double *)c->x.p, F->out.p);
  else
    hipLaunchKernelGGL(fl_field_kernel<2>, gr, bl, 0, c->stream, c->nv, which, c->mu, (const int *)F->sptr.p, (const int *)F->dinc.p,
                       (const double *)F->contrib.p, (const double *)c->x.p, F->out.p);
  HIPCHK(c, hipGetLastError());
  CHK(fl_time_end(c, 1));
  return fl_download(c, F->out.p, (size_t)width, out);
}

int cfdh_flow_integrals_impl(cfdh_ctx *c, double *out) {
  const char *who = "cfdh_flow_integrals";
  CHK(fl_supported(c, who));
  if (!out) return cfdh_fail(c, CFDH_E_ARG, "%s: out is NULL", who);
  if (!c->params_set || !c->state_set) return cfdh_fail(c, CFDH_E_STATE, "%s: parameters (cfdh_set_params) and a state are needed", who);
  const int nb = red_grid(c, c->nc);
  const dim3 gr(nb), bl(TPB);
  CHK(fl_time_begin(c, 1));
  if (c->dim == 3)
    hipLaunchKernelGGL(fl_integrals_kernel<3>, gr, bl, 0, c->stream, c->nc, c->rho, c->mu, (const int *)c->cells.p, (const double *)c->coords.p,
                       (const double *)c->x.p, c->red_partial.p);
  else
    hipLaunchKernelGGL(fl_integrals_kernel<2>, gr, bl, 0, c->stream, c->nc, c->rho, c->mu, (const int *)c->cells.p, (const double *)c->coords.p,
                       (const double *)c->x.p, c->red_partial.p);
  HIPCHK(c, hipGetLastError());
  CHK(fl_time_end(c, 1));
  ScalarRead h;
  CHK(scalars_finish(c, c->red_out.p + RO_FLOW, RO_FLOW_N, 0, nb, &h));
  return scalars_read(c, h, out);
}

int cfdh_flow_stats_reset_impl(cfdh_ctx *c) {
  CHK(fl_supported(c, "cfdh_flow_stats_reset"));
  CHK(fl_need(c));
  FlowData *F = c->fl;
  const size_t nv = (size_t)c->nv;
  HIPCHK(c, F->sU.alloc(nv * c->dim));
  for (dbuf<double> *b : {&F->sU2, &F->sPhi, &F->sGam, &F->sMax}) HIPCHK(c, b->alloc(nv));
  for (dbuf<double> *b : {&F->sU, &F->sU2, &F->sPhi, &F->sGam, &F->sMax}) HIPCHK(c, b->zero(c->stream));
  F->W = 0.0;
  F->count = 0;
  F->stats = true;
  return 0;
}

int cfdh_flow_stats_accumulate_impl(cfdh_ctx *c, double weight) {
  const char *who = "cfdh_flow_stats_accumulate";
  CHK(fl_supported(c, who));
  if (!cfdh_flow::finite(weight) || !(weight > 0.0)) return cfdh_fail(c, CFDH_E_ARG, "%s: the weight must be finite and > 0", who);
  if (!c->fl || !c->fl->stats) return cfdh_fail(c, CFDH_E_STATE, "%s: cfdh_flow_stats_reset was not called", who);
  if (!c->params_set || !c->state_set) return cfdh_fail(c, CFDH_E_STATE, "%s: parameters (cfdh_set_params) and a state are needed", who);
  FlowData *F = c->fl;
  if (c->nv > 0) {
    CHK(fl_cell_pass(c));
    const dim3 gr((c->nv + TPB - 1) / TPB), bl(TPB);
    CHK(fl_time_begin(c, 1));
    if (c->dim == 3)
      hipLaunchKernelGGL(fl_accumulate_kernel<3>, gr, bl, 0, c->stream, c->nv, weight, c->mu, (const int *)F->sptr.p, (const int *)F->dinc.p,
                         (const double *)F->contrib.p, (const double *)c->x.p, F->sU.p, F->sU2.p, F->sPhi.p, F->sGam.p, F->sMax.p);
    else
      hipLaunchKernelGGL(fl_accumulate_kernel<2>, gr, bl, 0, c->stream, c->nv, weight, c->mu, (const int *)F->sptr.p, (const int *)F->dinc.p,
                         (const double *)F->contrib.p, (const double *)c->x.p, F->sU.p, F->sU2.p, F->sPhi.p, F->sGam.p, F->sMax.p);
    HIPCHK(c, hipGetLastError());
    CHK(fl_time_end(c, 1));
  }
  F->W += weight;
  F->count++;
  return 0;
}

int cfdh_flow_stats_get_impl(cfdh_ctx *c, int which, int64_t *n, double *out) {
  const char *who = "cfdh_flow_stats_get";
  CHK(fl_supported(c, who));
  if (!n) return cfdh_fail(c, CFDH_E_ARG, "%s: n is NULL", who);
  if (which < 0 || which > 5) return cfdh_fail(c, CFDH_E_ARG, "%s: unknown field %d (0 mean velocity, 1 fluctuation energy, 2 mean dissipation, 3 mean shear rate, 4 peak shear rate, 5 {W, count})", who, which);
  if (!c->fl || !c->fl->stats) return cfdh_fail(c, CFDH_E_STATE, "%s: cfdh_flow_stats_reset was not called", who);
  FlowData *F = c->fl;
  if (which == 5) {
    *n = 2;
    if (out) { out[0] = F->W; out[1] = (double)F->count; }
    return 0;
  }
  if (!(F->W > 0.0)) return cfdh_fail(c, CFDH_E_STATE, "%s: nothing accumulated since the last reset", who);
  const size_t width = which == 0 ? (size_t)c->dim : 1;
  *n = (int64_t)(width * (size_t)c->nv);
  if (!out || c->nv == 0) return 0;
  const dim3 gr((c->nv + TPB - 1) / TPB), bl(TPB);
  if (c->dim == 3)
    hipLaunchKernelGGL(fl_derive_kernel<3>, gr, bl, 0, c->stream, c->nv, which, F->W, (const double *)F->sU.p, (const double *)F->sU2.p,
                       (const double *)F->sPhi.p, (const double *)F->sGam.p, (const double *)F->sMax.p, F->out.p);
  else
    hipLaunchKernelGGL(fl_derive_kernel<2>, gr, bl, 0, c->stream, c->nv, which, F->W, (const double *)F->sU.p, (const double *)F->sU2.p,
                       (const double *)F->sPhi.p, (const double *)F->sGam.p, (const double *)F->sMax.p, F->out.p);
  HIPCHK(c, hipGetLastError());
  return fl_download(c, F->out.p, width, out);
}

int64_t cfdh_flow_info(const cfdh_ctx *c, int what) {
  if (what == 106) return c->fl ? 1 : 0;
  if (what == 107) return c->n_flow_cell_passes;
  if (what == 109 || what == 110) {  // nanoseconds of the last cell pass / of the last kernel behind it
    const int k = what - 109;
    float ms = 0.f;
    if (!c->fl_timed[k] || hipEventSynchronize(c->fl_ev[2 * k + 1]) != hipSuccess || hipEventElapsedTime(&ms, c->fl_ev[2 * k], c->fl_ev[2 * k + 1]) != hipSuccess)
      return 0;
    return (int64_t)((double)ms * 1e6);
  }
  return c->fl && c->fl->stats ? c->fl->count : 0;
}
