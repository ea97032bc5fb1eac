// Lagrangian particle tracking on the closed-form P1 contexts (cfdh_particles_*, include/cfdh.h): massless particles follow
// w(x, s) = (1 - s) u_prev(x) + s u_sol(x) over the step the flow solver has just taken, by explicit midpoint substeps, and
// collect their path length and shear exposure on the way.  One lane owns one particle from the first substep to the last: it
// evaluates the P1 velocity from the barycentric coordinates of its cell, walks from cell to cell through the neighbour table and
// stops for good at the first exterior facet.  Nobody else touches the particle: no atomics, and two steps from the same state give
// the same bytes.  The tables are built by the plain C++ header cfdh_particles_host.hpp.
//
// The arithmetic of a substep is kept free of fused multiply-adds: tests/particles_twin.py restates it operation by operation, and
// the decisions of the walk (inside a cell or not, which facet first) then fall the same way on both sides except on a tie.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <limits>
#include <new>

#include "cfdh_internal.hpp"
#include "cfdh_particles_host.hpp"
#include "cfdh_wave.hpp"

#pragma clang fp contract(off)

struct ParticleData {
  int cap = 0, n = 0, nsub = 1;
  long long active = 0;               // particles with status 0
  double t_last = -std::numeric_limits<double>::infinity();  // time after the last step
  std::vector<int> cell_int;          // caller's cell -> device-ordered cell, -1: not held
  std::vector<double> h_aff;          // host copy of the affine table (seed checks)
  dbuf<int> nb;                       // [nc][d + 1]
  dbuf<double> aff;                   // [nc][d d + d]
  dbuf<double> x, t_birth, t_end, path, expo;  // x: [d][cap]
  dbuf<int> cell, status;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  ~ParticleData() {
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
  }
};

namespace {

struct PtArgs {
  const double *aff, *u0, *u1;
  const int *nb, *cells, *fmarker;
  double *x, *t_end, *path, *expo;
  int *cell, *status;
  int n, cap, nsub;
  double dt, t0, mu;
};

template <int D>
__device__ __forceinline__ void pt_lambda(const double *__restrict__ T, const double (&y)[D], double (&lam)[D + 1]) {
  double r[D];
#pragma unroll
  for (int i = 0; i < D; i++) r[i] = y[i] - T[D * D + i];
  double s = 0.0;
#pragma unroll
  for (int a = 1; a <= D; a++) {
    double l = 0.0;
#pragma unroll
    for (int i = 0; i < D; i++) l = l + T[(a - 1) * D + i] * r[i];
    lam[a] = l;
    s = s + l;
  }
  lam[0] = 1.0 - s;
}

// w = sum_a lambda_a ((1 - s) u_prev,a + s u_sol,a) in cell c
template <int D>
__device__ __forceinline__ void pt_velocity(const PtArgs &p, int c, const double (&lam)[D + 1], double s, double (&w)[D]) {
  const double s1 = 1.0 - s;
#pragma unroll
  for (int i = 0; i < D; i++) w[i] = 0.0;
#pragma unroll
  for (int a = 0; a <= D; a++) {
    const int v = p.cells[(size_t)(D + 1) * c + a];
#pragma unroll
    for (int i = 0; i < D; i++) {
      const double ua = s1 * p.u0[(size_t)D * v + i] + s * p.u1[(size_t)D * v + i];
      w[i] = w[i] + lam[a] * ua;
    }
  }
}

// gamma_dot = sqrt(2 D:D), D = sym grad w at s, constant in cell c
template <int D>
__device__ __forceinline__ double pt_shear_rate(const PtArgs &p, int c, double s) {
  const double *T = p.aff + (size_t)c * (D * D + D);
  const double s1 = 1.0 - s;
  double g[D + 1][D], G[D][D];
#pragma unroll
  for (int j = 0; j < D; j++) {
    double t = 0.0;
#pragma unroll
    for (int a = 1; a <= D; a++) { g[a][j] = T[(a - 1) * D + j]; t = t + g[a][j]; }
    g[0][j] = -t;
  }
#pragma unroll
  for (int i = 0; i < D; i++)
#pragma unroll
    for (int j = 0; j < D; j++) G[i][j] = 0.0;
#pragma unroll
  for (int a = 0; a <= D; a++) {
    const int v = p.cells[(size_t)(D + 1) * c + a];
#pragma unroll
    for (int i = 0; i < D; i++) {
      const double ua = s1 * p.u0[(size_t)D * v + i] + s * p.u1[(size_t)D * v + i];
#pragma unroll
      for (int j = 0; j < D; j++) G[i][j] = G[i][j] + ua * g[a][j];
    }
  }
  double dd = 0.0;
#pragma unroll
  for (int i = 0; i < D; i++)
#pragma unroll
    for (int j = 0; j < D; j++) {
      const double e = 0.5 * (G[i][j] + G[j][i]);
      dd = dd + e * e;
    }
  return sqrt(2.0 * dd);
}

// The walk from x (which stays where it is) to y, starting in cell c.  0: y lies in c now; 1: an exterior facet was met, tc is the
// clamped crossing parameter and ext the facet's index in the context's facet list, c the cell that holds it; 2: more than
// MAX_CROSSINGS cells were crossed.
template <int D>
__device__ __forceinline__ int pt_walk(const PtArgs &p, const double (&x)[D], const double (&y)[D], int &c, double &tc, int &ext) {
  for (int cross = 0;;) {
    const double *T = p.aff + (size_t)c * (D * D + D);
    double ly[D + 1], lx[D + 1];
    pt_lambda<D>(T, y, ly);
    bool out = false;
#pragma unroll
    for (int f = 0; f <= D; f++) out = out || ly[f] < -cfdh_particles::TOL_INSIDE;
    if (!out) return 0;
    pt_lambda<D>(T, x, lx);
    int best = -1;
    double tb = 0.0;
#pragma unroll
    for (int f = 0; f <= D; f++)
      if (ly[f] < -cfdh_particles::TOL_INSIDE) {
        const double t = lx[f] / (lx[f] - ly[f]);
        if (best < 0 || t < tb) { best = f; tb = t; }
      }
    const int nbr = p.nb[(size_t)(D + 1) * c + best];
    if (nbr < 0) {
      tc = tb > 0.0 ? tb : 0.0;
      tc = tc > 1.0 ? 1.0 : tc;
      ext = -1 - nbr;
      return 1;
    }
    if (++cross > cfdh_particles::MAX_CROSSINGS) return 2;
    c = nbr;
  }
}

template <int D>
__global__ __launch_bounds__(TPB) void pt_advect_kernel(PtArgs p) {
  const int q = blockIdx.x * TPB + threadIdx.x;
  if (q >= p.n) return;
  int st = p.status[q];
  if (st != 0) return;
  int c = p.cell[q];
  double x[D], path = p.path[q], expo = p.expo[q], t_end = 0.0;
#pragma unroll
  for (int i = 0; i < D; i++) x[i] = p.x[(size_t)i * p.cap + q];
  const double h = p.dt / p.nsub, hh = 0.5 * h;
  for (int k = 0; k < p.nsub; k++) {
    const double s0 = (double)k / p.nsub, sm = s0 + 0.5 / p.nsub;
    double lam[D + 1], k1[D], k2[D], xm[D], xn[D], tc = 0.0;
    int ext = 0;
    pt_lambda<D>(p.aff + (size_t)c * (D * D + D), x, lam);
    pt_velocity<D>(p, c, lam, s0, k1);
#pragma unroll
    for (int i = 0; i < D; i++) xm[i] = x[i] + hh * k1[i];
    int cm = c;
    int r = pt_walk<D>(p, x, xm, cm, tc, ext);
    if (r == 2) { st = -1; t_end = p.t0 + k * h; break; }
    int cg = c;  // the cell of the shear rate: the midpoint's, the start cell when the substep degrades to Euler
    if (r == 1) {
#pragma unroll
      for (int i = 0; i < D; i++) k2[i] = k1[i];
    } else {
      pt_lambda<D>(p.aff + (size_t)cm * (D * D + D), xm, lam);
      pt_velocity<D>(p, cm, lam, sm, k2);
      cg = cm;
    }
#pragma unroll
    for (int i = 0; i < D; i++) xn[i] = x[i] + h * k2[i];
    int cn = c;
    r = pt_walk<D>(p, x, xn, cn, tc, ext);
    if (r == 2) { st = -1; t_end = p.t0 + k * h; break; }
    const double gam = pt_shear_rate<D>(p, cg, sm);
    double tau = h;
    if (r == 1) {
#pragma unroll
      for (int i = 0; i < D; i++) xn[i] = x[i] + tc * (xn[i] - x[i]);
      tau = tc * h;
      st = 1 + p.fmarker[ext];
      t_end = p.t0 + (k + tc) * h;
    }
    double d2 = 0.0;
#pragma unroll
    for (int i = 0; i < D; i++) { const double d = xn[i] - x[i]; d2 = d2 + d * d; x[i] = xn[i]; }
    path = path + sqrt(d2);
    expo = expo + (tau * p.mu) * gam;
    c = cn;
    if (r == 1) break;
  }
#pragma unroll
  for (int i = 0; i < D; i++) p.x[(size_t)i * p.cap + q] = x[i];
  p.cell[q] = c;
  p.path[q] = path;
  p.expo[q] = expo;
  if (st != 0) { p.status[q] = st; p.t_end[q] = t_end; }
}

// per-block counts of the particles that are active / have left through a facet / are lost: partial[v nb + block]
__global__ __launch_bounds__(TPB) void pt_count_kernel(int n, const int *__restrict__ status, double *__restrict__ partial) {
  __shared__ double sh[4];
  double a = 0.0, e = 0.0, l = 0.0;
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
    const int s = status[i];
    a += s == 0 ? 1.0 : 0.0; e += s > 0 ? 1.0 : 0.0; l += s < 0 ? 1.0 : 0.0;
  }
  a = block_sum(a, sh); e = block_sum(e, sh); l = block_sum(l, sh);
  if (threadIdx.x == 0) { partial[blockIdx.x] = a; partial[gridDim.x + blockIdx.x] = e; partial[2 * gridDim.x + blockIdx.x] = l; }
}

int pt_need(cfdh_ctx *c, const char *who) {
  if (!c->pt) return cfdh_fail(c, CFDH_E_STATE, "%s: cfdh_particles_enable was not called", who);
  return 0;
}

template <class T>
int pt_download(cfdh_ctx *c, const T *dev, size_t n, std::vector<T> &h) {
  h.resize(n);
  if (!n) return 0;
  HIPCHK(c, hipMemcpyAsync(h.data(), dev, sizeof(T) * n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

}  // namespace

void cfdh_particles_free(cfdh_ctx *c) {
  delete c->pt;
  c->pt = nullptr;
}

int cfdh_particles_enable_impl(cfdh_ctx *c, int64_t capacity, int32_t nsub) {
  const char *who = "cfdh_particles_enable";
  if (c->ipcs) return cfdh_fail(c, CFDH_E_ARG, "%s: not available on an incremental pressure-correction context (cfdh_create_ipcs)", who);
  if (c->gen) return cfdh_fail(c, CFDH_E_ARG, "%s: particles live on the closed-form P1 contexts (cfdh_create), not on the generic element kernels", who);
  if (c->nranks > 1 || c->nvo != c->nv) return cfdh_fail(c, CFDH_E_ARG, "%s: not available in partitioned runs", who);
  if (nsub < 1) return cfdh_fail(c, CFDH_E_ARG, "%s: nsub must be >= 1", who);
  if (capacity < 1 || capacity > (1ll << 30)) return cfdh_fail(c, CFDH_E_ARG, "%s: capacity must lie in [1, 2^30]", who);
  if (c->pt) {
    if (capacity != c->pt->cap) return cfdh_fail(c, CFDH_E_ARG, "%s: the capacity is fixed by the first call (%d); a later call changes nsub only", who, c->pt->cap);
    c->pt->nsub = nsub;
    return 0;
  }
  const int D = c->dim;
  std::vector<int> nb;
  std::vector<double> aff;
  std::string why;
  if (!cfdh_particles::build_neighbours(D, c->nv, c->nc, c->h_cells.data(), c->nfac, c->fac_cell.data(), c->fac_local.data(), nb, why) ||
      !cfdh_particles::build_affine(D, c->nc, c->h_cells.data(), c->h_coords.data(), aff, why))
    return cfdh_fail(c, CFDH_E_ARG, "%s: %s", who, why.c_str());
  ParticleData *P = new (std::nothrow) ParticleData();
  if (!P) return cfdh_fail(c, CFDH_E_NOMEM, "out of host memory");
  c->pt = P;
  int rc = [&]() -> int {
    P->cap = (int)capacity; P->nsub = nsub;
    int ncu = 0;
    for (int e : c->cell_user) ncu = std::max(ncu, e + 1);
    P->cell_int.assign((size_t)ncu, -1);
    for (int e = 0; e < c->nc; e++) P->cell_int[c->cell_user[e]] = e;
    HIPCHK(c, P->nb.upload(nb, c->stream));
    HIPCHK(c, P->aff.upload(aff, c->stream));
    const size_t cap = (size_t)capacity;
    HIPCHK(c, P->x.alloc(cap * D));
    for (dbuf<double> *b : {&P->x, &P->t_birth, &P->t_end, &P->path, &P->expo}) {
      if (b != &P->x) HIPCHK(c, b->alloc(cap));
      HIPCHK(c, b->zero(c->stream));
    }
    for (dbuf<int> *b : {&P->cell, &P->status}) {
      HIPCHK(c, b->alloc(cap));
      HIPCHK(c, b->zero(c->stream));
    }
    HIPCHK(c, hipEventCreate(&P->ev0));
    HIPCHK(c, hipEventCreate(&P->ev1));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // the host vectors go out of scope
    P->h_aff.swap(aff);
    return 0;
  }();
  if (rc) cfdh_particles_free(c);
  return rc;
}

int cfdh_particles_seed_impl(cfdh_ctx *c, int64_t n, const double *x, const int32_t *cell, double t_birth) {
  const char *who = "cfdh_particles_seed";
  CHK(pt_need(c, who));
  ParticleData *P = c->pt;
  const int D = c->dim;
  std::vector<int> ci;
  std::string why;
  if (!cfdh_particles::check_seeds(D, n, x, cell, (int64_t)P->cell_int.size(), P->cell_int.data(), P->h_aff.data(), t_birth, ci, why))
    return cfdh_fail(c, CFDH_E_ARG, "%s: %s", who, why.c_str());
  if (n > (int64_t)P->cap - P->n) return cfdh_fail(c, CFDH_E_ARG, "%s: %lld more particles do not fit the capacity (%d held of %d)", who, (long long)n, P->n, P->cap);
  if (n == 0) return 0;
  const size_t m = (size_t)n, at = (size_t)P->n;
  std::vector<double> col(m), tb(m, t_birth), te(m, std::numeric_limits<double>::quiet_NaN()), zero(m, 0.0);
  std::vector<int> izero(m, 0);
  hipStream_t s = c->stream;
  for (int i = 0; i < D; i++) {
    for (size_t k = 0; k < m; k++) col[k] = x[(size_t)D * k + i];
    HIPCHK(c, hipMemcpyAsync(P->x.p + (size_t)i * P->cap + at, col.data(), sizeof(double) * m, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipStreamSynchronize(s));  // col is filled again
  }
  HIPCHK(c, hipMemcpyAsync(P->t_birth.p + at, tb.data(), sizeof(double) * m, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(P->t_end.p + at, te.data(), sizeof(double) * m, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(P->path.p + at, zero.data(), sizeof(double) * m, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(P->expo.p + at, zero.data(), sizeof(double) * m, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(P->cell.p + at, ci.data(), sizeof(int) * m, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(P->status.p + at, izero.data(), sizeof(int) * m, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipStreamSynchronize(s));
  P->n += (int)n;
  P->active += n;
  return 0;
}

int cfdh_particles_clear_impl(cfdh_ctx *c) {
  CHK(pt_need(c, "cfdh_particles_clear"));
  c->pt->n = 0;
  c->pt->active = 0;
  return 0;
}

int cfdh_particles_step_impl(cfdh_ctx *c, double t0, cfdh_particle_stats *stats) {
  const char *who = "cfdh_particles_step";
  cfdh_particle_stats st;
  memset(&st, 0, sizeof st);
  if (stats) *stats = st;
  CHK(pt_need(c, who));
  if (!c->params_set || !c->state_set) return cfdh_fail(c, CFDH_E_STATE, "%s: parameters (cfdh_set_params) and a state are needed", who);
  if (!cfdh_particles::finite(t0)) return cfdh_fail(c, CFDH_E_ARG, "%s: t0 is not finite", who);
  ParticleData *P = c->pt;
  const auto w0 = std::chrono::steady_clock::now();
  st.stepped = P->active;
  if (P->n > 0) {
    PtArgs a;
    a.aff = P->aff.p; a.u0 = c->xprev.p; a.u1 = c->x.p; a.nb = P->nb.p; a.cells = c->cells.p; a.fmarker = c->d_fac_marker.p;
    a.x = P->x.p; a.t_end = P->t_end.p; a.path = P->path.p; a.expo = P->expo.p; a.cell = P->cell.p; a.status = P->status.p;
    a.n = P->n; a.cap = P->cap; a.nsub = P->nsub; a.dt = c->dt; a.t0 = t0; a.mu = c->mu;
    const dim3 gr((P->n + TPB - 1) / TPB), bl(TPB);
    HIPCHK(c, hipEventRecord(P->ev0, c->stream));
    if (c->dim == 3) hipLaunchKernelGGL(pt_advect_kernel<3>, gr, bl, 0, c->stream, a);
    else hipLaunchKernelGGL(pt_advect_kernel<2>, gr, bl, 0, c->stream, a);
    HIPCHK(c, hipEventRecord(P->ev1, c->stream));
    c->n_particle_launches++;
    HIPCHK(c, hipGetLastError());
    const int nb = red_grid(c, P->n);
    hipLaunchKernelGGL(pt_count_kernel, dim3(nb), dim3(TPB), 0, c->stream, P->n, (const int *)P->status.p, c->red_partial.p);
    HIPCHK(c, hipGetLastError());
    ScalarRead h;
    CHK(scalars_finish(c, c->red_out.p + RO_RESULT, 3, 0, nb, &h));
    double cnt[3];
    CHK(scalars_read(c, h, cnt));
    st.active = (int64_t)cnt[0]; st.exited = (int64_t)cnt[1]; st.lost = (int64_t)cnt[2];
    P->active = st.active;
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, P->ev0, P->ev1));
    st.ms_kernel = ms;
  }
  P->t_last = t0 + c->dt;
  c->n_particle_steps++;
  st.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count();
  if (stats) *stats = st;
  return 0;
}

int cfdh_particles_get_impl(cfdh_ctx *c, int which, int64_t *n, void *out) {
  const char *who = "cfdh_particles_get";
  CHK(pt_need(c, who));
  if (which < 0 || which > 6) return cfdh_fail(c, CFDH_E_ARG, "%s: unknown field %d (0 x, 1 cell, 2 status, 3 age, 4 path, 5 exposure, 6 t_end)", who, which);
  if (!n) return cfdh_fail(c, CFDH_E_ARG, "%s: n is NULL", who);
  ParticleData *P = c->pt;
  *n = P->n;
  if (!out || P->n == 0) return 0;
  const size_t m = (size_t)P->n;
  const int D = c->dim;
  std::vector<double> hd;
  std::vector<int> hi;
  if (which == 0) {
    double *o = (double *)out;
    for (int i = 0; i < D; i++) {
      CHK(pt_download(c, P->x.p + (size_t)i * P->cap, m, hd));
      for (size_t k = 0; k < m; k++) o[(size_t)D * k + i] = hd[k];
    }
  } else if (which == 1 || which == 2) {
    int32_t *o = (int32_t *)out;
    CHK(pt_download(c, which == 1 ? P->cell.p : P->status.p, m, hi));
    for (size_t k = 0; k < m; k++) o[k] = which == 1 ? c->cell_user[hi[k]] : hi[k];
  } else if (which == 3) {
    double *o = (double *)out;
    std::vector<double> tb;
    CHK(pt_download(c, P->t_birth.p, m, tb));
    CHK(pt_download(c, P->t_end.p, m, hd));
    CHK(pt_download(c, P->status.p, m, hi));
    for (size_t k = 0; k < m; k++) o[k] = hi[k] != 0 ? hd[k] - tb[k] : std::max(P->t_last - tb[k], 0.0);
  } else {
    CHK(pt_download(c, which == 4 ? P->path.p : (which == 5 ? P->expo.p : P->t_end.p), m, hd));
    memcpy(out, hd.data(), sizeof(double) * m);
  }
  return 0;
}
