// Cut-plane sections of the closed-form P1 contexts (cfdh_section_*, include/cfdh.h): area, flow rate, pressure, momentum and energy
// integrals over the exact intersection of a plane (a line in 2-D) with the mesh, from the u_sol that sits in HBM between
// cfdh_solve_step and cfdh_advance.
//
// The cut, once per set of sections.  cfdh_section::build_cut (cfdh_section_host.hpp) lists, per section, the cut and taken cells in
// ascending caller's index with everything that was decided about them: the local edges that carry the polygon vertices, their t
// and the measures of the sub-simplices.  The kernel reads those decisions and no coordinate.
//
// Evaluation.  sc_eval_kernel (one lane per entry) gathers u and p at the d + 1 vertices of its cell, evaluates at the polygon
// vertices and integrates the ten quantities with a rule that is exact for them.  A block works on at most 256 consecutive entries
// of one section (the block table is built with the cut) and reduces them with block_sum, in a fixed order; sc_sum_kernel adds the
// blocks of a section in block order and writes the row, or adds w times the row to the mean accumulators.  No atomics: two calls
// return the same bytes, and the row of a section does not depend on the other sections of the set.
#include <hip/hip_runtime.h>

#include <cmath>
#include <new>

#include "cfdh_internal.hpp"
#include "cfdh_section_host.hpp"
#include "cfdh_wave.hpp"

struct SectionData {
  int K = 0, nblk = 0;
  // host copies for cfdh_section_get_cut
  std::vector<long long> ptr;
  std::vector<int> cell_user, straddling;
  std::vector<double> measure;
  long long total = 0, maxlen = 0;
  // the entries and the block table
  dbuf<int> ecell, ecode;   // [total]
  dbuf<double> et, em;      // [total][np], [total][nt]
  dbuf<int> blk;            // [nblk][3]: section, first entry, entries (<= 256)
  dbuf<int> bptr;           // [K + 1]: the blocks of section k
  dbuf<double> normal;      // [K][3]
  dbuf<double> partial;     // [nblk][NQ]
  dbuf<double> rows;        // [K][NQ]: cfdh_section_now before its download
  // series
  size_t cap = 0, nrec = 0;
  dbuf<double> series;      // [cap][K][NQ]
  std::vector<double> t;
  // means: allocated by the first reset
  bool means = false;
  dbuf<double> acc;         // [K][NQ] sum w row
  double W = 0.0;
  long long count_acc = 0;
};

namespace {

constexpr int NQ = cfdh_section::NQ;
constexpr unsigned long long SC_SERIES_MAX_BYTES = 1ull << 40;

// u [nv][D] and p [nv] are the two parts of the state
template <int D>
__global__ __launch_bounds__(TPB) void sc_eval_kernel(const int *__restrict__ blk, const int *__restrict__ ecell, const int *__restrict__ ecode,
                                                     const double *__restrict__ et, const double *__restrict__ em, const int *__restrict__ cells,
                                                     const double *__restrict__ u, const double *__restrict__ p, const double *__restrict__ normal,
                                                     double rho, double *__restrict__ partial) {
  constexpr int NP = cfdh_section::np_of(D), NT = cfdh_section::nt_of(D);
  __shared__ double sh[4];
  const int k = blk[3 * blockIdx.x], first = blk[3 * blockIdx.x + 1], count = blk[3 * blockIdx.x + 2];
  double row[NQ];
#pragma unroll
  for (int s = 0; s < NQ; s++) row[s] = 0.0;
  if ((int)threadIdx.x < count) {
    const size_t i = (size_t)first + threadIdx.x;
    const int e = ecell[i];
    double U[D + 1][D], P[D + 1], t[NP], m[NT], n[3];
#pragma unroll
    for (int a = 0; a <= D; a++) {
      const int v = cells[(size_t)(D + 1) * e + a];
#pragma unroll
      for (int j = 0; j < D; j++) U[a][j] = u[(size_t)D * v + j];
      P[a] = p[v];
    }
#pragma unroll
    for (int j = 0; j < NP; j++) t[j] = et[(size_t)NP * i + j];
#pragma unroll
    for (int j = 0; j < NT; j++) m[j] = em[(size_t)NT * i + j];
#pragma unroll
    for (int j = 0; j < 3; j++) n[j] = normal[3 * k + j];
    cfdh_section::entry_row<D>(ecode[i], t, m, U, P, n, rho, row);
  }
#pragma unroll
  for (int s = 0; s < NQ; s++) {
    const double r = block_sum(row[s], sh);
    if (threadIdx.x == 0) partial[(size_t)NQ * blockIdx.x + s] = r;
  }
}

// one lane per (section, slot): the blocks of the section in order.  A section without blocks gets +0.0.
template <bool ACC>
__global__ __launch_bounds__(TPB) void sc_sum_kernel(int n, const int *__restrict__ bptr, const double *__restrict__ partial, double w,
                                                    double *__restrict__ out) {
  const int j = blockIdx.x * TPB + threadIdx.x;
  if (j >= n) return;
  const int k = j / NQ, s = j - NQ * k;
  double a = 0.0;
  for (int b = bptr[k]; b < bptr[k + 1]; b++) a += partial[(size_t)NQ * b + s];
  if constexpr (ACC) out[j] += w * a;
  else out[j] = a;
}

// the contexts that carry the sections; everything else is refused before any device work
int sc_supported(cfdh_ctx *c, const char *who) {
  if (c->ipcs) return cfdh_fail(c, CFDH_E_ARG, "%s: not available on an incremental pressure-correction context (cfdh_create_ipcs)", who);
  if (c->gen) return cfdh_fail(c, CFDH_E_ARG, "%s: the sections live on the closed-form P1 contexts (cfdh_create), not on the generic element kernels", who);
  if (c->nranks > 1 || c->nvo != c->nv) return cfdh_fail(c, CFDH_E_ARG, "%s: not available in partitioned runs", who);
  return 0;
}

void sc_remove_set(cfdh_ctx *c) {
  delete c->sec;
  c->sec = nullptr;
}

// device events around the eval and sum kernels, read by cfdh_info 125
int sc_time_begin(cfdh_ctx *c) {
  for (hipEvent_t &e : c->sc_ev)
    if (!e) HIPCHK(c, hipEventCreate(&e));
  HIPCHK(c, hipEventRecord(c->sc_ev[0], c->stream));
  return 0;
}
int sc_time_end(cfdh_ctx *c) {
  HIPCHK(c, hipEventRecord(c->sc_ev[1], c->stream));
  c->sc_timed = true;
  return 0;
}

// the rows of the current state into out [K][NQ], or w times them added to the accumulators
int sc_launch(cfdh_ctx *c, double *out, bool acc, double w) {
  SectionData *S = c->sec;
  const int D = c->dim;
  const double *u = c->x.p, *p = c->x.p + (size_t)D * c->nv;
  CHK(sc_time_begin(c));
  if (S->nblk > 0) {
    if (D == 3)
      hipLaunchKernelGGL(sc_eval_kernel<3>, dim3(S->nblk), dim3(TPB), 0, c->stream, (const int *)S->blk.p, (const int *)S->ecell.p, (const int *)S->ecode.p,
                         (const double *)S->et.p, (const double *)S->em.p, (const int *)c->cells.p, u, p, (const double *)S->normal.p, c->rho, S->partial.p);
    else
      hipLaunchKernelGGL(sc_eval_kernel<2>, dim3(S->nblk), dim3(TPB), 0, c->stream, (const int *)S->blk.p, (const int *)S->ecell.p, (const int *)S->ecode.p,
                         (const double *)S->et.p, (const double *)S->em.p, (const int *)c->cells.p, u, p, (const double *)S->normal.p, c->rho, S->partial.p);
    HIPCHK(c, hipGetLastError());
  }
  const int n = S->K * NQ;
  if (acc)
    hipLaunchKernelGGL(sc_sum_kernel<true>, dim3((n + TPB - 1) / TPB), dim3(TPB), 0, c->stream, n, (const int *)S->bptr.p, (const double *)S->partial.p, w, S->acc.p);
  else
    hipLaunchKernelGGL(sc_sum_kernel<false>, dim3((n + TPB - 1) / TPB), dim3(TPB), 0, c->stream, n, (const int *)S->bptr.p, (const double *)S->partial.p, w, out);
  HIPCHK(c, hipGetLastError());
  CHK(sc_time_end(c));
  c->n_section_launches++;
  return 0;
}

int sc_download(cfdh_ctx *c, void *host, const void *dev, size_t bytes) {
  if (bytes == 0) return 0;
  HIPCHK(c, hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

// the checks every evaluating call shares
int sc_ready(cfdh_ctx *c, const char *who, bool state) {
  if (!c->sec) return cfdh_fail(c, CFDH_E_STATE, "%s: no sections (cfdh_section_set)", who);
  if (state && (!c->params_set || !c->state_set)) return cfdh_fail(c, CFDH_E_STATE, "%s: parameters (cfdh_set_params) and a state are needed", who);
  return 0;
}

}  // namespace

// cfdh_destroy: the buffers and the timing events
void cfdh_section_destroy(cfdh_ctx *c) {
  sc_remove_set(c);
  for (hipEvent_t &e : c->sc_ev) {
    if (e) (void)hipEventDestroy(e);
    e = nullptr;
  }
  c->sc_timed = false;
}

int cfdh_section_set_impl(cfdh_ctx *c, int32_t K, const double *origin, const double *normal, const double *radius) {
  const char *who = "cfdh_section_set";
  CHK(sc_supported(c, who));
  if (K < 0 || K > cfdh_section::MAX_SECTIONS) return cfdh_fail(c, CFDH_E_ARG, "%s: K must lie in [0, %d]", who, cfdh_section::MAX_SECTIONS);
  if (K == 0) { sc_remove_set(c); return 0; }
  if (!origin || !normal) return cfdh_fail(c, CFDH_E_ARG, "%s: origin or normal is NULL", who);
  const int D = c->dim;
  if (c->cell_user.size() != (size_t)c->nc || c->cell_flipped.size() != (size_t)c->nc)
    return cfdh_fail(c, CFDH_E_STATE, "%s: the context does not know the order and orientation of its cells", who);
  std::vector<double> planes((size_t)K * (2 * D + 1));
  for (int k = 0; k < K; k++) {
    double *pl = &planes[(size_t)(2 * D + 1) * k];
    for (int i = 0; i < D; i++) { pl[i] = origin[D * k + i]; pl[D + i] = normal[D * k + i]; }
    pl[2 * D] = radius ? radius[k] : 0.0;
  }
  cfdh_section::Cut C;
  std::string why;
  if (!cfdh_section::build_cut(D, c->nv, c->nc, c->h_cells.data(), c->h_coords.data(), c->cell_user.data(), c->cell_flipped.data(), K, planes.data(), C, why))
    return cfdh_fail(c, CFDH_E_ARG, "%s: %s", who, why.c_str());
  // the old set, its series and its means go only now: a refused call leaves the context unchanged
  SectionData *S = new (std::nothrow) SectionData();
  if (!S) return cfdh_fail(c, CFDH_E_NOMEM, "out of host memory");
  sc_remove_set(c);
  c->sec = S;
  S->K = K;
  S->total = C.total;
  S->maxlen = C.maxlen;
  S->ptr = C.ptr;
  S->straddling = C.straddling;
  const int NT = cfdh_section::nt_of(D);
  S->cell_user.resize((size_t)C.total);
  S->measure.resize((size_t)C.total);
  for (long long i = 0; i < C.total; i++) {
    S->cell_user[i] = c->cell_user[C.cell[i]];
    double m = 0.0;
    for (int j = 0; j < NT; j++) m += C.meas[(size_t)NT * i + j];
    S->measure[i] = m;
  }
  std::vector<int> blk, bptr((size_t)K + 1, 0);
  for (int k = 0; k < K; k++) {
    for (long long f = C.ptr[k]; f < C.ptr[k + 1]; f += TPB) {
      blk.push_back(k);
      blk.push_back((int)f);
      blk.push_back((int)std::min<long long>(TPB, C.ptr[k + 1] - f));
    }
    bptr[k + 1] = (int)(blk.size() / 3);
  }
  S->nblk = (int)(blk.size() / 3);
  int rc = 0;
  auto up = [&]() -> int {
    HIPCHK(c, S->ecell.upload(C.cell, c->stream));
    HIPCHK(c, S->ecode.upload(C.code, c->stream));
    HIPCHK(c, S->et.upload(C.t, c->stream));
    HIPCHK(c, S->em.upload(C.meas, c->stream));
    HIPCHK(c, S->blk.upload(blk, c->stream));
    HIPCHK(c, S->bptr.upload(bptr, c->stream));
    HIPCHK(c, S->normal.upload(C.normal, c->stream));
    HIPCHK(c, S->partial.alloc((size_t)S->nblk * NQ));
    HIPCHK(c, S->rows.alloc((size_t)K * NQ));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // the host vectors go out of scope
    return 0;
  };
  rc = up();
  if (rc) sc_remove_set(c);
  return rc;
}

int cfdh_section_get_cut_impl(cfdh_ctx *c, int32_t *K, int64_t *ptr, int32_t *cell, double *measure, int32_t *straddling) {
  const char *who = "cfdh_section_get_cut";
  CHK(sc_supported(c, who));
  if (!K) return cfdh_fail(c, CFDH_E_ARG, "%s: K is NULL", who);
  const SectionData *S = c->sec;
  *K = S ? S->K : 0;
  if (!S) return 0;
  if (ptr)
    for (int k = 0; k <= S->K; k++) ptr[k] = S->ptr[k];
  if (straddling)
    for (int k = 0; k < S->K; k++) straddling[k] = S->straddling[k];
  if (!cell && !measure) return 0;
  if (!cell || !measure) return cfdh_fail(c, CFDH_E_ARG, "%s: pass both of cell / measure or neither", who);
  for (long long i = 0; i < S->total; i++) { cell[i] = S->cell_user[i]; measure[i] = S->measure[i]; }
  return 0;
}

int cfdh_section_now_impl(cfdh_ctx *c, int32_t *K, double *out) {
  const char *who = "cfdh_section_now";
  CHK(sc_supported(c, who));
  if (!K) return cfdh_fail(c, CFDH_E_ARG, "%s: K is NULL", who);
  CHK(sc_ready(c, who, false));
  SectionData *S = c->sec;
  *K = S->K;
  if (!out) return 0;
  CHK(sc_ready(c, who, true));
  CHK(sc_launch(c, S->rows.p, false, 0.0));
  return sc_download(c, out, S->rows.p, sizeof(double) * S->K * NQ);
}

int cfdh_section_series_enable_impl(cfdh_ctx *c, int64_t rows) {
  const char *who = "cfdh_section_series_enable";
  CHK(sc_supported(c, who));
  if (rows < 0 || rows > 0x7fffffffll) return cfdh_fail(c, CFDH_E_ARG, "%s: rows must lie in [0, 2^31 - 1]", who);
  CHK(sc_ready(c, who, false));
  SectionData *S = c->sec;
  S->series.release();
  S->cap = S->nrec = 0;
  S->t.clear();
  if (rows == 0) return 0;
  const unsigned long long per = 8ull * NQ * S->K;
  if ((unsigned long long)rows > SC_SERIES_MAX_BYTES / per)
    return cfdh_fail(c, CFDH_E_ARG, "%s: %lld row blocks of %d sections are more than 2^40 bytes", who, (long long)rows, S->K);
  HIPCHK(c, S->series.alloc((size_t)rows * S->K * NQ));
  S->cap = (size_t)rows;
  S->t.reserve(S->cap);
  return 0;
}

int cfdh_section_record_impl(cfdh_ctx *c, double t) {
  const char *who = "cfdh_section_record";
  CHK(sc_supported(c, who));
  CHK(sc_ready(c, who, false));
  SectionData *S = c->sec;
  if (S->cap == 0) return cfdh_fail(c, CFDH_E_STATE, "%s: cfdh_section_series_enable was not called", who);
  CHK(sc_ready(c, who, true));
  if (S->nrec == S->cap)
    return cfdh_fail(c, CFDH_E_STATE, "%s: the series buffer holds its %lld row blocks; empty it with cfdh_section_series_get(ctx, &rows, t, out)", who, (long long)S->cap);
  CHK(sc_launch(c, S->series.p + S->nrec * S->K * NQ, false, 0.0));
  S->t.push_back(t);
  S->nrec++;
  return 0;
}

int cfdh_section_series_get_impl(cfdh_ctx *c, int64_t *rows, double *t, double *out) {
  const char *who = "cfdh_section_series_get";
  CHK(sc_supported(c, who));
  if (!rows) return cfdh_fail(c, CFDH_E_ARG, "%s: rows is NULL", who);
  CHK(sc_ready(c, who, false));
  SectionData *S = c->sec;
  if (S->cap == 0) return cfdh_fail(c, CFDH_E_STATE, "%s: cfdh_section_series_enable was not called", who);
  *rows = (int64_t)S->nrec;
  if (!out) return 0;
  CHK(sc_download(c, out, S->series.p, sizeof(double) * S->nrec * S->K * NQ));
  if (t)
    for (size_t k = 0; k < S->nrec; k++) t[k] = S->t[k];
  S->nrec = 0;
  S->t.clear();
  return 0;
}

int cfdh_section_mean_reset_impl(cfdh_ctx *c) {
  const char *who = "cfdh_section_mean_reset";
  CHK(sc_supported(c, who));
  CHK(sc_ready(c, who, false));
  SectionData *S = c->sec;
  HIPCHK(c, S->acc.alloc((size_t)S->K * NQ));
  HIPCHK(c, S->acc.zero(c->stream));
  S->W = 0.0;
  S->count_acc = 0;
  S->means = true;
  return 0;
}

int cfdh_section_mean_accumulate_impl(cfdh_ctx *c, double weight) {
  const char *who = "cfdh_section_mean_accumulate";
  CHK(sc_supported(c, who));
  if (!cfdh_section::finite(weight) || !(weight > 0.0)) return cfdh_fail(c, CFDH_E_ARG, "%s: the weight must be finite and > 0", who);
  if (!c->sec || !c->sec->means) return cfdh_fail(c, CFDH_E_STATE, "%s: cfdh_section_mean_reset was not called", who);
  CHK(sc_ready(c, who, true));
  SectionData *S = c->sec;
  CHK(sc_launch(c, nullptr, true, weight));
  S->W += weight;
  S->count_acc++;
  return 0;
}

int cfdh_section_mean_get_impl(cfdh_ctx *c, int32_t *K, double *out, double *w_count) {
  const char *who = "cfdh_section_mean_get";
  CHK(sc_supported(c, who));
  if (!K) return cfdh_fail(c, CFDH_E_ARG, "%s: K is NULL", who);
  if (!c->sec || !c->sec->means) return cfdh_fail(c, CFDH_E_STATE, "%s: cfdh_section_mean_reset was not called", who);
  SectionData *S = c->sec;
  *K = S->K;
  if (w_count) { w_count[0] = S->W; w_count[1] = (double)S->count_acc; }
  if (!out) return 0;
  if (!(S->W > 0.0)) return cfdh_fail(c, CFDH_E_STATE, "%s: nothing accumulated since the last reset", who);
  CHK(sc_download(c, out, S->acc.p, sizeof(double) * S->K * NQ));
  for (int j = 0; j < S->K * NQ; j++) out[j] /= S->W;
  return 0;
}

int64_t cfdh_section_info(const cfdh_ctx *c, int what) {
  const SectionData *S = c->sec;
  switch (what) {
    case 120: return S ? S->K : 0;
    case 121: return S ? S->total : 0;
    case 122: return S ? S->maxlen : 0;
    case 123: return c->n_section_launches;
    case 124: return S ? (int64_t)S->nrec : 0;
    case 125: {  // nanoseconds of the last evaluation (eval and sum kernel)
      float ms = 0.f;
      if (!c->sc_timed || hipEventSynchronize(c->sc_ev[1]) != hipSuccess || hipEventElapsedTime(&ms, c->sc_ev[0], c->sc_ev[1]) != hipSuccess) return 0;
      return (int64_t)((double)ms * 1e6);
    }
    default: return 0;
  }
}
