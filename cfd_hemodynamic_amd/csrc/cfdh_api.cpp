// extern "C" entry points of libcfdh.so (see include/cfdh.h).
#include <algorithm>
#include <cmath>
#include <numeric>

#include <dlfcn.h>

#include "cfdh_internal.hpp"
#include "cfdh_ipcs.hpp"
#include "cfdh_traction_host.hpp"

std::string g_cfdh_last_error;

int cfdh_prepare_assembly(cfdh_ctx *c);

// every entry point makes the context's device current for the calling thread
#define ENTER(c)                         \
  do {                                   \
    if (!(c)) return CFDH_E_ARG;         \
    (void)hipSetDevice((c)->device);     \
  } while (0)

// entry points of the Newton solvers on a context of cfdh_create_ipcs, and the reverse
#define NOT_IPCS(c, name)                                                                                                    \
  do {                                                                                                                       \
    if ((c) && (c)->ipcs) return cfdh_fail((c), CFDH_E_STATE, name ": not available on an incremental pressure-correction context (cfdh_create_ipcs)"); \
  } while (0)
#define NEED_IPCS(c, name)                                                                                         \
  do {                                                                                                             \
    if (!(c)) return CFDH_E_ARG;                                                                                   \
    if (!(c)->ipcs) return cfdh_fail((c), CFDH_E_STATE, name ": the context was not created by cfdh_create_ipcs"); \
    (void)hipSetDevice((c)->device);                                                                               \
  } while (0)

// whole-field host <-> device copies of an IPCS context (caller's numbering: no permutation); NULL keeps the device copy
static int ipcs_put(cfdh_ctx *c, dbuf<double> &dst, const double *src) {
  if (!src) return 0;
  c->ipcs->n_field_copies++;
  HIPCHK(c, hipMemcpyAsync(dst.p, src, sizeof(double) * dst.n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}
static int ipcs_get(cfdh_ctx *c, const dbuf<double> &src, double *dst) {
  if (!dst) return 0;
  c->ipcs->n_field_copies++;
  HIPCHK(c, hipMemcpyAsync(dst, src.p, sizeof(double) * src.n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}
static int ipcs_copy(cfdh_ctx *c, const dbuf<double> &src, dbuf<double> &dst) {
  HIPCHK(c, hipMemcpyAsync(dst.p, src.p, sizeof(double) * src.n, hipMemcpyDeviceToDevice, c->stream));
  return 0;
}

namespace {
// a device allocation that lives for one call of cfdh_krylov_vec_op
template <class T>
struct HookBuf {
  T *p = nullptr;
  ~HookBuf() { if (p) (void)hipFree(p); }
  // `count` zeroed entries, the first `filled` of them from src (NULL: none)
  int put(cfdh_ctx *c, const T *src, size_t count, size_t filled) {
    HIPCHK(c, hipMalloc((void **)&p, sizeof(T) * count));
    HIPCHK(c, hipMemsetAsync(p, 0, sizeof(T) * count, c->stream));
    if (src && filled) HIPCHK(c, hipMemcpyAsync(p, src, sizeof(T) * filled, hipMemcpyHostToDevice, c->stream));
    return 0;
  }
  int get(cfdh_ctx *c, T *dst, size_t count) const {
    HIPCHK(c, hipMemcpy(dst, p, sizeof(T) * count, hipMemcpyDeviceToHost));
    return 0;
  }
};
}  // namespace

extern "C" {

int cfdh_abi_version(void) { return CFDH_ABI_VERSION; }

const char *cfdh_last_error(const cfdh_ctx *c) { return c ? c->err.c_str() : g_cfdh_last_error.c_str(); }

int cfdh_default_options(cfdh_options *o) {
  if (!o) return CFDH_E_ARG;
  // PETSc defaults + the caps the reference sets (stabilized_schur.py:269-274)
  o->snes_rtol = 1e-8; o->snes_atol = 1e-50; o->snes_stol = 1e-8; o->snes_max_it = 100;
  o->ksp_rtol = 1e-5; o->ksp_atol = 1e-50; o->ksp_max_it = 1000; o->ksp_restart = 200;
  o->cheb_degree = 3; o->cheb_ratio = 10.0; o->schur_full = 2;
  o->amg_smooth_degree = 1; o->amg_smooth_ratio = 8.0; o->amg_theta = -1.0; o->amg_max_coarse = 1000;
  o->pc_refresh = 0; o->remove_p_mean = 1; o->verbose = 0; o->pc_type = 1; o->cc_smooth_degree = 2;
  o->ksp_guess = getenv("CFDH_KSP_GUESS") ? atoi(getenv("CFDH_KSP_GUESS")) : 4;
  return 0;
}

static int create_ctx(cfdh_ctx **out, int device, int gdim, int etype, int64_t nv, int64_t nv_owned, int64_t nc, const int32_t *cells,
                      const double *coords, int64_t nfacets, const int32_t *facet_cells, const int32_t *facet_local,
                      const int32_t *facet_marker) {
  if (!out) return cfdh_fail(nullptr, CFDH_E_ARG, "null output pointer");
  *out = nullptr;
  if (gdim != 2 && gdim != 3) return cfdh_fail(nullptr, CFDH_E_ARG, "gdim must be 2 (P1 triangles) or 3 (P1 tetrahedra)");
  if (etype < 0 || etype > 3) return cfdh_fail(nullptr, CFDH_E_ARG, "unknown element type %d", etype);
  if (!cells || !coords || (nfacets > 0 && (!facet_cells || !facet_local)))
    return cfdh_fail(nullptr, CFDH_E_ARG, "null mesh array");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return cfdh_fail(nullptr, CFDH_E_HIP, "no HIP device available: libcfdh has no CPU fallback");
  if (device < 0 || device >= ndev) return cfdh_fail(nullptr, CFDH_E_ARG, "device %d out of range (%d devices)", device, ndev);
  cfdh_ctx *c = new (std::nothrow) cfdh_ctx();
  if (!c) return cfdh_fail(nullptr, CFDH_E_NOMEM, "out of host memory");
  c->device = device;
  cfdh_default_options(&c->opt);
  { const char *e = getenv("CFDH_NO_GRAPH"); c->use_graph = !(e && e[0] == '1'); }
  { const char *e = getenv("CFDH_SOLVE_LEAN"); c->lean = !(e && e[0] == '0'); }  // 0: the solve paths without the lean prologue / epilogue / kept coupling product (A/B runs, tests)
  { const char *e = getenv("CFDH_AMG_HEAD"); c->amg_head = !(e && e[0] == '0'); }  // 0: the AMG sweeps address through sptr / rowptr only (A/B runs, tests)
  { const char *e = getenv("CFDH_AMG_HEAD_W"); c->amg_head_w = e ? atoi(e) : 0; }  // forced head width (tests: tails on any mesh)
  {
    cfdh_ctx::SolveEnv &v = c->env;
    const char *e;
    if ((e = getenv("CFDH_KRYLOV_FP32"))) v.krylov_fp32 = atoi(e);
    v.guess_check = getenv("CFDH_GUESS_CHECK") != nullptr;
    e = getenv("CFDH_NO_ATTAINABLE_STOP"); v.no_attainable_stop = e && e[0] == '1';
    if ((e = getenv("CFDH_GS_REFINE_FROM"))) v.gs_refine_from = atoi(e);
    if ((e = getenv("CFDH_KSP_LAG"))) v.ksp_lag = atoi(e);
    if ((e = getenv("CFDH_GS_ETA2"))) v.gs_eta2 = atof(e);
    if ((e = getenv("CFDH_L_CYCLES"))) v.l_cycles = atoi(e);
    if ((e = getenv("CFDH_A_CYCLES"))) v.a_cycles = atoi(e);
    e = getenv("CFDH_DL0_COARSE_SWEEPS"); v.dl0_coarse_sweeps = e && e[0] == '1';
    e = getenv("CFDH_ASM_STAGE"); v.asm_stage = !(e && e[0] == '0');  // 0: the assembly addresses its lists through blk_vptr / blk_cptr (A/B runs, tests)
  }
  // No hipGraph replay under a rocprofiler-sdk tool on a HIP runtime >= 7.2.  That runtime submits the kernel packets of a graph
  // launch with ONE doorbell; ROCr's intercepted queue hands such a batch to the profiler's queue interceptor as (pointer into
  // the ring, packet count) without splitting it at the ring's wrap-around, and the interceptor walks `count` packets linearly:
  // the first graph launch whose packets straddle the end of the ring makes it read past the ring's mapping -- the SIGSEGV at
  // a page-aligned address below cfdh_pc_apply -> hipGraphLaunch of VERDICT round 3 (frames resolved in DESIGN.md section 6).
  // bench.py never met it because torch loads its own HIP 7.0 runtime first, which rings the doorbell per packet.  The kernels
  // are the same with direct launches, so a kernel trace loses nothing.  CFDH_GRAPH_UNDER_PROFILER=1 overrides.
  if (c->use_graph && (getenv("ROCP_TOOL_LIBRARIES") || dlsym(RTLD_DEFAULT, "rocprofiler_configure"))) {
    int rt = 0;
    const char *ov = getenv("CFDH_GRAPH_UNDER_PROFILER");
    if (!(ov && ov[0] == '1') && hipRuntimeGetVersion(&rt) == hipSuccess && rt >= 70200000) c->use_graph = false;
  }
  memset(&c->last_stats, 0, sizeof c->last_stats);
  int rc = 0;
  do {
    if (hipSetDevice(device) != hipSuccess) { rc = cfdh_fail(nullptr, CFDH_E_HIP, "hipSetDevice(%d) failed", device); break; }
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { rc = cfdh_fail(nullptr, CFDH_E_HIP, "hipStreamCreate failed"); break; }
    rc = gdim == 3 ? k3_upload_quadrature(c) : k_upload_quadrature(c);
    if (rc) break;
    if (etype != 0) {
      rc = gdim == 3 ? kg3_upload_tables(c) : kg_upload_tables(c);
      if (rc) break;
      rc = gdim == 3 ? cfdh_build_mesh_gen3(c, etype, nv, nv_owned, nc, cells, coords, nfacets, facet_cells, facet_local, facet_marker)
                     : cfdh_build_mesh_gen(c, etype, nv, nv_owned, nc, cells, coords, nfacets, facet_cells, facet_local, facet_marker);
      break;
    }
    rc = gdim == 3 ? cfdh_build_mesh3(c, nv, nv_owned, nc, cells, coords, nfacets, facet_cells, facet_local, facet_marker)
                   : cfdh_build_mesh(c, nv, nv_owned, nc, cells, coords, nfacets, facet_cells, facet_local, facet_marker);
  } while (0);
  if (rc) {
    g_cfdh_last_error = c->err.empty() ? g_cfdh_last_error : c->err;
    cfdh_destroy(c);
    return rc;
  }
  *out = c;
  return 0;
}

int cfdh_create(cfdh_ctx **out, int device, int gdim, int64_t nv, int64_t nv_owned, int64_t nc, const int32_t *cells,
                const double *coords, int64_t nfacets, const int32_t *facet_cells, const int32_t *facet_local,
                const int32_t *facet_marker) {
  return create_ctx(out, device, gdim, CFDH_ELEM_P1, nv, nv_owned, nc, cells, coords, nfacets, facet_cells, facet_local, facet_marker);
}

int cfdh_create_elem(cfdh_ctx **out, int device, int gdim, int elem, int64_t nn, int64_t nc, const int32_t *cells, const double *node_coords,
                     int64_t nfacets, const int32_t *facet_cells, const int32_t *facet_local, const int32_t *facet_marker) {
  return create_ctx(out, device, gdim, elem, nn, nn, nc, cells, node_coords, nfacets, facet_cells, facet_local, facet_marker);
}

int cfdh_create_elem_part(cfdh_ctx **out, int device, int gdim, int elem, int64_t nn, int64_t nn_owned, int64_t nc, const int32_t *cells,
                          const double *node_coords, int64_t nfacets, const int32_t *facet_cells, const int32_t *facet_local, const int32_t *facet_marker) {
  return create_ctx(out, device, gdim, elem, nn, nn_owned, nc, cells, node_coords, nfacets, facet_cells, facet_local, facet_marker);
}

void cfdh_destroy(cfdh_ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  cfdh_ipcs_free(c);
  cfdh_scalar_free(c);
  cfdh_particles_free(c);
  cfdh_flow_destroy(c);
  cfdh_sample_destroy(c);
  cfdh_section_destroy(c);
  comm_finalize(c);
  c->hS.clear(); c->hL.clear(); c->hA.clear(); c->hLg.clear();
  for (hipEvent_t e : c->ev_pool) (void)hipEventDestroy(e);
  for (auto &e : c->pc_graphs) for (auto &x : e.exec) if (x) (void)hipGraphExecDestroy(x);
  if (c->h_pinned) (void)hipHostFree(c->h_pinned);
  if (c->h_stage) (void)hipHostFree(c->h_stage);
  if (c->ev_h) (void)hipEventDestroy(c->ev_h);
  if (c->h_big) (void)hipHostFree(c->h_big);
  if (c->h_ring) (void)hipHostFree(c->h_ring);
  for (hipEvent_t e : c->ev_ring) if (e) (void)hipEventDestroy(e);
  hipStream_t s = c->stream;
  delete c;
  if (s) (void)hipStreamDestroy(s);
}

int cfdh_set_params(cfdh_ctx *c, double dt, double rho, double mu, double mu_facet, const double f[3]) {
  ENTER(c);
  if (!(dt > 0) || !(rho > 0) || !(mu > 0)) return cfdh_fail(c, CFDH_E_ARG, "dt, rho, mu must be positive");
  const bool changed = !c->params_set || dt != c->dt || rho != c->rho || mu != c->mu;
  c->dt = dt; c->rho = rho; c->mu = mu; c->muf = mu_facet;
  c->f[0] = f ? f[0] : 0.0; c->f[1] = f ? f[1] : 0.0; c->f[2] = (f && c->dim == 3) ? f[2] : 0.0;
  c->params_set = true;
  if (changed) { c->mom_valid = false; c->pc_valid = false; }
  if (c->ipcs) c->ipcs->assembled = false;
  return 0;
}

int cfdh_set_options(cfdh_ctx *c, const cfdh_options *o) {
  if (!c || !o) return CFDH_E_ARG;
  if (o->ksp_restart < 1 || o->ksp_restart > CFDH_KSP_RESTART_MAX || o->cheb_degree < 1 || o->cc_smooth_degree < 1 || !(o->cheb_ratio > 1) || o->amg_smooth_degree < 1 ||
      !(o->amg_smooth_ratio > 1) || o->amg_max_coarse < 8 || o->amg_max_coarse > 4000 || o->ksp_guess < 0 || o->ksp_guess > 8)
    return cfdh_fail(c, CFDH_E_ARG, "option out of range");
  const bool pc_changed = o->amg_theta != c->opt.amg_theta || o->amg_max_coarse != c->opt.amg_max_coarse ||
                          o->amg_smooth_ratio != c->opt.amg_smooth_ratio || o->pc_type != c->opt.pc_type ||
                          o->amg_smooth_degree != c->opt.amg_smooth_degree ||  // composite operators exist for degree 1 only
                          o->schur_full != c->opt.schur_full;  // the velocity hierarchy covers owned + ghost vertices only for schur_full == 2 (ras)
  c->opt = *o;
  if (pc_changed) c->pc_valid = false;
  if (pc_changed && c->ipcs) c->ipcs->pset_dirty = true;
  c->pc_graph_valid = false;  // degrees / schur_full are baked into the captured graph
  return 0;
}

int cfdh_clear_dirichlet(cfdh_ctx *c) {
  if (c && c->ipcs) return cfdh_ipcs_clear_dirichlet(c);
  ENTER(c);
  // only the entries some object wrote (the arrays start out zero): O(#boundary vertices) per step, not O(nv)
  const int st = c->dim + 1;
  for (int v : c->bc_touched) {
    c->h_bcflag[v] = 0;
    for (int i = 0; i < st; i++) { c->h_bcval[(size_t)st * v + i] = 0.0; c->h_bcmult[(size_t)st * v + i] = 0.0; }
  }
  c->bc_pending.insert(c->bc_pending.end(), c->bc_touched.begin(), c->bc_touched.end());  // must be reset on the device too
  c->bc_touched.clear();
  c->bc_touched_sent = 0;
  c->n_pbc = 0;
  c->bc_dirty = true;
  c->bc_version++;
  return 0;
}

int cfdh_add_dirichlet(cfdh_ctx *c, int field, int64_t n, const int32_t *nodes, const double *values) {
  if (c && c->ipcs) {
    if ((field != 0 && field != 1) || n < 0 || (n > 0 && (!nodes || !values))) return cfdh_fail(c, CFDH_E_ARG, "bad Dirichlet arguments");
    return cfdh_ipcs_add_dirichlet(c, field, n, nodes, values, false);
  }
  if (!c || (field != 0 && field != 1) || n < 0 || (n > 0 && (!nodes || !values))) return cfdh_fail(c, CFDH_E_ARG, "bad Dirichlet arguments");
  for (int64_t k = 0; k < n; k++)
    if (nodes[k] < 0 || nodes[k] >= c->nv) return cfdh_fail(c, CFDH_E_ARG, "Dirichlet node %d out of range", (int)nodes[k]);
  const int d = c->dim, st = d + 1;  // per vertex: d velocity components, then the pressure
  for (int64_t k = 0; k < n; k++) {
    const int v = c->perm[nodes[k]];
    c->bc_touched.push_back(v);
    if (field == 0) {
      for (int i = 0; i < d; i++) {
        c->h_bcflag[v] |= (unsigned char)(1u << i);
        c->h_bcval[(size_t)st * v + i] = values[(size_t)d * k + i];
        c->h_bcmult[(size_t)st * v + i] += 1.0;
      }
    } else {
      c->h_bcflag[v] |= (unsigned char)(1u << d);
      c->h_bcval[(size_t)st * v + d] = values[k];
      c->h_bcmult[(size_t)st * v + d] += 1.0;
      c->n_pbc++;
    }
  }
  c->bc_dirty = true;
  return 0;
}

int cfdh_update_dirichlet(cfdh_ctx *c, int field, int64_t n, const int32_t *nodes, const double *values) {
  if (c && c->ipcs) {
    if ((field != 0 && field != 1) || n < 0 || (n > 0 && (!nodes || !values))) return cfdh_fail(c, CFDH_E_ARG, "bad Dirichlet arguments");
    return cfdh_ipcs_add_dirichlet(c, field, n, nodes, values, true);
  }
  if (!c || (field != 0 && field != 1) || n < 0 || (n > 0 && (!nodes || !values))) return cfdh_fail(c, CFDH_E_ARG, "bad Dirichlet arguments");
  const int d = c->dim, st = d + 1;
  const unsigned need = field == 0 ? ((1u << d) - 1u) : (1u << d);
  for (int64_t k = 0; k < n; k++) {
    if (nodes[k] < 0 || nodes[k] >= c->nv) return cfdh_fail(c, CFDH_E_ARG, "Dirichlet node %d out of range", (int)nodes[k]);
    if ((c->h_bcflag[c->perm[nodes[k]]] & need) != need) return cfdh_fail(c, CFDH_E_ARG, "cfdh_update_dirichlet: node %d is not constrained", (int)nodes[k]);
  }
  for (int64_t k = 0; k < n; k++) {
    const int v = c->perm[nodes[k]];
    c->bc_pending.push_back(v);  // the node is in bc_touched already (an add constrained it): only its device entry is stale
    if (field == 0) for (int i = 0; i < d; i++) c->h_bcval[(size_t)st * v + i] = values[(size_t)d * k + i];
    else c->h_bcval[(size_t)st * v + d] = values[k];
  }
  if (n > 0) c->bc_dirty = true;
  return 0;
}

// user arrays (u [nv][2], p [nv], user numbering) -> internal vector layout
// Host <-> device field transfers of the literal reference loop (scenario.py:306-307 copies the state through the
// host every step): staged through one pinned buffer (pageable copies run at a fraction of the PCIe rate) and
// permuted between the caller's numbering and the internal layout with all host threads.
typedef std::vector<double> hvec;
static int stage_buffer(cfdh_ctx *c, double **h) {
  if (!c->h_stage) HIPCHK(c, hipHostMalloc((void **)&c->h_stage, sizeof(double) * (size_t)c->NL));
  *h = c->h_stage;
  return 0;
}
static void pack_vec(const cfdh_ctx *c, const double *u, const double *p, std::vector<double> &out, const std::vector<double> *keep) {
  const int nvo = c->nvo, nv = c->nv, d = c->dim;
  out.resize((size_t)c->NL);
  if (keep) out = *keep;
#pragma omp parallel for schedule(static) num_threads(cfdh_host_threads()) if (nv > 20000)
  for (int k = 0; k < nv; k++) {
    const int v = c->iperm[k];
    const size_t uo = k < nvo ? (size_t)d * k : (size_t)(d + 1) * k, po = k < nvo ? (size_t)d * nvo + k : (size_t)(d + 1) * k + d;
    if (u) for (int i = 0; i < d; i++) out[uo + i] = u[(size_t)d * v + i];
    if (p) out[po] = p[v];
  }
}
static void unpack_vec(const cfdh_ctx *c, const std::vector<double> &in, double *u, double *p) {
  const int nvo = c->nvo, nv = c->nv, d = c->dim;
#pragma omp parallel for schedule(static) num_threads(cfdh_host_threads()) if (nv > 20000)
  for (int k = 0; k < nv; k++) {
    const int v = c->iperm[k];
    const size_t uo = k < nvo ? (size_t)d * k : (size_t)(d + 1) * k, po = k < nvo ? (size_t)d * nvo + k : (size_t)(d + 1) * k + d;
    if (u) for (int i = 0; i < d; i++) u[(size_t)d * v + i] = in[uo + i];
    if (p) p[v] = in[po];
  }
}
static int download_vec(cfdh_ctx *c, const double *dev, std::vector<double> &h) {
  double *st;
  CHK(stage_buffer(c, &st));
  h.resize((size_t)c->NL);
  HIPCHK(c, hipMemcpyAsync(st, dev, sizeof(double) * h.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  memcpy(h.data(), st, sizeof(double) * h.size());
  return 0;
}
static int upload_vec(cfdh_ctx *c, const std::vector<double> &h, double *dev) {
  double *st;
  CHK(stage_buffer(c, &st));
  memcpy(st, h.data(), sizeof(double) * h.size());
  HIPCHK(c, hipMemcpyAsync(dev, st, sizeof(double) * h.size(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

int cfdh_set_state(cfdh_ctx *c, const double *u_prev, const double *p_prev, const double *u, const double *p) {
  if (c && c->ipcs) {
    ENTER(c);
    IpcsData *I = c->ipcs;
    CHK(ipcs_put(c, I->u_prev, u_prev)); CHK(ipcs_put(c, I->p_prev, p_prev)); CHK(ipcs_put(c, I->u_sol, u)); CHK(ipcs_put(c, I->p_sol, p));
    c->state_set = true; I->assembled = false;
    return 0;
  }
  ENTER(c);
  std::vector<double> h, cur;
  if (u_prev || p_prev) {
    const std::vector<double> *keep = nullptr;
    if (!(u_prev && p_prev)) { CHK(download_vec(c, c->xprev.p, cur)); keep = &cur; }
    pack_vec(c, u_prev, p_prev, h, keep);
    CHK(upload_vec(c, h, c->xprev.p));
    if (u_prev) c->mom_valid = false;
  }
  if (u || p) {
    const std::vector<double> *keep = nullptr;
    if (!(u && p)) { CHK(download_vec(c, c->x.p, cur)); keep = &cur; }
    pack_vec(c, u, p, h, keep);
    CHK(upload_vec(c, h, c->x.p));
  }
  c->state_set = true;
  return 0;
}

int cfdh_get_solution(cfdh_ctx *c, double *u, double *p) {
  if (c && c->ipcs) { ENTER(c); CHK(ipcs_get(c, c->ipcs->u_sol, u)); return ipcs_get(c, c->ipcs->p_sol, p); }
  ENTER(c);
  std::vector<double> h;
  CHK(download_vec(c, c->x.p, h));
  unpack_vec(c, h, u, p);
  return 0;
}

int cfdh_get_previous(cfdh_ctx *c, double *u, double *p) {
  if (c && c->ipcs) { ENTER(c); CHK(ipcs_get(c, c->ipcs->u_prev, u)); return ipcs_get(c, c->ipcs->p_prev, p); }
  ENTER(c);
  std::vector<double> h;
  CHK(download_vec(c, c->xprev.p, h));
  unpack_vec(c, h, u, p);
  return 0;
}

int cfdh_get_residual(cfdh_ctx *c, double *ru, double *rp) {
  NOT_IPCS(c, "cfdh_get_residual");
  ENTER(c);
  std::vector<double> h;
  CHK(download_vec(c, c->F.p, h));
  // ghost entries of F are not defined: report zeros there
  for (size_t k = (size_t)(c->dim + 1) * c->nvo; k < h.size(); k++) h[k] = 0.0;
  unpack_vec(c, h, ru, rp);
  return 0;
}

int cfdh_advance(cfdh_ctx *c) {
  if (c && c->ipcs) { ENTER(c); CHK(ipcs_copy(c, c->ipcs->u_sol, c->ipcs->u_prev)); return ipcs_copy(c, c->ipcs->p_sol, c->ipcs->p_prev); }
  ENTER(c);
  CHK(v_copy(c, c->NL, c->x.p, c->xprev.p));
  c->mom_valid = false;
  return 0;
}

int cfdh_advance_field(cfdh_ctx *c, int field) {
  if (c && c->ipcs) {
    ENTER(c);
    if (field != 0 && field != 1) return cfdh_fail(c, CFDH_E_ARG, "cfdh_advance_field: field must be 0 (velocity) or 1 (pressure)");
    return field == 0 ? ipcs_copy(c, c->ipcs->u_sol, c->ipcs->u_prev) : ipcs_copy(c, c->ipcs->p_sol, c->ipcs->p_prev);
  }
  ENTER(c);
  const size_t nu = (size_t)c->dim * c->nvo;
  if (field == 0) {
    CHK(v_copy(c, (int)nu, c->x.p, c->xprev.p));  // ghost entries follow with the halo exchange before the next assembly
    c->mom_valid = false;
  } else if (field == 1) {
    CHK(v_copy(c, c->nvo, c->x.p + nu, c->xprev.p + nu));
  } else {
    return cfdh_fail(c, CFDH_E_ARG, "cfdh_advance_field: field must be 0 (velocity) or 1 (pressure)");
  }
  return 0;
}

int cfdh_set_time_scheme(cfdh_ctx *c, double theta, double a0, double a1, double a2) {
  NOT_IPCS(c, "cfdh_set_time_scheme");
  ENTER(c);
  if (!(theta > 0) || theta > 1 || !(a0 > 0)) return cfdh_fail(c, CFDH_E_ARG, "time scheme needs 0 < theta <= 1 and a0 > 0");
  if (theta != c->ts_theta || a0 != c->ts_a[0]) c->pc_valid = false;  // a0/(theta dt) scales the preconditioner
  if (theta != c->ts_theta || a0 != c->ts_a[0] || a1 != c->ts_a[1] || a2 != c->ts_a[2]) c->jac_valid = false;
  c->ts_theta = theta; c->ts_a[0] = a0; c->ts_a[1] = a1; c->ts_a[2] = a2;
  return 0;
}

// per-cell facet bits of the assembly kernel: bits 0..d exterior facet, bits d+1..2d+1 backflow facet (marker == bf_marker);
// generic elements: bit f exterior, 4 + f pressure boundary (gdim 2: slot in gpbidx), 8 + f backflow.  gdim 3 (up to 6 facets per
// cell): the pressure boundaries are not in the flag word but in the slot array g3_pbslot [nc][NF] (0xff: none) and the cell list g3_pcells
static int upload_cell_facet_flags(cfdh_ctx *c) {
  if (c->gen) {
    const bool g3 = c->dim == 3;
    const int nf = g3 ? (c->etype == 2 ? 6 : 4) : 4;
    std::vector<unsigned short> gf((size_t)c->nc, 0);
    std::vector<unsigned char> pbi;
    if (!c->pb_markers.empty()) pbi.assign(nf * (size_t)c->nc, g3 ? 0xff : 0);
    for (int k = 0; k < c->nfac; k++) {
      gf[c->fac_cell[k]] |= (unsigned short)(1u << c->fac_local[k]);
      if (c->bf_marker >= 0 && c->fac_marker[k] == c->bf_marker) gf[c->fac_cell[k]] |= (unsigned short)(256u << c->fac_local[k]);
      for (size_t b = 0; b < c->pb_markers.size(); b++)
        if (c->fac_marker[k] == c->pb_markers[b]) {
          if (!g3) gf[c->fac_cell[k]] |= (unsigned short)(16u << c->fac_local[k]);
          pbi[nf * (size_t)c->fac_cell[k] + c->fac_local[k]] = (unsigned char)b;
        }
    }
    if (g3) {
      std::vector<int> pcl;
      for (int e = 0; e < (int)pbi.size() / nf; e++)
        for (int f = 0; f < nf; f++)
          if (pbi[nf * (size_t)e + f] != 0xff) { pcl.push_back(e); break; }
      c->g3_npcells = (int)pcl.size();
      if (!pcl.empty()) {
        HIPCHK(c, c->g3_pbslot.upload(pbi, c->stream));
        HIPCHK(c, c->g3_pcells.upload(pcl, c->stream));
      }
    } else if (!pbi.empty()) {
      HIPCHK(c, c->gpbidx.upload(pbi, c->stream));
    }
    HIPCHK(c, c->gflag.upload(gf, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->jac_valid = false;
    c->pc_valid = false;
    return 0;
  }
  std::vector<unsigned char> cflag((size_t)c->nc, 0);
  for (int k = 0; k < c->nfac; k++) {
    cflag[c->fac_cell[k]] |= (unsigned char)(1u << c->fac_local[k]);
    if (c->bf_marker >= 0 && c->fac_marker[k] == c->bf_marker)
      cflag[c->fac_cell[k]] |= (unsigned char)((c->dim == 3 ? 16u : 8u) << c->fac_local[k]);
  }
  HIPCHK(c, c->cflag.upload(cflag, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->jac_valid = false;
  c->pc_valid = false;
  return 0;
}

int cfdh_set_boundary_terms(cfdh_ctx *c, int ds_terms, int backflow_marker, double beta) {
  NOT_IPCS(c, "cfdh_set_boundary_terms");
  ENTER(c);
  if (beta < 0) return cfdh_fail(c, CFDH_E_ARG, "backflow beta must be >= 0");
  if (beta > 0 && c->form == CFDH_FORM_ROTATIONAL)
    return cfdh_fail(c, CFDH_E_ARG, "cfdh_set_boundary_terms: the rotational formulation takes its backflow term per pressure boundary (cfdh_set_pressure_boundaries_ex)");
  if (!c->tb_markers.empty() && (ds_terms != 0 || beta > 0))
    return cfdh_fail(c, CFDH_E_ARG, "cfdh_set_boundary_terms: traction boundaries are set (cfdh_set_traction_boundaries): they need ds_terms = 0 and carry their own backflow term");
  if (!(beta > 0)) backflow_marker = -1;
  const bool changed = (ds_terms != 0) != c->ds_terms || beta != c->bf_beta || backflow_marker != c->bf_marker;
  c->ds_terms = ds_terms != 0; c->bf_beta = beta; c->bf_marker = backflow_marker;
  if (!changed) return 0;
  return upload_cell_facet_flags(c);
}

int cfdh_set_facet_markers(cfdh_ctx *c, int64_t nfacets, const int32_t *markers) {
  if (c && c->ipcs) {
    ENTER(c);
    IpcsData *I = c->ipcs;
    if (nfacets != (int64_t)I->fmarker.size() || (nfacets > 0 && !markers)) return cfdh_fail(c, CFDH_E_ARG, "cfdh_set_facet_markers: one marker per exterior facet of cfdh_create_ipcs");
    I->fmarker.assign(markers, markers + nfacets);
    if (nfacets > 0) { HIPCHK(c, I->d_fmarker.upload(I->fmarker, c->stream)); HIPCHK(c, hipStreamSynchronize(c->stream)); }
    return 0;
  }
  ENTER(c);
  if (nfacets != c->nfac_user) return cfdh_fail(c, CFDH_E_ARG, "cfdh_set_facet_markers: %lld markers for the %d exterior facets of cfdh_create", (long long)nfacets, c->nfac_user);
  if (nfacets > 0 && !markers) return cfdh_fail(c, CFDH_E_ARG, "null marker array");
  for (int k = 0; k < c->nfac; k++) c->fac_marker[k] = markers[c->fac_user[k]];
  if (c->nfac) {
    HIPCHK(c, c->d_fac_marker.upload(c->fac_marker, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  // the PCD operator's inlet facets and outlet rows follow the markers
  if (c->pcd_set) { c->pcd_ready = false; c->pc_valid = false; }
  // the backflow term and the pressure boundaries follow the markers: refresh the per-cell flags (invalidates Jacobian and preconditioner)
  if (c->bf_marker >= 0 || !c->pb_markers.empty()) return upload_cell_facet_flags(c);
  // ... and so do the traction boundaries: new work list at the next assembly
  if (!c->tb_markers.empty()) { c->tb_ready = false; c->jac_valid = false; c->pc_valid = false; }
  return 0;
}

// contexts the rotational form exists for (the rest are follow-ups): gdim 2 on the generic kernels, and P2 tetrahedra / Q1 hexahedra
// in gdim 3 (the P1 tetrahedron, closed-form or generic, has no rotational variant)
static int rotational_supported(cfdh_ctx *c, const char *who) {
  if (c->dim != 2 && !(c->dim == 3 && c->gen && (c->etype == 1 || c->etype == 2)))
    return cfdh_fail(c, CFDH_E_ARG, "%s: the rotational formulation exists for gdim 2, and for P2 / Q1 cells in gdim 3", who);
  if (!c->gen)
    return cfdh_fail(c, CFDH_E_ARG, "%s: the rotational formulation runs on the generic element kernels; create P1 contexts with CFDH_ELEM_P1_GENERIC", who);
  if (c->nranks > 1 || c->nvo != c->nv) return cfdh_fail(c, CFDH_E_ARG, "%s: the rotational formulation is not available in partitioned runs", who);
  return 0;
}

int cfdh_set_formulation(cfdh_ctx *c, int form) {
  NOT_IPCS(c, "cfdh_set_formulation");
  ENTER(c);
  if (form != CFDH_FORM_CONVECTIVE && form != CFDH_FORM_ROTATIONAL) return cfdh_fail(c, CFDH_E_ARG, "cfdh_set_formulation: unknown form %d", form);
  if (form == c->form) return 0;
  if (form == CFDH_FORM_ROTATIONAL) {
    if (!c->tb_markers.empty())
      return cfdh_fail(c, CFDH_E_ARG, "cfdh_set_formulation: traction boundaries are set (they belong to the convective formulation)");
    CHK(rotational_supported(c, "cfdh_set_formulation"));
    if (c->bf_marker >= 0 && c->bf_beta > 0)
      return cfdh_fail(c, CFDH_E_ARG, "cfdh_set_formulation: the rotational formulation cannot be combined with the backflow term (beta > 0)");
  } else if (!c->pb_markers.empty()) {
    return cfdh_fail(c, CFDH_E_ARG, "cfdh_set_formulation: pressure boundaries are set (they belong to the rotational formulation)");
  } else if (c->gen && c->pcd_set) {
    return cfdh_fail(c, CFDH_E_ARG, "cfdh_set_formulation: the PCD operator is set (on the generic element kernels it belongs to the rotational formulation)");
  }
  c->form = form;
  c->jac_valid = false;
  c->pc_valid = false;
  return 0;
}

// both entry points (the validation messages of the plain call are kept); nitsche NULL: all on, beta_backflow NULL: all 0
static int set_pressure_boundaries(cfdh_ctx *c, int n, const int32_t *markers, const double *values, double beta_nitsche,
                                   const uint8_t *nitsche, const double *beta_backflow) {
  if (n < 0 || n > CFDH_MAX_PBND) return cfdh_fail(c, CFDH_E_ARG, "cfdh_set_pressure_boundaries: 0 <= n <= %d", CFDH_MAX_PBND);
  if (n > 0 && (!markers || !values)) return cfdh_fail(c, CFDH_E_ARG, "cfdh_set_pressure_boundaries: null marker / value array");
  if (!(beta_nitsche >= 0) || !std::isfinite(beta_nitsche)) return cfdh_fail(c, CFDH_E_ARG, "cfdh_set_pressure_boundaries: beta_nitsche must be finite and >= 0");
  for (int k = 0; k < n; k++) {
    if (!std::isfinite(values[k])) return cfdh_fail(c, CFDH_E_ARG, "cfdh_set_pressure_boundaries: value %d is not finite", k);
    for (int l = 0; l < k; l++)
      if (markers[l] == markers[k]) return cfdh_fail(c, CFDH_E_ARG, "cfdh_set_pressure_boundaries: marker %d listed twice", (int)markers[k]);
  }
  if (n > 0) {
    CHK(rotational_supported(c, "cfdh_set_pressure_boundaries"));
    if (c->form != CFDH_FORM_ROTATIONAL)
      return cfdh_fail(c, CFDH_E_ARG, "cfdh_set_pressure_boundaries: pressure boundaries need the rotational formulation (cfdh_set_formulation)");
  }
  unsigned nit = 0;
  std::vector<double> bf((size_t)n, 0.0);
  for (int k = 0; k < n; k++) {
    if (!nitsche || nitsche[k]) nit |= 1u << k;
    if (beta_backflow) {
      if (!(beta_backflow[k] >= 0) || !std::isfinite(beta_backflow[k]))
        return cfdh_fail(c, CFDH_E_ARG, "cfdh_set_pressure_boundaries_ex: beta_backflow %d must be finite and >= 0", k);
      bf[k] = beta_backflow[k];
    }
  }
  bool same = (size_t)n == c->pb_markers.size() && beta_nitsche == c->pb_beta && nit == c->pb_nitsche;
  for (int k = 0; same && k < n; k++) same = markers[k] == c->pb_markers[k] && bf[k] == c->pb_backflow[k];
  c->pb_values.assign(values, values + n);
  if (same) return 0;  // values only: they enter the residual, Jacobian and preconditioner stay valid
  c->pb_markers.assign(markers, markers + n);
  c->pb_beta = beta_nitsche;
  c->pb_nitsche = nit;
  c->pb_backflow = bf;
  return upload_cell_facet_flags(c);
}

int cfdh_set_pressure_boundaries(cfdh_ctx *c, int n, const int32_t *markers, const double *values, double beta_nitsche) {
  NOT_IPCS(c, "cfdh_set_pressure_boundaries");
  ENTER(c);
  return set_pressure_boundaries(c, n, markers, values, beta_nitsche, nullptr, nullptr);
}

int cfdh_set_pressure_boundaries_ex(cfdh_ctx *c, int n, const int32_t *markers, const double *values, double beta_nitsche,
                                    const uint8_t *nitsche, const double *beta_backflow) {
  NOT_IPCS(c, "cfdh_set_pressure_boundaries_ex");
  ENTER(c);
  return set_pressure_boundaries(c, n, markers, values, beta_nitsche, nitsche, beta_backflow);
}

int cfdh_set_traction_boundaries(cfdh_ctx *c, int n, const int32_t *markers, const double *values, double beta_nitsche, const uint8_t *tangential,
                                 const double *beta_backflow) {
  ENTER(c);
  const char *who = "cfdh_set_traction_boundaries";
  if (c->ipcs) return cfdh_fail(c, CFDH_E_ARG, "%s: not available on an incremental pressure-correction context (cfdh_create_ipcs)", who);
  std::string why;
  if (!cfdh_traction::check_boundaries(n, CFDH_MAX_PBND, markers, values, beta_nitsche, beta_backflow, why))
    return cfdh_fail(c, CFDH_E_ARG, "%s: %s", who, why.c_str());
  if (n > 0) {
    if (c->gen) return cfdh_fail(c, CFDH_E_ARG, "%s: traction boundaries exist on the closed-form P1 kernels (cfdh_create), not on the generic element kernels", who);
    if (c->nranks > 1 || c->nvo != c->nv) return cfdh_fail(c, CFDH_E_ARG, "%s: not available in partitioned runs", who);
    if (c->form != CFDH_FORM_CONVECTIVE) return cfdh_fail(c, CFDH_E_ARG, "%s: traction boundaries belong to the convective formulation", who);
    if (c->ds_terms) return cfdh_fail(c, CFDH_E_ARG, "%s: needs ds_terms = 0 (cfdh_set_boundary_terms)", who);
    if (c->bf_marker >= 0 && c->bf_beta > 0)
      return cfdh_fail(c, CFDH_E_ARG, "%s: the backflow term of cfdh_set_boundary_terms is active; give it per boundary (beta_backflow)", who);
  }
  unsigned tang = 0;
  std::vector<double> bf((size_t)n, 0.0);
  for (int k = 0; k < n; k++) {
    if (!tangential || tangential[k]) tang |= 1u << k;
    if (beta_backflow) bf[k] = beta_backflow[k];
  }
  bool same = (size_t)n == c->tb_markers.size() && beta_nitsche == c->tb_beta && tang == c->tb_tangential;
  for (int k = 0; same && k < n; k++) same = markers[k] == c->tb_markers[k] && bf[k] == c->tb_backflow[k];
  if (n == 0 && same) return 0;
  c->tb_values.assign(values, values + n);
  if (!same) {
    c->tb_markers.assign(markers, markers + n);
    c->tb_beta = beta_nitsche;
    c->tb_tangential = tang;
    c->tb_backflow = bf;
    c->tb_ready = false;
    c->jac_valid = false;
    c->pc_valid = false;
  }
  if (n > 0) CHK(cfdh_traction_upload_coef(c));  // values only: they enter the residual, Jacobian and preconditioner stay valid
  return 0;
}

int cfdh_set_schur_pcd(cfdh_ctx *c, int inlet_marker, int outlet_marker, int time_term) {
  NOT_IPCS(c, "cfdh_set_schur_pcd");
  ENTER(c);
  CHK(cfdh_pcd_supported(c, "cfdh_set_schur_pcd"));
  if (time_term != 0 && time_term != 1) return cfdh_fail(c, CFDH_E_ARG, "cfdh_set_schur_pcd: time_term must be 0 or 1");
  const bool markers_changed = !c->pcd_set || inlet_marker != c->pcd_in || outlet_marker != c->pcd_out;
  c->pcd_in = inlet_marker; c->pcd_out = outlet_marker; c->pcd_time = time_term;
  c->pcd_set = true;
  if (markers_changed) { c->pcd_ready = false; c->pc_valid = false; }
  return 0;
}

int cfdh_set_ksp_forcing(cfdh_ctx *c, int version, double rtol_0, double rtol_max, double gamma, double alpha, double threshold) {
  NOT_IPCS(c, "cfdh_set_ksp_forcing");
  ENTER(c);
  if (version != 0 && version != 2) return cfdh_fail(c, CFDH_E_ARG, "cfdh_set_ksp_forcing: version 0 (off) or 2");
  if (version == 2 && !(rtol_0 > 0 && rtol_0 < 1 && rtol_max > 0 && rtol_max < 1 && gamma > 0 && gamma <= 1 && alpha > 1 && alpha <= 2 &&
                        threshold > 0 && threshold < 1))
    return cfdh_fail(c, CFDH_E_ARG, "cfdh_set_ksp_forcing: need 0 < rtol_0, rtol_max, threshold < 1, 0 < gamma <= 1, 1 < alpha <= 2");
  c->ew_version = version;
  if (version == 2) { c->ew_rtol0 = rtol_0; c->ew_rtol_max = rtol_max; c->ew_gamma = gamma; c->ew_alpha = alpha; c->ew_threshold = threshold; }
  return 0;
}

int cfdh_get_newton_history(cfdh_ctx *c, int32_t *n, double *fnorm, double *ksp_rtol, int32_t *ksp_its, double *ksp_rel_res) {
  NOT_IPCS(c, "cfdh_get_newton_history");
  if (!c || !n) return CFDH_E_ARG;
  const size_t m = c->hist_fnorm.size();
  *n = (int32_t)m;
  for (size_t k = 0; k < m; k++) {
    if (fnorm) fnorm[k] = c->hist_fnorm[k];
    if (ksp_rtol) ksp_rtol[k] = c->hist_rtol[k];
    if (ksp_its) ksp_its[k] = c->hist_its[k];
    if (ksp_rel_res) ksp_rel_res[k] = c->hist_relres[k];
  }
  return 0;
}

int cfdh_get_pcd_operator(cfdh_ctx *c, int64_t *nnz, int32_t *rowptr, int32_t *col, double *vals, double *mass_diag) {
  NOT_IPCS(c, "cfdh_get_pcd_operator");
  if (!c || !nnz) return CFDH_E_ARG;
  ENTER(c);
  *nnz = c->nnzv;
  if (!rowptr && !col && !vals && !mass_diag) return 0;
  if (!rowptr || !col || !vals) return cfdh_fail(c, CFDH_E_ARG, "pass all of rowptr/col/vals or none");
  CHK(cfdh_pcd_supported(c, "cfdh_get_pcd_operator"));
  if (!c->pcd_set) return cfdh_fail(c, CFDH_E_STATE, "cfdh_get_pcd_operator: cfdh_set_schur_pcd was not called");
  if (!c->params_set || !c->state_set) return cfdh_fail(c, CFDH_E_STATE, "cfdh_get_pcd_operator: parameters and state are needed");
  CHK(k_pcd_assemble(c, c->x.p));
  std::vector<double> K(c->pcd_K.n);
  std::vector<int> sptr(c->pcd_sptr.n);
  HIPCHK(c, hipMemcpyAsync(K.data(), c->pcd_K.p, sizeof(double) * K.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(sptr.data(), c->pcd_sptr.p, sizeof(int) * sptr.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const int nvo = c->nvo;
  int64_t pos = 0;
  std::vector<std::pair<int, int>> ord;
  for (int vu = 0; vu < nvo; vu++) {
    const int r = c->perm[vu];
    ord.clear();
    for (int k = c->h_vptr[r]; k < c->h_vptr[r + 1]; k++) ord.push_back({c->iperm[c->h_vcol[k]], k - c->h_vptr[r]});
    std::sort(ord.begin(), ord.end());
    rowptr[vu] = (int32_t)pos;
    const size_t base = (size_t)sptr[r >> 6] + (r & 63);
    for (auto &e : ord) { col[pos] = e.first; vals[pos] = K[base + 64 * (size_t)e.second]; pos++; }
  }
  rowptr[nvo] = (int32_t)pos;
  if (mass_diag) for (int vu = 0; vu < nvo; vu++) mass_diag[vu] = c->h_pcd_md[c->perm[vu]];
  return 0;
}

int cfdh_apply_preconditioner(cfdh_ctx *c, const double *r, double *z) {
  NOT_IPCS(c, "cfdh_apply_preconditioner");
  if (!c || !r || !z) return CFDH_E_ARG;
  ENTER(c);
  if (!c->jac_valid) return cfdh_fail(c, CFDH_E_STATE, "no Jacobian assembled yet");
  CHK(cfdh_pc_update(c, false));
  std::vector<double> h;
  pack_vec(c, r, r + (size_t)c->dim * c->nv, h, nullptr);
  CHK(upload_vec(c, h, c->xt.p));
  CHK(cfdh_pc_apply(c, c->xt.p, c->dvec.p));
  std::vector<double> o;
  CHK(download_vec(c, c->dvec.p, o));
  for (int k = 0; k < c->nvo; k++) {
    const int v = c->iperm[k], d = c->dim;
    for (int i = 0; i < d; i++) z[(size_t)d * v + i] = o[(size_t)d * k + i];
    z[(size_t)d * c->nv + v] = o[(size_t)d * c->nvo + k];
  }
  return 0;
}

int cfdh_apply_operator(cfdh_ctx *c, const double *r, double *z, double *w) {
  NOT_IPCS(c, "cfdh_apply_operator");
  if (!c || !r || !z || !w) return CFDH_E_ARG;
  ENTER(c);
  if (c->nranks > 1 || c->nvo != c->nv) return cfdh_fail(c, CFDH_E_STATE, "cfdh_apply_operator: one GPU only");
  if (!c->jac_valid) return cfdh_fail(c, CFDH_E_STATE, "no Jacobian assembled yet");
  CHK(cfdh_pc_update(c, false));
  std::vector<double> h;
  pack_vec(c, r, r + (size_t)c->dim * c->nv, h, nullptr);
  CHK(upload_vec(c, h, c->xt.p));
  CHK(cfdh_apply_operator_dev(c, c->xt.p, c->dvec.p));  // w lands in the Krylov work vector
  std::vector<double> oz, ow;
  CHK(download_vec(c, c->dvec.p, oz));
  CHK(download_vec(c, c->kw.p, ow));
  for (int k = 0; k < c->nvo; k++) {
    const int v = c->iperm[k], d = c->dim;
    for (int i = 0; i < d; i++) { z[(size_t)d * v + i] = oz[(size_t)d * k + i]; w[(size_t)d * v + i] = ow[(size_t)d * k + i]; }
    z[(size_t)d * c->nv + v] = oz[(size_t)d * c->nvo + k];
    w[(size_t)d * c->nvo + v] = ow[(size_t)d * c->nvo + k];
  }
  return 0;
}

// ---- test hook: the step's FGMRES on the caller's right-hand side, with a trace of its last cycle -------------------------------
int cfdh_fgmres_solve(cfdh_ctx *c, const double *b, int newton_index, double *x, int32_t *its, int32_t *reason, cfdh_fgmres_trace *trace) {
  NOT_IPCS(c, "cfdh_fgmres_solve");
  ENTER(c);
  if (!b || !x || !its || !reason) return cfdh_fail(c, CFDH_E_ARG, "cfdh_fgmres_solve: null array");
  if (newton_index < -1 || newton_index >= cfdh_ctx::GUESS_NEWTON)
    return cfdh_fail(c, CFDH_E_ARG, "cfdh_fgmres_solve: newton_index = %d outside -1 .. %d", newton_index, cfdh_ctx::GUESS_NEWTON - 1);
  if (trace && trace->m < c->opt.ksp_restart)
    return cfdh_fail(c, CFDH_E_ARG, "cfdh_fgmres_solve: the trace holds %d columns, ksp_restart is %d", (int)trace->m, c->opt.ksp_restart);
  if (c->nranks > 1 || c->nvo != c->nv) return cfdh_fail(c, CFDH_E_STATE, "cfdh_fgmres_solve: one GPU only");
  if (!c->jac_valid) return cfdh_fail(c, CFDH_E_STATE, "no Jacobian assembled yet");
  HIPCHK(c, c->hook_b.alloc(c->NL)); HIPCHK(c, c->hook_x.alloc(c->NL));
  std::vector<double> h;
  pack_vec(c, b, b + (size_t)c->dim * c->nv, h, nullptr);
  CHK(upload_vec(c, h, c->hook_b.p));
  FgmresTrace tr;
  int kits = 0, kreason = 0;
  CHK(cfdh_fgmres_hook(c, c->hook_b.p, c->hook_x.p, newton_index, &kits, &kreason, trace ? &tr : nullptr));
  *its = kits; *reason = kreason;
  const int d = c->dim, nv = c->nv;
  const size_t n = (size_t)(d + 1) * nv;
  std::vector<double> o;
  auto fetch = [&](const double *dev, double *out) -> int {  // one device vector into the caller's numbering
    if (!out) return 0;
    CHK(download_vec(c, dev, o));
    unpack_vec(c, o, out, out + (size_t)d * nv);
    return 0;
  };
  CHK(fetch(c->hook_x.p, x));
  if (!trace) return 0;
  const int m = c->opt.ksp_restart, k = tr.k, M = trace->m;
  trace->cycles = tr.cycles; trace->k = k; trace->guess_used = tr.guess_used ? 1 : 0; trace->fp32_used = tr.fp32_used ? 1 : 0;
  trace->bn = tr.bn; trace->tol = tr.tol; trace->beta = tr.beta;
  trace->n_res = (int32_t)tr.res.size();
  CHK(fetch(tr.x0.p, trace->x0));
  CHK(fetch(tr.x_start.p, trace->x_start));
  const size_t ld = ((size_t)c->NL + 1) & ~(size_t)1;  // leading dimension of the Krylov workspace
  if (trace->V && tr.cycles > 0) {
    CHK(fetch(tr.v0.p, trace->V));
    for (int i = 1; i <= k; i++) CHK(fetch(c->kV.p + (size_t)i * ld, trace->V + (size_t)i * n));
  }
  if (trace->Z) for (int j = 0; j < k; j++) CHK(fetch(c->kZ.p + (size_t)j * ld, trace->Z + (size_t)j * n));
  for (int j = 0; j < k; j++) {
    if (trace->H) for (int i = 0; i <= j + 1; i++) trace->H[(size_t)j * (M + 1) + i] = tr.H[(size_t)j * (m + 1) + i];
    if (trace->ww) trace->ww[j] = tr.ww[j];
    if (trace->nrm2) trace->nrm2[j] = tr.nrm2[j];
    if (trace->second_pass) trace->second_pass[j] = tr.second_pass[j];
    if (trace->y && j < (int)tr.y.size()) trace->y[j] = tr.y[j];
  }
  if (trace->res) for (int i = 0; i < (int)tr.res.size() && i < trace->max_res; i++) trace->res[i] = tr.res[i];
  for (int i = 0; i < (int)tr.cycle_beta.size() && i < trace->max_cycles; i++) {
    if (trace->cycle_beta) trace->cycle_beta[i] = tr.cycle_beta[i];
    if (trace->cycle_est) trace->cycle_est[i] = i < (int)tr.cycle_est.size() ? tr.cycle_est[i] : std::nan("");
  }
  return 0;
}

// ---- test hook: ONE Krylov vector wrapper (v_* of cfdh_krylov_vec.hip) on caller data, launched as the solver launches it ------
int cfdh_krylov_vec_op(cfdh_ctx *c, int op, int n, int ld, int nvec, const double *A, const double *B, const double *x, const double *y,
                       const double *coef, double scalar, int flags, double *out1, double *out2, float *out32, int32_t *nscal,
                       double *scal_host, double *scal_dev, double *scal_mirror) {
  NOT_IPCS(c, "cfdh_krylov_vec_op");
  ENTER(c);
  if (c->nranks > 1 || c->nvo != c->nv) return cfdh_fail(c, CFDH_E_STATE, "cfdh_krylov_vec_op: one GPU only");
  // ---- everything the production callers guarantee is checked here, before any launch
  if (op < 0 || op >= CFDH_KVOP_COUNT) return cfdh_fail(c, CFDH_E_ARG, "cfdh_krylov_vec_op: unknown op %d", op);
  if (n < 1) return cfdh_fail(c, CFDH_E_ARG, "cfdh_krylov_vec_op: n = %d < 1", n);
  if (nvec < 1) return cfdh_fail(c, CFDH_E_ARG, "cfdh_krylov_vec_op: nvec = %d < 1", nvec);
  if (ld < n) return cfdh_fail(c, CFDH_E_ARG, "cfdh_krylov_vec_op: ld = %d < n = %d", ld, n);
  if (ld & 1) return cfdh_fail(c, CFDH_E_ARG, "cfdh_krylov_vec_op: odd ld = %d (the columns must stay 16-byte aligned)", ld);
  const bool f32 = op == CFDH_KVOP_MULTIDOT32 || op == CFDH_KVOP_GS_UPDATE32;
  if (f32 && (ld & 3)) return cfdh_fail(c, CFDH_E_ARG, "cfdh_krylov_vec_op: ld = %d is not a multiple of 4 (fp32 basis copy)", ld);
  if ((op == CFDH_KVOP_GUESS || op == CFDH_KVOP_GRAM) && nvec > 8)
    return cfdh_fail(c, CFDH_E_ARG, "cfdh_krylov_vec_op: k = %d kept vectors outside 1 .. 8", nvec);
  // which inputs and outputs the op uses
  bool nA = false, nB = false, nx = true, ny = false, nc = false, o1 = false, o2 = false, o32 = false;
  switch (op) {
    case CFDH_KVOP_DOT: case CFDH_KVOP_NORM2_PAIR: ny = true; break;
    case CFDH_KVOP_NORM2: break;
    case CFDH_KVOP_NORM2_TRIPLE: ny = nA = true; break;
    case CFDH_KVOP_NORMINF_DIFF: ny = (flags & 1) != 0; break;
    case CFDH_KVOP_SUB_MEAN: case CFDH_KVOP_NORM_SCALE_INV: case CFDH_KVOP_SCALE: case CFDH_KVOP_SCALE_TO: o1 = true; break;
    case CFDH_KVOP_MULTIDOT: case CFDH_KVOP_MULTIDOT32: case CFDH_KVOP_GRAM: nA = true; break;
    case CFDH_KVOP_MULTIAXPY: case CFDH_KVOP_LINCOMB: case CFDH_KVOP_GS_UPDATE_NORMALIZE: nA = nc = o1 = true; break;
    case CFDH_KVOP_LINCOMB_KEEP: nA = nc = o1 = o2 = true; break;
    case CFDH_KVOP_GS_UPDATE32: nA = nc = o1 = o32 = true; break;
    case CFDH_KVOP_STORE32: o32 = true; break;
    case CFDH_KVOP_GUESS: nA = nB = nc = o1 = o2 = true; break;
    case CFDH_KVOP_AXPY: case CFDH_KVOP_WAXPY: case CFDH_KVOP_PMULT: ny = o1 = true; break;
  }
  if ((nA && !A) || (nB && !B) || (nx && !x) || (ny && !y) || (nc && !coef) || (o1 && !out1) || (o2 && !out2) || (o32 && !out32) ||
      !nscal || !scal_host || !scal_dev || !scal_mirror)
    return cfdh_fail(c, CFDH_E_ARG, "cfdh_krylov_vec_op: op %d misses an array", op);
  const bool to_ring = (flags & 2) != 0;
  const bool mirrored = op == CFDH_KVOP_MULTIDOT || op == CFDH_KVOP_MULTIDOT32 || op == CFDH_KVOP_GS_UPDATE32;
  CHK(ensure_krylov(c));
  if ((size_t)(nvec + 2) * 1024 > c->red_partial.n) HIPCHK(c, c->red_partial.alloc((size_t)(nvec + 2) * 1024 + 1024));
  if (mirrored && (size_t)nvec + 2 > (to_ring ? c->h_ring_stride : (size_t)HP_MIRROR_N))
    return cfdh_fail(c, CFDH_E_ARG, "cfdh_krylov_vec_op: nvec = %d does not fit the host-mapped words", nvec);

  const size_t N = (size_t)n, LD = (size_t)ld, blk = LD * (size_t)nvec;
  HookBuf<double> dA, dB, dx, dy, dc, d1, d2, ds;
  HookBuf<float> dA32, d32;
  if (nA && !f32) { if (op == CFDH_KVOP_NORM2_TRIPLE) CHK(dA.put(c, A, LD, N)); else CHK(dA.put(c, A, blk, blk)); }
  std::vector<float> a32;
  if (nA && f32) {  // the fp32 copy of the basis, as v_store32 rounds it
    a32.resize(blk);
    for (size_t i = 0; i < blk; i++) a32[i] = (float)A[i];
    CHK(dA32.put(c, a32.data(), blk, blk));
  }
  if (nB) CHK(dB.put(c, B, blk, blk));
  if (nx) CHK(dx.put(c, x, LD, N));
  if (ny) CHK(dy.put(c, y, LD, N));
  const int ncoef = op == CFDH_KVOP_GS_UPDATE_NORMALIZE ? nvec + 1 : (op == CFDH_KVOP_GUESS ? 8 * (nvec + 1) : nvec);
  if (nc) CHK(dc.put(c, coef, (size_t)ncoef, (size_t)ncoef));
  if (o1) CHK(d1.put(c, nullptr, LD, 0));
  if (o2) CHK(d2.put(c, nullptr, LD, 0));
  if (o32) CHK(d32.put(c, nullptr, LD, 0));
  CHK(ds.put(c, nullptr, (size_t)std::max(nvec + 2, 8 * 9), 0));  // device scalars: h, the Gram slots, a norm
  HIPCHK(c, hipStreamSynchronize(c->stream));
  // the host-mapped words the op may write start from a pattern no result has
  double *mir_host = to_ring && mirrored ? c->h_ring + (size_t)((nvec - 1) % cfdh_ctx::KRING) * c->h_ring_stride : c->h_pinned + HP_MIRROR;
  double *mir_dev = to_ring && mirrored ? c->h_ring_dev + (size_t)((nvec - 1) % cfdh_ctx::KRING) * c->h_ring_stride : scalars_mirror(c);
  const int nmir_max = mirrored ? nvec + 2 : 16;
  for (int i = 0; i < nmir_max; i++) mir_host[i] = -7.25;
  int ns = 0, nd = 0, nm = 0;  // scalars returned by the wrapper / left on the device / in the host-mapped words
  const double *dev_src = ds.p;
  switch (op) {
    case CFDH_KVOP_DOT: CHK(v_dot(c, n, dx.p, dy.p, scal_host)); ns = nd = nm = 1; dev_src = c->red_out.p; break;
    case CFDH_KVOP_NORM2: CHK(v_norm2(c, n, dx.p, scal_host)); ns = nd = nm = 1; dev_src = c->red_out.p; break;
    case CFDH_KVOP_NORM2_PAIR: CHK(v_norm2_pair(c, n, dx.p, dy.p, scal_host, scal_host + 1)); ns = nd = nm = 2; dev_src = c->red_out.p; break;
    case CFDH_KVOP_NORM2_TRIPLE: CHK(v_norm2_triple(c, n, dx.p, dy.p, dA.p, scal_host)); ns = nd = nm = 3; dev_src = c->red_out.p; break;
    case CFDH_KVOP_NORMINF_DIFF: CHK(v_norminf_diff(c, n, dx.p, ny ? dy.p : nullptr, scal_host)); ns = nd = nm = 1; dev_src = c->red_out.p; break;
    case CFDH_KVOP_SUB_MEAN:
      HIPCHK(c, hipMemcpyAsync(d1.p, dx.p, sizeof(double) * N, hipMemcpyDeviceToDevice, c->stream));
      CHK(v_sub_mean(c, n, d1.p)); nd = 1; dev_src = c->red_out.p + RO_MEAN; break;
    case CFDH_KVOP_NORM_SCALE_INV:
      CHK(v_norm_to_dev(c, n, dx.p, ds.p));
      CHK(v_scale_inv_dev(c, n, dx.p, ds.p, d1.p)); nd = 1; break;
    case CFDH_KVOP_MULTIDOT: {
      const bool ww = (flags & 1) != 0;
      CHK(v_multidot(c, n, dA.p, ld, nvec, dx.p, ds.p, ww, mir_dev)); nd = nm = nvec + (ww ? 1 : 0); break;
    }
    case CFDH_KVOP_MULTIDOT32: CHK(v_multidot32(c, n, dA32.p, ld, nvec, dx.p, ds.p, mir_dev)); nd = nm = nvec + 1; break;
    case CFDH_KVOP_GRAM: CHK(v_gram(c, n, dA.p, ld, nvec, dx.p, ds.p)); nd = 8 * (nvec + 1); break;
    case CFDH_KVOP_MULTIAXPY:
      HIPCHK(c, hipMemcpyAsync(d1.p, dx.p, sizeof(double) * N, hipMemcpyDeviceToDevice, c->stream));
      CHK(v_multiaxpy(c, n, dA.p, ld, nvec, dc.p, d1.p)); break;
    case CFDH_KVOP_LINCOMB:
      HIPCHK(c, hipMemcpyAsync(d1.p, dx.p, sizeof(double) * N, hipMemcpyDeviceToDevice, c->stream));
      CHK(v_lincomb(c, n, dA.p, ld, nvec, dc.p, d1.p)); break;
    case CFDH_KVOP_LINCOMB_KEEP:
      HIPCHK(c, hipMemcpyAsync(d1.p, dx.p, sizeof(double) * N, hipMemcpyDeviceToDevice, c->stream));
      CHK(v_lincomb_keep(c, n, dA.p, ld, nvec, dc.p, d1.p, d2.p)); break;
    case CFDH_KVOP_GS_UPDATE_NORMALIZE: CHK(v_gs_update_normalize(c, n, dA.p, ld, nvec, dc.p, dx.p, d1.p, ds.p)); nd = 1; break;
    case CFDH_KVOP_GS_UPDATE32:
      // the slot layout of an iteration: [h_0 .. h_j, w.w, measured norm]; the norm is the only word written here
      CHK(v_gs_update32(c, n, dA32.p, ld, nvec, dc.p, dx.p, d1.p, d32.p, ds.p, mir_dev + (nvec + 1))); nd = 1; nm = nvec + 2; break;
    case CFDH_KVOP_STORE32: CHK(v_store32(c, n, dx.p, d32.p)); break;
    case CFDH_KVOP_GUESS: {
      CHK(v_guess_combine(c, n, dA.p, dB.p, ld, nvec, dc.p, dx.p, d1.p, d2.p));
      bool used = false; int rank = 0;
      CHK(v_guess_read(c, nvec, scal_host, &used, &rank, scal_host + 3));
      scal_host[1] = used ? 1.0 : 0.0; scal_host[2] = (double)rank;
      if (flags & 1) CHK(v_scale_inv_lean(c, n, d2.p));
      ns = nm = 3 + nvec;
      // device side: the squared norm, then y as guess_combine_kernel read it
      HIPCHK(c, hipMemcpyAsync(ds.p, c->red_out.p + RO_LEAN_S2, sizeof(double), hipMemcpyDeviceToDevice, c->stream));
      HIPCHK(c, hipMemcpyAsync(ds.p + 1, c->ky.p, sizeof(double) * nvec, hipMemcpyDeviceToDevice, c->stream));
      nd = 1 + nvec; break;
    }
    case CFDH_KVOP_AXPY:
      HIPCHK(c, hipMemcpyAsync(d1.p, dy.p, sizeof(double) * N, hipMemcpyDeviceToDevice, c->stream));
      CHK(v_axpy(c, n, scalar, dx.p, d1.p)); break;
    case CFDH_KVOP_WAXPY: CHK(v_waxpy(c, n, scalar, dx.p, dy.p, d1.p)); break;
    case CFDH_KVOP_SCALE:
      HIPCHK(c, hipMemcpyAsync(d1.p, dx.p, sizeof(double) * N, hipMemcpyDeviceToDevice, c->stream));
      CHK(v_scale(c, n, scalar, d1.p)); break;
    case CFDH_KVOP_SCALE_TO: CHK(v_scale_to(c, n, scalar, dx.p, d1.p)); break;
    case CFDH_KVOP_PMULT: CHK(v_pointwise_mult(c, n, dx.p, dy.p, d1.p)); break;
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (nd) HIPCHK(c, hipMemcpy(scal_dev, dev_src, sizeof(double) * nd, hipMemcpyDeviceToHost));
  for (int i = 0; i < nm; i++) scal_mirror[i] = mir_host[i];
  nscal[0] = ns; nscal[1] = nd; nscal[2] = nm;
  if (o1) CHK(d1.get(c, out1, N));
  if (o2) CHK(d2.get(c, out2, N));
  if (o32) CHK(d32.get(c, out32, N));
  return 0;
}

// ---- read-only view of the built hierarchies (cfdh_get_amg_operator / cfdh_get_amg_vectors)
static int amg_pick(cfdh_ctx *c, const char *name, int hier, int level, AmgHier **H, AmgLevel **L) {
  if (!c->pc_valid) return cfdh_fail(c, CFDH_E_STATE, "%s: no preconditioner built yet (cfdh_apply_preconditioner or cfdh_solve_step first)", name);
  *H = nullptr;
  *L = nullptr;
  if (hier == CFDH_AMG_HIER_H) {
    if (c->opt.pc_type != 1 || c->Hlev.n <= 0) return cfdh_fail(c, CFDH_E_STATE, "%s: H exists for pc_type 1 only", name);
    *L = &c->Hlev;
    return 0;
  }
  if (hier == CFDH_AMG_HIER_DL0) {  // the distributed level has its own operators and no AmgLevel: the callers take c->dl0
    if (c->gp_n <= 0 || !c->hLg.valid || !c->dl0.on) return cfdh_fail(c, CFDH_E_STATE, "%s: no distributed finest pressure level on this context", name);
    *H = &c->hLg;
    return 0;
  }
  if (hier != CFDH_AMG_HIER_A && hier != CFDH_AMG_HIER_P && hier != CFDH_AMG_HIER_PG) return cfdh_fail(c, CFDH_E_ARG, "%s: unknown hierarchy %d", name, hier);
  if (hier == CFDH_AMG_HIER_A && c->opt.pc_type == 0) return cfdh_fail(c, CFDH_E_STATE, "%s: pc_type 0 has no velocity hierarchy", name);
  if (hier == CFDH_AMG_HIER_PG && c->gp_n <= 0) return cfdh_fail(c, CFDH_E_STATE, "%s: no replicated pressure space (cfdh_set_global_pressure_space)", name);
  AmgHier *h = hier == CFDH_AMG_HIER_A ? &c->hA : hier == CFDH_AMG_HIER_PG ? &c->hLg : (c->opt.pc_type == 0 ? &c->hS : &c->hL);
  if (!h->valid) return cfdh_fail(c, CFDH_E_STATE, "%s: hierarchy %d is not built", name, hier);
  if (level < 0 || level >= (int)h->lev.size()) return cfdh_fail(c, CFDH_E_ARG, "%s: level %d of %d", name, level, (int)h->lev.size());
  *H = h;
  *L = h->lev[level];
  return 0;
}
// Level 0 of a rank's own hierarchies numbers the local nodes (all of them, or the owned ones, which come first and are permuted
// among themselves); level 0 of the replicated hierarchy numbers the global pressure space, which the library never renumbers.
static bool amg_local_dim(const cfdh_ctx *c, int n) { return n == (int)c->perm.size() || n == c->nvo; }

int cfdh_get_amg_operator(cfdh_ctx *c, int hier, int level, int which, int64_t *nrow, int64_t *ncol, int64_t *nnz, int32_t *rowptr,
                          int32_t *col, double *vals) {
  NOT_IPCS(c, "cfdh_get_amg_operator");
  if (!c || !nrow || !ncol || !nnz) return CFDH_E_ARG;
  ENTER(c);
  AmgHier *H = nullptr;
  AmgLevel *L = nullptr;
  CHK(amg_pick(c, "cfdh_get_amg_operator", hier, level, &H, &L));
  const bool dl0 = hier == CFDH_AMG_HIER_DL0;
  if (dl0 ? (which != CFDH_AMG_OP_A && which != CFDH_AMG_OP_P && which != CFDH_AMG_OP_PT) : (which < CFDH_AMG_OP_A || which > CFDH_AMG_OP_SC))
    return cfdh_fail(c, CFDH_E_ARG, "cfdh_get_amg_operator: unknown operator %d", which);
  if (!H || dl0) level = 0;
  const CsrDev &M = dl0 ? (which == CFDH_AMG_OP_A ? c->dl0.A : which == CFDH_AMG_OP_P ? c->dl0.P : c->dl0.PT)
                        : which == CFDH_AMG_OP_A ? L->A : which == CFDH_AMG_OP_P ? L->P : which == CFDH_AMG_OP_G ? L->G : which == CFDH_AMG_OP_SB ? L->Sb : L->Sc;
  if (M.n <= 0 || !M.rowptr.p || !M.col.p || !M.val.p)
    return cfdh_fail(c, CFDH_E_STATE, "cfdh_get_amg_operator: operator %d of level %d is not kept in fp64 CSR (P: CFDH_AMG_KEEP=1 before the build)", which, level);
  *nrow = M.n; *ncol = M.m; *nnz = M.nnz;
  if (!rowptr && !col && !vals) return 0;
  if (!rowptr || !col || !vals) return cfdh_fail(c, CFDH_E_ARG, "pass all of rowptr/col/vals or none");
  std::vector<int> rp((size_t)M.n + 1), cl((size_t)M.nnz);
  std::vector<double> vl((size_t)M.nnz);
  HIPCHK(c, hipMemcpyAsync(rp.data(), M.rowptr.p, sizeof(int) * rp.size(), hipMemcpyDeviceToHost, c->stream));
  if (M.nnz > 0) {
    HIPCHK(c, hipMemcpyAsync(cl.data(), M.col.p, sizeof(int) * cl.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(vl.data(), M.val.p, sizeof(double) * vl.size(), hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (rp[M.n] != M.nnz) return cfdh_fail(c, CFDH_E_STATE, "cfdh_get_amg_operator: rowptr ends at %d, the operator holds %d entries", rp[M.n], M.nnz);
  // level 0 lives in the internal numbering: rows / columns that number it go back to the caller's
  const bool local0 = level == 0 && hier != CFDH_AMG_HIER_PG;
  const bool rows0 = local0 && which != CFDH_AMG_OP_G && which != CFDH_AMG_OP_PT && amg_local_dim(c, M.n);
  const bool cols0 = local0 && (which == CFDH_AMG_OP_A || which == CFDH_AMG_OP_SB || which == CFDH_AMG_OP_G || which == CFDH_AMG_OP_PT) && amg_local_dim(c, M.m);
  // the restriction of the distributed level sums every coarse row in the stored order: its entries stay in that order
  const bool resort = cols0 && which != CFDH_AMG_OP_PT;
  int64_t pos = 0;
  std::vector<std::pair<int, double>> row;
  for (int ru = 0; ru < M.n; ru++) {
    const int r = rows0 ? c->perm[ru] : ru;
    rowptr[ru] = (int32_t)pos;
    row.clear();
    for (int k = rp[r]; k < rp[r + 1]; k++) row.push_back({cols0 ? c->iperm[cl[k]] : cl[k], vl[k]});
    // a stable sort by column only: the order in which the build stored equal or descending columns stays visible to the caller
    if (resort) std::stable_sort(row.begin(), row.end(), [](const std::pair<int, double> &a, const std::pair<int, double> &b) { return a.first < b.first; });
    for (auto &e : row) { col[pos] = e.first; vals[pos] = e.second; pos++; }
  }
  rowptr[M.n] = (int32_t)pos;
  return 0;
}

int cfdh_get_amg_head(cfdh_ctx *c, int hier, int level, int which, int32_t *width) {
  NOT_IPCS(c, "cfdh_get_amg_head");
  if (!c || !width) return CFDH_E_ARG;
  ENTER(c);
  AmgHier *H = nullptr;
  AmgLevel *L = nullptr;
  if (hier == CFDH_AMG_HIER_DL0) return cfdh_fail(c, CFDH_E_ARG, "cfdh_get_amg_head: the distributed level has no head copies");
  CHK(amg_pick(c, "cfdh_get_amg_head", hier, level, &H, &L));
  const bool single = hier == CFDH_AMG_HIER_H;
  if (single ? which != CFDH_AMG_OP_A : (which != CFDH_AMG_OP_SB && which != CFDH_AMG_OP_SC))
    return cfdh_fail(c, CFDH_E_ARG, "cfdh_get_amg_head: operator %d has no head copy", which);
  const CsrDev &M = single ? L->A : which == CFDH_AMG_OP_SB ? L->Sb : L->Sc;
  *width = M.head_w;
  return 0;
}

int cfdh_get_amg_vectors(cfdh_ctx *c, int hier, int level, int which, int64_t *n, double *out) {
  NOT_IPCS(c, "cfdh_get_amg_vectors");
  if (!c || !n) return CFDH_E_ARG;
  ENTER(c);
  AmgHier *H = nullptr;
  AmgLevel *L = nullptr;
  CHK(amg_pick(c, "cfdh_get_amg_vectors", hier, level, &H, &L));
  const bool dl0 = hier == CFDH_AMG_HIER_DL0;
  if (!H || dl0) level = 0;
  if (dl0 && which != CFDH_AMG_VEC_WDINV && which != CFDH_AMG_VEC_ORDER && which != CFDH_AMG_VEC_DL0_SHAPE)
    return cfdh_fail(c, CFDH_E_ARG, "cfdh_get_amg_vectors: the distributed level has no item %d", which);
  AmgLevel dl0_view;  // n and nothing else: the vectors of the distributed level live in c->dl0
  if (dl0) { dl0_view.n = c->nv; L = &dl0_view; }
  const bool perm0 = level == 0 && hier != CFDH_AMG_HIER_PG && amg_local_dim(c, L->n);
  auto fetch = [&](const void *src, size_t bytes, void *dst) -> int {
    HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
  };
  const int nvo = c->nvo;
  switch (which) {
    case CFDH_AMG_VEC_DINV:
    case CFDH_AMG_VEC_WDINV: {
      const dbuf<double> &v = dl0 ? c->dl0.wdinv : which == CFDH_AMG_VEC_DINV ? L->dinv : L->wdinv;
      if (!v.p || (int)v.n < L->n) return cfdh_fail(c, CFDH_E_STATE, "cfdh_get_amg_vectors: vector %d is not there", which);
      *n = L->n;
      if (!out) return 0;
      std::vector<double> h((size_t)L->n);
      CHK(fetch(v.p, sizeof(double) * h.size(), h.data()));
      for (int i = 0; i < L->n; i++) out[i] = h[perm0 ? c->perm[i] : i];
      return 0;
    }
    case CFDH_AMG_VEC_AGG: {
      if (!L->agg.p || (int)L->agg.n < L->n) return cfdh_fail(c, CFDH_E_STATE, "cfdh_get_amg_vectors: the aggregate ids were not kept (CFDH_AMG_KEEP=1 before the build)");
      *n = L->n;
      if (!out) return 0;
      std::vector<int> h((size_t)L->n);
      CHK(fetch(L->agg.p, sizeof(int) * h.size(), h.data()));
      for (int i = 0; i < L->n; i++) out[i] = (double)h[perm0 ? c->perm[i] : i];
      return 0;
    }
    case CFDH_AMG_VEC_COARSE_INV: {
      if (!H || H->coarse_n <= 0 || !H->coarse_inv.p) return cfdh_fail(c, CFDH_E_STATE, "cfdh_get_amg_vectors: no dense coarsest inverse");
      *n = (int64_t)H->coarse_n * H->coarse_n;
      if (!out) return 0;
      // a hierarchy of one level: its coarsest operator is level 0, which lives in the internal numbering
      if (H->lev.size() == 1 && hier != CFDH_AMG_HIER_PG && amg_local_dim(c, H->coarse_n)) {
        const size_t m = (size_t)H->coarse_n;
        std::vector<double> h(m * m);
        CHK(fetch(H->coarse_inv.p, sizeof(double) * h.size(), h.data()));
        for (size_t i = 0; i < m; i++)
          for (size_t j = 0; j < m; j++) out[i * m + j] = h[(size_t)c->perm[i] * m + (size_t)c->perm[j]];
        return 0;
      }
      return fetch(H->coarse_inv.p, sizeof(double) * (size_t)*n, out);
    }
    case CFDH_AMG_VEC_D: {
      if (L->Dn <= 0 || !L->D.p) return cfdh_fail(c, CFDH_E_STATE, "cfdh_get_amg_vectors: level %d has no folded dense correction", level);
      *n = (int64_t)L->n * L->Dn;
      if (!out) return 0;
      std::vector<float> h((size_t)*n);
      CHK(fetch(L->D.p, sizeof(float) * h.size(), h.data()));
      for (int i = 0; i < L->n; i++) {
        const size_t r = (size_t)(perm0 ? c->perm[i] : i);
        for (int j = 0; j < L->Dn; j++) out[(size_t)i * L->Dn + j] = (double)h[r * L->Dn + j];
      }
      return 0;
    }
    case CFDH_AMG_VEC_LAMBDA:
      *n = 2;
      if (out) { out[0] = L->lmax; out[1] = L->lmin; }
      return 0;
    case CFDH_AMG_VEC_CC_SCALARS:
      *n = 2;
      if (out) { out[0] = c->cc_alpha; out[1] = c->cc_beta; }
      return 0;
    case CFDH_AMG_VEC_CC_ML: {
      if (!c->ccMl.p || (int)c->ccMl.n < nvo) return cfdh_fail(c, CFDH_E_STATE, "cfdh_get_amg_vectors: no lumped mass (pc_type 1, 2)");
      *n = nvo;
      if (!out) return 0;
      std::vector<double> h((size_t)nvo);
      CHK(fetch(c->ccMl.p, sizeof(double) * h.size(), h.data()));
      for (int i = 0; i < nvo; i++) out[i] = h[c->perm[i]];
      return 0;
    }
    case CFDH_AMG_VEC_CC_PBC: {
      if (!c->ccPbc.p || (int)c->ccPbc.n < nvo) return cfdh_fail(c, CFDH_E_STATE, "cfdh_get_amg_vectors: no pressure flags (pc_type 1, 2)");
      *n = nvo;
      if (!out) return 0;
      std::vector<unsigned char> h((size_t)nvo);
      CHK(fetch(c->ccPbc.p, h.size(), h.data()));
      for (int i = 0; i < nvo; i++) out[i] = (double)h[c->perm[i]];
      return 0;
    }
    case CFDH_AMG_VEC_SPGEMM_ROWS:
      if (!H) return cfdh_fail(c, CFDH_E_ARG, "cfdh_get_amg_vectors: H is built without sparse products");
      *n = 3;
      if (out) for (int q = 0; q < 3; q++) out[q] = (double)H->spgemm_rows[q];
      return 0;
    case CFDH_AMG_VEC_SHAPE: {
      const int nl = H ? (int)H->lev.size() : 1;
      *n = 4 + 5 * (int64_t)nl;
      if (!out) return 0;
      out[0] = nl; out[1] = H ? H->coarse_n : 0; out[2] = H ? H->ncol : 1; out[3] = H && H->fused ? 1 : 0;
      for (int l = 0; l < nl; l++) {
        const AmgLevel *q = H ? H->lev[l] : L;
        double *o = out + 4 + 5 * l;
        o[0] = q->n; o[1] = q->Dn; o[2] = q->fine ? 1 : 0; o[3] = q->sell ? 1 : 0; o[4] = q->agg.p ? 1 : 0;
      }
      return 0;
    }
    case CFDH_AMG_VEC_A00_LMAX:
      if (c->opt.pc_type != 0) return cfdh_fail(c, CFDH_E_STATE, "cfdh_get_amg_vectors: the Chebyshev solve on A00 belongs to pc_type 0");
      *n = 1;
      if (out) out[0] = c->lmaxA;
      return 0;
    case CFDH_AMG_VEC_A00_DINV: {
      const size_t nu = (size_t)c->dim * nvo;
      if (c->opt.pc_type != 0 || !c->dinvA.p || c->dinvA.n < nu) return cfdh_fail(c, CFDH_E_STATE, "cfdh_get_amg_vectors: 1 / diag(A00) belongs to pc_type 0");
      *n = (int64_t)nu;
      if (!out) return 0;
      std::vector<double> h(nu);
      CHK(fetch(c->dinvA.p, sizeof(double) * nu, h.data()));
      for (int i = 0; i < nvo; i++)
        for (int q = 0; q < c->dim; q++) out[(size_t)c->dim * i + q] = h[(size_t)c->dim * c->perm[i] + q];
      return 0;
    }
    case CFDH_AMG_VEC_DL0_SHAPE: {
      if (!dl0) return cfdh_fail(c, CFDH_E_ARG, "cfdh_get_amg_vectors: item %d belongs to CFDH_AMG_HIER_DL0", which);
      *n = 8;
      if (!out) return 0;
      // the decisions of k_dl0_down / k_dl0_up, through the functions they call (cfdh_internal.hpp)
      const cfdh_ctx::DistL0 &d = c->dl0;
      out[0] = d.n1; out[1] = d.ghost_rhs ? 1 : 0;
      out[2] = cfdh_pre_takes_sell(d.A, cfdh_dl0_rule_A(c)) ? 1 : 0;
      out[3] = cfdh_post_takes_sell(d.A, cfdh_dl0_rule_A(c)) ? 1 : 0;
      out[4] = cfdh_prolong_takes_sell(d.P, cfdh_dl0_rule_P(c)) ? 1 : 0;
      out[5] = cfdh_dl0_coarse_fused(c) ? 1 : 0;
      out[6] = c->nvo; out[7] = c->nv;
      return 0;
    }
    case CFDH_AMG_VEC_ORDER:
      *n = L->n;
      if (out) for (int i = 0; i < L->n; i++) out[i] = (double)(perm0 ? c->perm[i] : i);
      return 0;
    default:
      return cfdh_fail(c, CFDH_E_ARG, "cfdh_get_amg_vectors: unknown item %d", which);
  }
}

int cfdh_set_previous2(cfdh_ctx *c, const double *u_prev2) {
  if (c && c->ipcs) { ENTER(c); if (!u_prev2) return cfdh_fail(c, CFDH_E_ARG, "u_prev2 is NULL"); return ipcs_put(c, c->ipcs->u_n1, u_prev2); }
  ENTER(c);
  if (!u_prev2) return cfdh_fail(c, CFDH_E_ARG, "u_prev2 is NULL");
  std::vector<double> h;
  pack_vec(c, u_prev2, nullptr, h, nullptr);
  CHK(upload_vec(c, h, c->xprev2.p));
  return 0;
}

int cfdh_get_previous2(cfdh_ctx *c, double *u_prev2) {
  if (c && c->ipcs) { ENTER(c); return ipcs_get(c, c->ipcs->u_n1, u_prev2); }
  ENTER(c);
  std::vector<double> h;
  CHK(download_vec(c, c->xprev2.p, h));
  unpack_vec(c, h, u_prev2, nullptr);
  return 0;
}

int cfdh_shift_history(cfdh_ctx *c) {
  NOT_IPCS(c, "cfdh_shift_history");
  ENTER(c);
  CHK(v_copy(c, c->NL, c->xprev.p, c->xprev2.p));
  return 0;
}

int cfdh_assemble(cfdh_ctx *c, int want_jacobian) {
  NOT_IPCS(c, "cfdh_assemble");
  ENTER(c);
  if (!c->params_set) return cfdh_fail(c, CFDH_E_STATE, "cfdh_set_params was not called");
  CHK(cfdh_prepare_assembly(c));
  CHK(comm_halo(c, c->x.p));
  CHK(k_assemble(c, c->x.p, want_jacobian ? 1 : 2));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

int cfdh_get_csr(cfdh_ctx *c, int64_t *nnz, int32_t *rowptr, int32_t *col, double *vals) {
  NOT_IPCS(c, "cfdh_get_csr");
  if (!c || !nnz) return CFDH_E_ARG;
  *nnz = (long long)(c->dim + 1) * (c->dim + 1) * c->nnzv;
  if (!rowptr && !col && !vals) return 0;
  if (!rowptr || !col || !vals) return cfdh_fail(c, CFDH_E_ARG, "pass all of rowptr/col/vals or none");
  if (!c->jac_valid) return cfdh_fail(c, CFDH_E_STATE, "no Jacobian assembled yet");
  std::vector<double> a00, a01, a10, a11;
  CHK(cfdh_download_blocks(c, a00, a01, a10, a11));
  const int nvo = c->nvo, nv = c->nv, d = c->dim;
  // rows in user numbering: u rows d*v+i (v < nvo), then p rows d*nvo+v
  int64_t pos = 0;
  std::vector<std::pair<int, int>> ord;  // (user column vertex, slot k)
  auto emit_rows = [&](int kind) {
    for (int vu = 0; vu < nvo; vu++) {
      const int r = c->perm[vu];
      ord.clear();
      for (int k = c->h_vptr[r]; k < c->h_vptr[r + 1]; k++) ord.push_back({c->iperm[c->h_vcol[k]], k});
      std::sort(ord.begin(), ord.end());
      const int nrow = kind == 0 ? d : 1;
      for (int i = 0; i < nrow; i++) {
        const int row = kind == 0 ? d * vu + i : d * nvo + vu;
        rowptr[row] = (int32_t)pos;
        for (auto &e : ord)
          for (int j = 0; j < d; j++) {
            col[pos] = d * e.first + j;
            vals[pos] = kind == 0 ? a00[(size_t)d * d * e.second + (size_t)d * i + j] : a10[(size_t)d * e.second + j];
            pos++;
          }
        for (auto &e : ord) {
          col[pos] = d * nv + e.first;
          vals[pos] = kind == 0 ? a01[(size_t)d * e.second + i] : a11[e.second];
          pos++;
        }
      }
    }
  };
  emit_rows(0);
  emit_rows(1);
  rowptr[(d + 1) * nvo] = (int32_t)pos;
  return 0;
}

int cfdh_spmv(cfdh_ctx *c, const double *x, double *y) {
  NOT_IPCS(c, "cfdh_spmv");
  if (!c || !x || !y) return CFDH_E_ARG;
  if (!c->jac_valid) return cfdh_fail(c, CFDH_E_STATE, "no Jacobian assembled yet");
  std::vector<double> h;
  pack_vec(c, x, x + (size_t)c->dim * c->nv, h, nullptr);
  CHK(upload_vec(c, h, c->xt.p));
  CHK(k_spmv_full(c, c->xt.p, c->dvec.p));
  std::vector<double> o;
  CHK(download_vec(c, c->dvec.p, o));
  for (int k = 0; k < c->nvo; k++) {
    const int v = c->iperm[k], d = c->dim;
    for (int i = 0; i < d; i++) y[(size_t)d * v + i] = o[(size_t)d * k + i];
    y[(size_t)d * c->nvo + v] = o[(size_t)d * c->nvo + k];
  }
  return 0;
}

int cfdh_set_global_pressure_space(cfdh_ctx *c, int64_t nvg, int64_t ncg, const int32_t *cells, const double *coords,
                                   const int32_t *owned_global, int64_t n_pbc, const int32_t *pbc_nodes) {
  NOT_IPCS(c, "cfdh_set_global_pressure_space");
  ENTER(c);
  if (nvg <= 0 || ncg <= 0 || !cells || !coords || !owned_global || (n_pbc > 0 && !pbc_nodes))
    return cfdh_fail(c, CFDH_E_ARG, "bad global pressure space arguments");
  const int n = (int)nvg;
  const int D = c->dim, NLc = D + 1;  // vertex records of the halo vectors: D + 1 doubles
  const int NCc = c->gen ? c->nloc : D + 1;  // global cells [ncg][nodes per cell], coords [nvg][D]
  for (int64_t k = 0; k < (int64_t)NCc * ncg; k++) if (cells[k] < 0 || cells[k] >= n) return cfdh_fail(c, CFDH_E_ARG, "global cell vertex out of range");
  std::vector<unsigned char> pbc(n, 0);
  for (int64_t k = 0; k < n_pbc; k++) {
    if (pbc_nodes[k] < 0 || pbc_nodes[k] >= n) return cfdh_fail(c, CFDH_E_ARG, "global Dirichlet node out of range");
    pbc[pbc_nodes[k]] = 1;
  }
  // global P1 stiffness as (row, col, value) triplets -> CSR with Dirichlet rows/cols removed
  std::vector<std::vector<std::pair<int, double>>> rows(n);
  if (c->gen) {  // P2 / Q1: the element's own stiffness by quadrature (csrc/cfdh_gen.hip), as h_Lval holds it for the local part
    std::vector<double> K((size_t)NCc * NCc);
    for (int64_t e = 0; e < ncg; e++) {
      const int32_t *v = cells + (size_t)NCc * e;
      CHK(D == 3 ? cfdh_gen3_element_stiffness(c, v, coords, K.data()) : cfdh_gen_element_stiffness(c, v, coords, K.data()));
      for (int a = 0; a < NCc; a++) {
        if (pbc[v[a]]) continue;
        for (int b = 0; b < NCc; b++) if (!pbc[v[b]]) rows[v[a]].push_back({v[b], K[(size_t)a * NCc + b]});
      }
    }
  }
  for (int64_t e = 0; e < ncg && D == 3 && !c->gen; e++) {
    // tetrahedra: rows of the inverse of [x1-x0 | x2-x0 | x3-x0] are grad lambda_1..3, volume |det| / 6
    const int32_t *v = cells + 4 * e;
    double d[3][3], cr[3][3], g[4][3];
    for (int a = 0; a < 3; a++)
      for (int i = 0; i < 3; i++) d[a][i] = coords[3 * (size_t)v[a + 1] + i] - coords[3 * (size_t)v[0] + i];
    for (int a = 0; a < 3; a++) {
      const double *p = d[(a + 1) % 3], *q = d[(a + 2) % 3];
      cr[a][0] = p[1] * q[2] - p[2] * q[1]; cr[a][1] = p[2] * q[0] - p[0] * q[2]; cr[a][2] = p[0] * q[1] - p[1] * q[0];
    }
    const double det = d[0][0] * cr[0][0] + d[0][1] * cr[0][1] + d[0][2] * cr[0][2], vol = std::fabs(det) / 6.0;
    if (!(vol > 0)) return cfdh_fail(c, CFDH_E_ARG, "zero-volume global cell");
    for (int a = 0; a < 3; a++)
      for (int i = 0; i < 3; i++) g[a + 1][i] = cr[a][i] / det;
    for (int i = 0; i < 3; i++) g[0][i] = -(g[1][i] + g[2][i] + g[3][i]);
    for (int a = 0; a < 4; a++) {
      if (pbc[v[a]]) continue;
      for (int b = 0; b < 4; b++) {
        if (pbc[v[b]]) continue;
        rows[v[a]].push_back({v[b], vol * (g[a][0] * g[b][0] + g[a][1] * g[b][1] + g[a][2] * g[b][2])});
      }
    }
  }
  for (int64_t e = 0; e < ncg && D == 2 && !c->gen; e++) {
    const int32_t *v = cells + 3 * e;
    const double x0 = coords[2 * v[0]], y0 = coords[2 * v[0] + 1], x1 = coords[2 * v[1]], y1 = coords[2 * v[1] + 1],
                 x2 = coords[2 * v[2]], y2 = coords[2 * v[2] + 1];
    const double det = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0), area = 0.5 * std::fabs(det);
    if (!(area > 0)) return cfdh_fail(c, CFDH_E_ARG, "zero-area global cell");
    const double g[3][2] = {{(y1 - y2) / det, (x2 - x1) / det}, {(y2 - y0) / det, (x0 - x2) / det}, {(y0 - y1) / det, (x1 - x0) / det}};
    for (int a = 0; a < 3; a++) {
      if (pbc[v[a]]) continue;
      for (int b = 0; b < 3; b++) {
        if (pbc[v[b]]) continue;
        rows[v[a]].push_back({v[b], area * (g[a][0] * g[b][0] + g[a][1] * g[b][1])});
      }
    }
  }
  CsrHost &L = c->gp_L;
  L.n = L.m = n; L.rowptr.assign(n + 1, 0); L.col.clear(); L.val.clear();
  for (int i = 0; i < n; i++) {
    if (pbc[i]) { L.col.push_back(i); L.val.push_back(1.0); }
    else {
      auto &r = rows[i];
      std::sort(r.begin(), r.end());
      for (size_t k = 0; k < r.size(); k++) {
        if (k > 0 && r[k].first == r[k - 1].first) L.val.back() += r[k].second;
        else { L.col.push_back(r[k].first); L.val.push_back(r[k].second); }
      }
    }
    L.rowptr[i + 1] = (int)L.col.size();
  }
  c->gp_singular = (n_pbc == 0);
  std::vector<int> l2g(c->nvo);
  for (int k = 0; k < c->nvo; k++) {
    const int g = owned_global[c->iperm[k]];
    if (g < 0 || g >= n) return cfdh_fail(c, CFDH_E_ARG, "owned_global out of range");
    l2g[k] = g;
  }
  HIPCHK(c, c->gp_l2g.upload(l2g, c->stream));
  HIPCHK(c, c->gp_rhs.alloc(n)); HIPCHK(c, c->gp_sol.alloc(n));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  // global ids of all local vertices (ghost ids through one halo exchange) and the inverse map: the overlapping
  // velocity preconditioner matches the matrix rows it receives from the owners of its ghosts by global id
  c->h_gid.clear(); c->h_g2l.clear();
  c->rasp.ready = false;
  if (c->nranks > 1 && c->ng > 0 && c->nnbr > 0) {
    std::vector<double> hv((size_t)c->NL, -1.0);
    for (int k = 0; k < c->nvo; k++) hv[(size_t)D * k] = (double)l2g[k];  // first velocity slot of the vertex record
    if (!c->pcw.p) HIPCHK(c, c->pcw.alloc(c->NL));
    HIPCHK(c, c->pcw.upload(hv, c->stream));
    CHK(comm_halo(c, c->pcw.p));
    HIPCHK(c, hipMemcpyAsync(hv.data(), c->pcw.p, sizeof(double) * hv.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, c->pcw.zero(c->stream));
    c->h_gid.assign(c->nv, -1);
    c->h_g2l.assign(n, -1);
    bool ok = true;
    for (int k = 0; k < c->nvo; k++) c->h_gid[k] = l2g[k];
    for (int i = 0; i < c->ng; i++) {
      const double gd = hv[(size_t)NLc * c->nvo + (size_t)NLc * i];
      if (!(gd >= 0 && gd < n)) { ok = false; break; }
      c->h_gid[c->nvo + i] = (int)gd;
    }
    if (ok) for (int k = 0; k < c->nv; k++) c->h_g2l[c->h_gid[k]] = k;
    else { c->h_gid.clear(); c->h_g2l.clear(); }
  }
  c->gp_allgather = false;
  if (c->nranks > 1 && c->nccl_comm) {
    // gather plan.  One all-reduce of an owner map (rank+1 at the owned global ids) tells every rank who owns
    // what; parts send their owned values in ascending global-id order, so the position of global vertex g in
    // the gathered buffer follows from the map alone.
    std::vector<double> own(n, 0.0);
    for (int k = 0; k < c->nvo; k++) own[l2g[k]] = (double)(c->rank + 1);
    HIPCHK(c, c->gp_rhs.upload(own, c->stream));
    CHK(comm_allreduce_dev(c, c->gp_rhs.p, n, 0));
    HIPCHK(c, hipMemcpyAsync(own.data(), c->gp_rhs.p, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<int> cnt(c->nranks, 0), src(n);
    for (int g = 0; g < n; g++) {
      const int r = (int)own[g] - 1;
      if (own[g] != (double)(r + 1) || r < 0 || r >= c->nranks)
        return cfdh_fail(c, CFDH_E_ARG, "global vertex %d is owned by %g parts (expected exactly one)", g, own[g]);
      cnt[r]++;
    }
    int maxcnt = 0;
    for (int r = 0; r < c->nranks; r++) maxcnt = std::max(maxcnt, cnt[r]);
    if (cnt[c->rank] != c->nvo) return cfdh_fail(c, CFDH_E_STATE, "owner map disagrees with nv_owned");
    std::fill(cnt.begin(), cnt.end(), 0);
    for (int g = 0; g < n; g++) { const int r = (int)own[g] - 1; src[g] = r * maxcnt + cnt[r]++; }
    std::vector<std::pair<int, int>> byg(c->nvo);
    for (int k = 0; k < c->nvo; k++) byg[k] = {l2g[k], k};
    std::sort(byg.begin(), byg.end());
    std::vector<int> sidx(c->nvo);
    for (int k = 0; k < c->nvo; k++) sidx[k] = byg[k].second;
    HIPCHK(c, c->gp_send_idx.upload(sidx, c->stream));
    HIPCHK(c, c->gp_src_idx.upload(src, c->stream));
    HIPCHK(c, c->gp_sendbuf.alloc((size_t)maxcnt)); HIPCHK(c, c->gp_recvbuf.alloc((size_t)maxcnt * c->nranks));
    HIPCHK(c, c->gp_sendbuf.zero(c->stream));  // the padding beyond nv_owned stays zero
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->gp_maxcnt = maxcnt;
    // known-answer pass through the gather: every rank sends the global ids of its owned vertices and must find
    // g at position g afterwards; otherwise the all-reduce of the padded vector stays in charge
    {
      std::vector<double> ids((size_t)maxcnt, 0.0), back(n);
      for (int k = 0; k < c->nvo; k++) ids[k] = (double)byg[k].first;
      HIPCHK(c, c->gp_sendbuf.upload(ids, c->stream));
      CHK(comm_allgather_dev(c, c->gp_sendbuf.p, c->gp_recvbuf.p, maxcnt));
      CHK(k_gather_global(c, n, c->gp_src_idx.p, c->gp_recvbuf.p, c->gp_rhs.p));
      HIPCHK(c, hipMemcpyAsync(back.data(), c->gp_rhs.p, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, c->gp_sendbuf.zero(c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      bool ok = true;
      for (int g = 0; g < n && ok; g++) ok = back[g] == (double)g;
      double bad = ok ? 0.0 : 1.0;  // every rank takes the same decision
      CHK(comm_allreduce_host(c, &bad, 1));
      c->gp_allgather = bad == 0.0;
      if (!c->gp_allgather && c->rank == 0)
        fprintf(stderr, "[cfdh] WARNING: all-gather self-check failed; the pressure right-hand side is all-reduced instead\n");
    }
  }
  c->gp_n = n;
  c->gp_dirty = true;
  c->pc_valid = false;
  return 0;
}

int cfdh_solve_step(cfdh_ctx *c, cfdh_stats *stats) {
  NOT_IPCS(c, "cfdh_solve_step");
  ENTER(c);
  cfdh_stats st;
  c->err.clear();
  int rc = cfdh_newton_step(c, &st);
  if (stats) *stats = st;
  return rc;
}

int cfdh_functional(cfdh_ctx *c, int kind, int marker, double *out) {
  if (!out) return CFDH_E_ARG;
  ENTER(c);
  if (c->ipcs) return cfdh_ipcs_functional(c, kind, marker, out);
  return k_functional(c, kind, marker, out);
}

int cfdh_wall_shear_stress(cfdh_ctx *c, double *shear) {
  ENTER(c);
  if (c->ipcs) {  // P2 velocity, CG1 field on the vertices (caller's numbering); entries away from the wall stay zero
    IpcsData *I = c->ipcs;
    if (!c->params_set) return cfdh_fail(c, CFDH_E_STATE, "cfdh_set_params was not called");
    const size_t n = (size_t)I->D * (size_t)I->nvert;
    if (!c->wss.p) { HIPCHK(c, c->wss.alloc(n)); HIPCHK(c, c->wss.zero(c->stream)); }
    CHK(k_ipcs_wss(c, c->wss.p));
    if (!shear) return 0;
    I->n_field_copies++;
    HIPCHK(c, hipMemcpyAsync(shear, c->wss.p, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
  }
  const size_t d = (size_t)c->dim;
  if (!c->wss.p) HIPCHK(c, c->wss.alloc(d * (size_t)c->nv));
  CHK(comm_halo(c, c->x.p));
  CHK(k_wss(c, c->wss.p));
  if (!shear) return 0;
  std::vector<double> h(d * (size_t)c->nv);
  HIPCHK(c, hipMemcpyAsync(h.data(), c->wss.p, sizeof(double) * h.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int k = 0; k < c->nv; k++) {
    const int v = c->iperm[k];
    for (size_t i = 0; i < d; i++) shear[d * (size_t)v + i] = h[d * (size_t)k + i];
  }
  return 0;
}

// ---- cycle-averaged wall shear indices (kernels: cfdh_wallstats.hip) ------------------------------------------------------
static inline size_t ws_nv(const cfdh_ctx *c) { return c->ipcs ? (size_t)c->ipcs->nvert : (size_t)c->nv; }  // vertices of the WSS field

int cfdh_wall_stats_reset(cfdh_ctx *c) {
  ENTER(c);
  const size_t d = (size_t)c->dim, n = ws_nv(c);
  HIPCHK(c, c->ws_S.alloc(d * n)); HIPCHK(c, c->ws_A.alloc(n)); HIPCHK(c, c->ws_M.alloc(n)); HIPCHK(c, c->ws_out.alloc(d * n));
  HIPCHK(c, c->ws_S.zero(c->stream)); HIPCHK(c, c->ws_A.zero(c->stream)); HIPCHK(c, c->ws_M.zero(c->stream));
  c->ws_W = 0.0;
  c->ws_count = 0;
  c->ws_ready = true;
  return 0;
}

int cfdh_wall_stats_accumulate(cfdh_ctx *c, double weight) {
  ENTER(c);
  if (!std::isfinite(weight) || !(weight > 0.0)) return cfdh_fail(c, CFDH_E_ARG, "cfdh_wall_stats_accumulate: the weight must be finite and > 0");
  if (!c->ws_ready) return cfdh_fail(c, CFDH_E_STATE, "cfdh_wall_stats_accumulate: cfdh_wall_stats_reset was not called");
  CHK(cfdh_wall_shear_stress(c, nullptr));  // always recomputed: facet work only
  CHK(k_ws_accumulate(c, (int)ws_nv(c), weight, c->wss.p));
  c->ws_W += weight;
  c->ws_count++;
  return 0;
}

int cfdh_wall_stats_get(cfdh_ctx *c, int which, int64_t *n, double *out) {
  ENTER(c);
  if (!n) return cfdh_fail(c, CFDH_E_ARG, "cfdh_wall_stats_get: null count pointer");
  if (which < 0 || which > 5) return cfdh_fail(c, CFDH_E_ARG, "cfdh_wall_stats_get: which in [0, 5]");
  if (!c->ws_ready) return cfdh_fail(c, CFDH_E_STATE, "cfdh_wall_stats_get: cfdh_wall_stats_reset was not called");
  if (which == 5) {
    *n = 2;
    if (out) { out[0] = c->ws_W; out[1] = (double)c->ws_count; }
    return 0;
  }
  if (!(c->ws_W > 0.0)) return cfdh_fail(c, CFDH_E_STATE, "cfdh_wall_stats_get: nothing accumulated since the last reset");
  const size_t nv = ws_nv(c), d = which == 3 ? (size_t)c->dim : 1;
  *n = (int64_t)(d * nv);
  if (!out) return 0;
  CHK(k_ws_derive(c, (int)nv, which, c->ws_out.p));
  if (c->ipcs) {
    HIPCHK(c, hipMemcpyAsync(out, c->ws_out.p, sizeof(double) * d * nv, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
  }
  std::vector<double> h(d * nv);
  HIPCHK(c, hipMemcpyAsync(h.data(), c->ws_out.p, sizeof(double) * h.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (size_t k = 0; k < nv; k++) {
    const size_t v = (size_t)c->iperm[k];
    for (size_t i = 0; i < d; i++) out[d * v + i] = h[d * k + i];
  }
  return 0;
}

int cfdh_profile_enable(cfdh_ctx *c, int on) {
  NOT_IPCS(c, "cfdh_profile_enable");
  ENTER(c);
  prof_flush(c);
  c->prof_on = on != 0;
  if (c->prof_on) {
    // calibration: the elapsed time of an EMPTY event pair on this stream (kind 7).  Every measured launch
    // carries this much in excess of the kernel's own duration; callers may subtract the average.
    for (int i = 0; i < 256; i++) { prof_begin(c, 7); prof_end(c, 7); }
    prof_flush(c);
  }
  return 0;
}
int cfdh_profile_get(cfdh_ctx *c, int kind, double *total_ms, int64_t *launches) {
  NOT_IPCS(c, "cfdh_profile_get");
  if (!c || kind < 0 || kind >= 12) return CFDH_E_ARG;
  prof_flush(c);
  if (total_ms) *total_ms = c->prof[kind].total_ms;
  if (launches) *launches = c->prof[kind].launches;
  return 0;
}
int cfdh_profile_reset(cfdh_ctx *c) {
  NOT_IPCS(c, "cfdh_profile_reset");
  ENTER(c);
  prof_flush(c);
  for (auto &p : c->prof) { p.total_ms = 0; p.launches = 0; }
  c->n_allreduce = c->n_halo = c->n_host_sync = c->n_krylov = c->n_allgather = 0;
  c->n_cycles = c->n_guess_projections = c->n_iter_sync = 0;
  c->n_krylov_discarded = 0;
  return 0;
}

int64_t cfdh_info(const cfdh_ctx *c, int what) {
  if (!c) return -1;
  if (c->ipcs) {
    const IpcsData *I = c->ipcs;
    switch (what) {
      case 0: case 1: return I->nn;
      case 2: return I->nc;
      case 3: return (int64_t)I->op.col2.size();
      case 6: return (int64_t)I->hLam.lev.size();
      case 15: return I->last.host_syncs;
      case 18: return 1;
      case 26: return I->D;
      case 29: return I->NL;
      case 80: return I->last.launches;
      case 81: return I->nvert;
      case 82: return I->n_field_copies;
      case 83: return 1;
      case 84: case 90: return c->ws_count;  // accumulations of the wall shear indices since the last reset
      case 91: return I->scheme;
      case 92: return I->n_assemblies;
      case 106: case 107: case 108: case 109: case 110: return 0;  // flow diagnostics: refused on this kind of context
      case 111: case 112: case 113: case 114: case 115: case 116: case 117: case 118: case 119: return 0;  // point sampler: the same
      case 120: case 121: case 122: case 123: case 124: case 125: return 0;  // cut-plane sections: the same
      default: return -1;
    }
  }
  switch (what) {
    case 0: return c->nvo;
    case 1: return c->nv;
    case 2: return c->nc;
    case 3: return c->nnzv;
    case 4: return c->opt.pc_type >= 1 ? c->hL.fine_nnz : c->hS.fine_nnz;
    case 5: return c->ninc;
    case 6: return (int64_t)(c->opt.pc_type >= 1 ? c->hL.lev.size() : c->hS.lev.size());
    case 7: return c->nblk;
    case 8: return c->hA.fine_nnz;
    case 9: return c->gp_allgather ? c->gp_maxcnt : 0;
    case 10: return c->nccl_comm ? 1 : 0;
    case 11: return c->dl0.on ? c->dl0.n1 : 0;
    case 12: return c->ras ? 1 : 0;
    case 13: return c->n_allreduce;
    case 14: return c->n_halo;
    case 15: return c->n_host_sync;
    case 16: return c->n_krylov;
    case 17: return c->n_allgather;
    case 18: return c->nranks;
    case 26: return c->dim;
    case 30: case 31: case 32: case 33: case 34: case 35: case 36: case 37: case 38: case 39:
    case 40: case 41: case 42: case 43: case 44: case 45: case 46: case 47: case 48: case 49:
    case 50: case 51: case 52: case 53: case 54: case 55: case 56: case 57: case 58: case 59:
    case 60: case 61: case 62: case 63: case 64: case 65: case 66: case 67: case 68: case 69: {
      const AmgHier &h = what < 50 ? c->hA : (c->opt.pc_type >= 1 ? c->hL : c->hS);
      const size_t l = (size_t)(what % 10);
      if (l >= h.lev.size()) return 0;
      return ((what / 10) & 1) ? (int64_t)h.lev[l]->n : (int64_t)h.lev[l]->A.nnz;
    }
    case 28: return c->etype;
    case 70: return c->n_guess_solves;  // linear solves started from a projected guess (cfdh_options.ksp_guess)
    case 71: return c->n_guess_solves ? (int64_t)(1e6 * c->guess_reduction_sum / (double)c->n_guess_solves) : 0;  // mean |r0| / |b| of those, in 1e-6
    case 29: return c->nloc;
    case 73: return c->n_krylov_discarded;  // FGMRES iterations launched ahead of the host's convergence test and discarded (not in krylov_its)
    case 74: return c->n_pc_builds;
    case 84: return c->n_cycles;      // FGMRES cycles whose true residual was read back (reset with 13..17)
    case 86: return c->n_guess_projections;  // linear solves whose prologue projected a guess, used or not (reset with 13..17)
    case 87: return c->n_iter_sync;   // host synchronisations inside the FGMRES cycles (batches of iterations, re-orthogonalisations; reset with 13..17)
    case 88: return c->guess_last_rank;  // rank the pivoted Cholesky found in the last Gram system of a projected guess (-1: none yet)
    case 89: return c->guess_last_k;     // ... and the number of kept vectors it had
    case 85: return c->lean ? 1 : 0;  // lean solve path switched on (CFDH_SOLVE_LEAN)
    case 90: return c->ws_count;      // accumulations of the wall shear indices since the last cfdh_wall_stats_reset
    case 75: return c->pc_valid ? 1 : 0;
    case 76: return c->singular;
    case 77: return c->form;
    case 78: return c->opt.pc_type;   // Schur approximation in use: 0 SELFP, 1 Cahouet-Chabard, 2 PCD
    case 79: return c->ew_version;    // Eisenstat-Walker forcing version (0: off)
    case 93: return (int64_t)c->tb_markers.size();  // traction boundaries set (cfdh_set_traction_boundaries)
    case 94: return c->n_traction_launches;          // launches of the traction kernel since cfdh_create
    case 95: return c->sc ? 1 : 0;                   // passive scalar enabled (cfdh_scalar_enable)
    case 96: return c->n_scalar_steps;               // scalar steps taken
    case 97: return c->n_scalar_asm;                 // launches of the scalar assembly kernel since cfdh_create
    case 98: return c->blk_vl_max;                   // P1 triangle assembly: longest / shortest per-block vertex list ...
    case 99: return c->blk_vl_min;
    case 100: return c->blk_cl_max;                  // ... and cell list (0 on contexts that do not build them)
    case 101: return c->blk_cl_min;
    case 102: return c->env.asm_stage ? 1 : 0;       // fixed-stride lists in use (CFDH_ASM_STAGE as this context read it)
    case 103: return c->pt ? 1 : 0;                  // particles enabled (cfdh_particles_enable)
    case 104: return c->n_particle_steps;            // particle steps taken
    case 105: return c->n_particle_launches;         // launches of the advection kernel since cfdh_create
    case 106: case 107: case 108: case 109: case 110: return cfdh_flow_info(c, what);  // flow diagnostics: buffers exist, cell passes, accumulations since the reset, ns of the last kernels
    case 111: case 112: case 113: case 114: case 115: case 116: case 117: case 118: case 119: return cfdh_sample_info(c, what);  // point sampler: points, located, sample launches, waiting row blocks, ns of the last locate / sample kernel, the bin grid
    case 120: case 121: case 122: case 123: case 124: case 125: return cfdh_section_info(c, what);  // cut-plane sections: sections, entries, longest list, evaluations, waiting row blocks, ns of the last evaluation
    case 72: return c->n_attainable_stops;  // solves stopped at the attainable accuracy (reason CFDH_KSP_CONVERGED_ATTAINABLE), above their tolerance
    case 27: return (int64_t)(1000.0 * c->ms_pc_build_dev);  // microseconds of the last device-side preconditioner build (0: host build)
    case 19: return c->opt.pc_type >= 1 ? c->hL.nnz_S0 : c->hS.nnz_S0;
    case 20: return c->hA.nnz_S0;
    case 21: return c->opt.pc_type >= 1 ? c->hL.nnz_G0 : c->hS.nnz_G0;
    case 22: return c->hA.nnz_G0;
    case 23: { const AmgHier &h = c->opt.pc_type >= 1 ? c->hL : c->hS; return h.lev.size() > 1 ? h.lev[1]->n : 0; }
    case 24: return c->hA.lev.size() > 1 ? c->hA.lev[1]->n : 0;
    case 25: { const AmgHier &h = c->opt.pc_type >= 1 ? c->hL : c->hS; return h.fused ? 1 : 0; }
    default: return -1;
  }
}

// ---- volumetric flow diagnostics (cfdh_flow.hip) -------------------------------------------------------------------------------

int cfdh_flow_field(cfdh_ctx *c, int which, int64_t *n, double *out) {
  ENTER(c);
  return cfdh_flow_field_impl(c, which, n, out);
}

int cfdh_flow_integrals(cfdh_ctx *c, double *out) {
  ENTER(c);
  return cfdh_flow_integrals_impl(c, out);
}

int cfdh_flow_stats_reset(cfdh_ctx *c) {
  ENTER(c);
  return cfdh_flow_stats_reset_impl(c);
}

int cfdh_flow_stats_accumulate(cfdh_ctx *c, double weight) {
  ENTER(c);
  return cfdh_flow_stats_accumulate_impl(c, weight);
}

int cfdh_flow_stats_get(cfdh_ctx *c, int which, int64_t *n, double *out) {
  ENTER(c);
  return cfdh_flow_stats_get_impl(c, which, n, out);
}

// ---- point sampler (cfdh_sample.hip) -------------------------------------------------------------------------------------------

int cfdh_sample_set_points(cfdh_ctx *c, int64_t n, const double *x, double tol) {
  ENTER(c);
  return cfdh_sample_set_points_impl(c, n, x, tol);
}

int cfdh_sample_set_grid(cfdh_ctx *c, const double *origin, const double *spacing, const int64_t *dims, double tol) {
  ENTER(c);
  return cfdh_sample_set_grid_impl(c, origin, spacing, dims, tol);
}

int cfdh_sample_get_location(cfdh_ctx *c, int64_t *n, int32_t *cell, double *lambda, double *x) {
  ENTER(c);
  return cfdh_sample_get_location_impl(c, n, cell, lambda, x);
}

int cfdh_sample_now(cfdh_ctx *c, int64_t *n, double *out) {
  ENTER(c);
  return cfdh_sample_now_impl(c, n, out);
}

int cfdh_sample_series_enable(cfdh_ctx *c, int64_t rows) {
  ENTER(c);
  return cfdh_sample_series_enable_impl(c, rows);
}

int cfdh_sample_record(cfdh_ctx *c, double t) {
  ENTER(c);
  return cfdh_sample_record_impl(c, t);
}

int cfdh_sample_series_get(cfdh_ctx *c, int64_t *rows, double *t, double *out) {
  ENTER(c);
  return cfdh_sample_series_get_impl(c, rows, t, out);
}

int cfdh_sample_mean_reset(cfdh_ctx *c) {
  ENTER(c);
  return cfdh_sample_mean_reset_impl(c);
}

int cfdh_sample_mean_accumulate(cfdh_ctx *c, double weight) {
  ENTER(c);
  return cfdh_sample_mean_accumulate_impl(c, weight);
}

int cfdh_sample_mean_get(cfdh_ctx *c, int which, int64_t *n, double *out) {
  ENTER(c);
  return cfdh_sample_mean_get_impl(c, which, n, out);
}

// ---- cut-plane sections (cfdh_section.hip) ----------------------------------------------------------------------------------------

int cfdh_section_set(cfdh_ctx *c, int32_t K, const double *origin, const double *normal, const double *radius) {
  ENTER(c);
  return cfdh_section_set_impl(c, K, origin, normal, radius);
}

int cfdh_section_get_cut(cfdh_ctx *c, int32_t *K, int64_t *ptr, int32_t *cell, double *measure, int32_t *straddling) {
  ENTER(c);
  return cfdh_section_get_cut_impl(c, K, ptr, cell, measure, straddling);
}

int cfdh_section_now(cfdh_ctx *c, int32_t *K, double *out) {
  ENTER(c);
  return cfdh_section_now_impl(c, K, out);
}

int cfdh_section_series_enable(cfdh_ctx *c, int64_t rows) {
  ENTER(c);
  return cfdh_section_series_enable_impl(c, rows);
}

int cfdh_section_record(cfdh_ctx *c, double t) {
  ENTER(c);
  return cfdh_section_record_impl(c, t);
}

int cfdh_section_series_get(cfdh_ctx *c, int64_t *rows, double *t, double *out) {
  ENTER(c);
  return cfdh_section_series_get_impl(c, rows, t, out);
}

int cfdh_section_mean_reset(cfdh_ctx *c) {
  ENTER(c);
  return cfdh_section_mean_reset_impl(c);
}

int cfdh_section_mean_accumulate(cfdh_ctx *c, double weight) {
  ENTER(c);
  return cfdh_section_mean_accumulate_impl(c, weight);
}

int cfdh_section_mean_get(cfdh_ctx *c, int32_t *K, double *out, double *w_count) {
  ENTER(c);
  return cfdh_section_mean_get_impl(c, K, out, w_count);
}

// ---- Lagrangian particle tracking (cfdh_particles.hip) ------------------------------------------------------------------------

int cfdh_particles_enable(cfdh_ctx *c, int64_t capacity, int32_t nsub) {
  ENTER(c);
  return cfdh_particles_enable_impl(c, capacity, nsub);
}

int cfdh_particles_seed(cfdh_ctx *c, int64_t n, const double *x, const int32_t *cell, double t_birth) {
  ENTER(c);
  return cfdh_particles_seed_impl(c, n, x, cell, t_birth);
}

int cfdh_particles_clear(cfdh_ctx *c) {
  ENTER(c);
  return cfdh_particles_clear_impl(c);
}

int cfdh_particles_step(cfdh_ctx *c, double t0, cfdh_particle_stats *stats) {
  ENTER(c);
  return cfdh_particles_step_impl(c, t0, stats);
}

int cfdh_particles_get(cfdh_ctx *c, int which, int64_t *n, void *out) {
  ENTER(c);
  return cfdh_particles_get_impl(c, which, n, out);
}

// ---- passive scalar transport (cfdh_scalar.hip) --------------------------------------------------------------------------------

int cfdh_scalar_enable(cfdh_ctx *c, double D, double s, double theta_c) {
  ENTER(c);
  return cfdh_scalar_enable_impl(c, D, s, theta_c);
}

int cfdh_scalar_set_dirichlet(cfdh_ctx *c, int64_t n, const int32_t *nodes, const double *values) {
  ENTER(c);
  return cfdh_scalar_set_dirichlet_impl(c, n, nodes, values);
}

int cfdh_scalar_set_state(cfdh_ctx *c, const double *cc) {
  ENTER(c);
  if (!cc) return cfdh_fail(c, CFDH_E_ARG, "cfdh_scalar_set_state: null array");
  return cfdh_scalar_state_impl(c, cc, nullptr);
}

int cfdh_scalar_get_state(cfdh_ctx *c, double *cc) {
  ENTER(c);
  if (!cc) return cfdh_fail(c, CFDH_E_ARG, "cfdh_scalar_get_state: null array");
  return cfdh_scalar_state_impl(c, nullptr, cc);
}

int cfdh_scalar_set_tolerances(cfdh_ctx *c, double rtol, double atol, int32_t max_it) {
  ENTER(c);
  return cfdh_scalar_set_tolerances_impl(c, rtol, atol, max_it);
}

int cfdh_scalar_step(cfdh_ctx *c, cfdh_scalar_stats *stats) {
  ENTER(c);
  c->err.clear();
  return cfdh_scalar_step_impl(c, stats);
}

int cfdh_scalar_get_operator(cfdh_ctx *c, int64_t *nnz, int32_t *rowptr, int32_t *col, double *vals, double *rhs) {
  if (!c || !nnz) return CFDH_E_ARG;
  ENTER(c);
  return cfdh_scalar_get_operator_impl(c, nnz, rowptr, col, vals, rhs);
}

int cfdh_scalar_functional(cfdh_ctx *c, int kind, int marker, double *out) {
  if (!out) return CFDH_E_ARG;
  ENTER(c);
  return cfdh_scalar_functional_impl(c, kind, marker, out);
}

int cfdh_scalar_krylov_solve(cfdh_ctx *c, const double *b, const double *x0, double rtol, double atol, int max_it, double *x,
                             cfdh_scalar_stats *stats, double *scalars, double *p) {
  ENTER(c);
  if (!b || !x0 || !x || !stats) return cfdh_fail(c, CFDH_E_ARG, "cfdh_scalar_krylov_solve: null array");
  if (!(rtol >= 0) || !(rtol < 1) || !(atol >= 0) || max_it < 1)
    return cfdh_fail(c, CFDH_E_ARG, "cfdh_scalar_krylov_solve: 0 <= rtol < 1, atol >= 0, max_it >= 1");
  c->err.clear();
  return cfdh_scalar_krylov_solve_impl(c, b, x0, rtol, atol, max_it, x, stats, scalars, p);
}

int cfdh_scalar_get_order(cfdh_ctx *c, int32_t *row) {
  if (!row) return CFDH_E_ARG;
  ENTER(c);
  return cfdh_scalar_get_order_impl(c, row);
}

// ---- incremental pressure correction (cfdh_ipcs.hip, cfdh_ipcs_krylov.hip, cfdh_ipcs_setup.cpp) ----------------------------------------------------------------------

int cfdh_create_ipcs(cfdh_ctx **out, int device, int gdim, int64_t nn, int64_t nvert, int64_t nc, const int32_t *cells, const double *node_coords,
                     int64_t nfacets, const int32_t *facet_cells, const int32_t *facet_local, const int32_t *facet_marker) {
  if (!out) return cfdh_fail(nullptr, CFDH_E_ARG, "null output pointer");
  *out = nullptr;
  if (gdim != 2 && gdim != 3) return cfdh_fail(nullptr, CFDH_E_ARG, "gdim must be 2 (P2/P1 triangles) or 3 (P2/P1 tetrahedra)");
  if (!cells || !node_coords || nfacets < 0 || (nfacets > 0 && (!facet_cells || !facet_local))) return cfdh_fail(nullptr, CFDH_E_ARG, "null mesh array");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return cfdh_fail(nullptr, CFDH_E_HIP, "no HIP device available: libcfdh has no CPU fallback");
  if (device < 0 || device >= ndev) return cfdh_fail(nullptr, CFDH_E_ARG, "device %d out of range (%d devices)", device, ndev);
  cfdh_ctx *c = new (std::nothrow) cfdh_ctx();
  if (!c) return cfdh_fail(nullptr, CFDH_E_NOMEM, "out of host memory");
  c->device = device;
  cfdh_default_options(&c->opt);
  c->use_graph = false;  // plain stream order
  memset(&c->last_stats, 0, sizeof c->last_stats);
  int rc = 0;
  if (hipSetDevice(device) != hipSuccess) rc = cfdh_fail(nullptr, CFDH_E_HIP, "hipSetDevice(%d) failed", device);
  else if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) rc = cfdh_fail(nullptr, CFDH_E_HIP, "hipStreamCreate failed");
  else rc = cfdh_ipcs_create(c, gdim, nn, nvert, nc, cells, node_coords, nfacets, facet_cells, facet_local, facet_marker);
  if (rc) {
    g_cfdh_last_error = c->err.empty() ? g_cfdh_last_error : c->err;
    cfdh_destroy(c);
    return rc;
  }
  *out = c;
  return 0;
}

int cfdh_ipcs_set_form(cfdh_ctx *c, double conv_coeff, double force_coeff) {
  NEED_IPCS(c, "cfdh_ipcs_set_form");
  if (!(conv_coeff >= 0) || !std::isfinite(conv_coeff) || !std::isfinite(force_coeff)) return cfdh_fail(c, CFDH_E_ARG, "cfdh_ipcs_set_form: conv_coeff >= 0 and finite coefficients");
  c->ipcs->conv_coeff = conv_coeff; c->ipcs->force_coeff = force_coeff; c->ipcs->force_default = false;
  c->ipcs->assembled = false;
  return 0;
}

int cfdh_ipcs_set_tolerances(cfdh_ctx *c, const double rtol[3], double atol, const int32_t max_it[3]) {
  NEED_IPCS(c, "cfdh_ipcs_set_tolerances");
  if (!rtol || !max_it || !(atol >= 0)) return cfdh_fail(c, CFDH_E_ARG, "cfdh_ipcs_set_tolerances: bad arguments");
  for (int k = 0; k < 3; k++)
    if (!(rtol[k] >= 0) || !(rtol[k] < 1) || max_it[k] < 1) return cfdh_fail(c, CFDH_E_ARG, "cfdh_ipcs_set_tolerances: 0 <= rtol < 1, max_it >= 1");
  for (int k = 0; k < 3; k++) { c->ipcs->rtol[k] = rtol[k]; c->ipcs->max_it[k] = max_it[k]; }
  c->ipcs->atol = atol;
  return 0;
}

int cfdh_ipcs_step(cfdh_ctx *c, cfdh_ipcs_stats *stats) {
  NEED_IPCS(c, "cfdh_ipcs_step");
  c->err.clear();
  cfdh_ipcs_stats st;
  const int rc = cfdh_ipcs_step_impl(c, &st);
  if (stats) *stats = st;
  return rc;
}

int cfdh_ipcs_get_operator(cfdh_ctx *c, int which, int64_t *nnz, int32_t *rowptr, int32_t *col, double *vals) {
  NEED_IPCS(c, "cfdh_ipcs_get_operator");
  IpcsData *I = c->ipcs;
  const int D = I->D;
  if (!nnz || which < 0 || which >= 3 + 2 * D) return cfdh_fail(c, CFDH_E_ARG, "cfdh_ipcs_get_operator: which in [0, %d)", 3 + 2 * D);
  if (which == 0 && I->scheme == CFDH_IPCS_MIDPOINT)
    return cfdh_fail(c, CFDH_E_STATE, "cfdh_ipcs_get_operator: A1 of the ipcs_midpoint scheme is a block matrix (cfdh_ipcs_get_block_operator)");
  const std::vector<int> &ptr = which == 1 ? I->op.ptr1 : which < 3 ? I->op.ptr2 : which < 3 + D ? I->op.bptr : I->op.gptr;
  const std::vector<int> &cl = which == 1 ? I->op.col1 : which < 3 ? I->op.col2 : which < 3 + D ? I->op.bcol : I->op.gcol;
  *nnz = (int64_t)cl.size();
  if (!rowptr && !col && !vals) return 0;
  if (!rowptr || !col || !vals) return cfdh_fail(c, CFDH_E_ARG, "pass all of rowptr/col/vals or none");
  std::copy(ptr.begin(), ptr.end(), rowptr);
  std::copy(cl.begin(), cl.end(), col);
  if (which >= 3) {
    const std::vector<double> &v = which < 3 + D ? I->op.B : I->op.G;
    const int d = which < 3 + D ? which - 3 : which - 3 - D;
    for (size_t k = 0; k < cl.size(); k++) vals[k] = v[(size_t)D * k + d];
    return 0;
  }
  if (which == 0) {
    if (!I->assembled) CHK(cfdh_ipcs_assemble(c));
  } else {
    if (!c->params_set) return cfdh_fail(c, CFDH_E_STATE, "cfdh_set_params was not called");
    I->assembled = false;
    CHK(cfdh_ipcs_assemble(c));  // brings L and rho M up to date with the Dirichlet data and rho
  }
  const double *src = which == 0 ? I->A1v.p : which == 1 ? I->Lv.p : I->RMv.p;
  HIPCHK(c, hipMemcpyAsync(vals, src, sizeof(double) * cl.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

int cfdh_ipcs_set_scheme(cfdh_ctx *c, int scheme) {
  NEED_IPCS(c, "cfdh_ipcs_set_scheme");
  if (scheme != CFDH_IPCS_BDF2 && scheme != CFDH_IPCS_MIDPOINT) return cfdh_fail(c, CFDH_E_ARG, "cfdh_ipcs_set_scheme: unknown scheme %d", scheme);
  return cfdh_ipcs_set_scheme_impl(c, scheme);
}

int cfdh_ipcs_get_block_operator(cfdh_ctx *c, int which, int64_t *nnz, int32_t *rowptr, int32_t *col, double *vals) {
  NEED_IPCS(c, "cfdh_ipcs_get_block_operator");
  IpcsData *I = c->ipcs;
  if (!nnz || which < 0 || which > 1) return cfdh_fail(c, CFDH_E_ARG, "cfdh_ipcs_get_block_operator: which in [0, 2)");
  if (I->scheme != CFDH_IPCS_MIDPOINT)
    return cfdh_fail(c, CFDH_E_STATE, "cfdh_ipcs_get_block_operator: the context runs the ipcs_bdf2 scheme (cfdh_ipcs_set_scheme)");
  *nnz = (int64_t)I->op.col2.size();
  if (!rowptr && !col && !vals) return 0;
  if (!rowptr || !col || !vals) return cfdh_fail(c, CFDH_E_ARG, "pass all of rowptr/col/vals or none");
  std::copy(I->op.ptr2.begin(), I->op.ptr2.end(), rowptr);
  std::copy(I->op.col2.begin(), I->op.col2.end(), col);
  if (!I->assembled) CHK(cfdh_ipcs_assemble(c));
  HIPCHK(c, hipMemcpyAsync(vals, which == 0 ? I->A1B.p : I->AfreeB.p, sizeof(double) * I->op.col2.size() * I->D * I->D, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

int cfdh_ipcs_get_intermediate(cfdh_ctx *c, int which, double *out) {
  NEED_IPCS(c, "cfdh_ipcs_get_intermediate");
  IpcsData *I = c->ipcs;
  if (!out || which < 0 || which > 6) return cfdh_fail(c, CFDH_E_ARG, "cfdh_ipcs_get_intermediate: which in [0, 6]");
  const dbuf<double> *src[7] = {&I->us, &I->phi, &I->b1, &I->b2, &I->b3, &I->kp, &I->pp};
  I->n_field_copies++;
  HIPCHK(c, hipMemcpyAsync(out, src[which]->p, sizeof(double) * src[which]->n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

int cfdh_ipcs_apply_pressure_pc(cfdh_ctx *c, const double *r, double *z) {
  NEED_IPCS(c, "cfdh_ipcs_apply_pressure_pc");
  if (!r || !z) return cfdh_fail(c, CFDH_E_ARG, "cfdh_ipcs_apply_pressure_pc: null array");
  return cfdh_ipcs_apply_pc(c, r, z);
}

int cfdh_ipcs_krylov_solve(cfdh_ctx *c, int which, const double *b, const double *x0, double rtol, double atol, int max_it, double *x,
                           cfdh_ipcs_stats *stats, double *scalars) {
  NEED_IPCS(c, "cfdh_ipcs_krylov_solve");
  if (!b || !x0 || !x || !stats) return cfdh_fail(c, CFDH_E_ARG, "cfdh_ipcs_krylov_solve: null array");
  if (which < 0 || which > 2) return cfdh_fail(c, CFDH_E_ARG, "cfdh_ipcs_krylov_solve: which = %d outside 0 .. 2", which);
  if (!(rtol >= 0) || !(rtol < 1) || !(atol >= 0) || max_it < 1)
    return cfdh_fail(c, CFDH_E_ARG, "cfdh_ipcs_krylov_solve: 0 <= rtol < 1, atol >= 0, max_it >= 1");
  c->err.clear();
  return cfdh_ipcs_krylov_solve_impl(c, which, b, x0, rtol, atol, max_it, x, stats, scalars);
}

}  // extern "C"
