// Set-up of a pressure-correction context: creation, Dirichlet data, and the uploads of everything that changes between steps
// only through the host (the pressure Laplacian with its hierarchy, rho M, the constants of ipcs_midpoint).  The arithmetic is
// cfdh_ipcs_host.hpp's; this file allocates and uploads.
#include <hip/hip_runtime.h>

#include "cfdh_internal.hpp"
#include "cfdh_mesh_host.hpp"
#include "cfdh_ipcs.hpp"

namespace H = cfdh_ipcs_host;

int cfdh_ipcs_create(cfdh_ctx *c, int gdim, int64_t nn64, int64_t nvert64, int64_t nc64, const int32_t *cells, const double *coords,
                     int64_t nfac, const int32_t *fcell, const int32_t *flocal, const int32_t *fmarker) {
  const int D = gdim, NL = D == 2 ? 6 : 10, NV = D + 1;
  cfdh_mesh::Wording W;
  W.facet = "cfdh_create_ipcs: bad exterior facet";
  std::string why;
  if (!H::ip_check_mesh(D, nn64, nvert64, nc64, cells, why) || !cfdh_mesh::check_facets(nfac, fcell, flocal, nc64, NV, W, why))
    return cfdh_fail(c, CFDH_E_ARG, "%s", why.c_str());
  const int nn = (int)nn64, nvert = (int)nvert64, nc = (int)nc64;
  IpcsData *I = new (std::nothrow) IpcsData();
  if (!I) return cfdh_fail(c, CFDH_E_NOMEM, "out of host memory");
  c->ipcs = I;
  c->dim = D; c->nv = nn; c->nvo = nn; c->ng = 0; c->nc = nc; c->nloc = NL; c->etype = 0; c->gen = false; c->nranks = 1;
  c->nfac = c->nfac_user = (int)nfac;
  I->D = D; I->NL = NL; I->nn = nn; I->nvert = nvert; I->nc = nc;
  I->cells.assign(cells, cells + (size_t)NL * nc);
  I->coords.assign(coords, coords + (size_t)D * nn);
  I->fcell.assign(fcell, fcell + nfac); I->flocal.assign(flocal, flocal + nfac);
  I->fmarker.assign((size_t)nfac, 0);
  if (fmarker) I->fmarker.assign(fmarker, fmarker + nfac);
  hipStream_t s = c->stream;
  // reduction scratch of the shared helpers (AMG set-up uses red_out)
  CHK(cfdh_alloc_reduction(c, false));  // no ev_h in this context
  memset(c->h_pinned, 0, HP_WORDS * sizeof(double));

  IpOps &O = I->op;
  H::ip_reference(D, I->ref);
  if (!H::ip_geometry(D, nc, cells, coords, I->geo, why)) return cfdh_fail(c, CFDH_E_ARG, "%s", why.c_str());
  H::ip_constant_operators(I->ref, nn, nvert, nc, I->cells.data(), I->geo.data(), O);
  const size_t nnz2 = O.col2.size(), nnz1 = O.col1.size();
  // device copies
  HIPCHK(c, I->d_cells.upload(I->cells, s)); HIPCHK(c, I->d_coords.upload(I->coords, s)); HIPCHK(c, I->d_geo.upload(I->geo, s));
  HIPCHK(c, I->d_T2.upload(I->ref.T2, s));
  HIPCHK(c, I->rp2.upload(O.ptr2, s)); HIPCHK(c, I->col2.upload(O.col2, s));
  HIPCHK(c, I->Mv.upload(O.M, s)); HIPCHK(c, I->Kv.upload(O.K, s));
  HIPCHK(c, I->eptr.upload(O.eptr, s)); HIPCHK(c, I->elist.upload(O.elist, s));
  HIPCHK(c, I->d_gptr.upload(O.gptr, s)); HIPCHK(c, I->d_gcol.upload(O.gcol, s));
  HIPCHK(c, I->Gv.upload(O.G, s)); HIPCHK(c, I->BTv.upload(O.BT, s));
  HIPCHK(c, I->d_bptr.upload(O.bptr, s)); HIPCHK(c, I->d_bcol.upload(O.bcol, s)); HIPCHK(c, I->Bv.upload(O.B, s));
  HIPCHK(c, I->d_m1.upload(O.m1, s));
  HIPCHK(c, I->rp1.upload(O.ptr1, s)); HIPCHK(c, I->col1.upload(O.col1, s)); HIPCHK(c, I->Mpv.upload(O.Mp, s));
  HIPCHK(c, I->Lv.alloc(nnz1));
  HIPCHK(c, I->Afree.alloc(nnz2)); HIPCHK(c, I->A1v.alloc(nnz2)); HIPCHK(c, I->RMv.alloc(nnz2));
  HIPCHK(c, I->dinv1.alloc(nn)); HIPCHK(c, I->dinv3.alloc(nn));
  HIPCHK(c, I->cw.alloc((size_t)nc * NL * D));
  const size_t n1 = (size_t)nn * D;
  dbuf<double> *uv[] = {&I->u_sol, &I->u_prev, &I->u_n1, &I->us, &I->b1, &I->b3, &I->kr, &I->krh, &I->kp, &I->kv, &I->ks, &I->kt, &I->ky, &I->kz, &I->uval};
  for (auto *b : uv) { HIPCHK(c, b->alloc(n1)); HIPCHK(c, b->zero(s)); }
  dbuf<double> *pv[] = {&I->p_sol, &I->p_prev, &I->phi, &I->b2, &I->pr, &I->pz, &I->pp, &I->pq, &I->lift2, &I->prhs};
  for (auto *b : pv) { HIPCHK(c, b->alloc(nvert)); HIPCHK(c, b->zero(s)); }
  HIPCHK(c, I->ucnt.alloc(nn)); HIPCHK(c, I->ucnt.zero(s));
  HIPCHK(c, I->uflag.alloc(nn)); HIPCHK(c, I->uflag.zero(s));
  HIPCHK(c, I->pflag.alloc(nvert)); HIPCHK(c, I->pflag.zero(s));
  HIPCHK(c, I->S.alloc(IP_NS)); HIPCHK(c, I->S.zero(s));
  HIPCHK(c, I->P.alloc(2 * IP_NB)); HIPCHK(c, I->P.zero(s));
  std::vector<int> wv, wptr, wfac;  // alive until the synchronisation below
  if (nfac > 0) {
    HIPCHK(c, I->d_fcell.upload(I->fcell, s)); HIPCHK(c, I->d_flocal.upload(I->flocal, s)); HIPCHK(c, I->d_fmarker.upload(I->fmarker, s));
    HIPCHK(c, I->fout.alloc((size_t)nfac));
    cfdh_mesh::wall_vertex_facets(NL, NV, nfac, I->fcell.data(), I->flocal.data(), I->cells.data(), nvert, wv, wptr, wfac);
    I->n_wallv = (int)wv.size();
    HIPCHK(c, I->wv_list.upload(wv, s)); HIPCHK(c, I->wv_ptr.upload(wptr, s)); HIPCHK(c, I->wv_fac.upload(wfac, s));
  }
  I->h_uflag.assign(nn, 0); I->h_ucnt.assign(nn, 0.0); I->h_uval.assign(n1, 0.0);
  I->h_pflag.assign(nvert, 0); I->h_pcnt.assign(nvert, 0.0); I->h_pval.assign(nvert, 0.0);
  HIPCHK(c, hipStreamSynchronize(s));
  std::vector<int>().swap(O.eptr); std::vector<int>().swap(O.elist);  // the device holds them; nothing on the host reads them again
  return 0;
}

void cfdh_ipcs_free(cfdh_ctx *c) {
  if (!c->ipcs) return;
  c->ipcs->hLam.clear();
  delete c->ipcs;
  c->ipcs = nullptr;
}

// ---- Dirichlet data ------------------------------------------------------------------------------------------------
int cfdh_ipcs_clear_dirichlet(cfdh_ctx *c) {
  IpcsData *I = IP(c);
  std::fill(I->h_uflag.begin(), I->h_uflag.end(), 0); std::fill(I->h_ucnt.begin(), I->h_ucnt.end(), 0.0); std::fill(I->h_uval.begin(), I->h_uval.end(), 0.0);
  std::fill(I->h_pflag.begin(), I->h_pflag.end(), 0); std::fill(I->h_pcnt.begin(), I->h_pcnt.end(), 0.0); std::fill(I->h_pval.begin(), I->h_pval.end(), 0.0);
  I->ubc_dirty = I->pbc_dirty = I->pset_dirty = I->uset_dirty = true;
  I->assembled = false;
  return 0;
}
int cfdh_ipcs_add_dirichlet(cfdh_ctx *c, int field, int64_t n, const int32_t *nodes, const double *values, bool update) {
  IpcsData *I = IP(c);
  const int lim = field == 0 ? I->nn : I->nvert, D = I->D;
  for (int64_t k = 0; k < n; k++) {
    if (nodes[k] < 0 || nodes[k] >= lim) return cfdh_fail(c, CFDH_E_ARG, "Dirichlet node %d out of range", (int)nodes[k]);
    if (update && !(field == 0 ? I->h_uflag[nodes[k]] : I->h_pflag[nodes[k]]))
      return cfdh_fail(c, CFDH_E_ARG, "cfdh_update_dirichlet: node %d is not constrained", (int)nodes[k]);
  }
  for (int64_t k = 0; k < n; k++) {
    const int v = nodes[k];
    if (field == 0) {
      if (!update) { I->h_uflag[v] = 1; I->h_ucnt[v] += 1.0; I->uset_dirty = true; }
      for (int d = 0; d < D; d++) I->h_uval[(size_t)D * v + d] = values[(size_t)D * k + d];
    } else {
      if (!update) { I->h_pflag[v] = 1; I->h_pcnt[v] += 1.0; I->pset_dirty = true; }
      I->h_pval[v] = values[k];
    }
  }
  if (field == 0) I->ubc_dirty = true; else I->pbc_dirty = true;
  I->assembled = false;
  return 0;
}

// pressure Laplacian with its Dirichlet rows, the hierarchy, and the constant parts of b2
static int ip_prepare_pressure(cfdh_ctx *c) {
  IpcsData *I = IP(c);
  const int nv = I->nvert;
  hipStream_t s = c->stream;
  if (I->pset_dirty || !I->hLam.valid) {
    std::vector<double> Lc;
    CsrHost La;  // without the explicit zeros of the eliminated rows / columns: what the hierarchy is built from
    La.n = La.m = nv;
    H::ip_constrain_laplacian(I->op, I->h_pflag, I->h_pcnt, Lc, La.rowptr, La.col, La.val, I->singular);
    HIPCHK(c, hipMemcpyAsync(I->Lv.p, Lc.data(), sizeof(double) * Lc.size(), hipMemcpyHostToDevice, s));
    HIPCHK(c, I->pflag.upload(I->h_pflag, s));
    HIPCHK(c, hipStreamSynchronize(s));
    I->hLam.clear();
    int rc = -1;
    if (cfdh_amg_dev_enabled(c)) {
      CsrDev Ld;
      if (cfdh_upload_csr(c, La, Ld, nullptr, CFDH_UP_CSR) == 0) {
        HIPCHK(c, hipStreamSynchronize(s));
        rc = cfdh_amg_setup_dev(c, I->hLam, Ld, I->singular, 1);
      }
      if (rc != 0) {
        if (c->opt.verbose) fprintf(stderr, "[cfdh] device-side AMG set-up gave up (%s): building the pressure hierarchy on the host\n", c->err.c_str());
        c->err.clear(); I->hLam.clear();
      }
    }
    if (rc != 0) CHK(cfdh_amg_setup(c, I->hLam, La, I->singular, 1));
    I->pset_dirty = false;
    I->pbc_dirty = true;
  }
  if (I->pbc_dirty && I->scheme == CFDH_IPCS_MIDPOINT) {  // the lifting depends on p_prev: formed on the device each step (ip_plift_kernel)
    HIPCHK(c, I->pval.upload(I->h_pval, s)); HIPCHK(c, I->pcnt.upload(I->h_pcnt, s));
    HIPCHK(c, hipStreamSynchronize(s));
    I->pbc_dirty = false;
  }
  if (I->pbc_dirty) {
    std::vector<double> lift, fix;
    H::ip_lifting(I->op, I->h_pflag, I->h_pcnt, I->h_pval, lift, fix);
    HIPCHK(c, hipMemcpyAsync(I->lift2.p, lift.data(), sizeof(double) * nv, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(I->prhs.p, fix.data(), sizeof(double) * nv, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipStreamSynchronize(s));
    I->pbc_dirty = false;
  }
  return 0;
}

int ip_prepare(cfdh_ctx *c) {
  IpcsData *I = IP(c);
  hipStream_t s = c->stream;
  if (!c->params_set) return cfdh_fail(c, CFDH_E_STATE, "cfdh_set_params was not called");
  if (I->ubc_dirty) {
    HIPCHK(c, I->uflag.upload(I->h_uflag, s)); HIPCHK(c, I->ucnt.upload(I->h_ucnt, s)); HIPCHK(c, I->uval.upload(I->h_uval, s));
    HIPCHK(c, hipStreamSynchronize(s));
    I->ubc_dirty = false;
  }
  CHK(ip_prepare_pressure(c));
  if (I->rm_rho != c->rho) {  // rho M and its Jacobi weights
    std::vector<double> rm, di;
    H::ip_rho_mass(I->op, c->rho, rm, di);
    HIPCHK(c, hipMemcpyAsync(I->RMv.p, rm.data(), sizeof(double) * rm.size(), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(I->dinv3.p, di.data(), sizeof(double) * di.size(), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipStreamSynchronize(s));
    I->rm_rho = c->rho;
  }
  return 0;
}

// ---- ipcs_midpoint: the constants of the vector-coupled form, built once
static int ip_mid_build(cfdh_ctx *c) {
  IpcsData *I = IP(c);
  if (I->mid_built) return 0;
  const int D = I->D;
  hipStream_t s = c->stream;
  IpMid &Q = I->mid;
  H::ip_midpoint_constants(I->ref, I->op, I->nn, I->nc, I->cells.data(), I->geo.data(), I->fcell.size(), I->fcell.data(), I->flocal.data(), Q);
  const size_t nnz2 = I->op.col2.size();
  HIPCHK(c, I->ESv.upload(Q.ES, s)); HIPCHK(c, I->BTPv.upload(Q.BTP, s));
  HIPCHK(c, I->nptr.upload(Q.nptr, s)); HIPCHK(c, I->nlist.upload(Q.nlist, s));
  HIPCHK(c, I->Lfree.upload(I->op.L, s));
  HIPCHK(c, I->AfreeB.alloc(nnz2 * D * D)); HIPCHK(c, I->A1B.alloc(nnz2 * D * D));
  HIPCHK(c, I->dinvB.alloc((size_t)I->nn * D)); HIPCHK(c, I->conv.alloc((size_t)I->nn * D));
  HIPCHK(c, hipStreamSynchronize(s));
  I->mid_built = true;
  return 0;
}

int cfdh_ipcs_set_scheme_impl(cfdh_ctx *c, int scheme) {
  IpcsData *I = IP(c);
  if (scheme == I->scheme) return 0;
  if (scheme == CFDH_IPCS_MIDPOINT) CHK(ip_mid_build(c));
  I->scheme = scheme;
  I->mid_valid = false; I->assembled = false;
  I->pbc_dirty = true;              // lift2 / prhs hold the other scheme's data
  HIPCHK(c, I->us.zero(c->stream));  // the initial guess of solve 1 belongs to the other scheme's u*
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}
