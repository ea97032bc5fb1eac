// Host driver of the per-step solve (stabilized_schur.py:313-334): Newton with a
// backtracking line search (SNES newtonls/bt), right-preconditioned FGMRES
// (KSPFGMRES, restart/caps of :272-273) and a GPU block-Schur preconditioner in
// the factorisation the reference configures (PCFIELDSPLIT Schur, :231-235) with
// GPU-friendly sub-solvers instead of GMRES+ILU(0)/ILU(0):
//   pc_type 1 (default): velocity block = one AMG V-cycle of the scalar proxy of A00
//     (both components at once); Schur complement of Cahouet-Chabard type,
//     S^-1 ~ (a' L^-1 + b' M_l^-1) H^-1 -- Chebyshev(2) on the mass-like H, one AMG
//     V-cycle on the P1 Laplacian L; block upper-triangular (default) / FULL / lower;
//   pc_type 0: the reference's SELFP matrix Sp = A11 - A10 diag(A00)^-1 A01 with an
//     AMG V-cycle, Jacobi-Chebyshev on A00.
// Hierarchies are built on the host and lagged.  All vectors stay in HBM; the host
// sees a few scalars per iteration.
#include <algorithm>
#include <chrono>
#include <cmath>

#include "cfdh_internal.hpp"
#include "cfdh_krylov_host.hpp"

int cfdh_host_threads();

static double wall_ms() {
  using namespace std::chrono;
  return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

int cfdh_download_blocks(cfdh_ctx *c, std::vector<double> &a00, std::vector<double> &a01, std::vector<double> &a10,
                         std::vector<double> &a11) {
  const size_t nz = (size_t)c->nnzv, d = (size_t)c->dim;
  a00.resize(d * d * nz); a01.resize(d * nz); a10.resize(d * nz); a11.resize(nz);
  HIPCHK(c, hipMemcpyAsync(a00.data(), c->A00.p, sizeof(double) * d * d * nz, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(a01.data(), c->A01.p, sizeof(double) * d * nz, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(a10.data(), c->A10.p, sizeof(double) * d * nz, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(a11.data(), c->A11.p, sizeof(double) * nz, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

// Sp = A11 - A10 diag(A00)^-1 A01 on the owned vertices (rank-local, like the
// reference's per-rank ASM blocks)
static int build_schur_host(cfdh_ctx *c, CsrHost &S) {
  std::vector<double> a00, a01, a10, a11;
  CHK(cfdh_download_blocks(c, a00, a01, a10, a11));
  const int nvo = c->nvo;
  const std::vector<int> &vp = c->h_vptr, &vc = c->h_vcol;
  std::vector<double> dinv(2 * (size_t)nvo);
  for (int v = 0; v < nvo; v++) {
    const size_t k = (size_t)c->h_vdiag[v];
    dinv[2 * v] = 1.0 / a00[4 * k]; dinv[2 * v + 1] = 1.0 / a00[4 * k + 3];
  }
  S.n = S.m = nvo;
  std::vector<std::vector<int>> cols(nvo);
  std::vector<std::vector<double>> vals(nvo);
#pragma omp parallel num_threads(cfdh_host_threads())
  {
    std::vector<int> mark(nvo, -1), list;
    std::vector<double> acc(nvo, 0.0);
#pragma omp for schedule(dynamic, 512)
    for (int i = 0; i < nvo; i++) {
      list.clear();
      for (int k = vp[i]; k < vp[i + 1]; k++) {
        const int w = vc[k];
        if (w >= nvo) continue;
        if (mark[w] != i) { mark[w] = i; acc[w] = 0.0; list.push_back(w); }
        acc[w] += a11[k];
        const double s0 = a10[2 * (size_t)k] * dinv[2 * w], s1 = a10[2 * (size_t)k + 1] * dinv[2 * w + 1];
        if (s0 == 0.0 && s1 == 0.0) continue;
        for (int k2 = vp[w]; k2 < vp[w + 1]; k2++) {
          const int j = vc[k2];
          if (j >= nvo) continue;
          if (mark[j] != i) { mark[j] = i; acc[j] = 0.0; list.push_back(j); }
          acc[j] -= s0 * a01[2 * (size_t)k2] + s1 * a01[2 * (size_t)k2 + 1];
        }
      }
      std::sort(list.begin(), list.end());
      cols[i] = list;
      vals[i].resize(list.size());
      for (size_t t = 0; t < list.size(); t++) vals[i][t] = acc[list[t]];
    }
  }
  S.rowptr.assign(nvo + 1, 0);
  for (int i = 0; i < nvo; i++) S.rowptr[i + 1] = S.rowptr[i] + (int)cols[i].size();
  S.col.resize(S.rowptr[nvo]); S.val.resize(S.rowptr[nvo]);
  for (int i = 0; i < nvo; i++) {
    std::copy(cols[i].begin(), cols[i].end(), S.col.begin() + S.rowptr[i]);
    std::copy(vals[i].begin(), vals[i].end(), S.val.begin() + S.rowptr[i]);
  }
  return 0;
}

// Do-nothing boundary (ds_terms off) and the natural pressure boundaries of the rotational form (which has no ds pair): the nodes
// of every exterior facet that is not a no-slip / inflow facet (all velocity components of all its nodes constrained) form the
// outflow boundary of the preconditioner's pressure Poisson problem: bit 1.
static void mark_outflow_nodes(const cfdh_ctx *c, std::vector<unsigned char> &pbc) {
  const unsigned umask = (1u << c->dim) - 1u;
  const int nvo = c->nvo;
  for (int k = 0; k < c->nfac; k++) {
    const int e = c->fac_cell[k], fl = c->fac_local[k];
    int loc[8], nn = 0;
    if (c->gen) nn = c->dim == 3 ? cfdh_facet_nodes3(c, fl, loc) : cfdh_facet_nodes(c, fl, loc);
    else for (int q = 0; q <= c->dim; q++) if (q != fl) loc[nn++] = q;
    bool fixed = true;
    for (int q = 0; q < nn; q++) fixed = fixed && (c->h_bcflag[c->h_cells[(size_t)c->nloc * e + loc[q]]] & umask) == umask;
    if (fixed) continue;
    for (int q = 0; q < nn; q++) {
      const int v = c->h_cells[(size_t)c->nloc * e + loc[q]];
      if (v < nvo) pbc[v] |= 2;
    }
  }
}

// pc_type 2: the Dirichlet rows of the PCD operator's A_p -- every vertex of a facet marked as the outlet (bcs_pcd of
// stabilized_pcd.py:215-218, PCDPC_vY) -- as bit 1, next to the pressure-Dirichlet bit 0.  The same array gives the flags of the
// apply pass (bit 0: Dirichlet row of A_p, bit 1: pressure-Dirichlet row of the Jacobian).
static void mark_pcd_outlet(const cfdh_ctx *c, std::vector<unsigned char> &pbc) {
  for (int k = 0; k < c->nfac; k++) {
    if (c->fac_marker[k] != c->pcd_out) continue;
    const int e = c->fac_cell[k], fl = c->fac_local[k];
    int loc[8], nn = 0;
    if (c->gen) nn = c->dim == 3 ? cfdh_facet_nodes3(c, fl, loc) : cfdh_facet_nodes(c, fl, loc);
    else for (int q = 0; q <= c->dim; q++) if (q != fl) loc[nn++] = q;
    for (int q = 0; q < nn; q++) {
      const int v = c->h_cells[(size_t)c->nloc * e + loc[q]];
      if (v < c->nvo) pbc[v] |= 2;
    }
  }
}
static int upload_pcd_flags(cfdh_ctx *c, const std::vector<unsigned char> &pbc) {
  std::vector<unsigned char> fl(pbc.size());
  for (size_t i = 0; i < pbc.size(); i++) fl[i] = (unsigned char)((pbc[i] ? 1u : 0u) | ((pbc[i] & 1u) ? 2u : 0u));
  HIPCHK(c, c->pcd_flag.upload(fl, c->stream));
  return 0;
}

// pc_type 1 -- host side of the Cahouet-Chabard-type preconditioner (all rank-local, owned x owned):
//   * hA : SA hierarchy of the scalar proxy (A00_xx + A00_yy)/2 of the velocity block, applied to both
//          components at once (the xy coupling of the symmetric-gradient term is dropped: Korn-equivalent);
//   * hL : SA hierarchy of the P1 pressure Laplacian (Dirichlet rows where p is prescribed) -- geometry
//          and Dirichlet set only, so it is built once;
//   * H  = (I + a'T) M_l + b' A11 with a' = 2 rho/dt, b' = mu, T = diag(A11)/diag(L) (nodal tau/rho):
//          S^-1 ~ (a' L^-1 + b' M_l^-1) [ (I + a'T) + b' A11 M_l^-1 ]^-1 for
//          S = A11 + (1/2) B A00^-1 B^T ~ A11 + (a' L^-1 + b' M_l^-1)^-1   (A11 = (tau/rho)-weighted Laplacian).
static int upload_csr_plain(cfdh_ctx *c, const CsrHost &H, CsrDev &D);

// Hierarchy of a level-0 operator assembled on the host (partitioned runs: ghost rows, replicated pressure space): the sparse
// products, aggregation and formats still run on the device (cfdh_amg_dev.hip) -- the operator is uploaded once.  Falls back to
// the host build when the device build is switched off or gives up.
static int amg_setup_from_host(cfdh_ctx *c, AmgHier &H, const CsrHost &A, bool singular, int ncol) {
  static const bool host_multi = getenv("CFDH_AMG_HOST_MULTI") && getenv("CFDH_AMG_HOST_MULTI")[0] == '1';
  if (cfdh_amg_dev_enabled(c) && !host_multi) {
    CsrDev Ad;
    if (upload_csr_plain(c, A, Ad) == 0 && cfdh_amg_setup_dev(c, H, Ad, singular, ncol) == 0) return 0;
    if (c->opt.verbose) fprintf(stderr, "[cfdh] device-side AMG set-up gave up (%s): building this hierarchy on the host\n", c->err.c_str());
    c->err.clear();
  }
  return cfdh_amg_setup(c, H, A, singular, ncol);
}

// Replicated pressure space of a partitioned run (cfdh_set_global_pressure_space): geometry only, built once per Dirichlet set.
static int build_global_pressure(cfdh_ctx *c) {
  const int nvo = c->nvo;
  if (c->gp_n > 0 && (c->gp_dirty || !c->hLg.valid)) {
    const bool dist = c->nranks > 1 && (int)c->h_gid.size() == c->nv && c->ng > 0;
    c->hLg.keep_host0 = dist;
    CHK(amg_setup_from_host(c, c->hLg, c->gp_L, c->gp_singular, 1));
    c->gp_dirty = false;
    // Distributed finest level: this rank's rows of the global level-0 operator / prolongator (the hierarchy is
    // geometry-only and identical on all ranks, so no exchange is needed to build them).  The cycle is then the
    // SAME arithmetic as the replicated one -- Jacobi sweeps are row-local once the ghost values are there.
    cfdh_ctx::DistL0 &d = c->dl0;
    d.on = false;
    if (dist && c->hLg.lev.size() >= 2) {
      const CsrHost &A0 = c->hLg.h_A0, &P0 = c->hLg.h_P0;
      const std::vector<double> &w0 = c->hLg.h_wdinv0;
      const int nv = c->nv, n1 = c->hLg.lev[1]->n;
      bool ok = (int)w0.size() == c->gp_n && A0.n == c->gp_n && P0.n == c->gp_n && P0.m == n1;
      CsrHost Al, Pl, Pt;
      Al.n = nvo; Al.m = nv; Al.rowptr.assign(nvo + 1, 0);
      for (int i = 0; i < nvo && ok; i++) {
        const int g = c->h_gid[i];
        for (int k = A0.rowptr[g]; k < A0.rowptr[g + 1]; k++) {
          const int loc = c->h_g2l[A0.col[k]];
          if (loc < 0) { ok = false; break; }  // a neighbour of an owned vertex is always local (every overlap holds the cells of the owned vertices)
          Al.col.push_back(loc); Al.val.push_back(A0.val[k]);
        }
        Al.rowptr[i + 1] = (int)Al.col.size();
      }
      Pl.n = nv; Pl.m = n1; Pl.rowptr.assign(nv + 1, 0);
      std::vector<int> cnt(n1 + 1, 0);
      for (int i = 0; i < nv && ok; i++) {
        const int g = c->h_gid[i];
        for (int k = P0.rowptr[g]; k < P0.rowptr[g + 1]; k++) {
          Pl.col.push_back(P0.col[k]); Pl.val.push_back(P0.val[k]);
          if (i < nvo) cnt[P0.col[k] + 1]++;
        }
        Pl.rowptr[i + 1] = (int)Pl.col.size();
      }
      if (ok) {
        Pt.n = n1; Pt.m = nvo; Pt.rowptr.assign(n1 + 1, 0);
        for (int I = 0; I < n1; I++) Pt.rowptr[I + 1] = Pt.rowptr[I] + cnt[I + 1];
        Pt.col.resize(Pt.rowptr[n1]); Pt.val.resize(Pt.rowptr[n1]);
        std::vector<int> fill(Pt.rowptr.begin(), Pt.rowptr.end() - 1);
        for (int i = 0; i < nvo; i++)  // ascending owned index within every coarse row: fixed summation order
          for (int k = Pl.rowptr[i]; k < Pl.rowptr[i + 1]; k++) { const int q = fill[Pl.col[k]]++; Pt.col[q] = i; Pt.val[q] = Pl.val[k]; }
        std::vector<double> wl(nv);
        for (int i = 0; i < nv; i++) wl[i] = w0[c->h_gid[i]];
        CHK(cfdh_upload_csr(c, Al, d.A, &wl)); CHK(cfdh_upload_csr(c, Pl, d.P)); CHK(cfdh_upload_csr(c, Pt, d.PT));
        HIPCHK(c, d.wdinv.upload(wl, c->stream));
        HIPCHK(c, d.b.alloc(nv)); HIPCHK(c, d.xa.alloc(nv)); HIPCHK(c, d.r.alloc(nvo)); HIPCHK(c, d.x1.alloc(nv));
        HIPCHK(c, d.b.zero(c->stream)); HIPCHK(c, d.xa.zero(c->stream));  // their ghost parts stay zero when the rhs's ghost layer is not exchanged
        HIPCHK(c, hipStreamSynchronize(c->stream));
        d.n1 = n1;
        d.on = true;
        // Round 4: the ghost layer of the cycle's right-hand side is NOT exchanged any more -- the pre-smoothed iterate W b is taken
        // as zero on the ghost vertices.  That perturbs the pre-smoothing on the interface rows only; measured with 4 ranks
        // (gpurun_out/r4_d.log, r4_e.log): dfg_1 22.6 / 22.6 iterations per step with / without the exchange, stenosis 87.5 / 87.5,
        // tetrahedra 70.2 / 70.5, cavity 26.7 / 26.7 -- one halo exchange per FGMRES iteration less.  CFDH_DL0_GHOST_RHS=1 restores it.
        { const char *e = getenv("CFDH_DL0_GHOST_RHS"); d.ghost_rhs = e && e[0] == '1'; }
      }
      double bad = d.on ? 0.0 : 1.0;  // all ranks or none
      CHK(comm_allreduce_host(c, &bad, 1));
      d.on = bad == 0.0;
      c->hLg.h_A0 = CsrHost(); c->hLg.h_P0 = CsrHost(); c->hLg.h_wdinv0.clear();
    }
  }
  return 0;
}

static int build_cc_host(cfdh_ctx *c) {
  std::vector<double> a00, a01, a10, a11;
  CHK(cfdh_download_blocks(c, a00, a01, a10, a11));
  const int nvo = c->nvo;
  const std::vector<int> &vp = c->h_vptr, &vc = c->h_vcol;
  // --- scalar proxy of A00
  // Partitioned run with the upper-triangular factor: restricted additive Schwarz with one layer of overlap.  The
  // local operator is the principal submatrix on owned + ghost vertices; the ghost rows are fetched from their
  // owners (entry k of every owned row travels in round k of the ordinary halo exchange, tagged with the global
  // column id).  With exact subdomain solves this brings the iteration count of 4-8 strips back to the
  // single-domain one; without overlap (block Jacobi) it grows by half.
  const bool ras = c->nranks > 1 && c->gp_n > 0 && c->opt.schur_full == 2 && (int)c->h_gid.size() == c->nv && c->ng > 0;
  {
    const int nloc = ras ? c->nv : nvo;
    CsrHost Ah;
    Ah.n = Ah.m = nloc;
    Ah.rowptr.assign(nloc + 1, 0);
    int maxlen = 0;
    for (int i = 0; i < nvo; i++) {
      for (int k = vp[i]; k < vp[i + 1]; k++) {
        const int w = vc[k];
        if (w >= nloc) continue;
        // mean of the diagonal entries of the dim x dim block: (A00_xx + A00_yy [+ A00_zz]) / dim
        double v = 0.0;
        for (int q = 0; q < c->dim; q++) v += a00[(size_t)c->dim * c->dim * k + (size_t)q * (c->dim + 1)];
        v /= c->dim;
        if (v == 0.0 && w != i) continue;
        Ah.col.push_back(w); Ah.val.push_back(v);
      }
      Ah.rowptr[i + 1] = (int)Ah.col.size();
      maxlen = std::max(maxlen, Ah.rowptr[i + 1] - Ah.rowptr[i]);
    }
    if (ras) {
      double ml = (double)maxlen;  // rounds = longest owned row over all ranks
      CHK(comm_allreduce_host(c, &ml, 1));
      const int rounds = (int)ml;
      if (!c->pcw.p) { HIPCHK(c, c->pcw.alloc(c->NL)); }
      std::vector<std::vector<std::pair<int, double>>> grow(c->ng);
      std::vector<double> hv((size_t)c->NL);
      for (int k = 0; k < rounds; k++) {
        std::fill(hv.begin(), hv.end(), -1.0);
        for (int i = 0; i < nvo; i++) {
          const int p = Ah.rowptr[i] + k;
          // the pair (global column id, value) rides in the first two velocity slots of the vertex record
          if (p < Ah.rowptr[i + 1]) { hv[(size_t)c->dim * i] = (double)c->h_gid[Ah.col[p]]; hv[(size_t)c->dim * i + 1] = Ah.val[p]; }
        }
        HIPCHK(c, c->pcw.upload(hv, c->stream));
        CHK(comm_halo(c, c->pcw.p));
        const size_t W = (size_t)c->dim + 1;  // doubles per vertex record
        HIPCHK(c, hipMemcpyAsync(hv.data() + W * (size_t)nvo, c->pcw.p + W * (size_t)nvo, sizeof(double) * W * (size_t)c->ng,
                                 hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (int g = 0; g < c->ng; g++) {
          const double gd = hv[W * (size_t)nvo + W * (size_t)g];
          if (!(gd >= 0)) continue;
          const int loc = c->h_g2l[(int)gd];
          if (loc >= 0) grow[g].push_back({loc, hv[W * (size_t)nvo + W * (size_t)g + 1]});
        }
      }
      HIPCHK(c, c->pcw.zero(c->stream));
      for (int g = 0; g < c->ng; g++) {
        auto &r = grow[g];
        std::sort(r.begin(), r.end());
        bool diag = false;
        for (auto &e : r) { Ah.col.push_back(e.first); Ah.val.push_back(e.second); diag |= e.first == nvo + g; }
        if (!diag) return cfdh_fail(c, CFDH_E_COMM, "ghost row %d arrived without its diagonal", g);
        Ah.rowptr[nvo + g + 1] = (int)Ah.col.size();
      }
      if (!c->ras_b.p) { HIPCHK(c, c->ras_b.alloc((size_t)c->dim * c->nv)); HIPCHK(c, c->ras_x.alloc((size_t)c->dim * c->nv)); }
    }
    c->ras = ras;
    CHK(amg_setup_from_host(c, c->hA, Ah, false, c->dim));
  }
  // --- pressure Laplacian hierarchy (once per Dirichlet set)
  // pbc bit0: the pressure dof is Dirichlet (identity row in H, z_p = r_p); bit1: Dirichlet in L only --
  // with a do-nothing boundary (ds_terms off) the vertices of every exterior facet that is not a
  // no-slip/inflow facet form the outflow boundary of the pressure Poisson problem.
  std::vector<unsigned char> pbc(nvo);
  const unsigned pbit = 1u << c->dim;  // bits 0..dim-1: velocity components, bit dim: pressure
  for (int i = 0; i < nvo; i++) pbc[i] = (c->h_bcflag[i] & pbit) ? 1 : 0;
  const bool pcd = c->opt.pc_type == 2;  // PCD: the same velocity and pressure-Laplacian hierarchies, A_p's own Dirichlet set, no H
  if (pcd) mark_pcd_outlet(c, pbc);
  else if (!c->ds_terms || c->form == CFDH_FORM_ROTATIONAL) mark_outflow_nodes(c, pbc);
  if (pcd) CHK(upload_pcd_flags(c, pbc));
  if (!c->hL.valid || c->hL_pbc != pbc || c->hL_singular != c->singular) {
    CsrHost Lh;
    Lh.n = Lh.m = nvo;
    Lh.rowptr.assign(nvo + 1, 0);
    for (int i = 0; i < nvo; i++) {
      if (pbc[i]) { Lh.col.push_back(i); Lh.val.push_back(1.0); }
      else
        for (int k = vp[i]; k < vp[i + 1]; k++) {
          const int w = vc[k];
          if (w >= nvo || pbc[w]) continue;
          Lh.col.push_back(w); Lh.val.push_back(c->h_Lval[k]);
        }
      Lh.rowptr[i + 1] = (int)Lh.col.size();
    }
    bool any_pbc = false;
    for (int i = 0; i < nvo; i++) any_pbc |= pbc[i] != 0;
    // a part without pressure-Dirichlet rows has a pure-Neumann (singular) local Laplacian
    CHK(amg_setup_from_host(c, c->hL, Lh, c->singular != 0 || !any_pbc, 1));
    c->hL_pbc = pbc;
    c->hL_singular = c->singular;
    std::vector<double> ml(nvo);
    for (int i = 0; i < nvo; i++) ml[i] = pbc[i] ? 0.0 : c->h_Ml[i];
    HIPCHK(c, c->ccMl.upload(ml, c->stream));
    HIPCHK(c, c->ccPbc.upload(pbc, c->stream));
  }
  CHK(build_global_pressure(c));
  if (pcd) { HIPCHK(c, hipStreamSynchronize(c->stream)); return 0; }
  // --- H
  c->cc_alpha = c->rho * c->ts_a[0] / (c->ts_theta * c->dt);  // = 2 rho/dt for the midpoint scheme
  c->cc_beta = c->mu;
  {
    CsrHost Hh;
    Hh.n = Hh.m = nvo;
    Hh.rowptr.assign(nvo + 1, 0);
    for (int i = 0; i < nvo; i++) {
      if (pbc[i] & 1) { Hh.col.push_back(i); Hh.val.push_back(1.0); }
      else {
        const size_t kd = (size_t)c->h_vdiag[i];
        const double T = c->h_Lval[kd] > 0 ? a11[kd] / c->h_Lval[kd] : 0.0;
        for (int k = vp[i]; k < vp[i + 1]; k++) {
          const int w = vc[k];
          if (w >= nvo || (pbc[w] & 1)) continue;
          double v = c->cc_beta * a11[k];
          if (w == i) v += (1.0 + c->cc_alpha * T) * c->h_Ml[i];
          Hh.col.push_back(w); Hh.val.push_back(v);
        }
      }
      Hh.rowptr[i + 1] = (int)Hh.col.size();
    }
    CsrDev Hd;
    if (cfdh_amg_dev_enabled(c) && upload_csr_plain(c, Hh, Hd) == 0) CHK(cfdh_level_setup_dev(c, c->Hlev, Hd, 8.0, 1));
    else CHK(cfdh_level_setup(c, c->Hlev, Hh, 8.0, 1));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

// The same preconditioner data built where the Jacobian lives (cfdh_amg_dev.hip): no download of the blocks, sparse
// products / aggregation / formats by kernels.
static int upload_csr_plain(cfdh_ctx *c, const CsrHost &H, CsrDev &D) {
  D.n = H.n; D.m = H.m; D.nnz = H.nnz();
  HIPCHK(c, D.rowptr.upload(H.rowptr, c->stream));
  HIPCHK(c, D.col.upload(H.col, c->stream));
  HIPCHK(c, D.val.upload(H.val, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}
static int download_csr_plain(cfdh_ctx *c, const CsrDev &D, CsrHost &H) {
  H.n = D.n; H.m = D.m;
  H.rowptr.resize((size_t)D.n + 1); H.col.resize(D.nnz); H.val.resize(D.nnz);
  HIPCHK(c, hipMemcpyAsync(H.rowptr.data(), D.rowptr.p, sizeof(int) * ((size_t)D.n + 1), hipMemcpyDeviceToHost, c->stream));
  if (D.nnz) {
    HIPCHK(c, hipMemcpyAsync(H.col.data(), D.col.p, sizeof(int) * (size_t)D.nnz, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(H.val.data(), D.val.p, sizeof(double) * (size_t)D.nnz, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}
// Round 4: partitioned runs build here too.  The ghost rows of the overlapping velocity proxy are fetched from their owners by
// halo exchanges of device buffers (cfdh_proxy_ras_dev), H drops the ghost columns in its kernel, and nothing of the Jacobian is
// downloaded.  What is collective (the ghost-row exchange) succeeds or fails on all ranks alike; the hierarchy set-up behind it is
// rank-local, so a rank whose device set-up gives up finishes on the host from a copy of its operator without the others noticing.
static int build_cc_dev(cfdh_ctx *c) {
  const int nvo = c->nvo;
  const std::vector<int> &vp = c->h_vptr, &vc = c->h_vcol;
  const double t0 = wall_ms();
  const bool multi = c->nranks > 1;
  const bool ras = multi && c->gp_n > 0 && c->opt.schur_full == 2 && (int)c->h_gid.size() == c->nv && c->ng > 0;
  c->ras = false;
  {
    CsrDev Ah, keep;
    if (ras) {
      CHK(cfdh_proxy_ras_dev(c, Ah));
      if (!c->ras_b.p) { HIPCHK(c, c->ras_b.alloc((size_t)c->dim * c->nv)); HIPCHK(c, c->ras_x.alloc((size_t)c->dim * c->nv)); }
    } else CHK(cfdh_proxy_dev(c, Ah));
    c->ras = ras;
    if (multi) {  // the set-up consumes its operator
      keep.n = Ah.n; keep.m = Ah.m; keep.nnz = Ah.nnz;
      HIPCHK(c, keep.rowptr.alloc((size_t)Ah.n + 1)); HIPCHK(c, keep.col.alloc((size_t)std::max(Ah.nnz, 1))); HIPCHK(c, keep.val.alloc((size_t)std::max(Ah.nnz, 1)));
      HIPCHK(c, hipMemcpyAsync(keep.rowptr.p, Ah.rowptr.p, sizeof(int) * ((size_t)Ah.n + 1), hipMemcpyDeviceToDevice, c->stream));
      HIPCHK(c, hipMemcpyAsync(keep.col.p, Ah.col.p, sizeof(int) * (size_t)Ah.nnz, hipMemcpyDeviceToDevice, c->stream));
      HIPCHK(c, hipMemcpyAsync(keep.val.p, Ah.val.p, sizeof(double) * (size_t)Ah.nnz, hipMemcpyDeviceToDevice, c->stream));
    }
    const int rc = cfdh_amg_setup_dev(c, c->hA, Ah, false, c->dim);
    if (rc != 0) {
      if (!multi) return rc;
      if (c->opt.verbose) fprintf(stderr, "[cfdh] device-side AMG set-up gave up (%s): building the velocity hierarchy on the host\n", c->err.c_str());
      c->err.clear(); c->hA.clear();
      CsrHost Ahh;
      CHK(download_csr_plain(c, keep, Ahh));
      CHK(cfdh_amg_setup(c, c->hA, Ahh, false, c->dim));
    }
  }
  const double t1 = wall_ms();
  // pressure Laplacian hierarchy: geometry and Dirichlet set only (see build_cc_host for the pbc bits)
  std::vector<unsigned char> pbc(nvo);
  const unsigned pbit = 1u << c->dim;
  for (int i = 0; i < nvo; i++) pbc[i] = (c->h_bcflag[i] & pbit) ? 1 : 0;
  const bool pcd = c->opt.pc_type == 2;
  if (pcd) mark_pcd_outlet(c, pbc);
  else if (!c->ds_terms || c->form == CFDH_FORM_ROTATIONAL) mark_outflow_nodes(c, pbc);
  if (pcd) CHK(upload_pcd_flags(c, pbc));
  if (!c->hL.valid || c->hL_pbc != pbc || c->hL_singular != c->singular) {
    CsrHost Lh;
    Lh.n = Lh.m = nvo;
    Lh.rowptr.assign(nvo + 1, 0);
    Lh.col.reserve(c->nnzv); Lh.val.reserve(c->nnzv);
    bool any_pbc = false;
    for (int i = 0; i < nvo; i++) {
      any_pbc |= pbc[i] != 0;
      if (pbc[i]) { Lh.col.push_back(i); Lh.val.push_back(1.0); }
      else
        for (int k = vp[i]; k < vp[i + 1]; k++) {
          const int w = vc[k];
          if (w >= nvo || pbc[w]) continue;
          Lh.col.push_back(w); Lh.val.push_back(c->h_Lval[k]);
        }
      Lh.rowptr[i + 1] = (int)Lh.col.size();
    }
    if (multi) CHK(amg_setup_from_host(c, c->hL, Lh, c->singular != 0 || !any_pbc, 1));
    else {
      CsrDev Ld;
      CHK(upload_csr_plain(c, Lh, Ld));
      CHK(cfdh_amg_setup_dev(c, c->hL, Ld, c->singular != 0 || !any_pbc, 1));
    }
    c->hL_pbc = pbc;
    c->hL_singular = c->singular;
    std::vector<double> ml(nvo);
    for (int i = 0; i < nvo; i++) ml[i] = pbc[i] ? 0.0 : c->h_Ml[i];
    HIPCHK(c, c->ccMl.upload(ml, c->stream));
    HIPCHK(c, c->ccPbc.upload(pbc, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  if (multi) CHK(build_global_pressure(c));
  const double t2 = wall_ms();
  if (pcd) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->ms_pc_build_dev = wall_ms() - t0;
    return 0;
  }
  c->cc_alpha = c->rho * c->ts_a[0] / (c->ts_theta * c->dt);
  c->cc_beta = c->mu;
  {
    CsrDev Hd;
    CHK(cfdh_cc_h_dev(c, c->cc_alpha, c->cc_beta, Hd));
    CHK(cfdh_level_setup_dev(c, c->Hlev, Hd, 8.0, 1));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->ms_pc_build_dev = wall_ms() - t0;
  if (c->opt.verbose)
    fprintf(stderr, "[cfdh] preconditioner built on the device: velocity hierarchy %.1f ms, pressure Laplacian %.1f ms, H %.1f ms\n", t1 - t0, t2 - t1,
            wall_ms() - t2);
  return 0;
}
static int build_cc(cfdh_ctx *c) {
  // CFDH_PC_HOST_ASSEMBLY=1: level-0 operators of a partitioned run assembled on the host as in rounds 2-3 (comparison, tests)
  static const bool host_multi = (getenv("CFDH_AMG_HOST_MULTI") && getenv("CFDH_AMG_HOST_MULTI")[0] == '1') ||
                                 (getenv("CFDH_PC_HOST_ASSEMBLY") && getenv("CFDH_PC_HOST_ASSEMBLY")[0] == '1');
  if (c->nranks > 1 && cfdh_amg_dev_enabled(c) && !host_multi) return build_cc_dev(c);  // no per-rank fall-back across a collective
  if (c->nranks == 1 && cfdh_amg_dev_enabled(c)) {
    const int rc = build_cc_dev(c);
    if (rc == 0) return 0;
    // the device build gave up (a product row beyond its tables, a zero pivot): keep the message, build on the host
    if (c->opt.verbose) fprintf(stderr, "[cfdh] device-side hierarchy set-up failed (%s): host build\n", c->err.c_str());
    c->hL.clear(); c->hA.clear();
  }
  return build_cc_host(c);
}

// refresh the parts of the preconditioner that follow the current Jacobian:
// always the Jacobi diagonal and the spectral bound of D^-1 A00; the Sp
// hierarchy only when asked (lagged preconditioner)
int cfdh_pc_update(cfdh_ctx *c, bool refresh_amg) {
  const int nu = c->dim * c->nvo;
  if (c->opt.pc_type == 2) {
    CHK(cfdh_pcd_supported(c, "pc_type 2"));
    if (!c->pcd_set) return cfdh_fail(c, CFDH_E_STATE, "pc_type 2 (PCD) needs cfdh_set_schur_pcd");
  } else if (c->dim == 3 && c->opt.pc_type != 1) {
    return cfdh_fail(c, CFDH_E_ARG, "tetrahedral contexts support pc_type 1 and 2 only");
  }
  if (c->opt.pc_type == 1 || c->opt.pc_type == 2) {
    if (refresh_amg || !c->pc_valid) {
      c->pc_graph_valid = false;
      CHK(build_cc(c));
      c->pc_valid = true;
      c->pc_its_ref = 0;
      c->steps_since_refresh = 0;
      c->last_stats.pc_refreshes++;
    c->n_pc_builds++;
    }
    // PCD: K follows the iterate -- assembled once per Newton iteration (fenicsx_pctools reassembles K_p in every PC set-up)
    if (c->opt.pc_type == 2) CHK(k_pcd_assemble(c, c->x.p));
    return 0;
  }
  CHK(k_extract_diag(c));
  // lambda_max(D^-1 A00) by power iteration from a fixed start vector
  double *v = c->pu0.p, *w = c->pu1.p;
  CHK(v_copy(c, nu, c->prand.p, v));
  double lam = 1.0;
  for (int it = 0; it < 8; it++) {
    CHK(k_spmv_block(c, 1, v, w, nullptr, 0));
    CHK(v_pointwise_mult(c, nu, w, c->dinvA.p, w));
    CHK(v_norm_to_dev(c, nu, w, c->red_out.p + RO_POWER));
    CHK(v_scale_inv_dev(c, nu, w, c->red_out.p + RO_POWER, v));
  }
  CHK(scalars_read(c, ScalarRead{c->red_out.p + RO_POWER, 1, false}, &lam, false));  // a set-up read: not in cfdh_info 15
  if (!(lam > 0) || !std::isfinite(lam)) return cfdh_fail(c, CFDH_E_DIVERGED, "non-finite spectral estimate of D^-1 A00 (NaN in the Jacobian?)");
  c->lmaxA = 1.15 * lam;
  CHK(k_cheb_a00_coeffs(c));
  if (refresh_amg || !c->pc_valid) {
    c->pc_graph_valid = false;  // the hierarchies' buffers and coefficients are baked into the graphs
    CsrHost S;
    CHK(build_schur_host(c, S));
    bool any_pbc = false;
    for (int i = 0; i < c->nvo; i++) any_pbc |= (c->h_bcflag[i] & (1u << c->dim)) != 0;
    CHK(cfdh_amg_setup(c, c->hS, S, c->singular != 0 || !any_pbc, 1));
    c->pc_valid = true;
    c->pc_its_ref = 0;
    c->steps_since_refresh = 0;
    c->last_stats.pc_refreshes++;
    c->n_pc_builds++;
  }
  return 0;
}

static bool ras_ghost_rhs() {
  static const bool on = !(getenv("CFDH_RAS_GHOST_RHS") && getenv("CFDH_RAS_GHOST_RHS")[0] == '0');
  return on;
}

// The application is a sequence of stages separated by the exchanges of a partitioned run:
//   stage 0: y_u = V(A00~) r_u                                   | halo(y_u)
//   stage 1: t_p = r_p - A10 y_u ; zH = Cheb3(H) t_p ; y = M_l zH | all-reduce of the global pressure rhs
//   stage 2: t = V(L) y ; z_p = a' t + b' zH                      | halo(z_p)
//   stage 3: z_u = V(A00~)(r_u - A01 z_p)
// With one rank (no exchanges) all stages run back to back; each stage is graph-capturable.
// pc_type 2 (one rank): the stages of pc_type 1 with the PCD action in place of the Cahouet-Chabard one
//   stage 1: t = M_d^-1 t_p, s = K t (0 on the Dirichlet rows of A_p)
//   stage 2: y = V(A_p) s ; z_p = mu t + y (epilogue of the cycle's last kernel; r_p on pressure-Dirichlet rows, mu t on the outlet rows)
// Lean solve path: the scope in which the solver takes it at all -- one rank, the closed-form P1 triangle kernels, the
// Cahouet-Chabard or PCD preconditioner.  Everything else keeps the general code paths.
static bool lean_newton(const cfdh_ctx *c) {  // merged read-backs of the Newton iteration: whatever the preconditioner
  return c->lean && c->nranks == 1 && c->nv == c->nvo && c->dim == 2 && !c->gen;
}
static bool lean_scope(const cfdh_ctx *c) { return lean_newton(c) && (c->opt.pc_type == 1 || c->opt.pc_type == 2); }
// The coupling product of the preconditioner also stores q_u = A01 z_p (for the Krylov product that follows, see pc_then_product)
// unless z_p changes after the stages: the mean of a singular system is removed from it behind the graph.  The choice is baked
// into the captured graphs; every input of it invalidates them when it changes (hierarchy rebuild on a change of `singular` or of
// the options).
static bool lean_keep_qu(const cfdh_ctx *c) { return lean_scope(c) && c->opt.schur_full != 0 && !c->singular && c->qu.p != nullptr; }

// Rank-local pressure cycle t = V(L) y (y in pu1, t in pu2) and the combination out = alpha t + beta zH (r on the flagged rows;
// out2, if given, receives a second copy).  The combination runs in the epilogue of the cycle's last kernel when the fused cycle
// is used, as a kernel of its own otherwise.  CFDH_L_CYCLES = k > 1 (experiments, tests): k V-cycles as the stationary iteration
// t += V(y - L t).
static int pressure_cycle_combine(cfdh_ctx *c, double alpha, double beta, const double *zH, const double *r, const unsigned char *flag,
                                  double *out, double *out2) {
  const int nvo = c->nvo;
  if (c->env.l_cycles > 1 && c->hL.lev.size() >= 1 && c->hL.lev[0]->A.val.p) {
    AmgLevel *L0 = c->hL.lev[0];
    CHK(k_amg_vcycle(c, c->hL, c->pu1.p, c->pu2.p));
    for (int cyc = 1; cyc < c->env.l_cycles; cyc++) {
      CHK(k_csr_spmv(c, L0->A, c->pu2.p, L0->r.p, 1, c->pu1.p));   // r = y - L t
      CHK(k_amg_vcycle(c, c->hL, L0->r.p, L0->d0.p));
      CHK(v_axpy(c, nvo, 1.0, L0->d0.p, c->pu2.p));
    }
    CHK(k_cc_combine(c, nvo, alpha, beta, c->pu2.p, zH, r, flag, out));
    return out2 ? v_copy(c, nvo, out, out2) : 0;
  }
  c->epi.on = true; c->epi.done = false;
  c->epi.alpha = alpha; c->epi.beta = beta; c->epi.zH = zH; c->epi.r = r;
  c->epi.pbc = flag; c->epi.out = out;
  const int rc = k_amg_vcycle(c, c->hL, c->pu1.p, c->pu2.p);
  c->epi.on = false;
  CHK(rc);
  if (!c->epi.done) return k_cc_combine(c, nvo, alpha, beta, c->pu2.p, zH, r, flag, out, out2);
  c->epi.done = false;
  return out2 ? v_copy(c, nvo, out, out2) : 0;
}

static int pcd_stage(cfdh_ctx *c, const double *r, double *z, int stage) {
  const int nvo = c->nvo, nu = c->dim * nvo;
  const double *ru = r, *rp = r + nu;
  double *zu = z, *zp = z + nu;
  const bool upper = c->opt.schur_full == 2;
  switch (stage) {
    case 0:
      if (!upper) CHK(k_amg_vcycle(c, c->hA, ru, c->pu0.p));
      return 0;
    case 1:
      if (!upper) CHK(k_spmv_block(c, 3, c->pu0.p, c->pp0.p, rp, 0));   // t_p = r_p - A10 y_u
      return k_pcd_apply(c, upper ? rp : c->pp0.p, c->pu1.p);
    case 2:  // CFDH_L_CYCLES > 1: the converged A_p solve of the tests
      return pressure_cycle_combine(c, 1.0, c->mu, c->pcd_t.p, c->pcd_q.p, c->pcd_flag.p, zp, nullptr);
    case 3:
      if (c->opt.schur_full) {
        if (lean_keep_qu(c)) CHK(k_spmv_a01_keep(c, zp, c->pu0.p, ru, c->qu.p));
        else CHK(k_spmv_block(c, 2, zp, c->pu0.p, ru, 0));   // t_u = r_u - A01 z_p
        CHK(k_amg_vcycle(c, c->hA, c->pu0.p, zu));
      } else {
        CHK(v_copy(c, nu, c->pu0.p, zu));
      }
      return 0;
    default:
      return 0;
  }
}

static int pc_stage(cfdh_ctx *c, const double *r, double *z, int stage) {
  const int nvo = c->nvo, nu = c->dim * nvo;
  const double *ru = r, *rp = r + nu;
  double *zu = z, *zp = z + nu;
  const bool multi = c->nranks > 1;
  const bool global_p = c->gp_n > 0 && multi;
  if (c->opt.pc_type == 2) return pcd_stage(c, r, z, stage);
  if (c->opt.pc_type == 1) {
    const bool upper = c->opt.schur_full == 2;  // block upper-triangular: z_p = S^-1 r_p, z_u = A^-1 (r_u - A01 z_p)
    // logical stages: 0 first velocity cycle, 1 H solve, 2 pressure cycle, 3 coupling product, 4 overlapping velocity
    // cycle; a partitioned run with the distributed pressure level inserts the down sweep (10) after the H solve
    const bool dist = global_p && c->dl0.on;
    int ls = stage;
    if (dist) ls = stage <= 1 ? stage : (stage == 2 ? 10 : stage - 1);
    switch (ls) {
      case 0:
        if (upper) return 0;
        // in a partitioned run y_u lands in the halo scratch vector so that its ghosts can be refreshed
        CHK(k_amg_vcycle(c, c->hA, ru, multi ? c->pcw.p : c->pu0.p));
        return 0;
      case 1:
        if (upper) { /* t_p = r_p: used in place */ }
        else if (multi) CHK(k_spmv_block_ghost(c, 3, c->pcw.p, c->pp0.p, rp));   // t_p = r_p - A10 y_u (with ghosts)
        else CHK(k_spmv_block(c, 3, c->pu0.p, c->pp0.p, rp, 0));
        {
          // right-hand side of the pressure cycle.  Distributed finest level: straight into the level's own vector (ghost part zero);
          // with the ghost-layer exchange switched on (CFDH_DL0_GHOST_RHS=1) into the pressure slot of the halo scratch vector
          double *y = !dist ? c->pu1.p : (c->dl0.ghost_rhs ? c->pcw.p + nu : c->dl0.b.p);
          if (!(c->opt.cc_smooth_degree == 2 && k_cc_cheb2_scale(c, &c->Hlev, upper ? rp : c->pp0.p, c->pp1.p, c->ccMl.p, y))) {
            CHK(k_level_smooth(c, &c->Hlev, upper ? rp : c->pp0.p, c->pp1.p, c->opt.cc_smooth_degree));
            CHK(k_cc_scale(c, nvo, c->ccMl.p, c->pp1.p, y));
          }
        }
        if (dist) {
        } else if (global_p && c->gp_allgather) {
          CHK(k_gather_global(c, nvo, c->gp_send_idx.p, c->pu1.p, c->gp_sendbuf.p));  // owned values in global-id order
        } else if (global_p) {
          CHK(v_zero(c, c->gp_n, c->gp_rhs.p));
          CHK(k_scatter_global(c, nvo, c->gp_l2g.p, c->pu1.p, c->gp_rhs.p));
        }
        return 0;
      case 10:
        return k_dl0_down(c, c->pcw.p);  // pre-smoothing of the owned rows, owned part of the coarse right-hand side
      case 2: {
        double *zp_halo = (multi && c->opt.schur_full) ? c->pcw.p + nu : nullptr;  // z_p also into the halo scratch vector
        const double *tp = upper ? rp : c->pp0.p;
        if (dist) {
          CHK(k_dl0_up(c, c->pu2.p));    // replicated coarse cycle, prolongation, post-smoothing of the owned rows
        } else if (global_p) {
          if (c->gp_allgather) CHK(k_gather_global(c, c->gp_n, c->gp_src_idx.p, c->gp_recvbuf.p, c->gp_rhs.p));
          CHK(k_amg_vcycle(c, c->hLg, c->gp_rhs.p, c->gp_sol.p));  // the same global V-cycle on every rank
          CHK(k_gather_global(c, nvo, c->gp_l2g.p, c->gp_sol.p, c->pu2.p));
        } else {
          return pressure_cycle_combine(c, c->cc_alpha, c->cc_beta, c->pp1.p, tp, c->ccPbc.p, zp, zp_halo);
        }
        return k_cc_combine(c, nvo, c->cc_alpha, c->cc_beta, c->pu2.p, c->pp1.p, tp, c->ccPbc.p, zp, zp_halo);
      }
      case 3:
        if (c->opt.schur_full) {
          // t_u = r_u - A01 z_p (with ghosts); for the overlapping cycle straight into the velocity slots of the halo scratch vector
          // (the kernel reads the pressure slots and ghost records of that vector and writes its owned velocity slots: disjoint)
          if (multi) CHK(k_spmv_block_ghost(c, 2, c->pcw.p, c->ras ? c->pcw.p : c->pu0.p, ru));
          else if (lean_keep_qu(c)) CHK(k_spmv_a01_keep(c, zp, c->pu0.p, ru, c->qu.p));
          else CHK(k_spmv_block(c, 2, zp, c->pu0.p, ru, 0));
          if (multi && c->ras) {
            // experiment (CFDH_RAS_GHOST_RHS=0): no exchange of the overlap residual -- the right-hand side of the overlapping
            // cycle is zero on the ghost layer
            if (!ras_ghost_rhs()) CHK(v_zero(c, c->NL - c->NO, c->pcw.p + c->NO));
          }
          else {
            CHK(k_amg_vcycle(c, c->hA, c->pu0.p, zu));
            if (c->env.a_cycles > 1 && !multi && c->hA.lev[0]->A.val.p) {
              // experiment: further V-cycles on the velocity proxy (stationary iteration)
              AmgLevel *L0 = c->hA.lev[0];
              for (int cyc = 1; cyc < c->env.a_cycles; cyc++) {
                CHK(k_csr_spmv_ncol(c, L0->A, zu, L0->r.p, 1, c->pu0.p, c->dim));
                CHK(k_amg_vcycle(c, c->hA, L0->r.p, L0->d0.p));
                CHK(v_axpy(c, nu, 1.0, L0->d0.p, zu));
              }
            }
          }
        } else {
          CHK(v_copy(c, nu, multi ? c->pcw.p : c->pu0.p, zu));              // block lower-triangular variant
        }
        return 0;
      case 4:
        if (multi && c->ras && c->opt.schur_full) {
          // restricted additive Schwarz: cycle on owned + ghost vertices, keep the owned part
          CHK(k_ext_pack(c, c->pcw.p, c->ras_b.p));
          if (c->hA.fused && c->opt.amg_smooth_degree == 1 && c->hA.lev.size() >= 2) {
            c->up0_rows = nvo;  // the finest up-sweep writes the owned rows only, straight into z_u
            const int rc = k_amg_vcycle(c, c->hA, c->ras_b.p, zu);
            c->up0_rows = 0;
            CHK(rc);
          } else {
            CHK(k_amg_vcycle(c, c->hA, c->ras_b.p, c->ras_x.p));
            CHK(v_copy(c, nu, c->ras_x.p, zu));
          }
        }
        return 0;
      default:
        return 0;  // stage slot unused by this configuration
    }
  }
  if (stage != 0) return 0;  // pc_type 0 is rank-local: one stage
  CHK(k_cheb_a00(c, ru, c->pu0.p));                       // y_u = C(A00) r_u
  CHK(k_spmv_block(c, 3, c->pu0.p, c->pp0.p, rp, 0));     // t_p = r_p - A10 y_u
  CHK(k_amg_vcycle(c, c->hS, c->pp0.p, zp));              // z_p = V(Sp) t_p
  if (c->opt.schur_full) {
    CHK(k_spmv_block(c, 2, zp, c->pu0.p, ru, 0));         // t_u = r_u - A01 z_p
    CHK(k_cheb_a00(c, c->pu0.p, zu));                     // z_u = C(A00) t_u
  } else {
    CHK(v_copy(c, nu, c->pu0.p, zu));
  }
  return 0;
}

// exchange that follows stage `stage` in a partitioned run
static int pc_exchange(cfdh_ctx *c, int stage) {
  if (c->nranks <= 1 || c->opt.pc_type != 1) return 0;
  const bool dist = c->gp_n > 0 && c->dl0.on;
  int ls = stage;
  if (dist) ls = stage <= 1 ? stage : (stage == 2 ? 10 : stage - 1);
  switch (ls) {
    case 0: return c->opt.schur_full == 2 ? 0 : comm_halo(c, c->pcw.p);
    case 1:
      if (c->gp_n <= 0) return 0;
      if (dist) return c->dl0.ghost_rhs ? comm_halo(c, c->pcw.p) : 0;  // right-hand side of the pressure cycle on the ghost layer
      if (c->gp_allgather) return comm_allgather_dev(c, c->gp_sendbuf.p, c->gp_recvbuf.p, c->gp_maxcnt);
      return comm_allreduce_dev(c, c->gp_rhs.p, c->gp_n, 0);
    case 10: return comm_allreduce_dev(c, c->hLg.lev[1]->b.p, c->dl0.n1, 0);  // coarse right-hand side of the replicated levels
    case 2: return c->opt.schur_full ? comm_halo(c, c->pcw.p) : 0;
    case 3: return (c->ras && c->opt.schur_full && ras_ghost_rhs()) ? comm_halo(c, c->pcw.p) : 0;  // residual of the overlap layer
    default: return 0;
  }
}

// z = P^-1 r.  The kernels of one application have fixed shapes, so every stage is captured into a
// hipGraph and replayed (the Krylov loop is launch-bound otherwise: MI355X guide, "graph-replay-floor").
// Operands differ per Krylov slot (r = V_j, z = Z_j), so graphs are kept per (r, z) pair -- no staging
// copies; all are dropped when a hierarchy is rebuilt.
int cfdh_pc_apply(cfdh_ctx *c, const double *r, double *z) {
  const int nvo = c->nvo;
  const bool graph = c->use_graph && !c->prof_on;
  const bool multi = c->nranks > 1 && c->opt.pc_type == 1;
  if (multi && !c->pcw.p) { HIPCHK(c, c->pcw.alloc(c->NL)); HIPCHK(c, c->pcw.zero(c->stream)); }
  if (lean_scope(c) && c->opt.schur_full != 0 && !c->qu.p) {  // before any capture: the graphs hold its address
    HIPCHK(c, c->qu.alloc(2 * (size_t)c->nvo));
    c->pc_graph_valid = false;
  }
  if (!graph) {
    for (int st = 0; st < 6; st++) { CHK(pc_stage(c, r, z, st)); CHK(pc_exchange(c, st)); }
  } else {
    if (!c->pc_graph_valid) {
      for (auto &e : c->pc_graphs) for (auto &x : e.exec) if (x) (void)hipGraphExecDestroy(x);
      c->pc_graphs.clear();
      c->pc_graph_valid = true;
    }
    cfdh_ctx::PcGraph *pg = nullptr;
    for (auto &e : c->pc_graphs) if (e.r == r && e.z == z) { pg = &e; break; }
    if (!pg) {
      cfdh_ctx::PcGraph ng{r, z, {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}};
      // one rank: all four stages in one graph; partitioned: one graph per stage
      for (int gidx = 0; gidx < (multi ? 6 : 1); gidx++) {
        hipGraph_t g = nullptr;
        HIPCHK(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
        c->capturing = true;
        int rc = 0;
        if (multi) rc = pc_stage(c, r, z, gidx);
        else for (int st = 0; st < 6 && !rc; st++) rc = pc_stage(c, r, z, st);
        c->capturing = false;
        hipError_t e = hipStreamEndCapture(c->stream, &g);
        if (rc) return rc;
        if (e != hipSuccess || !g) return cfdh_fail(c, CFDH_E_HIP, "hipStreamEndCapture: %s", hipGetErrorString(e));
        e = hipGraphInstantiate(&ng.exec[gidx], g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
        if (e != hipSuccess) return cfdh_fail(c, CFDH_E_HIP, "hipGraphInstantiate: %s", hipGetErrorString(e));
      }
      c->pc_graphs.push_back(ng);
      pg = &c->pc_graphs.back();
    }
    if (!multi) {
      HIPCHK(c, hipGraphLaunch(pg->exec[0], c->stream));
    } else {
      for (int st = 0; st < 6; st++) { HIPCHK(c, hipGraphLaunch(pg->exec[st], c->stream)); CHK(pc_exchange(c, st)); }
    }
  }
  if (c->singular) CHK(v_sub_mean(c, nvo, z + (size_t)c->dim * nvo));
  return 0;
}

// One FGMRES iteration's operator: z = P^-1 r, then w = J z.  On the lean path the product takes A01 z_p from the buffer the
// preconditioner application has just filled on the same stream instead of reading the A01 block again.  While the kernel
// timers run the plain product is launched (its byte count is the one the timers' callers know).
static int pc_then_product(cfdh_ctx *c, const double *r, double *z, double *w) {
  CHK(cfdh_pc_apply(c, r, z));
  CHK(comm_halo(c, z));
  if (lean_keep_qu(c) && !c->prof_on) return k_spmv_full_kept(c, z, w, c->qu.p);
  return k_spmv_full(c, z, w);
}

// leading dimension of the Krylov and guess vectors: even, so that every V_j / Z_j / U_j stays 16-B aligned
static size_t krylov_ld(const cfdh_ctx *c) { return ((size_t)c->NL + 1) & ~(size_t)1; }

int cfdh_apply_operator_dev(cfdh_ctx *c, const double *r, double *z) {
  CHK(ensure_krylov(c));
  return pc_then_product(c, r, z, c->kw.p);
}

int ensure_krylov(cfdh_ctx *c) {
  const int m = c->opt.ksp_restart;
  if (c->kry_m == m && c->kV.p) return 0;
  const size_t NL = krylov_ld(c);
  c->pc_graph_valid = false;  // captured graphs hold pointers into V / Z
  HIPCHK(c, c->kV.alloc(NL * (m + 1)));
  HIPCHK(c, c->kZ.alloc(NL * m));
  HIPCHK(c, c->kw.alloc(NL));
  // kh also serves guess_project as the scratch of its Gram system: 8 (k + 1) doubles with k <= 8 kept vectors (the cap of
  // cfdh_set_options), whatever the restart length
  HIPCHK(c, c->kh.alloc(std::max(2 * (size_t)(m + 2) + 8, (size_t)8 * (8 + 1))));
  HIPCHK(c, c->ky.alloc(m + 8));
  // read-back ring of the iterations in flight: host-mapped slots of [h_0 .. h_j, w.w, measured norm] and one event each
  if (c->h_ring) { (void)hipHostFree(c->h_ring); c->h_ring = nullptr; }
  c->h_ring_stride = ((size_t)m + 5) & ~(size_t)1;
  HIPCHK(c, hipHostMalloc((void **)&c->h_ring, sizeof(double) * c->h_ring_stride * (cfdh_ctx::KRING + 1)));  // + one slot: staging of y
  HIPCHK(c, hipHostGetDevicePointer((void **)&c->h_ring_dev, c->h_ring, 0));
  for (auto &e : c->ev_ring) if (!e) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  HIPCHK(c, c->kV.zero(c->stream)); HIPCHK(c, c->kZ.zero(c->stream)); HIPCHK(c, c->kw.zero(c->stream));
  if ((size_t)(m + 2) * 1024 > c->red_partial.n) HIPCHK(c, c->red_partial.alloc((size_t)(m + 2) * 1024 + 1024));
  c->kry_m = m;
  return 0;
}

// ---- projected initial guess (cfdh_options.ksp_guess; PETSc's KSPGuess of Fischer type, with the CURRENT matrix) ----------
// The sequence of linear systems of a time-stepping run is smooth in time: the k-th Newton update of step n+1 is close to
// the k-th update of step n.  U = the last few solutions of solves with the same Newton index; W = J U (one SpMV each);
// x0 = U y with y = argmin |b - W y| from the normal equations (at most 8 x 8, solved on the host with a pivoted Cholesky that
// drops directions which have become numerically dependent).  |b - J x0| <= |b| by construction, so a bad history can only
// cost the SpMVs.  The Krylov workspace is free before the first cycle: V_1.. hold the halo-extended copies, Z_0.. hold W.
static int guess_ensure(cfdh_ctx *c) {
  const int m = c->opt.ksp_guess;
  const size_t ld = krylov_ld(c);
  if (m == c->guess_m && (m == 0 || c->guessU.p)) return 0;
  c->guess_m = m;
  for (int k = 0; k < cfdh_ctx::GUESS_NEWTON; k++) c->guess_cnt[k] = c->guess_head[k] = 0;
  if (m > 0) {
    HIPCHK(c, c->guessU.alloc(ld * (size_t)m * cfdh_ctx::GUESS_NEWTON)); HIPCHK(c, c->guessU.zero(c->stream));
    HIPCHK(c, c->guessX.alloc(ld * (size_t)cfdh_ctx::GUESS_NEWTON));
  }
  return 0;
}

// the solve in progress belongs to a ring of kept solutions (a Newton index below GUESS_NEWTON, with ksp_guess on)
static bool guess_ring_valid(const cfdh_ctx *c) {
  return c->guess_m > 0 && c->guess_slot >= 0 && c->guess_slot < cfdh_ctx::GUESS_NEWTON;
}
// kept vectors the projection of this solve can use (0: none, or the Krylov workspace is too small to hold their products)
static int guess_usable(const cfdh_ctx *c) {
  return (guess_ring_valid(c) && c->kry_m >= c->guess_m + 1) ? c->guess_cnt[c->guess_slot] : 0;
}
// iterations of the last solve with the same Newton index: the expected length of this one (0: unknown)
static int guess_expected_its(const cfdh_ctx *c) {
  return (c->guess_slot >= 0 && c->guess_slot < cfdh_ctx::GUESS_NEWTON) ? c->guess_last_its[c->guess_slot] : 0;
}

static int guess_project(cfdh_ctx *c, const double *b, double *x, bool *used) {
  *used = false;
  CHK(guess_ensure(c));
  const int k = guess_usable(c), n = c->NO;
  if (k == 0) return 0;
  const size_t ld = krylov_ld(c);
  double *U = c->guessU.p + ld * (size_t)c->guess_m * c->guess_slot;  // the ring of this Newton index (order is irrelevant to the projection)
  double *V = c->kV.p, *Z = c->kZ.p, *hd = c->kh.p;
  if (c->nranks > 1) {  // halo-extended copies in V_1.. (the kept vectors hold owned entries only)
    for (int i = 0; i < k; i++) {
      double *t = V + (size_t)(i + 1) * ld;
      CHK(v_copy(c, n, U + (size_t)i * ld, t));
      CHK(comm_halo(c, t));
    }
    CHK(k_spmv_full_multi(c, V + ld, Z, (int)ld, k));
  } else {
    CHK(k_spmv_full_multi(c, U, Z, (int)ld, k));  // one pass over the Jacobian for all kept vectors
  }
  // Gram system: hd[8 i + q] = W_q . W_i, hd[8 k + q] = W_q . b
  HIPCHK(c, hipMemsetAsync(hd, 0, sizeof(double) * 8 * (size_t)(k + 1), c->stream));
  CHK(v_gram(c, n, Z, (int)ld, k, b, hd));  // one pass over W and b, ONE read-back
  CHK(comm_allreduce_dev(c, hd, 8 * (k + 1), 0));  // ONE reduction over the ranks for the whole Gram system
  double gram[8 * 9];
  CHK(scalars_read(c, ScalarRead{hd, 8 * (k + 1), false}, gram));
  c->n_guess_projections++;
  if (c->opt.verbose > 1) {
    double bb = 0.0;
    CHK(v_norm2(c, n, b, &bb));
    fprintf(stderr, "[cfdh]     guess diag (newton %d): cos(W_i, b) =", c->guess_slot);
    for (int i = 0; i < k; i++) fprintf(stderr, " %.6f", gram[8 * k + i] / (std::sqrt(gram[9 * i]) * bb));
    fprintf(stderr, "; |W_i|/|b| =");
    for (int i = 0; i < k; i++) fprintf(stderr, " %.4f", std::sqrt(gram[9 * i]) / bb);
    fprintf(stderr, "\n");
  }
  double y[8];
  int rank = 0;
  const bool ok = cfdh_krylov::gram_solve(k, gram, y, &rank);
  c->guess_last_rank = rank; c->guess_last_k = k;
  if (!ok) return 0;
  // y travels through the pinned slot behind the read-back ring, as at the end of a cycle: no drain of the stream for a host
  // temporary (the slot is next written at the end of the first cycle, behind events recorded after this copy)
  double *ystage = c->h_ring + c->h_ring_stride * cfdh_ctx::KRING;
  for (int i = 0; i < k; i++) ystage[i] = y[i];
  HIPCHK(c, hipMemcpyAsync(c->ky.p, ystage, sizeof(double) * k, hipMemcpyHostToDevice, c->stream));
  CHK(v_lincomb(c, n, U, (int)ld, k, c->ky.p, x));  // x (zeroed by the caller) += U y
  // singular system: the guess, like every preconditioned vector, carries no constant-pressure component (the Krylov vectors
  // cannot remove one, and through the kept corrections it would feed back from step to step)
  if (c->singular) CHK(v_sub_mean(c, c->nvo, x + (size_t)c->dim * c->nvo));
  // r0 = b - J x0 = b - W y without another product (the true residual is formed after every cycle anyway)
  CHK(v_copy(c, n, b, V));
  CHK(v_multiaxpy(c, n, Z, (int)ld, k, c->ky.p, V));
  *used = true;
  return 0;
}

// The same projection on the lean path (one rank): the Gram system is solved on the device, ONE kernel then reads U, W and b once
// and writes x0 = U y, r0 = b - W y (into V_0) and the partial sums of |r0|^2 -- no zero-fill of x, no copy of b, two passes less
// over the kept vectors, and nothing is read back here: the caller reads |r0| and the "used" flag in one go (v_guess_read).
// *ran: the kernels were launched (x and V_0 are fully written, with y = 0 when the guess turns out unusable).
// Singular system: as on the general path, the mean pressure is removed from x0 after the combination and r0 stays b - W y.
static int guess_project_lean(cfdh_ctx *c, const double *b, double *x, bool *ran) {
  *ran = false;
  CHK(guess_ensure(c));
  const int k = guess_usable(c), n = c->NO;
  if (k == 0) return 0;
  const size_t ld = krylov_ld(c);
  double *U = c->guessU.p + ld * (size_t)c->guess_m * c->guess_slot;
  CHK(k_spmv_full_multi(c, U, c->kZ.p, (int)ld, k));
  CHK(v_gram(c, n, c->kZ.p, (int)ld, k, b, c->kh.p));  // every word the solve reads is written: no memset
  CHK(v_guess_combine(c, n, U, c->kZ.p, (int)ld, k, c->kh.p, b, x, c->kV.p));
  if (c->singular) CHK(v_sub_mean(c, c->nvo, x + (size_t)c->dim * c->nvo));
  c->n_guess_projections++;
  *ran = true;
  return 0;
}

// where guess_store would put the solution of the solve in progress (nullptr: nothing is kept)
// only while the ring of this Newton index is not full: then the slot is free, and a solve that fails after all has overwritten
// nothing.  In a full ring the slot holds the oldest live vector, which must survive a failed solve: guess_store copies.
static double *guess_store_target(cfdh_ctx *c) {
  const int slot = c->guess_slot, m = c->guess_m;
  if (!guess_ring_valid(c) || !c->guessU.p || c->guess_cnt[slot] >= m) return nullptr;
  const size_t ld = krylov_ld(c);
  return c->guessU.p + ld * (size_t)m * slot + (size_t)c->guess_head[slot] * ld;
}

// keep the solution of a converged solve for the guesses of later time steps (in_place: the last update of x wrote the copy already)
static int guess_store(cfdh_ctx *c, const double *x, bool in_place = false) {
  const int slot = c->guess_slot, m = c->guess_m;
  if (!guess_ring_valid(c)) return 0;
  const size_t ld = krylov_ld(c);
  double *U = c->guessU.p + ld * (size_t)m * slot;
  if (!in_place) CHK(v_copy(c, c->NO, x, U + (size_t)c->guess_head[slot] * ld));
  c->guess_stored[slot] = true;
  c->guess_head[slot] = (c->guess_head[slot] + 1) % m;
  if (c->guess_cnt[slot] < m) c->guess_cnt[slot]++;
  return 0;
}

// At the end of a converged step the kept solutions are replaced by what the solves were approximating: the remaining Newton
// correction x_k - x_final (J_k d = F(x_k), x_final = x_k - d up to the quadratic remainder).  The linear solves stop at
// rtol 1e-5; x_final is converged to snes_rtol, so the kept vectors lose the solver noise that otherwise bounds the quality of
// the next steps' projections at ~1e-4.
static int guess_refine(cfdh_ctx *c, int newton_its, const double *x_final) {
  const int m = c->guess_m;
  if (m <= 0 || !c->guessX.p) return 0;
  const size_t ld = krylov_ld(c);
  for (int k = 0; k < newton_its && k < cfdh_ctx::GUESS_NEWTON; k++) {
    if (!c->guess_stored[k]) continue;
    double *U = c->guessU.p + ld * (size_t)m * k;
    const int latest = (c->guess_head[k] + m - 1) % m;
    CHK(v_waxpy(c, c->NO, -1.0, x_final, c->guessX.p + (size_t)k * ld, U + (size_t)latest * ld));
  }
  return 0;
}

// ---- FGMRES ----------------------------------------------------------------------------------------------------------------
// Where V_0 of the next cycle comes from.
enum class V0From {
  rhs,           // zero guess: r0 = b, v_0 = b / |b| is formed straight from b
  guess,         // projected guess, general path: V_0 holds r0 = b - W y, unscaled
  guess_scaled,  // projected guess, lean path: V_0 = r0 / |r0| already, scaled on the device ahead of the read-back
  residual       // after a cycle: the true residual b - J x is formed and its norm read back
};
enum class Between { proceed, retry, stop };  // what the checks between two cycles decide

// State of one solve.
struct Fgmres {
  cfdh_ctx *c;
  const double *b;
  double *x;
  int n, m;
  size_t ld, ld32;
  double bn = 0.0, tol = 0.0;  // |b|, absolute tolerance
  // Long cycles at the default tolerance orthogonalise against an fp32 COPY of the basis (half the traffic of the two passes over
  // V, which are ~40 % of an iteration at depth 25).  Chosen per solve from the length of the last solve with the same Newton
  // index; never for tolerances below 1e-6 (parity runs), never again on a context whose watchdog tripped with the copy in use.
  // CFDH_KRYLOV_FP32 = 0: never, 2: always (where the tolerance allows).
  bool use32 = false;
  bool lean = false;  // lean prologue and epilogue (not with the fp32 copy of the basis, which keeps the general path)
  float *V32 = nullptr;
  int e_its = 0;  // expected length of this solve: the last solve with the same Newton index took that many iterations (0: unknown)
  cfdh_krylov::ArnoldiLsq lsq;
  // [0, m]: Gram-Schmidt coefficients of the iteration being processed; from HH2_AT(m): the m + 4 words a second pass reads back
  static constexpr size_t HH2_AT(int m) { return (size_t)m + 1; }
  static constexpr size_t HH_WORDS(int m) { return HH2_AT(m) + (size_t)m + 4; }
  std::vector<double> hh;
  int its = 0, reason = 0;
  int j_prev = 0;             // length of the last cycle
  bool converged = false;     // the last cycle ended with the recurrence below the tolerance
  double est_prev = 0.0;      // residual estimate at the end of the last cycle
  double beta_start = 0.0;    // true residual at its start
  double last_true = -1.0;    // true residual at the last disagreement between recurrence and true residual
  bool kept_copy = false;     // the copy guess_store makes is current (written by the last update of x)
  FgmresTrace *tr = nullptr;  // cfdh_fgmres_solve only
  Fgmres(cfdh_ctx *c_, const double *b_, double *x_)
      : c(c_), b(b_), x(x_), n(c_->NO), m(c_->kry_m), ld(krylov_ld(c_)), ld32((ld + 3) & ~(size_t)3),  // columns of the copy start on 16-B boundaries (float4 loads)
        lsq(c_->kry_m), hh(HH_WORDS(c_->kry_m)) {}
};

// Start of a solve on both paths: x0 (zero or the projected guess), |b|, the tolerance, and V_0 = r0 with its norm *beta when a
// guess is used.  s.reason != 0 on return: |b| is zero or not finite, nothing to iterate.
static int fgmres_start(Fgmres &s, double bnorm, V0From *src, double *beta) {
  cfdh_ctx *c = s.c;
  const cfdh_options &o = c->opt;
  const int n = s.n;
  double *V = c->kV.p;
  s.e_its = guess_expected_its(c);
  // In a partitioned run the copy costs one more all-reduce per iteration (the measured norm) and saves 1/nranks of the traffic it
  // saves on one GPU: taken only where a rank still holds >= 2 M unknowns (decided from the GLOBAL count: the same on every rank).
  const bool worth32 = c->nranks <= 1 || (c->nvo_global / c->nranks) * (c->dim + 1) >= 2.0e6;
  const int fp32_env = c->env.krylov_fp32;
  s.use32 = fp32_env > 0 && o.ksp_rtol >= 1e-6 && c->krylov_fp32_ok && ((s.e_its >= 20 && worth32) || fp32_env >= 2);
  s.lean = lean_scope(c) && !s.use32;
  double bn = bnorm;  // the caller may know |b| already (Newton: |F| of the accepted iterate)
  // prologue on the lean path: launched whole before anything is read back; needs |b| from the caller (Newton passes it)
  bool pro = false;
  if (s.lean && bn > 0.0 && std::isfinite(bn)) CHK(guess_project_lean(c, s.b, s.x, &pro));
  if (!pro) CHK(v_zero(c, c->NL, s.x));
  if (!(bn >= 0.0)) CHK(v_norm2(c, n, s.b, &bn));
  s.bn = bn;
  c->ksp_last_relres = bn == 0.0 ? 0.0 : 1.0;
  if (!std::isfinite(bn)) { s.reason = -9; return 0; }
  if (bn == 0.0) { s.reason = 2; return 0; }
  s.tol = std::max(o.ksp_rtol * bn, o.ksp_atol);
  const bool check = c->env.guess_check;
  bool guessed = false;
  *src = V0From::guess;
  if (pro) {
    // V_0 is normalised by a kernel that reads |r0|^2 on the device: it is queued BEFORE the read-back, so the device does not
    // idle while the host wakes up (the check hook below wants the unscaled vector: it scales afterwards)
    if (!check) { CHK(v_scale_inv_lean(c, n, V)); *src = V0From::guess_scaled; }
    int rank = 0;
    double y[8];
    CHK(v_guess_read(c, c->guess_cnt[c->guess_slot], beta, &guessed, &rank, y));
    c->guess_last_rank = rank; c->guess_last_k = c->guess_cnt[c->guess_slot];
    if (!guessed) CHK(v_zero(c, c->NL, s.x));  // rank 0 or non-finite coefficients: zero guess (the kernel wrote 0 U; a NaN in U must not survive)
  } else {
    CHK(guess_project(c, s.b, s.x, &guessed));
  }
  if (s.use32) {
    if (c->kV32.n < s.ld32 * (size_t)(s.m + 1)) HIPCHK(c, c->kV32.alloc(s.ld32 * (size_t)(s.m + 1)));
    s.V32 = c->kV32.p;
  }
  if (!guessed) { *src = V0From::rhs; *beta = bn; s.beta_start = bn; return 0; }
  // the cycle starts from the true residual of x0, as after a restart
  if (check) {
    // test hook: the residual assembled from the multi-vector product must be the true residual of x0
    double diff = 0.0, *w = c->kw.p;
    CHK(comm_halo(c, s.x));
    CHK(k_spmv_full(c, s.x, w));
    CHK(v_waxpy(c, n, -1.0, w, s.b, w));   // w = b - J x0
    CHK(v_waxpy(c, n, -1.0, V, w, w));     // w -= V_0
    CHK(v_norm2(c, n, w, &diff));
    if (!(diff <= 1e-10 * bn)) return cfdh_fail(c, CFDH_E_STATE, "projected guess: |(b - J x0) - (b - W y)| = %.3e |b|", diff / bn);
  }
  if (!pro) CHK(v_norm2(c, n, V, beta));  // (the lean path read it back with the "used" flag)
  c->n_guess_solves++; c->guess_reduction_sum += *beta / bn;
  if (o.verbose) fprintf(stderr, "[cfdh]     projected guess (newton %d, %d vectors): |r0| / |b| = %.3e\n", c->guess_slot, c->guess_cnt[c->guess_slot], *beta / bn);
  s.beta_start = *beta;
  return 0;
}

// True residual at a restart: V_0 = b - J x and its norm.
static int fgmres_true_residual(Fgmres &s, double *beta) {
  cfdh_ctx *c = s.c;
  double *V = c->kV.p, *w = c->kw.p;
  bool have_beta = false;
  CHK(comm_halo(c, s.x));
  // lean path: product, b - J x and the first pass of the norm in one kernel, one read-back (not while the kernel timers run:
  // they count the plain product)
  if (s.lean && !c->prof_on) CHK(k_resid_norm(c, s.x, s.b, V, beta, &have_beta));
  if (!have_beta) {
    CHK(k_spmv_full(c, s.x, w));
    CHK(v_waxpy(c, s.n, -1.0, w, s.b, V));
    CHK(v_norm2(c, s.n, V, beta));
  }
  c->n_cycles++;
  c->ksp_last_relres = *beta / s.bn;
  return 0;
}

// The checks between two cycles, on the true residual beta formed after the last one.
static int fgmres_between_cycles(Fgmres &s, double beta, Between *next) {
  cfdh_ctx *c = s.c;
  const cfdh_options &o = c->opt;
  const double tol = s.tol, est_prev = s.est_prev;
  const int j_prev = s.j_prev;
  *next = Between::proceed;
  // Orthogonality watchdog.  Unrefined classical Gram-Schmidt (PETSc's default) can lose the basis in a long cycle:
  // the recurrence then reports convergence while the true residual, formed here after every cycle anyway, does not
  // follow.  Once that is seen on a context, long cycles are re-orthogonalised (DGKS) from then on, and a cycle that
  // made the residual worse is taken back.
  const cfdh_krylov::BetweenCycles d = cfdh_krylov::between_cycles(j_prev, beta, est_prev, tol, s.bn, s.beta_start, s.last_true, s.use32,
                                                                   c->gs_refine_long, c->env.no_attainable_stop != 0);
  if (d.watchdog == cfdh_krylov::BetweenWatchdog::fp32_off) {
    // the fp32 copy is the first suspect: this solve and all later ones of the context go back to the fp64 basis
    s.use32 = false; c->krylov_fp32_ok = false;
    if (o.verbose) fprintf(stderr, "[cfdh]     fgmres: true residual %.3e vs recurrence %.3e after a %d-vector cycle with the fp32 basis copy: switched off\n", beta, est_prev, j_prev);
  } else if (d.watchdog == cfdh_krylov::BetweenWatchdog::refine_on) {
    c->gs_refine_long = true;
    if (o.verbose) fprintf(stderr, "[cfdh]     fgmres: true residual %.3e vs recurrence %.3e after a %d-vector cycle: re-orthogonalising long cycles from now on\n", beta, est_prev, j_prev);
    if (d.flow == cfdh_krylov::BetweenFlow::retry) {
      std::vector<double> &y = s.lsq.y;
      for (int i = 0; i < j_prev; i++) y[i] = -y[i];
      HIPCHK(c, hipMemcpyAsync(c->ky.p, y.data(), sizeof(double) * j_prev, hipMemcpyHostToDevice, c->stream));
      CHK(v_lincomb(c, s.n, c->kZ.p, (int)s.ld, j_prev, c->ky.p, s.x));
      s.kept_copy = false;
      HIPCHK(c, hipStreamSynchronize(c->stream));
      s.est_prev = s.beta_start;  // do not trip again on the restored iterate
      *next = Between::retry;
      return 0;
    }
  }
  // Attainable accuracy.  The convergence test of a cycle is the recurrence norm (as in PETSc, which never looks further);
  // here the true residual is formed after every cycle and another cycle follows if it disagrees.  When a second cycle
  // in a row ends "converged" by the recurrence without halving the true residual, that residual is the floor of this
  // system (rounding level of J x, or the component of b outside the range of a singular Jacobian: lid cavity at
  // ksp_rtol 1e-10) and the iteration stops instead of spending ksp_max_it on it.
  // The stop is bounded and reported as what it is: it applies only within 10x the tolerance or once the residual is six
  // orders below |b| (beyond what the reference's rtol = 1e-5 ever asks for); anything else runs on to ksp_max_it and fails
  // like PETSc's DIVERGED_ITS.  It returns its own reason code (CFDH_KSP_CONVERGED_ATTAINABLE) and is counted
  // (cfdh_info 72).  CFDH_NO_ATTAINABLE_STOP=1 disables it.
  // (the decision itself: cfdh_krylov::between_cycles, tested on the CPU)
  s.last_true = d.last_true;
  if (d.flow == cfdh_krylov::BetweenFlow::stop) {
    if (o.verbose) fprintf(stderr, "[cfdh]     fgmres: true residual %.3e stays above the tolerance %.3e although the recurrence converged twice: attainable accuracy, stopping\n", beta, tol);
    s.reason = CFDH_KSP_CONVERGED_ATTAINABLE;
    c->n_attainable_stops++;
    *next = Between::stop;
    return 0;
  }
  s.beta_start = beta;
  return 0;
}

// cfdh_fgmres_solve only: the iterate before the first cycle
static int trace_solve_start(Fgmres &s, bool guessed) {
  FgmresTrace *t = s.tr;
  cfdh_ctx *c = s.c;
  t->m = s.m; t->cycles = 0; t->k = 0;
  t->guess_used = guessed; t->fp32_used = false;
  t->bn = s.bn; t->tol = s.tol; t->beta = 0.0;
  t->H.assign((size_t)(s.m + 1) * s.m, 0.0);
  t->ww.assign(s.m, 0.0); t->nrm2.assign(s.m, 0.0); t->second_pass.assign(s.m, 0);
  t->y.clear(); t->res.clear(); t->cycle_beta.clear(); t->cycle_est.clear();
  HIPCHK(c, t->x0.alloc(c->NL)); HIPCHK(c, t->x_start.alloc(c->NL)); HIPCHK(c, t->v0.alloc(c->NL));
  HIPCHK(c, t->v0.zero(c->stream));
  HIPCHK(c, hipMemcpyAsync(t->x0.p, s.x, sizeof(double) * c->NL, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(t->x_start.p, s.x, sizeof(double) * c->NL, hipMemcpyDeviceToDevice, c->stream));
  return 0;
}
// ... and at the start of a cycle: the iterate, and V_0 before the next true residual overwrites it
static int trace_cycle_start(Fgmres &s, double beta) {
  FgmresTrace *t = s.tr;
  cfdh_ctx *c = s.c;
  t->cycles++; t->k = 0; t->beta = beta; t->fp32_used = s.use32;
  t->cycle_beta.push_back(beta);
  std::fill(t->H.begin(), t->H.end(), 0.0);
  std::fill(t->ww.begin(), t->ww.end(), 0.0); std::fill(t->nrm2.begin(), t->nrm2.end(), 0.0);
  std::fill(t->second_pass.begin(), t->second_pass.end(), 0);
  t->y.clear();
  HIPCHK(c, hipMemcpyAsync(t->x_start.p, s.x, sizeof(double) * c->NL, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(t->v0.p, c->kV.p, sizeof(double) * s.n, hipMemcpyDeviceToDevice, c->stream));
  return 0;
}

// Launch of iteration jj: z_jj = P^-1 v_jj, w = J z_jj, one Gram-Schmidt pass against V_0..V_jj into V_jj+1; the coefficients
// [h_0 .. h_jj, w.w, (measured norm)] land in the iteration's slot of the host-mapped ring, behind its event.
static int fgmres_launch(Fgmres &s, int jj) {
  cfdh_ctx *c = s.c;
  const int n = s.n, m = s.m;
  const size_t ld = s.ld, ld32 = s.ld32;
  double *V = c->kV.p, *w = c->kw.p, *hd = c->kh.p, *s_dev = hd + 2 * (m + 2) + 1;
  double *vj = V + (size_t)jj * ld, *zj = c->kZ.p + (size_t)jj * ld, *vn = V + (size_t)(jj + 1) * ld;
  double *slot = c->h_ring_dev + (size_t)(jj % cfdh_ctx::KRING) * c->h_ring_stride;
  CHK(pc_then_product(c, vj, zj, w));
  // classical Gram-Schmidt (PETSc's default for (F)GMRES): h = [V^T w ; w.w] comes from ONE fused multi-dot
  if (s.use32) {
    // the same Gram-Schmidt step against the fp32 copy: h = V32^T w, v_{j+1} = (w - V32 h) / |w - V32 h| with the norm
    // MEASURED (the identity below needs columns that are orthonormal to round-off); both the fp64 vector (input of the
    // next preconditioner application) and its fp32 copy are written
    CHK(v_multidot32(c, n, s.V32, (int)ld32, jj + 1, w, hd, slot));
    CHK(v_gs_update32(c, n, s.V32, (int)ld32, jj + 1, hd, w, vn, s.V32 + (size_t)(jj + 1) * ld32, s_dev, slot + (jj + 2)));
    HIPCHK(c, hipEventRecord(c->ev_ring[jj % cfdh_ctx::KRING], c->stream));
  } else {
    CHK(v_multidot(c, n, V, (int)ld, jj + 1, w, hd, true, slot));
    // h (all-reduced in a partitioned run) sits in the host-mapped slot: the event marks THAT; the update of w below
    // overlaps with the host's Hessenberg bookkeeping and the next launches
    HIPCHK(c, hipEventRecord(c->ev_ring[jj % cfdh_ctx::KRING], c->stream));
    // v_{j+1} = (w - V h) / s with s = sqrt(w.w - |h|^2) formed on the device from the reduced coefficients: update and
    // normalisation in one pass (the host forms the same norm for the Hessenberg matrix from its copy of h)
    CHK(v_gs_update_normalize(c, n, V, (int)ld, jj + 1, hd, w, vn, s_dev));
  }
  return 0;
}

// Second Gram-Schmidt pass on the (already scaled) vector of iteration j: vn = w'/s  ->  h2 = V^T vn, vn -= V h2, vn /= |vn|;
// in terms of w: h += s h2 (into s.hh), |w''| = s |vn| (into *hnorm).  The coefficients and the squared norm of the corrected vector
// travel in ONE reduction over the ranks: [h2 ; vn.vn] from one fused multi-dot, |vn - V h2|^2 = vn.vn - |h2|^2 (the basis is
// orthonormal to round-off here -- the fp32 copy measures its norm instead).  hs: the iteration's ring slot.
static int fgmres_second_pass(Fgmres &s, int j, const double *hs, double ww, double hh2, double *hnorm) {
  cfdh_ctx *c = s.c;
  const int n = s.n, m = s.m;
  double *V = c->kV.p, *hd = c->kh.p, *vn = V + (size_t)(j + 1) * s.ld;
  CHK(v_multidot(c, n, V, (int)s.ld, j + 1, vn, hd + (m + 2), true));
  CHK(v_multiaxpy(c, n, V, (int)s.ld, j + 1, hd + (m + 2), vn));
  if (s.use32) CHK(v_norm_to_dev(c, n, vn, hd + 2 * (m + 2)));
  double *h2 = s.hh.data() + Fgmres::HH2_AT(m);
  CHK(scalars_read(c, ScalarRead{hd + (m + 2), m + 4, false}, h2));
  c->n_iter_sync++;
  // scale of the first pass, formed by the function gs_update_normalize_kernel forms it with (the device word s_dev may belong to
  // an iteration that ran ahead by now); the fp32 path measured it: slot word j + 2
  const double sc = s.use32 ? hs[j + 2] : cfdh_krylov::gs_scale(ww, hh2);
  double h22 = 0.0;
  for (int i = 0; i <= j; i++) { s.hh[i] += sc * h2[i]; h22 += h2[i] * h2[i]; }
  double vnorm;
  if (s.use32) vnorm = h2[m + 2];
  else {
    const double d2 = h2[j + 1] - h22;
    vnorm = d2 > 0.0 ? std::sqrt(d2) : 0.0;
  }
  *hnorm = sc * vnorm;
  if (s.use32) { CHK(v_scale_inv_dev(c, n, vn, hd + 2 * (m + 2), vn)); CHK(v_store32(c, n, vn, s.V32 + (size_t)(j + 1) * s.ld32)); }
  else CHK(v_scale(c, n, vnorm > 0.0 ? 1.0 / vnorm : 0.0, vn));
  return 0;
}

// One cycle from V_0 of norm beta.  The device needs nothing from the host to go from one iteration to the next (the Gram-Schmidt
// update forms its own scale from the reduced coefficients), so iterations are LAUNCHED ahead of the host's bookkeeping: every
// iteration in flight publishes [h_0..h_j, w.w, (measured norm)] into its own slot of a host-mapped ring behind an event, and the
// host catches up -- Hessenberg column, Givens rotation, convergence test -- in batches, always leaving one iteration running so
// that the GPU never waits for the host.  How far to run ahead follows from the convergence rate seen so far (iterations the
// tolerance is still away at the current contraction factor, at most KRING - 3): an iteration launched beyond the one that
// converges is discarded (x uses the columns up to convergence only) and counted (cfdh_info 73).  Solves that decide a second
// Gram-Schmidt pass per vector (ksp_rtol < 1e-7, long cycles after the watchdog tripped) stay synchronous; the rare
// cancellation case (|w'|^2 < 1e-2 |w|^2) refines the vector when the host sees it and re-launches what ran ahead of it.
// On return s.j_prev is the number of columns of this cycle; s.reason = -9 on breakdown.
static int fgmres_cycle(Fgmres &s, double beta) {
  cfdh_ctx *c = s.c;
  const cfdh_options &o = c->opt;
  const int refine_from = c->env.gs_refine_from >= 0 ? c->env.gs_refine_from : (c->gs_refine_long ? 24 : (1 << 30));
  const int lagmax = (o.ksp_rtol < 1e-7 || c->prof_on) ? 0 : std::max(0, std::min(c->env.ksp_lag, cfdh_ctx::KRING - 3));
  const int maxl = std::min(s.m, o.ksp_max_it - s.its);  // iterations this cycle may run
  int j = 0;    // iterations processed by the host (complete Hessenberg columns)
  int jl = 0;   // iterations launched
  cfdh_krylov::LaunchAhead ahead;
  ahead.start(beta, s.e_its, s.its);
  s.lsq.start(beta);
  s.converged = false;
  double *hh = s.hh.data();
  while (!s.converged && s.reason == 0) {
    // launch: one iteration beyond the batch the host will process next stays in flight, unless the batch is predicted to
    // contain the converging iteration
    const bool sync_now = lagmax == 0 || j >= refine_from;
    const int want = ahead.in_flight(sync_now, lagmax);
    while (jl < maxl && jl - j < want) { CHK(fgmres_launch(s, jl)); jl++; }
    if (jl == j) break;  // cycle full (restart) or iteration cap
    int upto = ahead.process_upto(j, jl, maxl, sync_now);
    c->n_host_sync++; c->n_iter_sync++;
    HIPCHK(c, hipEventSynchronize(c->ev_ring[(upto - 1) % cfdh_ctx::KRING]));
    while (j < upto) {
      const double *hs = c->h_ring + (size_t)(j % cfdh_ctx::KRING) * c->h_ring_stride;
      double ww = hs[j + 1], hh2 = 0.0;
      for (int i = 0; i <= j; i++) { hh[i] = hs[i]; hh2 += hh[i] * hh[i]; }
      const double nrm2 = s.use32 ? hs[j + 2] * hs[j + 2] : ww - hh2;
      // PETSc's default never refines.  Here: tolerances down to ~1e-7 refine only when two digits
      // cancel; tighter solves (parity runs at 1e-10) use the DGKS criterion (|w'| < |w|/sqrt(2)),
      // because classical Gram-Schmidt then loses the orthogonality the deep convergence needs
      // ... and so can a long Krylov cycle: beyond ~two dozen vectors the unrefined basis may drift far enough from
      // orthogonality that the least-squares solution picks up huge spurious components (Newton corrections ten times
      // the size of the iterate on the tree domain, config 5) although the residual norm looks converged.  Paying the
      // second pass on every long cycle costs 14 % of a 3-D step whose 47-vector cycles never need it, so it is switched
      // on by the watchdog (CFDH_GS_REFINE_FROM=<j> forces it from vector j on)
      // (at the reference's tolerance: only when three digits cancel -- one classical pass then leaves an orthogonality
      // error of ~1e3 eps, far below rtol 1e-5.  With a good preconditioner w = J M^-1 v_j is close to v_j, so a threshold of
      // 1e-2 -- rounds 2 and 3 -- sent a third of all iterations of the headline run through the second pass for nothing.)
      const double eta2 = (o.ksp_rtol < 1e-7 || j >= refine_from) ? 0.5 : c->env.gs_eta2;
      double hnorm = std::sqrt(nrm2);
      int refined = 0;
      if (!(nrm2 > eta2 * ww)) {
        // what ran ahead used the unrefined vector: it is launched again, and its ring slots are not consumed by this batch
        refined = jl > j + 1 ? 2 : 1;
        if (jl > j + 1) { c->n_krylov_discarded += jl - (j + 1); jl = j + 1; upto = jl; }
        CHK(fgmres_second_pass(s, j, hs, ww, hh2, &hnorm));
      }
      if (s.tr) {
        double *Hj = &s.tr->H[(size_t)j * (s.m + 1)];
        for (int i = 0; i <= j; i++) Hj[i] = hh[i];
        Hj[j + 1] = hnorm;
        s.tr->ww[j] = ww; s.tr->nrm2[j] = nrm2; s.tr->second_pass[j] = refined;
      }
      const bool ok = s.lsq.add_column(j, hh, hnorm);
      j++;
      if (!ok) { s.reason = -9; break; }
      s.its++;
      const double res = s.lsq.residual(j);
      if (s.tr) s.tr->res.push_back(res);
      if (o.verbose > 1) fprintf(stderr, "[cfdh]     fgmres %3d  |r|/|b| = %.3e\n", s.its, res / s.bn);
      if (res <= s.tol) { s.converged = true; break; }
      ahead.observe(res, s.tol, s.its);
    }
  }
  if (jl > j) c->n_krylov_discarded += jl - j;  // launched ahead of the converging iteration: not part of the solution
  s.j_prev = j;
  return 0;
}

// x += Z y with y = H^-1 g of the cycle that has just ended.
static int fgmres_update_x(Fgmres &s) {
  cfdh_ctx *c = s.c;
  const int j = s.j_prev;
  const double *y = s.lsq.solve(j);
  // y travels through a pinned slot behind the ring (no stream synchronisation: the slot is rewritten at the end of the next
  // cycle at the earliest, after events recorded behind this copy have been waited for)
  double *ystage = c->h_ring + c->h_ring_stride * cfdh_ctx::KRING;
  for (int i = 0; i < j; i++) ystage[i] = y[i];
  HIPCHK(c, hipMemcpyAsync(c->ky.p, ystage, sizeof(double) * j, hipMemcpyHostToDevice, c->stream));
  // lean path: the update of a cycle that converged by the recurrence also writes the copy guess_store would make (a second
  // store instead of a pass over x) where that slot is free; any other update of x leaves the copy to guess_store
  double *keep = (s.lean && s.converged && s.its < c->opt.ksp_max_it) ? guess_store_target(c) : nullptr;
  if (keep) CHK(v_lincomb_keep(c, s.n, c->kZ.p, (int)s.ld, j, c->ky.p, s.x, keep));
  else CHK(v_lincomb(c, s.n, c->kZ.p, (int)s.ld, j, c->ky.p, s.x));
  s.kept_copy = keep != nullptr;
  s.est_prev = s.lsq.residual(j);
  if (s.tr) { s.tr->y.assign(y, y + j); s.tr->k = j; s.tr->cycle_est.push_back(s.est_prev); }
  return 0;
}

// Solve J x = b, x0 = 0 or the projected guess.  Right preconditioning, convergence on the true
// residual norm relative to |b| (KSP defaults: rtol, atol; KSP_NORM_UNPRECONDITIONED
// for FGMRES).  Classical Gram-Schmidt with one re-orthogonalisation pass; the
// 2j+3 scalars of an iteration come back in a single read.
int cfdh_fgmres(cfdh_ctx *c, const double *b, double *x, int *its_out, int *reason_out, double bnorm, FgmresTrace *tr) {
  CHK(ensure_krylov(c));
  Fgmres s(c, b, x);
  s.tr = tr;
  V0From src = V0From::rhs;
  double beta = 0.0;
  CHK(fgmres_start(s, bnorm, &src, &beta));
  if (tr) CHK(trace_solve_start(s, src != V0From::rhs));
  if (s.reason != 0) { *its_out = 0; *reason_out = s.reason; return 0; }
  double *V = c->kV.p;
  for (;;) {
    if (src == V0From::residual) {
      Between next;
      CHK(fgmres_true_residual(s, &beta));
      CHK(fgmres_between_cycles(s, beta, &next));
      if (next == Between::retry) continue;  // from the iterate before the last cycle
      if (next == Between::stop) break;
    }
    c->ksp_last_relres = beta / s.bn;  // true residual (r0 = b on the first pass)
    if (beta <= s.tol) { s.reason = 2; break; }
    if (s.its >= c->opt.ksp_max_it) { s.reason = -3; break; }
    if (!std::isfinite(beta)) { s.reason = -9; break; }
    if (src == V0From::rhs) CHK(v_scale_to(c, s.n, 1.0 / beta, b, V));
    else if (src != V0From::guess_scaled) CHK(v_scale(c, s.n, 1.0 / beta, V));
    if (s.use32) CHK(v_store32(c, s.n, V, s.V32));
    src = V0From::residual;
    if (tr) CHK(trace_cycle_start(s, beta));
    CHK(fgmres_cycle(s, beta));
    if (s.reason == -9) break;
    CHK(fgmres_update_x(s));
  }
  c->n_krylov += s.its;
  *its_out = s.its;
  *reason_out = s.reason;
  if (c->guess_slot >= 0 && c->guess_slot < cfdh_ctx::GUESS_NEWTON) c->guess_last_its[c->guess_slot] = s.its;
  if (s.reason > 0) CHK(guess_store(c, x, s.kept_copy));
  return 0;
}

// The solve of cfdh_fgmres_solve (include/cfdh.h): the preconditioner as cfdh_apply_preconditioner builds it, |b| handed over as
// the Newton iteration hands over |F| (the lean prologue needs it), the ring of the projected guess chosen by newton_index.
int cfdh_fgmres_hook(cfdh_ctx *c, const double *b, double *x, int newton_index, int *its, int *reason, FgmresTrace *tr) {
  CHK(cfdh_pc_update(c, false));
  CHK(guess_ensure(c));
  const int slot_before = c->guess_slot;
  const double relres_before = c->ksp_last_relres;
  const bool fp32_ok_before = c->krylov_fp32_ok, refine_before = c->gs_refine_long;
  double bn = 0.0;
  CHK(v_norm2(c, c->NO, b, &bn));
  c->guess_slot = newton_index;
  if (newton_index >= 0) c->guess_stored[newton_index] = false;
  const int rc = cfdh_fgmres(c, b, x, its, reason, bn, tr);
  c->guess_slot = slot_before;
  c->ksp_last_relres = relres_before;
  if (newton_index < 0) { c->krylov_fp32_ok = fp32_ok_before; c->gs_refine_long = refine_before; }
  if (rc) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

static int upload_bc(cfdh_ctx *c) {
  if (!c->bc_dirty) return 0;
  const int st = c->dim + 1;
  // vertices whose device entries may be stale: cleared since the last upload, or (re)written since
  // (entries of bc_touched below the watermark went up with an earlier upload; cfdh_update_dirichlet queues its nodes itself)
  c->bc_pending.insert(c->bc_pending.end(), c->bc_touched.begin() + (std::ptrdiff_t)std::min(c->bc_touched_sent, c->bc_touched.size()), c->bc_touched.end());
  if ((int)c->bc_mark.size() != c->nv) { c->bc_mark.assign(c->nv, -1); c->bc_full_upload = true; }
  c->bc_epoch++;
  size_t K = 0;
  for (int v : c->bc_pending)
    if (c->bc_mark[v] != c->bc_epoch) { c->bc_mark[v] = c->bc_epoch; c->bc_pending[K++] = v; }
  c->bc_pending.resize(K);
  // bc_touched keeps growing with duplicates when objects are re-added without a clear in between: compact it as well
  if (c->bc_touched.size() > 4 * (size_t)c->nv) { std::sort(c->bc_touched.begin(), c->bc_touched.end()); c->bc_touched.erase(std::unique(c->bc_touched.begin(), c->bc_touched.end()), c->bc_touched.end()); }
  c->bc_touched_sent = c->bc_touched.size();
  // staging of the sparse update: declared here so that they outlive the stream synchronisation below
  std::vector<unsigned char> fl;
  std::vector<double> va, mu;
  if (c->bc_full_upload || K > (size_t)c->nv / 8) {
    HIPCHK(c, hipMemcpyAsync(c->bcflag.p, c->h_bcflag.data(), c->h_bcflag.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->bcval.p, c->h_bcval.data(), sizeof(double) * c->h_bcval.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->bcmult.p, c->h_bcmult.data(), sizeof(double) * c->h_bcmult.size(), hipMemcpyHostToDevice, c->stream));
    c->bc_full_upload = false;
  } else if (K > 0) {
    // sparse update: (vertex, flag, values, multiplicities) of the K vertices, scattered on the device
    fl.resize(K); va.resize(K * st); mu.resize(K * st);
    for (size_t k = 0; k < K; k++) {
      const int v = c->bc_pending[k];
      fl[k] = c->h_bcflag[v];
      for (int i = 0; i < st; i++) { va[k * st + i] = c->h_bcval[(size_t)st * v + i]; mu[k * st + i] = c->h_bcmult[(size_t)st * v + i]; }
    }
    HIPCHK(c, c->bc_uidx.upload(c->bc_pending, c->stream));
    HIPCHK(c, c->bc_uflag.upload(fl, c->stream));
    HIPCHK(c, c->bc_uval.upload(va, c->stream));
    HIPCHK(c, c->bc_umult.upload(mu, c->stream));
    CHK(k_bc_scatter(c, (int)K, st, c->bc_uidx.p, c->bc_uflag.p, c->bc_uval.p, c->bc_umult.p));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->bc_pending.clear();
  c->bc_dirty = false;
  return 0;
}

int cfdh_prepare_assembly(cfdh_ctx *c) {
  CHK(upload_bc(c));
  if (!c->mom_valid) {
    CHK(comm_halo(c, c->xprev.p));
    CHK(k_moments(c));
  }
  return 0;
}

int cfdh_newton_step(cfdh_ctx *c, cfdh_stats *st) {
  const int n = c->NO, nvo = c->nvo;
  const cfdh_options &o = c->opt;
  const double t_begin = wall_ms();
  memset(st, 0, sizeof *st);
  c->last_stats = *st;
  if (!c->params_set) return cfdh_fail(c, CFDH_E_STATE, "cfdh_set_params was not called");
  if (!c->state_set) return cfdh_fail(c, CFDH_E_STATE, "cfdh_set_state was not called");
  CHK(cfdh_prepare_assembly(c));
  if (o.remove_p_mean) CHK(v_sub_mean(c, nvo, c->x.p + (size_t)c->dim * nvo));
  CHK(comm_halo(c, c->x.p));
  double t0 = wall_ms();
  CHK(k_assemble(c, c->x.p, 1));
  const bool lean = lean_newton(c);
  double fn, ns_nrm = 0.0, ns_abs = 0.0;
  if (lean) CHK(k_fnorm_nulltest(c, n, c->F.p, &fn, &ns_nrm, &ns_abs));  // |F| and the null-space numbers below: one read-back
  else CHK(v_norm2(c, n, c->F.p, &fn));
  st->ms_assemble += wall_ms() - t0;
  st->fnorm0 = fn;
  // constant-pressure null space (MatNullSpaceTest: |J n| < 1e-7 for the unit vector n).  PETSc's bound is absolute; on a
  // mesh in metres with millimetre cells every entry of J lies below it and ANY matrix would pass (3-D bifurcation with
  // do-nothing outlets: the pressure level is fixed, yet the test says singular and the projected solve stagnates at 2e-2).
  // The vector is therefore accepted only if it is also small relative to |J| n.
  {
    double nrm = ns_nrm, absnrm = ns_abs;
    if (!lean) CHK(k_nullspace_test(c, &nrm, &absnrm));
    const double np = c->nranks > 1 ? c->nvo_global : (double)nvo;
    const int sing = ((nrm / std::sqrt(np)) < 1e-7 && nrm <= 1e-6 * absnrm) ? 1 : 0;
    if (sing != c->singular) { c->singular = sing; c->pc_valid = false; }
  }
  bool force_refresh = (o.pc_refresh > 0 && c->steps_since_refresh >= o.pc_refresh);
  int reason = 0;
  double *x = c->x.p, *xt = c->xt.p, *d = c->dvec.p;
  // The trial point of the line search is assembled with its Jacobian, because an accepted point that has not converged
  // needs it next.  When the previous reduction predicts that the trial WILL meet the tolerance, only the residual is
  // assembled there (mode 2: same residual bit for bit, no matrix written); a wrong prediction costs one more pass.
  bool jac_current = true;
  double fn_before = 0.0;
  CHK(guess_ensure(c));
  c->hist_fnorm.clear(); c->hist_rtol.clear(); c->hist_its.clear(); c->hist_relres.clear();
  // Eisenstat-Walker forcing (cfdh_set_ksp_forcing): the tolerance of each solve is set here and handed to cfdh_fgmres through
  // c->opt.ksp_rtol, which is restored on every way out of the step
  struct RtolGuard { cfdh_options &o; double v; ~RtolGuard() { o.ksp_rtol = v; } } rtol_guard{c->opt, c->opt.ksp_rtol};
  double ew_rtol_prev = 0.0, ew_fn_prev = 0.0;
  for (int it = 0;; it++) {
    if (o.verbose) fprintf(stderr, "[cfdh]   newton %d |F| = %.6e\n", it, fn);
    if (!std::isfinite(fn)) { reason = CFDH_DIVERGED_FNORM_NAN; break; }
    if (fn < o.snes_atol) { reason = CFDH_CONVERGED_FNORM_ABS; break; }
    if (it > 0 && fn <= o.snes_rtol * st->fnorm0) { reason = CFDH_CONVERGED_FNORM_RELATIVE; break; }
    if (it >= o.snes_max_it) { reason = CFDH_DIVERGED_MAX_IT; break; }
    t0 = wall_ms();
    if (!jac_current) {
      CHK(k_assemble(c, x, 1));
      jac_current = true;
      st->ms_assemble += wall_ms() - t0;
      t0 = wall_ms();
    }
    const bool expect_converged = it > 0 && fn_before > 0.0 && 10.0 * (fn / fn_before) * fn <= o.snes_rtol * st->fnorm0;
    fn_before = fn;
    CHK(cfdh_pc_update(c, force_refresh || o.pc_refresh < 0));
    force_refresh = false;
    st->ms_pc_setup += wall_ms() - t0;
    t0 = wall_ms();
    int kits = 0, kreason = 0;
    if (c->ew_version == 2) {
      // PETSc's SNESKSPEW version 2: rtol_0 first; then gamma (|F_k| / |F_k-1|)^alpha, raised to gamma rtol_k-1^alpha when that
      // exceeds the threshold; capped at rtol_max
      double rt = c->ew_rtol0;
      if (it > 0) {
        rt = c->ew_gamma * std::pow(fn / ew_fn_prev, c->ew_alpha);
        const double stol = c->ew_gamma * std::pow(ew_rtol_prev, c->ew_alpha);
        if (stol > c->ew_threshold) rt = std::max(rt, stol);
        rt = std::min(rt, c->ew_rtol_max);
      }
      c->opt.ksp_rtol = rt;
      ew_rtol_prev = rt;
      ew_fn_prev = fn;
    }
    c->guess_slot = it;
    if (it < cfdh_ctx::GUESS_NEWTON) {
      c->guess_stored[it] = false;
      if (c->guessX.p) CHK(v_copy(c, n, x, c->guessX.p + (size_t)it * krylov_ld(c)));
    }
    CHK(cfdh_fgmres(c, c->F.p, d, &kits, &kreason, fn));
    int kits_failed = 0;
    if (kreason < 0 && c->pc_its_ref > 0) {
      // a lagged hierarchy that stopped working: rebuild once and retry
      CHK(cfdh_pc_update(c, true));
      st->krylov_its += kits;
      kits_failed = kits;
      CHK(cfdh_fgmres(c, c->F.p, d, &kits, &kreason, fn));
    }
    c->guess_slot = -1;
    c->hist_fnorm.push_back(fn); c->hist_rtol.push_back(c->opt.ksp_rtol); c->hist_its.push_back(kits_failed + kits);
    c->hist_relres.push_back(c->ksp_last_relres);
    st->krylov_its += kits;
    st->ms_solve += wall_ms() - t0;
    if (kreason < 0) { reason = CFDH_DIVERGED_LINEAR_SOLVE; cfdh_fail(c, CFDH_E_DIVERGED, "FGMRES failed (reason %d) after %d iterations", kreason, kits); break; }
    // adaptive lagging: rebuild when a solve needs 1.5x (+5) the iterations the fresh hierarchy needed.  The reference count
    // is the LARGEST solve of the step the hierarchy was built in and of the step after it: the solves of one step differ
    // (the first Newton iteration often only repairs boundary rows in a handful of iterations), and a reference taken from
    // such a solve made every later one trip the rule -- 16 rebuilds in a row during the start-up ramp of config 5.
    if (c->pc_its_ref == 0) c->pc_its_ref = std::max(kits, 1);
    else if (c->steps_since_refresh <= 1) c->pc_its_ref = std::max(c->pc_its_ref, kits);
    else if (o.pc_refresh == 0 && kits > (3 * c->pc_its_ref) / 2 + 5) force_refresh = true;
    // backtracking line search on 1/2 |F|^2 (Dennis-Schnabel, alpha = 1e-4)
    t0 = wall_ms();
    double lam = 1.0, fnew = 0.0, dn = 0.0, xn = 0.0;
    bool ok = false;
    for (int ls = 0; ls < 40; ls++) {
      CHK(v_waxpy(c, n, -lam, d, x, xt));
      CHK(comm_halo(c, xt));
      CHK(k_assemble(c, xt, expect_converged ? 2 : 1));  // residual (and Jacobian) at the trial point in one pass
      // lean path: |F(x_t)|, |d| and |x_t| in one reduction and one read-back
      if (lean) { double t3[3]; CHK(v_norm2_triple(c, n, c->F.p, d, xt, t3)); fnew = t3[0]; dn = t3[1]; xn = t3[2]; }
      else CHK(v_norm2(c, n, c->F.p, &fnew));
      if (std::isfinite(fnew) && (fnew * fnew <= fn * fn * (1.0 - 2.0e-4 * lam) || fnew < o.snes_atol)) { ok = true; break; }
      double l2 = std::isfinite(fnew) ? fn * fn * lam * lam / (2.0 * (0.5 * fnew * fnew - 0.5 * fn * fn + fn * fn * lam)) : 0.0;
      if (!(l2 > 0.1 * lam)) l2 = 0.1 * lam;
      if (l2 > 0.5 * lam) l2 = 0.5 * lam;
      lam = l2;
    }
    st->ms_assemble += wall_ms() - t0;
    if (!ok) { reason = CFDH_DIVERGED_LINE_SEARCH; break; }
    if (!lean) CHK(v_norm2_pair(c, n, d, xt, &dn, &xn));
    if (o.verbose) fprintf(stderr, "[cfdh]     step length %.3e, |dx| = %.3e, |x| = %.3e, %d FGMRES iterations\n", lam, dn, xn, kits);
    std::swap(c->x.p, c->xt.p);
    x = c->x.p; xt = c->xt.p;
    jac_current = !expect_converged;
    st->newton_its = it + 1;
    fn = fnew;
    if (lam * dn < o.snes_stol * xn && fn > o.snes_rtol * st->fnorm0 && fn >= o.snes_atol) {
      if (o.verbose) fprintf(stderr, "[cfdh]   newton %d |F| = %.6e (stol)\n", it + 1, fn);
      reason = CFDH_CONVERGED_SNORM_RELATIVE;
      break;
    }
  }
  if (reason > 0) CHK(guess_refine(c, st->newton_its, c->x.p));
  c->steps_since_refresh++;
  st->fnorm = fn;
  st->reason = reason;
  st->pc_refreshes = c->last_stats.pc_refreshes;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  st->ms_total = wall_ms() - t_begin;
  c->last_stats = *st;
  if (reason < 0) {
    if (c->err.empty() || reason != CFDH_DIVERGED_LINEAR_SOLVE) cfdh_fail(c, CFDH_E_DIVERGED, "Did not converge, reason: %d.", reason);
    return CFDH_E_DIVERGED;
  }
  return 0;
}
