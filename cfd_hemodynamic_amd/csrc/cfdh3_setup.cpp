// Host-side setup of a tetrahedral context (gdim == 3): internal vertex numbering along a 3-D Morton curve, the
// vertex-graph pattern of the 4x4 block matrix (create_matrix_block, stabilized_schur.py:191, on the P1/P1 spaces of
// :55-57 with gdim 3), the incidence lists of the LDS-accumulating assembly kernel, P1 stiffness / lumped mass for the
// Cahouet-Chabard preconditioner.  Single GPU: nv_owned must equal nv.
#include <algorithm>
#include <cmath>
#include <numeric>

#include "cfdh_internal.hpp"
#include "cfdh_mesh_host.hpp"

static const cfdh_mesh::Wording W_CLOSED3 = {"bad mesh sizes", "mesh too large for int32 indexing", "vertex", "vertex %d has no cell",
                                             "facet (cell, local) out of range"};

int cfdh_build_mesh3(cfdh_ctx *c, int64_t nv64, int64_t nvo64, int64_t nc64, const int32_t *cells, const double *coords,
                     int64_t nfac64, const int32_t *fcell, const int32_t *flocal, const int32_t *fmarker) {
  const int nv = (int)nv64, nvo = (int)nvo64, ncu = (int)nc64, nfac = (int)nfac64;
  std::string why;
  if (!cfdh_mesh::check_sizes(nv64, nvo64, nc64, 4, cells, 1ll << 28, 1ll << 29, W_CLOSED3, why) ||
      !cfdh_mesh::check_facets(nfac64, fcell, flocal, nc64, 4, W_CLOSED3, why))
    return cfdh_fail(c, CFDH_E_ARG, "%s", why.c_str());
  c->dim = 3; c->nloc = 4;
  // a part of a partitioned mesh: owned vertices first, ghosts after (as in 2-D); vectors [u owned 3 nvo | p owned nvo |
  // ghosts (ux, uy, uz, p) ng]
  c->nv = nv; c->nvo = nvo; c->ng = nv - nvo;
  c->NO = 4 * nvo; c->NL = 4 * nvo + 4 * c->ng;
  // ---- Morton numbering of the owned vertices (ghosts keep their order: grouped by owner)
  c->perm.resize(nv); c->iperm.resize(nv); c->h_coords.resize(3 * (size_t)nv);
  if (!cfdh_mesh::morton_numbering(3, 21, cfdh_renumber_enabled(), nv, nvo, coords, c->perm.data(), c->iperm.data(), c->h_coords.data(), why))
    return cfdh_fail(c, CFDH_E_ARG, "%s", why.c_str());
  // ---- cells in internal ids, sorted by smallest vertex, positively oriented
  {
    std::vector<int> cmap;
    cfdh_mesh::select_cells(4, ncu, nvo, cells, c->perm.data(), c->h_cells, c->cell_user, cmap);
    const int nck = c->nc = (int)c->cell_user.size();
    std::vector<unsigned char> flipped(nck, 0);
    const double *X = c->h_coords.data();
    for (int k = 0; k < nck; k++) {
      const int e = c->cell_user[k];
      int *v = &c->h_cells[4 * (size_t)k];
      for (int a = 0; a < 4; a++)
        for (int b = a + 1; b < 4; b++)
          if (v[a] == v[b]) return cfdh_fail(c, CFDH_E_ARG, "degenerate cell %d", e);
      double d[3][3];
      for (int a = 0; a < 3; a++)
        for (int i = 0; i < 3; i++) d[a][i] = X[3 * (size_t)v[a + 1] + i] - X[3 * (size_t)v[0] + i];
      const double det = d[0][0] * (d[1][1] * d[2][2] - d[1][2] * d[2][1]) - d[0][1] * (d[1][0] * d[2][2] - d[1][2] * d[2][0]) +
                         d[0][2] * (d[1][0] * d[2][1] - d[1][1] * d[2][0]);
      if (!(std::fabs(det) > 0)) return cfdh_fail(c, CFDH_E_ARG, "zero-volume cell %d", e);
      if (det < 0) { std::swap(v[2], v[3]); flipped[k] = 1; }
    }
    c->cell_flipped = flipped;
    c->fac_cell.clear(); c->fac_local.clear(); c->fac_marker.clear(); c->fac_user.clear();
    c->nfac_user = nfac;
    for (int k = 0; k < nfac; k++) {
      const int e = cmap[fcell[k]];
      if (e < 0) continue;
      int fl = flocal[k];
      if (flipped[e] && fl >= 2) fl = 5 - fl;  // local vertices 2 and 3 were swapped
      c->fac_cell.push_back(e); c->fac_local.push_back(fl);
      c->fac_marker.push_back(fmarker ? fmarker[k] : 0);
      c->fac_user.push_back(k);
    }
    c->nfac = (int)c->fac_cell.size();
  }
  const int nc = c->nc;
  // ---- vertex -> incident (cell, local) (vcell = 4 cell + local); vertex graph
  std::vector<int> vcptr, vcell;
  if (!cfdh_mesh::node_graph(4, nc, nvo, c->h_cells.data(), c->iperm.data(), vcptr, vcell, c->h_vptr, c->h_vcol, c->h_vdiag, W_CLOSED3, why))
    return cfdh_fail(c, CFDH_E_ARG, "%s", why.c_str());
  for (int v = 0; v < nvo; v++) {
    const int deg = c->h_vptr[v + 1] - c->h_vptr[v];
    if (deg > CFDH3_MAX_SLOTS) return cfdh_fail(c, CFDH_E_ARG, "vertex valence %d exceeds %d", deg, CFDH3_MAX_SLOTS);
  }
  const int ninc = vcptr[nvo];
  c->nnzv = (int)c->h_vcol.size();
  c->ninc = ninc;
  // ---- P1 stiffness and lumped mass (geometry only)
  c->h_Lval.assign(c->nnzv, 0.0);
  c->h_Ml.assign(nvo, 0.0);
  for (int e = 0; e < nc; e++) {
    const int *v = &c->h_cells[4 * (size_t)e];
    const double *X = c->h_coords.data();
    double d[3][3];
    for (int a = 0; a < 3; a++)
      for (int i = 0; i < 3; i++) d[a][i] = X[3 * (size_t)v[a + 1] + i] - X[3 * (size_t)v[0] + i];
    // rows of the inverse of [d0 d1 d2]^T-columns matrix = gradients of l_1..l_3: g_a = (d_b x d_c) / det
    double cr[3][3];
    for (int a = 0; a < 3; a++) {
      const double *p = d[(a + 1) % 3], *q = d[(a + 2) % 3];
      cr[a][0] = p[1] * q[2] - p[2] * q[1]; cr[a][1] = p[2] * q[0] - p[0] * q[2]; cr[a][2] = p[0] * q[1] - p[1] * q[0];
    }
    const double det = d[0][0] * cr[0][0] + d[0][1] * cr[0][1] + d[0][2] * cr[0][2];
    double g[4][3];
    for (int a = 0; a < 3; a++)
      for (int i = 0; i < 3; i++) g[a + 1][i] = cr[a][i] / det;
    for (int i = 0; i < 3; i++) g[0][i] = -(g[1][i] + g[2][i] + g[3][i]);
    const double vol = std::fabs(det) / 6.0;
    for (int a = 0; a < 4; a++) {
      if (v[a] >= nvo) continue;
      c->h_Ml[v[a]] += vol / 4.0;
      const int *nb = &c->h_vcol[c->h_vptr[v[a]]];
      const int deg = c->h_vptr[v[a] + 1] - c->h_vptr[v[a]];
      for (int b = 0; b < 4; b++) {
        const int sidx = (int)(std::lower_bound(nb, nb + deg, v[b]) - nb);
        c->h_Lval[c->h_vptr[v[a]] + sidx] += vol * (g[a][0] * g[b][0] + g[a][1] * g[b][1] + g[a][2] * g[b][2]);
      }
    }
  }
  // ---- assembly workgroups: consecutive rows, at most CFDH3_MAX_SLOTS value slots
  std::vector<int> blk_row(1, 0), blk_iptr(1, 0), inc_cell, inc_row;
  std::vector<unsigned long long> inc_slots;
  inc_cell.reserve(ninc); inc_row.reserve(ninc); inc_slots.reserve(ninc);
  {
    int r0 = 0;
    while (r0 < nvo) {
      int r1 = r0;
      const int s0 = c->h_vptr[r0];
      while (r1 < nvo && c->h_vptr[r1 + 1] - s0 <= CFDH3_MAX_SLOTS && r1 - r0 < 64) r1++;
      if (r1 == r0) return cfdh_fail(c, CFDH_E_ARG, "row too long for one assembly workgroup");
      // The rows of a workgroup are dealt to its four wavefronts (longest first, to the least loaded wavefront: deterministic),
      // and ALL incidences of a row are processed by the wavefront that got it.  Every LDS accumulator (row, column) then
      // receives its contributions from one wavefront only, in program order (and in lane order inside one ds_add_f64
      // instruction): a FIXED order -- the assembly is bitwise reproducible although it still sums in LDS.
      std::vector<int> order(r1 - r0);
      for (int r = r0; r < r1; r++) order[r - r0] = r;
      std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return vcptr[x + 1] - vcptr[x] > vcptr[y + 1] - vcptr[y]; });
      std::vector<int> wrows[4];
      int load[4] = {0, 0, 0, 0};
      for (int r : order) {
        int w = 0;
        for (int q = 1; q < 4; q++) if (load[q] < load[w]) w = q;
        wrows[w].push_back(r);
        load[w] += vcptr[r + 1] - vcptr[r];
      }
      for (int w = 0; w < 4; w++) {
        std::sort(wrows[w].begin(), wrows[w].end());
        for (int r : wrows[w]) {
          const int *nb = &c->h_vcol[c->h_vptr[r]];
          const int deg = c->h_vptr[r + 1] - c->h_vptr[r];
          for (int k = vcptr[r]; k < vcptr[r + 1]; k++) {
            const int e = vcell[k] >> 2;
            unsigned long long sl = 0;
            for (int b = 0; b < 4; b++) {
              const int wv = c->h_cells[4 * (size_t)e + b];
              const unsigned long long sidx = (unsigned long long)(c->h_vptr[r] - s0 + (int)(std::lower_bound(nb, nb + deg, wv) - nb));
              sl |= sidx << (16 * b);
            }
            inc_cell.push_back(vcell[k]); inc_row.push_back(r - r0); inc_slots.push_back(sl);
          }
        }
        if (w < 3) blk_iptr.push_back((int)inc_cell.size());  // [4 blk + w + 1]: end of wavefront w's list
      }
      blk_row.push_back(r1); blk_iptr.push_back((int)inc_cell.size());
      r0 = r1;
    }
  }
  c->a3_nblk = (int)blk_row.size() - 1;
  c->nblk = c->a3_nblk;
  // ---- uploads / allocations
  hipStream_t s = c->stream;
  std::vector<unsigned char> cflag(nc, 0);
  for (int k = 0; k < c->nfac; k++) cflag[c->fac_cell[k]] |= (unsigned char)(1u << c->fac_local[k]);
  HIPCHK(c, c->coords.upload(c->h_coords, s));
  HIPCHK(c, c->cells.upload(c->h_cells, s));
  HIPCHK(c, c->cflag.upload(cflag, s));
  HIPCHK(c, c->mom.alloc(12 * (size_t)nc));
  CHK(cfdh_upload_graph(c));
  HIPCHK(c, c->a3_blk_row.upload(blk_row, s));
  HIPCHK(c, c->a3_blk_iptr.upload(blk_iptr, s));
  HIPCHK(c, c->a3_inc_cell.upload(inc_cell, s));
  HIPCHK(c, c->a3_inc_row.upload(inc_row, s));
  HIPCHK(c, c->a3_inc_slots.upload(inc_slots, s));
  // with overlapping parts a cell is integrated (global functionals) only by the rank that owns its first vertex
  std::vector<unsigned char> cown(nc, 1);  // lives until the stream synchronisation at the end of this function
  for (int k = 0; k < nc; k++) cown[k] = cells[4 * (size_t)c->cell_user[k]] < nvo ? 1 : 0;
  HIPCHK(c, c->cell_owned.upload(cown, s));
  CHK(cfdh_upload_facets(c));
  CHK(cfdh_alloc_dirichlet(c));
  CHK(cfdh_alloc_state(c));
  CHK(cfdh_alloc_reduction(c, true));
  CHK(cfdh_alloc_precond_work(c, nvo, false));  // this builder has neither dinvA nor prand
  HIPCHK(c, hipStreamSynchronize(s));
  return 0;
}
