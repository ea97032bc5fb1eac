// The mesh set-up steps that the context builders share (cfdh_build_mesh, cfdh_build_mesh3, cfdh_build_mesh_gen,
// cfdh_build_mesh_gen3, cfdh_ipcs_create): index arithmetic on std::vector, no device and no context.  Plain C++17 without HIP,
// so that the CPU tests compile it with the host compiler (tests/mesh_host_shim.cpp, tests/mesh_host_main.cpp).  A step that
// refuses its input returns false and leaves the reason in `msg`; the builder hands it to cfdh_fail(c, CFDH_E_ARG, ...).
//
// Ghost convention (all builders): nodes [0, nvo) are owned, the rest are ghosts in the order of the halo plan.  Any ghost set
// that is closed under the halo plan is accepted -- one layer of cells, two (the default of PartComm.make_part) or more --
// and rows are assembled for owned nodes only.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <string>
#include <vector>

namespace cfdh_mesh {

// the few words in which the refusals of the builders differ
struct Wording {
  const char *owned_count = "bad owned node count";  // 0 < nvo <= nv violated
  const char *too_large = "mesh too large for int32 indexing";
  const char *node = "node";                         // "cell <node> index out of range"
  const char *no_cell = "node %d belongs to no cell";
  const char *facet = "facet (cell, local) out of range";
};

// ---- size and index checks: 0 < nvo <= nv, nc > 0, the builder's int32 limits, cell nodes in [0, nv)
inline bool check_sizes(int64_t nv, int64_t nvo, int64_t nc, int NL, const int32_t *cells, int64_t nv_max, int64_t nc_max, const Wording &w,
                        std::string &msg) {
  if (nvo <= 0 || nvo > nv) { msg = w.owned_count; return false; }
  if (nv <= 0 || nc <= 0) { msg = "bad mesh sizes"; return false; }
  if (nv > nv_max || nc > nc_max) { msg = w.too_large; return false; }
  for (int64_t k = 0; k < NL * nc; k++)
    if (cells[k] < 0 || cells[k] >= nv) { msg = std::string("cell ") + w.node + " index out of range"; return false; }
  return true;
}
// facets as (cell, local facet) with NF local facets
inline bool check_facets(int64_t nfac, const int32_t *fcell, const int32_t *flocal, int64_t nc, int NF, const Wording &w, std::string &msg) {
  for (int64_t k = 0; k < nfac; k++)
    if (fcell[k] < 0 || fcell[k] >= nc || flocal[k] < 0 || flocal[k] >= NF) { msg = w.facet; return false; }
  return true;
}

// ---- Morton numbering
inline uint64_t part1by1(uint64_t x) {  // 16 bits -> every second bit
  x &= 0x0000ffff;
  x = (x ^ (x << 8)) & 0x00ff00ff;
  x = (x ^ (x << 4)) & 0x0f0f0f0f;
  x = (x ^ (x << 2)) & 0x33333333;
  x = (x ^ (x << 1)) & 0x55555555;
  return x;
}
inline uint64_t part1by2(uint64_t x) {  // 10 bits -> every third bit
  x &= 0x000003ff;
  x = (x ^ (x << 16)) & 0xff0000ff;
  x = (x ^ (x << 8)) & 0x0300f00f;
  x = (x ^ (x << 4)) & 0x030c30c3;
  x = (x ^ (x << 2)) & 0x09249249;
  return x;
}
inline uint64_t spread3(uint64_t x) {  // 21 bits -> every third bit
  x &= 0x1fffff;
  x = (x | x << 32) & 0x1f00000000ffffull;
  x = (x | x << 16) & 0x1f0000ff0000ffull;
  x = (x | x << 8) & 0x100f00f00f00f00full;
  x = (x | x << 4) & 0x10c30c30c30c30c3ull;
  x = (x | x << 2) & 0x1249249249249249ull;
  return x;
}
// Owned nodes along a Morton curve of `bits` bits per axis over the bounding box of ALL nodes (D = 2: bits <= 16, D = 3:
// bits <= 21), stable in the input order; ghosts keep their place.  perm[user] = internal, iperm its inverse; xout [D nv] are the
// coordinates in internal order.  renumber = false: the identity.  Refuses coordinates without extent.
inline bool morton_numbering(int D, int bits, bool renumber, int nv, int nvo, const double *coords, int *perm, int *iperm, double *xout,
                             std::string &msg) {
  double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300}, ext = 0.0;
  for (int v = 0; v < nv; v++)
    for (int i = 0; i < D; i++) { lo[i] = std::min(lo[i], coords[(size_t)D * v + i]); hi[i] = std::max(hi[i], coords[(size_t)D * v + i]); }
  for (int i = 0; i < D; i++) ext = std::max(ext, hi[i] - lo[i]);
  if (!(ext > 0)) { msg = "degenerate coordinates"; return false; }
  std::vector<int> order(nvo);
  std::iota(order.begin(), order.end(), 0);
  if (renumber) {
    const double qmax = (double)((1ull << bits) - 1);
    std::vector<uint64_t> key(nvo);
    for (int v = 0; v < nvo; v++) {
      uint64_t k = 0;
      for (int i = 0; i < D; i++) {
        const uint64_t q = (uint64_t)std::min(qmax, (coords[(size_t)D * v + i] - lo[i]) / ext * qmax);
        k |= (D == 2 ? part1by1(q) : (bits <= 10 ? part1by2(q) : spread3(q))) << i;
      }
      key[v] = k;
    }
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return key[a] < key[b]; });
  }
  for (int k = 0; k < nvo; k++) { iperm[k] = order[k]; perm[order[k]] = k; }
  for (int v = nvo; v < nv; v++) { iperm[v] = v; perm[v] = v; }
  for (int k = 0; k < nv; k++)
    for (int i = 0; i < D; i++) xout[(size_t)D * k + i] = coords[(size_t)D * iperm[k] + i];
  return true;
}

// ---- closed-form builders: the cells that touch an owned node, in internal ids, sorted stably by their smallest node.
// cell_user[k] = user cell of internal cell k, cmap its inverse (-1: cell not kept).
inline void select_cells(int NL, int ncu, int nvo, const int32_t *cells, const int *perm, std::vector<int> &h_cells, std::vector<int> &cell_user,
                         std::vector<int> &cmap) {
  std::vector<std::pair<int, int>> keyed;
  keyed.reserve(ncu);
  for (int e = 0; e < ncu; e++) {
    int mn = perm[cells[(size_t)NL * e]];
    for (int a = 1; a < NL; a++) mn = std::min(mn, perm[cells[(size_t)NL * e + a]]);
    if (mn < nvo) keyed.push_back({mn, e});
  }
  std::stable_sort(keyed.begin(), keyed.end());
  const int nc = (int)keyed.size();
  h_cells.resize((size_t)NL * nc);
  cell_user.resize(nc);
  cmap.assign(ncu, -1);
  for (int k = 0; k < nc; k++) {
    const int e = keyed[k].second;
    cmap[e] = k; cell_user[k] = e;
    for (int a = 0; a < NL; a++) h_cells[(size_t)NL * k + a] = perm[cells[(size_t)NL * e + a]];
  }
}

// ---- node graph of the owned rows.  Incidence: inc[iptr[v] .. iptr[v + 1]) are the positions t = NL cell + local of node v in
// h_cells, cells ascending.  Graph: vcol[vptr[v] .. vptr[v + 1]) the sorted set of nodes of v's cells, vdiag[v] the position of
// v itself.  The first owned node in no cell is refused with its user number iperm[v].
inline bool node_graph(int NL, int nc, int nvo, const int *h_cells, const int *iperm, std::vector<int> &iptr, std::vector<int> &inc,
                       std::vector<int> &vptr, std::vector<int> &vcol, std::vector<int> &vdiag, const Wording &w, std::string &msg) {
  const size_t nt = (size_t)NL * nc;
  iptr.assign(nvo + 1, 0);
  for (size_t t = 0; t < nt; t++) if (h_cells[t] < nvo) iptr[h_cells[t] + 1]++;
  for (int v = 0; v < nvo; v++) iptr[v + 1] += iptr[v];
  inc.resize(iptr[nvo]);
  {
    std::vector<int> fill(iptr.begin(), iptr.end() - 1);
    for (size_t t = 0; t < nt; t++) if (h_cells[t] < nvo) inc[fill[h_cells[t]]++] = (int)t;
  }
  vptr.assign(nvo + 1, 0);
  vcol.clear();
  vdiag.resize(nvo);
  std::vector<int> tmp;
  for (int v = 0; v < nvo; v++) {
    if (iptr[v + 1] == iptr[v]) {
      char buf[96];
      snprintf(buf, sizeof buf, w.no_cell, iperm[v]);
      msg = buf;
      return false;
    }
    tmp.clear();
    for (int k = iptr[v]; k < iptr[v + 1]; k++) {
      const int *cv = h_cells + (size_t)NL * (inc[k] / NL);
      tmp.insert(tmp.end(), cv, cv + NL);
    }
    std::sort(tmp.begin(), tmp.end());
    tmp.erase(std::unique(tmp.begin(), tmp.end()), tmp.end());
    vdiag[v] = (int)vcol.size() + (int)(std::lower_bound(tmp.begin(), tmp.end(), v) - tmp.begin());
    vcol.insert(vcol.end(), tmp.begin(), tmp.end());
    vptr[v + 1] = (int)vcol.size();
  }
  return true;
}
// position of column j in row i of the graph
inline int graph_slot(const int *vptr, const int *vcol, int i, int j) {
  return (int)(std::lower_bound(vcol + vptr[i], vcol + vptr[i + 1], j) - vcol);
}

// ---- generic builders: slots and staging order of the atomics-free assembly
// slot[(cell NL + a) NL + b] = graph entry of (node a, node b) of the cell, -1 in the row of a ghost node (assembled by its owner)
inline void graph_slots(int NL, int nc, int nvo, const int *h_cells, const int *vptr, const int *vcol, std::vector<int> &slot) {
  slot.resize((size_t)nc * NL * NL);
  for (int e = 0; e < nc; e++) {
    const int *v = h_cells + (size_t)NL * e;
    for (int a = 0; a < NL; a++)
      for (int b = 0; b < NL; b++) slot[((size_t)e * NL + a) * NL + b] = v[a] < nvo ? graph_slot(vptr, vcol, v[a], v[b]) : -1;
  }
}
// Turns the graph slots into staging positions: the contributions to graph entry k take eptr[k] .. eptr[k + 1] - 1 in ascending
// (cell, a, b) order, so one lane per entry sums them in a fixed order.  Likewise for the residual: every (cell, a) of an owned
// node v gets `fper` consecutive positions of fptr[v] .. fptr[v + 1] - 1 in fdst [(cell NL + a) fper + j]; -1 for a ghost.
inline void staging_order(int NL, int nc, int nvo, int nnz, const int *h_cells, int fper, std::vector<int> &slot, std::vector<int> &eptr,
                          std::vector<int> &fptr, std::vector<int> &fdst) {
  eptr.assign((size_t)nnz + 1, 0);
  for (size_t t = 0; t < slot.size(); t++) if (slot[t] >= 0) eptr[slot[t] + 1]++;
  for (int k = 0; k < nnz; k++) eptr[k + 1] += eptr[k];
  {
    std::vector<int> fill(eptr.begin(), eptr.end() - 1);
    for (size_t t = 0; t < slot.size(); t++) if (slot[t] >= 0) slot[t] = fill[slot[t]]++;
  }
  const size_t nt = (size_t)nc * NL;
  fptr.assign((size_t)nvo + 1, 0);
  fdst.assign(nt * fper, -1);
  for (size_t t = 0; t < nt; t++) if (h_cells[t] < nvo) fptr[h_cells[t] + 1] += fper;
  for (int v = 0; v < nvo; v++) fptr[v + 1] += fptr[v];
  std::vector<int> fill(fptr.begin(), fptr.end() - 1);
  for (size_t t = 0; t < nt; t++)
    if (h_cells[t] < nvo)
      for (int j = 0; j < fper; j++) fdst[t * fper + j] = fill[h_cells[t]]++;
}

// ---- generic builders: stiffness and diagonal mass of the element on the graph (Cahouet-Chabard preconditioner).
// cell(e, K, Md) fills K [NL][NL] and the diagonal Md [NL] of the consistent mass of cell e and returns its measure.  Lval sums
// K over the graph slots (before staging_order) in (cell, a, b) order; Ml [nv] is the diagonal mass scaled to the total measure
// (HRZ lumping: row sums vanish at P2 vertices).
template <class CellFn>
inline void scatter_stiffness_mass(int NL, int nc, int nv, const int *h_cells, const std::vector<int> &slot, int nnz, CellFn cell,
                                   std::vector<double> &Lval, std::vector<double> &Ml) {
  Lval.assign(nnz, 0.0);
  Ml.assign(nv, 0.0);
  double msum = 0.0, dsum = 0.0;
  std::vector<double> K((size_t)NL * NL), Md(NL);
  for (int e = 0; e < nc; e++) {
    const int *v = h_cells + (size_t)NL * e;
    msum += cell(e, K.data(), Md.data());
    for (int a = 0; a < NL; a++) {
      Ml[v[a]] += Md[a];
      dsum += Md[a];
      for (int b = 0; b < NL; b++) {
        const int k = slot[((size_t)e * NL + a) * NL + b];
        if (k >= 0) Lval[k] += K[a * NL + b];
      }
    }
  }
  for (int v = 0; v < nv; v++) Ml[v] = Ml[v] * (msum / dsum);
}

// ---- P1 subspace of a P2 space on simplices with NV vertices: CSR rows over all nv nodes.  Vertex nodes (local positions
// 0 .. NV - 1) are numbered in ascending node order and carry 1; the edge node NV + q interpolates the two end vertices
// edges[q][0..1] with 1/2 each, smaller column first.  Returns the number of vertex nodes.
inline int p1_subspace(int NL, int NV, const int (*edges)[2], int nc, int nv, const int *h_cells, std::vector<int> &rowptr, std::vector<int> &col,
                       std::vector<double> &val) {
  std::vector<int> vid(nv, -1), ea(nv, -1), eb(nv, -1);
  for (int e = 0; e < nc; e++) {
    const int *v = h_cells + (size_t)NL * e;
    for (int q = 0; q < NV; q++) vid[v[q]] = 0;
    for (int q = 0; q < NL - NV; q++) { ea[v[NV + q]] = v[edges[q][0]]; eb[v[NV + q]] = v[edges[q][1]]; }
  }
  int nvert = 0;
  for (int v = 0; v < nv; v++) if (vid[v] == 0) vid[v] = nvert++;
  rowptr.assign(nv + 1, 0); col.clear(); val.clear();
  for (int v = 0; v < nv; v++) {
    if (vid[v] >= 0) { col.push_back(vid[v]); val.push_back(1.0); }
    else {
      int a = vid[ea[v]], b = vid[eb[v]];
      if (a > b) std::swap(a, b);
      col.push_back(a); val.push_back(0.5); col.push_back(b); val.push_back(0.5);
    }
    rowptr[v + 1] = (int)col.size();
  }
  return nvert;
}

// ---- wall vertices of a simplex mesh: the vertices (local positions 0 .. NV - 1, all but flocal) of the exterior facets, ascending,
// and for wall vertex k its exterior facets fac[ptr[k] .. ptr[k + 1]) in ascending facet index -- the gather lists of the wall
// shear stress on the P2/P1 context (one lane per wall vertex sums its facets in this order)
inline void wall_vertex_facets(int NL, int NV, int64_t nfac, const int *fcell, const int *flocal, const int *cells, int nvert, std::vector<int> &wv,
                               std::vector<int> &ptr, std::vector<int> &fac) {
  std::vector<int> cnt((size_t)nvert + 1, 0);
  for (int64_t f = 0; f < nfac; f++)
    for (int a = 0; a < NV; a++)
      if (a != flocal[f]) cnt[cells[(size_t)NL * fcell[f] + a] + 1]++;
  wv.clear();
  ptr.assign(1, 0);
  std::vector<int> pos((size_t)nvert, -1);
  for (int v = 0; v < nvert; v++)
    if (cnt[v + 1] > 0) { pos[v] = (int)wv.size(); wv.push_back(v); ptr.push_back(ptr.back() + cnt[v + 1]); }
  fac.resize((size_t)ptr.back());
  std::vector<int> fill(ptr.begin(), ptr.end() - 1);
  for (int64_t f = 0; f < nfac; f++)
    for (int a = 0; a < NV; a++)
      if (a != flocal[f]) fac[fill[pos[cells[(size_t)NL * fcell[f] + a]]]++] = (int)f;
}

// ---- determinant of the affine map of a 2-D cell from its first three nodes (X: coordinates [..][2], v: the cell's nodes); the
// builders refuse a cell whose determinant is not different from zero
inline double tri_det(const double *X, const int *v) {
  return (X[2 * v[1]] - X[2 * v[0]]) * (X[2 * v[2] + 1] - X[2 * v[0] + 1]) - (X[2 * v[1] + 1] - X[2 * v[0] + 1]) * (X[2 * v[2]] - X[2 * v[0]]);
}

// ---- shape checks of the generic cells (X: coordinates [..][D], v: the cell's nodes, adet = |det| of its affine map)
// Q1 quadrilateral: x3 = x1 + x2 - x0 up to 1e-9 sqrt|det|
inline bool is_parallelogram(const double *X, const int *v, double adet) {
  const double ex = X[2 * v[3]] - (X[2 * v[1]] + X[2 * v[2]] - X[2 * v[0]]), ey = X[2 * v[3] + 1] - (X[2 * v[1] + 1] + X[2 * v[2] + 1] - X[2 * v[0] + 1]);
  return !(std::hypot(ex, ey) > 1e-9 * std::sqrt(adet));
}
// Q1 hexahedron: x_v = x_0 + i (x_1 - x_0) + j (x_2 - x_0) + k (x_4 - x_0), every component up to 1e-9 cbrt|det|
inline bool is_parallelepiped(const double *X, const int *v, double adet) {
  const double tol = 1e-9 * std::cbrt(adet);
  auto x = [&](int a, int i) { return X[3 * (size_t)v[a] + i]; };
  for (int a = 0; a < 8; a++)
    for (int i = 0; i < 3; i++) {
      const double ex = x(0, i) + (a & 1) * (x(1, i) - x(0, i)) + ((a >> 1) & 1) * (x(2, i) - x(0, i)) + ((a >> 2) & 1) * (x(4, i) - x(0, i));
      if (std::fabs(x(a, i) - ex) > tol) return false;
    }
  return true;
}
// straight-sided P2 simplex: the first edge node that is not the midpoint of its edge, or -1 (D = 2: distance up to
// 1e-9 sqrt|det|, D = 3: every component up to 1e-9 cbrt|det|)
inline int p2_bent_edge(int D, const int (*edges)[2], const double *X, const int *v, double adet) {
  const int NV = D + 1, ne = D == 2 ? 3 : 6;
  const double tol = 1e-9 * (D == 2 ? std::sqrt(adet) : std::cbrt(adet));
  for (int q = 0; q < ne; q++) {
    double m[3] = {0, 0, 0};
    for (int d = 0; d < D; d++) m[d] = 0.5 * (X[(size_t)D * v[edges[q][0]] + d] + X[(size_t)D * v[edges[q][1]] + d]) - X[(size_t)D * v[NV + q] + d];
    if (D == 2 ? std::hypot(m[0], m[1]) > tol : (std::fabs(m[0]) > tol || std::fabs(m[1]) > tol || std::fabs(m[2]) > tol)) return q;
  }
  return -1;
}

// ---- fixed start vector of the power iterations: n values in [-0.5, 0.5) of a 64-bit LCG
inline std::vector<double> lcg_vector(size_t n) {
  std::vector<double> r(n);
  uint64_t st = 0x2545F4914F6CDD1Dull;
  for (auto &v : r) { st = st * 6364136223846793005ull + 1442695040888963407ull; v = ((st >> 11) * (1.0 / 9007199254740992.0)) - 0.5; }
  return r;
}

}  // namespace cfdh_mesh
