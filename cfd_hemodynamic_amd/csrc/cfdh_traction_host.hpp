// Work list of the traction-boundary kernel (cfdh_traction.hip), built on the host.  Plain C++, no HIP: compiled with g++ by
// tests/test_traction_host.py, like cfdh_mesh_host.hpp.
//
// The kernel adds the facet terms of cfdh_set_traction_boundaries to rows of F and A00 that the volume pass has already written,
// so every destination needs exactly one writer.  The list is therefore organised by destination row: for each vertex row that a
// traction facet touches, its (cell, local facet) pairs, and for each pair where the cell's d + 1 column blocks sit in that row.
//   facets of a boundary WITHOUT the tangential terms reach the rows of the facet's vertices;
//   facets of a boundary WITH them also reach the row of the opposite vertex (the Nitsche symmetry term tests with grad(lambda_a)).
// Order: rows ascending; the pairs of a row in the facet order of cfdh_create (at most one pair per facet and row).
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

namespace cfdh_traction {

constexpr int SLICE = 64;  // rows per slice = lanes of a wavefront: one lane owns a row

struct WorkList {
  int D = 2;
  int nrows = 0, npairs = 0, nslices = 0;
  // by row (what the tests read)
  std::vector<int> row;    // [nrows] destination rows, ascending
  std::vector<int> rptr;   // [nrows + 1] pairs of row r: [rptr[r], rptr[r + 1])
  std::vector<int> pcell;  // [npairs] cell
  std::vector<int> pmeta;  // [npairs] local index of the row vertex | local facet << 2 | boundary slot << 4
  std::vector<int> pslot;  // [npairs][D + 1] position in the vertex graph (value slot) of the column of the cell's vertex b in this row
  // the same in the layout the kernel reads: slices of SLICE consecutive rows, column-major inside a slice, so that the lanes of a
  // wavefront read consecutive words.  Slice s holds sptr[s + 1] - sptr[s] pair columns (its longest row); entry (column c, lane l)
  // is at (sptr[s] + c) * SLICE + l, the slots of vertex b at ((sptr[s] + c) * (D + 1) + b) * SLICE + l.  cell < 0: no pair.
  std::vector<int> sptr, dcell, dmeta, dslot;
};

inline int pack_meta(int a, int f, int k) { return a | (f << 2) | (k << 4); }

// cells [nc][D + 1]; exterior facets (fcell, flocal, fmarker) in the order of cfdh_create; boundary k = the facets whose marker is
// markers[k], tangential bit k: boundary k carries the tangential terms; vptr / vcol: vertex graph (columns ascending or not).
// false with the reason in `why` when a column of a cell is missing from the graph or an index is out of range.
inline bool build_worklist(int D, int nv, int nc, const int *cells, int nfac, const int *fcell, const int *flocal, const int *fmarker, int nb,
                           const int *markers, unsigned tangential, const int *vptr, const int *vcol, WorkList &w, std::string &why) {
  const int n1 = D + 1;
  w = WorkList();
  w.D = D;
  struct Pair { int row, cell, meta; };
  std::vector<Pair> pairs;
  std::vector<int> count((size_t)nv + 1, 0);
  for (int q = 0; q < nfac; q++) {
    int k = -1;
    for (int b = 0; b < nb; b++)
      if (fmarker[q] == markers[b]) { k = b; break; }
    if (k < 0) continue;
    const int e = fcell[q], f = flocal[q];
    if (e < 0 || e >= nc || f < 0 || f > D) { why = "traction work list: facet " + std::to_string(q) + " names no cell / local facet"; return false; }
    for (int a = 0; a < n1; a++) {
      if (a == f && !((tangential >> k) & 1u)) continue;
      const int r = cells[(size_t)n1 * e + a];
      if (r < 0 || r >= nv) { why = "traction work list: vertex out of range in cell " + std::to_string(e); return false; }
      pairs.push_back({r, e, pack_meta(a, f, k)});
      count[(size_t)r + 1]++;
    }
  }
  w.npairs = (int)pairs.size();
  // stable bucket sort by row keeps the facet order inside a row
  std::vector<int> first((size_t)nv + 1, 0);
  for (int v = 0; v < nv; v++) first[v + 1] = first[v] + count[v + 1];
  w.rptr.push_back(0);
  for (int v = 0; v < nv; v++)
    if (count[v + 1]) { w.row.push_back(v); w.rptr.push_back(first[v + 1]); }
  w.nrows = (int)w.row.size();
  w.pcell.assign(w.npairs, 0); w.pmeta.assign(w.npairs, 0); w.pslot.assign((size_t)n1 * w.npairs, 0);
  std::vector<int> fill(first.begin(), first.end() - 1);
  for (const Pair &p : pairs) {
    const int pos = fill[p.row]++;
    w.pcell[pos] = p.cell; w.pmeta[pos] = p.meta;
    for (int b = 0; b < n1; b++) {
      const int col = cells[(size_t)n1 * p.cell + b];
      int s = -1;
      for (int j = vptr[p.row]; j < vptr[p.row + 1]; j++)
        if (vcol[j] == col) { s = j; break; }
      if (s < 0) { why = "traction work list: vertex " + std::to_string(col) + " is no column of row " + std::to_string(p.row); return false; }
      w.pslot[(size_t)n1 * pos + b] = s;
    }
  }
  // sliced layout
  w.nslices = (w.nrows + SLICE - 1) / SLICE;
  w.sptr.assign((size_t)w.nslices + 1, 0);
  for (int s = 0; s < w.nslices; s++) {
    int width = 0;
    for (int r = s * SLICE; r < w.nrows && r < (s + 1) * SLICE; r++) width = std::max(width, w.rptr[r + 1] - w.rptr[r]);
    w.sptr[s + 1] = w.sptr[s] + width;
  }
  const size_t ncol = (size_t)w.sptr[w.nslices];
  w.dcell.assign(ncol * SLICE, -1); w.dmeta.assign(ncol * SLICE, 0); w.dslot.assign(ncol * n1 * SLICE, 0);
  for (int r = 0; r < w.nrows; r++) {
    const int s = r / SLICE, l = r % SLICE;
    for (int j = w.rptr[r]; j < w.rptr[r + 1]; j++) {
      const size_t c = (size_t)w.sptr[s] + (j - w.rptr[r]);
      w.dcell[c * SLICE + l] = w.pcell[j];
      w.dmeta[c * SLICE + l] = w.pmeta[j];
      for (int b = 0; b < n1; b++) w.dslot[(c * n1 + b) * SLICE + l] = w.pslot[(size_t)n1 * j + b];
    }
  }
  return true;
}

// argument checks of cfdh_set_traction_boundaries that need no context
inline bool check_boundaries(int n, int nmax, const int32_t *markers, const double *values, double beta_nitsche, const double *beta_backflow,
                             std::string &why) {
  auto finite = [](double v) { return v == v && v - v == 0.0; };
  if (n < 0 || n > nmax) { why = "0 <= n <= " + std::to_string(nmax); return false; }
  if (n > 0 && (!markers || !values)) { why = "null marker / value array"; return false; }
  if (!finite(beta_nitsche) || beta_nitsche < 0) { why = "beta_nitsche must be finite and >= 0"; return false; }
  for (int k = 0; k < n; k++) {
    if (!finite(values[k])) { why = "value " + std::to_string(k) + " is not finite"; return false; }
    if (beta_backflow && (!finite(beta_backflow[k]) || beta_backflow[k] < 0)) { why = "beta_backflow " + std::to_string(k) + " must be finite and >= 0"; return false; }
    for (int l = 0; l < k; l++)
      if (markers[l] == markers[k]) { why = "marker " + std::to_string(markers[k]) + " listed twice"; return false; }
  }
  return true;
}

}  // namespace cfdh_traction
