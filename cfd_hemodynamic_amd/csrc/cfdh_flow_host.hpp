// Inverted index of the volumetric flow diagnostics (cfdh_flow.hip), built on the host.  Plain C++, no HIP: compiled with g++ by
// tests/test_flow_twin.py, like cfdh_scalar_host.hpp.
//
// The recovery G_v = sum |c| G_c / sum |c| runs over the cells of a vertex in a fixed order, one lane per vertex.  The index needs
// `cells` only (not the vertex graph, which cfdh_scalar::WorkList is built from), and it stores the cell alone: the vertex pass
// reads a whole contribution row of the cell and does not care which corner the vertex is.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

namespace cfdh_flow {

constexpr int SLICE = 64;  // vertices per slice = lanes of a wavefront: one lane owns a vertex

struct CellIndex {
  int D = 2;
  int nv = 0, ninc = 0, nslices = 0, maxlen = 0;
  // by row (what the tests read): the cells of vertex v are inc[rptr[v] .. rptr[v + 1])
  std::vector<int> rptr, inc;
  // the same in the layout the kernels read, that of cfdh_scalar::WorkList::dinc: slices of SLICE consecutive vertices, column-major
  // inside a slice, so that the lanes of a wavefront read consecutive words.  Slice s holds sptr[s + 1] - sptr[s] columns (its
  // highest valence); entry (column k, lane l) is at (sptr[s] + k) * SLICE + l.  -1: no incidence.  The last slice is allocated in
  // full, so every lane of the last wavefront reads inside the array.
  std::vector<int> sptr, dinc;
};

// cells [nc][D + 1].  The cells of a vertex are listed in the order in which `visit` (a permutation of 0 .. nc - 1; null: the
// identity) names them: with visit[k] = the stored cell that the caller numbered k, that is ascending in the caller's cell index
// whatever order the context keeps its cells in.  false with the reason in `why` for a bad size or an index out of range.
inline bool build_index(int D, int nv, int nc, const int *cells, const int *visit, CellIndex &w, std::string &why) {
  const int n1 = D + 1;
  w = CellIndex();
  w.D = D;
  if ((D != 2 && D != 3) || nv < 0 || nc < 0) { why = "flow index: bad sizes"; return false; }
  if ((long long)nc * n1 > 0x7fffffffll) { why = "flow index: more than 2^31 incidences"; return false; }
  w.nv = nv;
  w.rptr.assign((size_t)nv + 1, 0);
  std::vector<char> seen(visit ? (size_t)nc : 0, 0);
  for (int k = 0; k < nc; k++) {
    const int e = visit ? visit[k] : k;
    if (e < 0 || e >= nc || (visit && seen[e])) { why = "flow index: visit is no permutation of the cells"; return false; }
    if (visit) seen[e] = 1;
    for (int a = 0; a < n1; a++) {
      const int v = cells[(size_t)n1 * e + a];
      if (v < 0 || v >= nv) { why = "flow index: vertex out of range in cell " + std::to_string(e); return false; }
      for (int b = 0; b < a; b++)
        if (cells[(size_t)n1 * e + b] == v) { why = "flow index: cell " + std::to_string(e) + " names a vertex twice"; return false; }
      w.rptr[(size_t)v + 1]++;
    }
  }
  for (int v = 0; v < nv; v++) {
    w.maxlen = std::max(w.maxlen, w.rptr[v + 1]);
    w.rptr[v + 1] += w.rptr[v];
  }
  w.ninc = w.rptr[nv];
  w.inc.assign((size_t)w.ninc, 0);
  std::vector<int> fill(w.rptr.begin(), w.rptr.end() - 1);
  for (int k = 0; k < nc; k++) {  // in visiting order: the order inside a row
    const int e = visit ? visit[k] : k;
    for (int a = 0; a < n1; a++) w.inc[fill[cells[(size_t)n1 * e + a]]++] = e;
  }
  w.nslices = (nv + SLICE - 1) / SLICE;
  w.sptr.assign((size_t)w.nslices + 1, 0);
  for (int s = 0; s < w.nslices; s++) {
    int width = 0;
    for (int v = s * SLICE; v < nv && v < (s + 1) * SLICE; v++) width = std::max(width, w.rptr[v + 1] - w.rptr[v]);
    w.sptr[s + 1] = w.sptr[s] + width;
  }
  w.dinc.assign((size_t)w.sptr[w.nslices] * SLICE, -1);
  for (int v = 0; v < nv; v++) {
    const int s = v / SLICE, l = v % SLICE;
    for (int j = w.rptr[v]; j < w.rptr[v + 1]; j++) w.dinc[((size_t)w.sptr[s] + (j - w.rptr[v])) * SLICE + l] = w.inc[j];
  }
  return true;
}

inline bool finite(double v) { return v == v && v - v == 0.0; }

// number of doubles per vertex of cfdh_flow_field(which) in dimension D; 0: no such field
inline int field_width(int D, int which) {
  switch (which) {
    case 0: return D * D;
    case 1: return D == 2 ? 1 : 3;
    case 2: case 3: case 4: return 1;
    case 5: case 6: return D == 3 ? 1 : 0;
    default: return 0;
  }
}

}  // namespace cfdh_flow
