// Work list and argument checks of the passive-scalar transport (cfdh_scalar.hip), built on the host.  Plain C++, no HIP: compiled
// with g++ by tests/test_scalar_twin.py, like cfdh_traction_host.hpp.
//
// The assembly kernel gives every row of the vertex graph one owner, so the list is organised by row: for each vertex its
// (cell, local index) incidences in ascending cell order, and for each incidence where the cell's d + 1 columns sit in that row.
// The incidence lists of the flow assemblies do not fit: the 2-D one is cut into workgroups of whole rows with block-local vertex
// and cell ids, the 3-D one addresses 16-double value slots relative to a workgroup, and neither is laid out per 64-row slice.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

namespace cfdh_scalar {

constexpr int SLICE = 64;  // rows per slice = lanes of a wavefront: one lane owns a row

struct WorkList {
  int D = 2;
  int nrows = 0, ninc = 0, nslices = 0, maxlen = 0;
  // by row (what the tests read)
  std::vector<int> rptr;       // [nrows + 1] incidences of row r: [rptr[r], rptr[r + 1])
  std::vector<int> inc;        // [ninc] cell * 4 + local index of the row vertex
  std::vector<unsigned> slot;  // [ninc] position in the row (8 bits each) of the column of the cell's vertex b
  // the same in the layout the kernel reads: slices of SLICE consecutive rows, column-major inside a slice, so that the lanes of a
  // wavefront read consecutive words.  Slice s holds sptr[s + 1] - sptr[s] incidence columns (its longest row); entry (column c,
  // lane l) is at (sptr[s] + c) * SLICE + l.  inc < 0: no incidence.
  std::vector<int> sptr, dinc;
  std::vector<unsigned> dslot;
};

// cells [nc][D + 1]; vptr / vcol: vertex graph of the nv rows (columns in any order).  false with the reason in `why` when an index
// is out of range, a column of a cell is missing from the graph or a row has more than 256 entries (8-bit positions).
inline bool build_worklist(int D, int nv, int nc, const int *cells, const int *vptr, const int *vcol, WorkList &w, std::string &why) {
  const int n1 = D + 1;
  w = WorkList();
  w.D = D;
  if ((D != 2 && D != 3) || nv < 0 || nc < 0) { why = "scalar work list: bad sizes"; return false; }
  w.nrows = nv;
  std::vector<int> count((size_t)nv + 1, 0);
  for (int e = 0; e < nc; e++)
    for (int a = 0; a < n1; a++) {
      const int r = cells[(size_t)n1 * e + a];
      if (r < 0 || r >= nv) { why = "scalar work list: vertex out of range in cell " + std::to_string(e); return false; }
      count[(size_t)r + 1]++;
    }
  w.rptr.assign((size_t)nv + 1, 0);
  for (int v = 0; v < nv; v++) {
    w.rptr[v + 1] = w.rptr[v] + count[v + 1];
    if (vptr[v + 1] - vptr[v] > 256) { why = "scalar work list: row " + std::to_string(v) + " has more than 256 entries"; return false; }
    w.maxlen = std::max(w.maxlen, vptr[v + 1] - vptr[v]);
  }
  w.ninc = w.rptr[nv];
  w.inc.assign(w.ninc, 0); w.slot.assign(w.ninc, 0u);
  std::vector<int> fill(w.rptr.begin(), w.rptr.end() - 1);
  for (int e = 0; e < nc; e++)  // ascending cells: the order inside a row
    for (int a = 0; a < n1; a++) {
      const int r = cells[(size_t)n1 * e + a];
      unsigned sl = 0;
      for (int b = 0; b < n1; b++) {
        const int col = cells[(size_t)n1 * e + b];
        int s = -1;
        for (int j = vptr[r]; j < vptr[r + 1]; j++)
          if (vcol[j] == col) { s = j - vptr[r]; break; }
        if (s < 0) { why = "scalar work list: vertex " + std::to_string(col) + " is no column of row " + std::to_string(r); return false; }
        sl |= (unsigned)s << (8 * b);
      }
      const int pos = fill[r]++;
      w.inc[pos] = e * 4 + a;
      w.slot[pos] = sl;
    }
  w.nslices = (nv + SLICE - 1) / SLICE;
  w.sptr.assign((size_t)w.nslices + 1, 0);
  for (int s = 0; s < w.nslices; s++) {
    int width = 0;
    for (int r = s * SLICE; r < nv && r < (s + 1) * SLICE; r++) width = std::max(width, w.rptr[r + 1] - w.rptr[r]);
    w.sptr[s + 1] = w.sptr[s] + width;
  }
  const size_t ncol = (size_t)w.sptr[w.nslices];
  w.dinc.assign(ncol * SLICE, -1); w.dslot.assign(ncol * SLICE, 0u);
  for (int r = 0; r < nv; r++) {
    const int s = r / SLICE, l = r % SLICE;
    for (int j = w.rptr[r]; j < w.rptr[r + 1]; j++) {
      const size_t c = (size_t)w.sptr[s] + (j - w.rptr[r]);
      w.dinc[c * SLICE + l] = w.inc[j];
      w.dslot[c * SLICE + l] = w.slot[j];
    }
  }
  return true;
}

inline bool finite(double v) { return v == v && v - v == 0.0; }

// argument checks of cfdh_scalar_enable that need no context
inline bool check_params(double D, double s, double theta, std::string &why) {
  if (!finite(D) || D < 0) { why = "the diffusivity must be finite and >= 0"; return false; }
  if (!finite(s)) { why = "the source must be finite"; return false; }
  if (!finite(theta) || !(theta > 0.0 && theta <= 1.0)) { why = "theta_c must lie in (0, 1]"; return false; }
  return true;
}

// ... and of cfdh_scalar_set_dirichlet
inline bool check_dirichlet(int64_t n, int64_t nv, const int32_t *nodes, const double *values, std::string &why) {
  if (n < 0) { why = "n must be >= 0"; return false; }
  if (n > 0 && (!nodes || !values)) { why = "null node / value array"; return false; }
  for (int64_t k = 0; k < n; k++) {
    if (nodes[k] < 0 || nodes[k] >= nv) { why = "node " + std::to_string(nodes[k]) + " out of range"; return false; }
    if (!finite(values[k])) { why = "value " + std::to_string(k) + " is not finite"; return false; }
  }
  return true;
}

}  // namespace cfdh_scalar
