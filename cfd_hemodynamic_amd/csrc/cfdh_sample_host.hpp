// Search structure of the point sampler (cfdh_sample.hip), built on the host.  Plain C++, no HIP: compiled with g++ by
// tests/test_sample_twin.py, like cfdh_flow_host.hpp.  Under hipcc the two small functions the locate kernel shares with the
// builder (the bin of a coordinate, the bin of a point) are also device functions, so that builder and kernel cannot disagree on
// the bin of a point.
//
// A uniform grid of cubic bins over the bounding box of the mesh.  Per bin the cells whose (inflated) bounding box overlaps the
// bin, in CSR, in ascending caller's cell index: a lane that scans the list of its point's bin in order and stops at the first
// cell that holds the point has found the lowest-indexed such cell, which is the definition of include/cfdh.h.
//
// Inflation.  A point with every barycentric coordinate >= -tol can lie outside the cell's box: put 1 + d tol on the vertex with
// the largest i-th coordinate and -tol on the d others, and x_i exceeds the box by tol times the sum of the d distances to that
// vertex, at most d tol times the box's extent.  That is the extreme case (x_i is linear in lambda), so a pad of d tol times the
// box's diagonal covers every such point; 8 machine epsilons of the diagonal are added for the rounding of lambda itself.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define CFDH_SAMPLE_HD __host__ __device__
#else
#define CFDH_SAMPLE_HD
#endif

namespace cfdh_sample {

constexpr int LIST_FACTOR = 16;            // the lists hold at most LIST_FACTOR nc entries in all
constexpr long long MAX_BINS = 1ll << 26;  // ... and there are at most that many bins (a thin tree in a large box)
constexpr double TOL_MAX = 1e-3;
constexpr long long MAX_ENTRIES = 0x7fffffffll;  // the CSR offsets are 32-bit: a mesh whose lists would be longer is refused

// what the kernel needs of the grid, passed by value
struct BinGrid {
  int D = 2;
  int nb[3] = {1, 1, 1};
  double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};  // the box of all inflated cell boxes
  double inv = 0.0;                             // 1 / bin edge
};

struct Bins {
  BinGrid g;
  double edge = 0.0, first_edge = 0.0, tol = 0.0;  // first_edge: the median cell-box edge the doubling started from
  int doublings = 0, maxlen = 0;                   // maxlen: the longest list
  long long nbins = 0, total = 0;
  std::vector<int> ptr, list;                      // cells of bin b: list[ptr[b] .. ptr[b + 1]), stored cell ids
};

inline bool finite(double v) { return v == v && v - v == 0.0; }

// bin of coordinate x on one axis, x inside [lo, hi].  Monotone in x (a rounded subtraction and a rounded product are), so every
// x of an interval [a, b] falls into [bin_of(a), bin_of(b)]: the lists are complete without any slack.
CFDH_SAMPLE_HD inline int bin_of(double x, double lo, double inv, int nb) {
  const double f = floor((x - lo) * inv);
  int i = f >= (double)nb ? nb - 1 : (int)f;
  return i < 0 ? 0 : i;
}

// bin of a point; -1 outside the box (and for a NaN)
CFDH_SAMPLE_HD inline long long point_bin(const BinGrid &g, const double *x) {
  long long b = 0, stride = 1;
  for (int a = 0; a < g.D; a++) {
    if (!(x[a] >= g.lo[a] && x[a] <= g.hi[a])) return -1;
    b += stride * bin_of(x[a], g.lo[a], g.inv, g.nb[a]);
    stride *= g.nb[a];
  }
  return b;
}

// coords [nv][D], cells [nc][D + 1] (the stored cells).  `visit` (a permutation of 0 .. nc - 1; null: the identity) names the
// stored cells in ascending caller's index, as for cfdh_flow::build_index: the lists come out in that order.
inline bool build_bins(int D, int nv, int nc, const double *coords, const int *cells, const int *visit, double tol, Bins &B, std::string &why) {
  const int n1 = D + 1;
  B = Bins();
  B.g.D = D;
  B.tol = tol;
  if ((D != 2 && D != 3) || nv < 0 || nc < 0) { why = "sample bins: bad sizes"; return false; }
  if (!finite(tol) || tol < 0.0 || tol > TOL_MAX) { why = "sample bins: tol must lie in [0, 1e-3]"; return false; }
  // every cell is in at least one bin, and the doubling stops at the first total <= LIST_FACTOR nc, which may be that large
  if ((long long)LIST_FACTOR * nc > MAX_ENTRIES) { why = "sample bins: more than 2^31 / 16 cells (the lists have 32-bit offsets)"; return false; }
  std::vector<double> box((size_t)nc * 2 * D), longest((size_t)nc);
  std::vector<char> seen(visit ? (size_t)nc : 0, 0);
  for (int k = 0; k < nc; k++) {
    const int e = visit ? visit[k] : k;
    if (e < 0 || e >= nc || (visit && seen[e])) { why = "sample bins: visit is no permutation of the cells"; return false; }
    if (visit) seen[e] = 1;
  }
  for (int e = 0; e < nc; e++) {
    double mn[3], mx[3], diag = 0.0, edge = 0.0;
    for (int a = 0; a < n1; a++) {
      const int v = cells[(size_t)n1 * e + a];
      if (v < 0 || v >= nv) { why = "sample bins: vertex out of range in cell " + std::to_string(e); return false; }
      for (int i = 0; i < D; i++) {
        const double xi = coords[(size_t)D * v + i];
        if (!finite(xi)) { why = "sample bins: non-finite coordinate of vertex " + std::to_string(v); return false; }
        if (a == 0 || xi < mn[i]) mn[i] = xi;
        if (a == 0 || xi > mx[i]) mx[i] = xi;
      }
    }
    for (int i = 0; i < D; i++) { diag += (mx[i] - mn[i]) * (mx[i] - mn[i]); edge = std::max(edge, mx[i] - mn[i]); }
    const double pad = (D * tol + 8.0 * 2.220446049250313e-16) * std::sqrt(diag);
    for (int i = 0; i < D; i++) {
      box[(size_t)2 * D * e + i] = mn[i] - pad;
      box[(size_t)2 * D * e + D + i] = mx[i] + pad;
      if (e == 0 || mn[i] - pad < B.g.lo[i]) B.g.lo[i] = mn[i] - pad;
      if (e == 0 || mx[i] + pad > B.g.hi[i]) B.g.hi[i] = mx[i] + pad;
    }
    longest[e] = edge;
  }
  double extent = 0.0;
  for (int i = 0; i < D; i++) extent = std::max(extent, B.g.hi[i] - B.g.lo[i]);
  if (nc > 0) {
    std::nth_element(longest.begin(), longest.begin() + nc / 2, longest.end());
    B.edge = longest[nc / 2];
  }
  if (!(B.edge > 0.0)) B.edge = extent > 0.0 ? extent : 1.0;
  B.first_edge = B.edge;
  // first and last bin of cell e on axis i
  auto span = [&](int e, int i, int &b0, int &b1) {
    b0 = bin_of(box[(size_t)2 * D * e + i], B.g.lo[i], B.g.inv, B.g.nb[i]);
    b1 = bin_of(box[(size_t)2 * D * e + D + i], B.g.lo[i], B.g.inv, B.g.nb[i]);
  };
  for (;; B.edge *= 2.0, B.doublings++) {
    B.g.inv = 1.0 / B.edge;
    bool fits = true;
    B.nbins = 1;
    for (int i = 0; i < 3; i++) B.g.nb[i] = 1;
    for (int i = 0; i < D && fits; i++) {
      const double f = std::floor((B.g.hi[i] - B.g.lo[i]) * B.g.inv);
      fits = f < (double)MAX_BINS;
      if (fits) { B.g.nb[i] = (int)f + 1; B.nbins *= B.g.nb[i]; fits = B.nbins <= MAX_BINS; }
    }
    if (!fits) continue;
    B.total = 0;
    for (int e = 0; e < nc && B.total <= (long long)LIST_FACTOR * nc; e++) {
      long long m = 1;
      for (int i = 0; i < D; i++) { int b0, b1; span(e, i, b0, b1); m *= b1 - b0 + 1; }
      B.total += m;
    }
    if (B.total <= (long long)LIST_FACTOR * nc) break;  // one bin per axis holds every cell once: the loop ends
  }
  B.ptr.assign((size_t)B.nbins + 1, 0);
  auto each_bin = [&](int e, auto &&f) {
    int b0[3] = {0, 0, 0}, b1[3] = {0, 0, 0};
    for (int i = 0; i < D; i++) span(e, i, b0[i], b1[i]);
    for (int k = b0[2]; k <= b1[2]; k++)
      for (int j = b0[1]; j <= b1[1]; j++)
        for (int i = b0[0]; i <= b1[0]; i++) f((size_t)i + (size_t)B.g.nb[0] * ((size_t)j + (size_t)B.g.nb[1] * (size_t)k));
  };
  for (int e = 0; e < nc; e++) each_bin(e, [&](size_t b) { B.ptr[b + 1]++; });
  for (long long b = 0; b < B.nbins; b++) {
    B.maxlen = std::max(B.maxlen, B.ptr[b + 1]);
    B.ptr[b + 1] += B.ptr[b];
  }
  B.list.assign((size_t)B.total, 0);
  std::vector<int> fill(B.ptr.begin(), B.ptr.end() - 1);
  for (int k = 0; k < nc; k++) {  // in visiting order: ascending caller's index inside every list
    const int e = visit ? visit[k] : k;
    each_bin(e, [&](size_t b) { B.list[fill[b]++] = e; });
  }
  return true;
}

}  // namespace cfdh_sample
