// Cut-plane sections (cfdh_section.hip), the part built on the host.  Plain C++, no HIP: compiled with g++ by
// tests/test_section_twin.py, like cfdh_sample_host.hpp.  Under hipcc the quadrature of one entry (entry_row) is also a device
// function: the kernel and the host evaluator of the tests run the same arithmetic on the same stored decisions.
//
// Definition (include/cfdh.h).  Section k is a point o, a unit normal n and a radius r (r <= 0: unbounded).  s_v = n . (x_v - o) is
// computed by signed_dist alone, once per vertex and section, so two cells that share a vertex agree on its side: above when
// s_v >= 0, below otherwise.  A cell is cut when it has a vertex above and one below.  The polygon vertices lie on the edges from an
// above vertex a to a below vertex b at t = s_a / (s_a - s_b) from a: a segment in 2-D, a triangle (1-3 split) or the convex
// quadrilateral (a0b0, a0b1, a1b1, a1b0) (2-2 split) in 3-D, the latter as the triangles (0, 1, 2) and (0, 2, 3).  A facet in the
// plane is therefore seen from its below side only (t = 0 three times); the cell above it is not cut.  With r > 0 a polygon is
// taken whole when the mean of its vertices lies within r of o and dropped otherwise; polygons with vertices on both sides of the
// sphere are counted (straddling), taken or dropped.
//
// What is stored per taken cell is everything that was decided: the stored cell, the local edges of the polygon vertices (code),
// their t and the measures of the sub-simplices.  The device never computes a sign or a t again.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define CFDH_SECTION_HD __host__ __device__
#define CFDH_SECTION_UNROLL _Pragma("unroll")
#else
#define CFDH_SECTION_HD
#define CFDH_SECTION_UNROLL
#endif

namespace cfdh_section {

constexpr int NQ = 10;                           // doubles per section row (CFDH_SECTION_NQ)
constexpr int MAX_SECTIONS = 256;
constexpr long long MAX_ENTRIES = 0x7fffffffll;  // entries in all: the block table of the kernel has 32-bit offsets

// polygon vertices / sub-simplices stored per entry
constexpr int np_of(int D) { return D == 2 ? 2 : 4; }
constexpr int nt_of(int D) { return D == 2 ? 1 : 2; }

// code of an entry: bits 4j, 4j + 1: local vertex a of polygon vertex j in the stored cell, bits 4j + 2, 4j + 3: local vertex b;
// bits 16 .. 18: the number of polygon vertices (2, 3 or 4).  A triangle repeats its vertex 0 as vertex 3, with measure 0 for the
// second sub-triangle, so that every entry of a dimension has one shape.
CFDH_SECTION_HD inline int code_a(int code, int j) { return (code >> (4 * j)) & 3; }
CFDH_SECTION_HD inline int code_b(int code, int j) { return (code >> (4 * j + 2)) & 3; }
CFDH_SECTION_HD inline int code_n(int code) { return (code >> 16) & 7; }

struct Cut {
  int D = 2, K = 0;
  long long total = 0, maxlen = 0;  // entries in all, the longest list
  std::vector<double> normal;       // [K][3] unit normals (0 in the third slot in 2-D)
  std::vector<long long> ptr;       // [K + 1]: the entries of section k are ptr[k] .. ptr[k + 1], in ascending caller's cell index
  std::vector<int> cell, code;      // [total] stored cell, code
  std::vector<double> t;            // [total][np]
  std::vector<double> meas;         // [total][nt]
  std::vector<int> straddling;      // [K]
};

inline bool finite(double v) { return v == v && v - v == 0.0; }

// the one place where the side of a vertex is computed
inline double signed_dist(int D, const double *n, const double *o, const double *x) {
  double s = 0.0;
  for (int i = 0; i < D; i++) s += n[i] * (x[i] - o[i]);
  return s;
}

// The NQ integrals over the polygon of one entry.  U [D + 1][D], P [D + 1]: the values at the vertices of the stored cell; n: the
// unit normal (3 entries).  u . n, p and u_i are linear on the polygon, so their values at its vertices determine them, and every
// integrand has degree <= 3.  Segments: 2-point Gauss.  Triangles: the 7-point rule of degree 3 with the weights 1/20 (vertices),
// 2/15 (edge midpoints) and 9/20 (centroid).
template <int D>
CFDH_SECTION_HD inline void entry_row(int code, const double *t, const double *m, const double (&U)[D + 1][D], const double (&P)[D + 1], const double *n,
                                      double rho, double (&row)[NQ]) {
  constexpr int NP = np_of(D), NT = nt_of(D), NV = D + 2;  // per polygon vertex: u [D], p, u . n
  double val[NP][NV];
  CFDH_SECTION_UNROLL
  for (int j = 0; j < NP; j++) {
    // the barycentric row of polygon vertex j in the cell: 1 - t at a, t at b.  Selected weights and statically indexed values: no
    // register array is indexed by a or b
    const int a = code_a(code, j), b = code_b(code, j);
    double lam[D + 1];
    CFDH_SECTION_UNROLL
    for (int k = 0; k <= D; k++) lam[k] = (a == k ? 1.0 - t[j] : 0.0) + (b == k ? t[j] : 0.0);
    double w = 0.0;
    CFDH_SECTION_UNROLL
    for (int i = 0; i < D; i++) {
      double v = 0.0;
      CFDH_SECTION_UNROLL
      for (int k = 0; k <= D; k++) v += lam[k] * U[k][i];
      val[j][i] = v;
      w += n[i] * v;
    }
    double pv = 0.0;
    CFDH_SECTION_UNROLL
    for (int k = 0; k <= D; k++) pv += lam[k] * P[k];
    val[j][D] = pv;
    val[j][D + 1] = w;
  }
  CFDH_SECTION_UNROLL
  for (int s = 0; s < NQ; s++) row[s] = 0.0;
  // f: the values at one quadrature point, wq: its weight times the measure
  auto add = [&](const double (&f)[NV], double wq) {
    double u2 = 0.0;
    CFDH_SECTION_UNROLL
    for (int i = 0; i < D; i++) {
      u2 += f[i] * f[i];
      row[7 + i] += wq * f[i];
    }
    const double p = f[D], w = f[D + 1];
    row[1] += wq * w;
    row[2] += wq * p;
    row[3] += wq * (w * w);
    row[4] += wq * u2;
    row[5] += wq * (p * w);
    row[6] += wq * (0.5 * rho * u2 * w);
  };
  if constexpr (D == 2) {
    const double g0 = 0.5 - 0.28867513459481288225, g1 = 0.5 + 0.28867513459481288225;  // (1 -+ 1 / sqrt 3) / 2
    double f[NV];
    CFDH_SECTION_UNROLL
    for (int c = 0; c < NV; c++) f[c] = g1 * val[0][c] + g0 * val[1][c];
    add(f, 0.5 * m[0]);
    CFDH_SECTION_UNROLL
    for (int c = 0; c < NV; c++) f[c] = g0 * val[0][c] + g1 * val[1][c];
    add(f, 0.5 * m[0]);
    row[0] = m[0];
  } else {
    CFDH_SECTION_UNROLL
    for (int tri = 0; tri < NT; tri++) {
      const int i0 = 0, i1 = tri + 1, i2 = tri + 2;
      const double mt = m[tri];
      double f[NV];
      add(val[i0], mt * (1.0 / 20.0));
      add(val[i1], mt * (1.0 / 20.0));
      add(val[i2], mt * (1.0 / 20.0));
      CFDH_SECTION_UNROLL
      for (int c = 0; c < NV; c++) f[c] = 0.5 * (val[i0][c] + val[i1][c]);
      add(f, mt * (2.0 / 15.0));
      CFDH_SECTION_UNROLL
      for (int c = 0; c < NV; c++) f[c] = 0.5 * (val[i1][c] + val[i2][c]);
      add(f, mt * (2.0 / 15.0));
      CFDH_SECTION_UNROLL
      for (int c = 0; c < NV; c++) f[c] = 0.5 * (val[i2][c] + val[i0][c]);
      add(f, mt * (2.0 / 15.0));
      CFDH_SECTION_UNROLL
      for (int c = 0; c < NV; c++) f[c] = (val[i0][c] + val[i1][c] + val[i2][c]) * (1.0 / 3.0);
      add(f, mt * (9.0 / 20.0));
      row[0] += mt;
    }
  }
}

// coords [nv][D], cells [nc][D + 1] (the stored cells), caller_index [nc]: the caller's index of stored cell e (a permutation;
// null: the identity), flipped [nc]: 1 where the stored cell has its last two vertices swapped against the caller's (null: none).
// planes [K][2 D + 1]: origin, normal (any non-zero length), radius.  The lists come out in ascending caller's index, and the
// polygon of a cell is built from its vertices in the caller's local order, so neither depends on how the cells are stored.
// max_entries: the refusal limit (the tests lower it).
inline bool build_cut(int D, int nv, int nc, const int *cells, const double *coords, const int *caller_index, const unsigned char *flipped, int K,
                      const double *planes, Cut &C, std::string &why, long long max_entries = MAX_ENTRIES) {
  const int n1 = D + 1, NP = np_of(D), NT = nt_of(D), stride = 2 * D + 1;
  C = Cut();
  C.D = D;
  if ((D != 2 && D != 3) || nv < 0 || nc < 0) { why = "section cut: bad sizes"; return false; }
  if (K < 0 || K > MAX_SECTIONS) { why = "section cut: K must lie in [0, 256]"; return false; }
  if (K > 0 && !planes) { why = "section cut: planes is NULL"; return false; }
  C.K = K;
  C.normal.assign((size_t)3 * K, 0.0);
  for (int k = 0; k < K; k++) {
    const double *pl = planes + (size_t)stride * k;
    for (int i = 0; i < stride; i++)
      if (!finite(pl[i])) { why = "section cut: entry " + std::to_string(i) + " of section " + std::to_string(k) + " is not finite"; return false; }
    double big = 0.0, len = 0.0;
    for (int i = 0; i < D; i++) big = std::max(big, std::fabs(pl[D + i]));
    if (!(big > 0.0)) { why = "section cut: the normal of section " + std::to_string(k) + " is zero"; return false; }
    for (int i = 0; i < D; i++) len += (pl[D + i] / big) * (pl[D + i] / big);  // scaled: no overflow, no underflow to zero
    len = std::sqrt(len);
    for (int i = 0; i < D; i++) C.normal[(size_t)3 * k + i] = (pl[D + i] / big) / len;
  }
  // stored cells in ascending caller's index
  std::vector<int> visit((size_t)nc);
  if (caller_index) {
    std::vector<char> seen((size_t)nc, 0);
    for (int e = 0; e < nc; e++) {
      const int u = caller_index[e];
      if (u < 0 || u >= nc || seen[u]) { why = "section cut: caller_index is no permutation of the cells"; return false; }
      seen[u] = 1;
      visit[u] = e;
    }
  } else {
    for (int e = 0; e < nc; e++) visit[e] = e;
  }
  for (size_t k = 0; k < (size_t)nc * n1; k++)
    if (cells[k] < 0 || cells[k] >= nv) { why = "section cut: vertex out of range in cell " + std::to_string(k / n1); return false; }
  for (size_t k = 0; k < (size_t)nv * D; k++)
    if (!finite(coords[k])) { why = "section cut: non-finite coordinate of vertex " + std::to_string(k / D); return false; }

  C.ptr.assign((size_t)K + 1, 0);
  C.straddling.assign((size_t)K, 0);
  std::vector<double> s((size_t)nv);
  for (int k = 0; k < K; k++) {
    const double *o = planes + (size_t)stride * k, *n = &C.normal[(size_t)3 * k];
    const double r = o[2 * D];
    for (int v = 0; v < nv; v++) s[v] = signed_dist(D, n, o, coords + (size_t)D * v);
    for (int kk = 0; kk < nc; kk++) {
      const int e = visit[kk];
      const int *cv = cells + (size_t)n1 * e;
      // local vertices in the caller's order: loc[a] is the stored local index of the caller's local vertex a
      int loc[4], ab[4], bl[4], na = 0, nb = 0;
      for (int a = 0; a < n1; a++) loc[a] = a;
      if (flipped && flipped[e]) std::swap(loc[n1 - 2], loc[n1 - 1]);
      for (int a = 0; a < n1; a++) {
        if (s[cv[loc[a]]] >= 0.0) ab[na++] = loc[a];
        else bl[nb++] = loc[a];
      }
      if (na == 0 || nb == 0) continue;
      int pa[4], pb[4], npoly;
      if (D == 2) {
        npoly = 2;
        if (na == 1) { pa[0] = ab[0]; pb[0] = bl[0]; pa[1] = ab[0]; pb[1] = bl[1]; }
        else { pa[0] = ab[0]; pb[0] = bl[0]; pa[1] = ab[1]; pb[1] = bl[0]; }
      } else if (na == 1) {
        npoly = 3;
        for (int j = 0; j < 3; j++) { pa[j] = ab[0]; pb[j] = bl[j]; }
      } else if (nb == 1) {
        npoly = 3;
        for (int j = 0; j < 3; j++) { pa[j] = ab[j]; pb[j] = bl[0]; }
      } else {
        npoly = 4;
        pa[0] = ab[0]; pb[0] = bl[0];
        pa[1] = ab[0]; pb[1] = bl[1];
        pa[2] = ab[1]; pb[2] = bl[1];
        pa[3] = ab[1]; pb[3] = bl[0];
      }
      double tt[4], X[4][3], cen[3] = {0, 0, 0};
      for (int j = 0; j < npoly; j++) {
        const int va = cv[pa[j]], vb = cv[pb[j]];
        tt[j] = s[va] / (s[va] - s[vb]);
        for (int i = 0; i < 3; i++) X[j][i] = 0.0;
        for (int i = 0; i < D; i++) {
          const double xa = coords[(size_t)D * va + i], xb = coords[(size_t)D * vb + i];
          X[j][i] = xa + tt[j] * (xb - xa);
          cen[i] += X[j][i];
        }
      }
      for (int i = 0; i < D; i++) cen[i] /= (double)npoly;
      if (r > 0.0) {
        auto dist2 = [&](const double *x) {
          double d2 = 0.0;
          for (int i = 0; i < D; i++) d2 += (x[i] - o[i]) * (x[i] - o[i]);
          return d2;
        };
        int in = 0;
        for (int j = 0; j < npoly; j++) in += dist2(X[j]) <= r * r ? 1 : 0;
        if (in != 0 && in != npoly) C.straddling[k]++;
        if (!(dist2(cen) <= r * r)) continue;
      }
      double m[2] = {0.0, 0.0};
      if (D == 2) {
        m[0] = std::hypot(X[1][0] - X[0][0], X[1][1] - X[0][1]);
      } else {
        for (int tri = 0; tri < npoly - 2; tri++) {
          const double *A = X[0], *B = X[tri + 1], *Cc = X[tri + 2];
          const double e1[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]}, e2[3] = {Cc[0] - A[0], Cc[1] - A[1], Cc[2] - A[2]};
          const double c0 = e1[1] * e2[2] - e1[2] * e2[1], c1 = e1[2] * e2[0] - e1[0] * e2[2], c2 = e1[0] * e2[1] - e1[1] * e2[0];
          m[tri] = 0.5 * std::sqrt(c0 * c0 + c1 * c1 + c2 * c2);
        }
      }
      if ((long long)C.cell.size() >= max_entries) { why = "section cut: more than " + std::to_string(max_entries) + " entries in all"; C = Cut(); return false; }
      int code = npoly << 16;
      for (int j = 0; j < NP; j++) {
        const int jj = j < npoly ? j : 0;  // a triangle repeats its vertex 0
        code |= (pa[jj] | (pb[jj] << 2)) << (4 * j);
        C.t.push_back(tt[jj]);
      }
      for (int j = 0; j < NT; j++) C.meas.push_back(m[j]);
      C.cell.push_back(e);
      C.code.push_back(code);
    }
    C.ptr[k + 1] = (long long)C.cell.size();
    C.maxlen = std::max(C.maxlen, C.ptr[k + 1] - C.ptr[k]);
  }
  C.total = (long long)C.cell.size();
  return true;
}

// The rows of every section on the host, entry by entry in list order, with the arithmetic of the kernel per entry (the sums over the
// entries are taken in another order there).  u [nv][D], p [nv] in the numbering of `cells`; out [K][NQ].
template <int D>
inline void eval_rows_d(const Cut &C, const int *cells, const double *u, const double *p, double rho, double *out) {
  constexpr int NP = np_of(D), NT = nt_of(D);
  for (int k = 0; k < C.K; k++) {
    double acc[NQ];
    for (int s = 0; s < NQ; s++) acc[s] = 0.0;
    for (long long i = C.ptr[k]; i < C.ptr[k + 1]; i++) {
      double U[D + 1][D], P[D + 1], row[NQ];
      for (int a = 0; a <= D; a++) {
        const int v = cells[(size_t)(D + 1) * C.cell[i] + a];
        for (int j = 0; j < D; j++) U[a][j] = u[(size_t)D * v + j];
        P[a] = p[v];
      }
      entry_row<D>(C.code[i], &C.t[(size_t)NP * i], &C.meas[(size_t)NT * i], U, P, &C.normal[(size_t)3 * k], rho, row);
      for (int s = 0; s < NQ; s++) acc[s] += row[s];
    }
    for (int s = 0; s < NQ; s++) out[(size_t)NQ * k + s] = acc[s];
  }
}
inline void eval_rows(const Cut &C, const int *cells, const double *u, const double *p, double rho, double *out) {
  if (C.D == 3) eval_rows_d<3>(C, cells, u, p, rho, out);
  else eval_rows_d<2>(C, cells, u, p, rho, out);
}

}  // namespace cfdh_section
