// Tables and argument checks of the Lagrangian particle tracker (cfdh_particles.hip), built on the host.  Plain C++, no HIP:
// compiled with g++ by tests/test_particles_host.py, like cfdh_mesh_host.hpp.
//
// Two tables over the device-ordered cells of a closed-form P1 context (d = gdim, local facet f is opposite local vertex f):
//   nb  [nc][d + 1]      the cell across facet f, or -1 - k for an exterior facet, k its index in the context's facet list
//   aff [nc][d d + d]    grad(lambda_1) .. grad(lambda_d) (d doubles each), then the coordinates of local vertex 0:
//                        lambda_a(y) = grad(lambda_a) . (y - X_0) for a >= 1, lambda_0 = 1 - sum_{a >= 1} lambda_a
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <string>
#include <vector>

namespace cfdh_particles {

constexpr int MAX_CROSSINGS = 64;     // cell crossings of one walk; one more and the particle is lost
constexpr double TOL_INSIDE = 1e-12;  // the walk ends in a cell with every lambda >= -TOL_INSIDE
constexpr double TOL_SEED = 1e-9;     // a seed lies in its cell with every lambda >= -TOL_SEED

inline int aff_stride(int D) { return D * D + D; }
inline bool finite(double v) { return v == v && v - v == 0.0; }

// cells [nc][D + 1] (vertex ids < nv); facets k < nfac: exterior facet fac_local[k] of cell fac_cell[k].  false with the reason
// in `why` when an index is out of range, a facet is shared by more than two cells, a facet of the list is not exterior or an
// exterior facet is missing from the list.
inline bool build_neighbours(int D, int nv, int nc, const int *cells, int nfac, const int *fac_cell, const int *fac_local, std::vector<int> &nb,
                             std::string &why) {
  const int n1 = D + 1;
  if ((D != 2 && D != 3) || nv < 0 || nc < 0 || nfac < 0) { why = "particle tables: bad sizes"; return false; }
  struct Key { std::array<int, 3> v; int cell, f; };
  std::vector<Key> keys((size_t)nc * n1);
  for (int e = 0; e < nc; e++)
    for (int f = 0; f < n1; f++) {
      Key &k = keys[(size_t)e * n1 + f];
      k.v = {-1, -1, -1};
      int q = 0;
      for (int a = 0; a < n1; a++) {
        const int v = cells[(size_t)e * n1 + a];
        if (v < 0 || v >= nv) { why = "particle tables: vertex out of range in cell " + std::to_string(e); return false; }
        if (a != f) k.v[q++] = v;
      }
      std::sort(k.v.begin(), k.v.begin() + D);
      k.cell = e; k.f = f;
    }
  std::sort(keys.begin(), keys.end(), [](const Key &a, const Key &b) { return a.v != b.v ? a.v < b.v : (a.cell != b.cell ? a.cell < b.cell : a.f < b.f); });
  const int EXT = INT32_MIN;  // exterior, facet index not known yet
  nb.assign((size_t)nc * n1, EXT);
  for (size_t i = 0; i < keys.size();) {
    size_t j = i + 1;
    while (j < keys.size() && keys[j].v == keys[i].v) j++;
    if (j - i > 2) { why = "particle tables: a facet of cell " + std::to_string(keys[i].cell) + " is shared by more than two cells"; return false; }
    if (j - i == 2) {
      nb[(size_t)keys[i].cell * n1 + keys[i].f] = keys[i + 1].cell;
      nb[(size_t)keys[i + 1].cell * n1 + keys[i + 1].f] = keys[i].cell;
    }
    i = j;
  }
  for (int k = 0; k < nfac; k++) {
    const int e = fac_cell[k], f = fac_local[k];
    if (e < 0 || e >= nc || f < 0 || f >= n1) { why = "particle tables: facet " + std::to_string(k) + " out of range"; return false; }
    int &slot = nb[(size_t)e * n1 + f];
    if (slot != EXT) { why = "particle tables: facet " + std::to_string(k) + " of the facet list is interior or listed twice"; return false; }
    slot = -1 - k;
  }
  for (size_t i = 0; i < nb.size(); i++)
    if (nb[i] == EXT) { why = "particle tables: an exterior facet of cell " + std::to_string(i / n1) + " is missing from the facet list"; return false; }
  return true;
}

// coords [nv][D]; aff [nc][aff_stride(D)].  false for a cell without volume.
inline bool build_affine(int D, int nc, const int *cells, const double *coords, std::vector<double> &aff, std::string &why) {
  const int n1 = D + 1, st = aff_stride(D);
  aff.assign((size_t)nc * st, 0.0);
  for (int e = 0; e < nc; e++) {
    const int *v = cells + (size_t)e * n1;
    double r[3][3] = {};
    for (int a = 1; a <= D; a++)
      for (int i = 0; i < D; i++) r[a - 1][i] = coords[(size_t)D * v[a] + i] - coords[(size_t)D * v[0] + i];
    double *g = &aff[(size_t)e * st];
    double det;
    if (D == 2) {
      det = r[0][0] * r[1][1] - r[0][1] * r[1][0];
      g[0] = r[1][1] / det; g[1] = -r[1][0] / det;
      g[2] = -r[0][1] / det; g[3] = r[0][0] / det;
    } else {
      double c0[3], c1[3], c2[3];  // r1 x r2, r2 x r0, r0 x r1
      c0[0] = r[1][1] * r[2][2] - r[1][2] * r[2][1]; c0[1] = r[1][2] * r[2][0] - r[1][0] * r[2][2]; c0[2] = r[1][0] * r[2][1] - r[1][1] * r[2][0];
      c1[0] = r[2][1] * r[0][2] - r[2][2] * r[0][1]; c1[1] = r[2][2] * r[0][0] - r[2][0] * r[0][2]; c1[2] = r[2][0] * r[0][1] - r[2][1] * r[0][0];
      c2[0] = r[0][1] * r[1][2] - r[0][2] * r[1][1]; c2[1] = r[0][2] * r[1][0] - r[0][0] * r[1][2]; c2[2] = r[0][0] * r[1][1] - r[0][1] * r[1][0];
      det = r[0][0] * c0[0] + r[0][1] * c0[1] + r[0][2] * c0[2];
      for (int i = 0; i < 3; i++) { g[i] = c0[i] / det; g[3 + i] = c1[i] / det; g[6 + i] = c2[i] / det; }
    }
    if (!(det != 0.0) || !finite(det)) { why = "particle tables: cell " + std::to_string(e) + " has no volume"; return false; }
    for (int i = 0; i < D; i++) g[D * D + i] = coords[(size_t)D * v[0] + i];
  }
  return true;
}

// lambda_0 .. lambda_D of y in the cell whose table row is T (the arithmetic of the kernel, operation by operation)
inline void barycentric(int D, const double *T, const double *y, double *lam) {
  double r[3] = {0, 0, 0};
  for (int i = 0; i < D; i++) r[i] = y[i] - T[D * D + i];
  double s = 0.0;
  for (int a = 1; a <= D; a++) {
    double l = 0.0;
    for (int i = 0; i < D; i++) l = l + T[(a - 1) * D + i] * r[i];
    lam[a] = l;
    s = s + l;
  }
  lam[0] = 1.0 - s;
}

// argument checks of cfdh_particles_seed: x [n][D], cell [n] in the caller's numbering (cell_int: caller's -> device-ordered cell,
// -1 for a cell the context does not hold).  On success `ci` holds the device-ordered cells.
inline bool check_seeds(int D, int64_t n, const double *x, const int32_t *cell, int64_t ncu, const int *cell_int, const double *aff, double t_birth,
                        std::vector<int> &ci, std::string &why) {
  if (n < 0) { why = "n must be >= 0"; return false; }
  if (n > 0 && (!x || !cell)) { why = "null position / cell array"; return false; }
  if (!finite(t_birth)) { why = "t_birth is not finite"; return false; }
  ci.assign((size_t)n, 0);
  for (int64_t k = 0; k < n; k++) {
    for (int i = 0; i < D; i++)
      if (!finite(x[(size_t)D * k + i])) { why = "position " + std::to_string(k) + " is not finite"; return false; }
    if (cell[k] < 0 || cell[k] >= ncu || cell_int[cell[k]] < 0) { why = "cell " + std::to_string(cell[k]) + " of particle " + std::to_string(k) + " out of range"; return false; }
    const int e = cell_int[cell[k]];
    double lam[4];
    barycentric(D, aff + (size_t)e * aff_stride(D), x + (size_t)D * k, lam);
    for (int a = 0; a <= D; a++)
      if (!(lam[a] >= -TOL_SEED)) { why = "particle " + std::to_string(k) + " does not lie in cell " + std::to_string(cell[k]); return false; }
    ci[(size_t)k] = e;
  }
  return true;
}

}  // namespace cfdh_particles
