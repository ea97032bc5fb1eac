// Stand-alone run of csrc/cfdh_particles_host.hpp for tests/test_particles_host.py, built with -fsanitize=address,undefined: reads a
// mesh (header of int32: D nv nc nfac; then cells, fac_cell, fac_local as int32 and coords as doubles), builds the neighbour and
// affine tables, checks them against their definitions and runs the seed checks; prints "ok ..." and returns 0, or says what failed.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "cfdh_particles_host.hpp"

static int die(const char *what, const std::string &why = "") {
  std::printf("FAILED %s %s\n", what, why.c_str());
  return 1;
}

template <class T>
static bool read_vec(std::FILE *f, std::vector<T> &v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char **argv) {
  if (argc < 2) return die("usage");
  std::FILE *f = std::fopen(argv[1], "rb");
  if (!f) return die("open");
  int hd[4];
  if (std::fread(hd, sizeof(int), 4, f) != 4) return die("header");
  const int D = hd[0], nv = hd[1], nc = hd[2], nfac = hd[3], n1 = D + 1;
  std::vector<int> cells, fcell, flocal;
  std::vector<double> coords;
  if (!read_vec(f, cells, (size_t)nc * n1) || !read_vec(f, fcell, (size_t)nfac) || !read_vec(f, flocal, (size_t)nfac) || !read_vec(f, coords, (size_t)nv * D))
    return die("read");
  std::fclose(f);

  std::string why;
  std::vector<int> nb;
  if (!cfdh_particles::build_neighbours(D, nv, nc, cells.data(), nfac, fcell.data(), flocal.data(), nb, why)) return die("neighbours", why);
  long long interior = 0, exterior = 0;
  std::vector<int> seen((size_t)nfac, 0);
  for (int e = 0; e < nc; e++)
    for (int fct = 0; fct < n1; fct++) {
      const int o = nb[(size_t)e * n1 + fct];
      if (o >= 0) {
        if (o >= nc || o == e) return die("neighbour out of range");
        int back = 0;
        for (int g = 0; g < n1; g++) back += nb[(size_t)o * n1 + g] == e;
        if (back != 1) return die("pairing not symmetric");
        // the two cells share every vertex of the facet
        for (int a = 0; a < n1; a++) {
          if (a == fct) continue;
          bool found = false;
          for (int b = 0; b < n1; b++) found = found || cells[(size_t)o * n1 + b] == cells[(size_t)e * n1 + a];
          if (!found) return die("neighbour does not hold the facet");
        }
        interior++;
      } else {
        const int k = -1 - o;
        if (k < 0 || k >= nfac || fcell[k] != e || flocal[k] != fct || seen[k]++) return die("exterior facet index");
        exterior++;
      }
    }
  if (exterior != nfac || interior % 2) return die("facet counts");

  std::vector<double> aff;
  if (!cfdh_particles::build_affine(D, nc, cells.data(), coords.data(), aff, why)) return die("affine", why);
  const int st = cfdh_particles::aff_stride(D);
  double worst = 0.0;
  std::vector<double> cen((size_t)nc * D, 0.0);
  for (int e = 0; e < nc; e++)
    for (int b = 0; b < n1; b++) {
      double lam[4];
      const double *y = &coords[(size_t)D * cells[(size_t)e * n1 + b]];
      cfdh_particles::barycentric(D, &aff[(size_t)e * st], y, lam);
      for (int a = 0; a < n1; a++) worst = std::fmax(worst, std::fabs(lam[a] - (a == b ? 1.0 : 0.0)));
      for (int i = 0; i < D; i++) cen[(size_t)e * D + i] += y[i] / n1;
    }
  if (!(worst <= 1e-12)) return die("lambda at the vertices");

  // seed checks: centroids in their cells pass, in the next cell they do not, nor does a NaN or a cell out of range
  std::vector<int> ident((size_t)nc), cell((size_t)nc), ci;
  for (int e = 0; e < nc; e++) ident[e] = cell[e] = e;
  if (!cfdh_particles::check_seeds(D, nc, cen.data(), cell.data(), nc, ident.data(), aff.data(), 0.0, ci, why)) return die("seeds", why);
  for (int e = 0; e < nc; e++)
    if (ci[e] != e) return die("seed cells");
  if (nc > 1) {
    for (int e = 0; e < nc; e++) cell[e] = (e + 1) % nc;
    if (cfdh_particles::check_seeds(D, nc, cen.data(), cell.data(), nc, ident.data(), aff.data(), 0.0, ci, why)) return die("seeds in the wrong cells accepted");
  }
  cell[0] = nc;
  if (cfdh_particles::check_seeds(D, 1, cen.data(), cell.data(), nc, ident.data(), aff.data(), 0.0, ci, why)) return die("cell out of range accepted");
  cell[0] = 0;
  cen[0] = std::nan("");
  if (cfdh_particles::check_seeds(D, 1, cen.data(), cell.data(), nc, ident.data(), aff.data(), 0.0, ci, why)) return die("NaN accepted");

  // a facet list with a hole, and one with an interior facet, are refused
  if (nfac > 0) {
    std::vector<int> nb2;
    if (cfdh_particles::build_neighbours(D, nv, nc, cells.data(), nfac - 1, fcell.data(), flocal.data(), nb2, why)) return die("missing exterior facet accepted");
  }
  std::printf("ok %lld interior %lld exterior\n", interior / 2, exterior);
  return 0;
}
