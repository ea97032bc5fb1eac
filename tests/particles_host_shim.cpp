// extern "C" wrappers around csrc/cfdh_particles_host.hpp for tests/test_particles_host.py (g++, loaded with ctypes).
#include <cstring>

#include "cfdh_particles_host.hpp"

namespace {
int fail(const std::string &why, char *msg, int nmsg) {
  if (msg && nmsg > 0) { std::strncpy(msg, why.c_str(), (size_t)nmsg - 1); msg[nmsg - 1] = 0; }
  return -1;
}
}  // namespace

extern "C" {

int ph_neighbours(int D, int nv, int nc, const int *cells, int nfac, const int *fac_cell, const int *fac_local, int *nb, char *msg, int nmsg) {
  std::vector<int> out;
  std::string why;
  if (!cfdh_particles::build_neighbours(D, nv, nc, cells, nfac, fac_cell, fac_local, out, why)) return fail(why, msg, nmsg);
  std::memcpy(nb, out.data(), sizeof(int) * out.size());
  return 0;
}

int ph_affine(int D, int nc, const int *cells, const double *coords, double *aff, char *msg, int nmsg) {
  std::vector<double> out;
  std::string why;
  if (!cfdh_particles::build_affine(D, nc, cells, coords, out, why)) return fail(why, msg, nmsg);
  std::memcpy(aff, out.data(), sizeof(double) * out.size());
  return 0;
}

void ph_barycentric(int D, const double *T, const double *y, double *lam) { cfdh_particles::barycentric(D, T, y, lam); }

int ph_check_seeds(int D, long long n, const double *x, const int *cell, long long ncu, const int *cell_int, const double *aff, double t_birth, int *ci,
                   char *msg, int nmsg) {
  std::vector<int> out;
  std::string why;
  if (!cfdh_particles::check_seeds(D, n, x, cell, ncu, cell_int, aff, t_birth, out, why)) return fail(why, msg, nmsg);
  if (n > 0) std::memcpy(ci, out.data(), sizeof(int) * out.size());
  return 0;
}

int ph_constants(double *tol_inside, double *tol_seed) {
  *tol_inside = cfdh_particles::TOL_INSIDE;
  *tol_seed = cfdh_particles::TOL_SEED;
  return cfdh_particles::MAX_CROSSINGS;
}
}
