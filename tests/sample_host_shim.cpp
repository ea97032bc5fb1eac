// extern "C" wrappers around csrc/cfdh_sample_host.hpp for tests/test_sample_twin.py (g++, loaded with ctypes).
#include <cstring>

#include "cfdh_sample_host.hpp"

namespace {
cfdh_sample::Bins g_bins;
}

extern "C" {

// builds the bins and keeps them; sizes[0..7] = bins, total list length, longest list, doublings, bins per axis [3];
// lengths[0..8] = edge, first edge, lo [3], hi [3]; -1 with the reason in msg
int sh_build(int D, int nv, int nc, const double *coords, const int *cells, const int *visit, double tol, long long *sizes, double *lengths, char *msg,
             int nmsg) {
  std::string why;
  if (!cfdh_sample::build_bins(D, nv, nc, coords, cells, visit, tol, g_bins, why)) {
    if (msg && nmsg > 0) { std::strncpy(msg, why.c_str(), (size_t)nmsg - 1); msg[nmsg - 1] = 0; }
    return -1;
  }
  sizes[0] = g_bins.nbins; sizes[1] = g_bins.total; sizes[2] = g_bins.maxlen; sizes[3] = g_bins.doublings;
  lengths[0] = g_bins.edge; lengths[1] = g_bins.first_edge;
  for (int i = 0; i < 3; i++) { sizes[4 + i] = g_bins.g.nb[i]; lengths[2 + i] = g_bins.g.lo[i]; lengths[5 + i] = g_bins.g.hi[i]; }
  return 0;
}

// copies of the bins built last: ptr [bins + 1], list [total]
void sh_get(int *ptr, int *list) {
  std::memcpy(ptr, g_bins.ptr.data(), sizeof(int) * g_bins.ptr.size());
  if (!g_bins.list.empty()) std::memcpy(list, g_bins.list.data(), sizeof(int) * g_bins.list.size());
}

// bin [n] of the points x [n][D] in the bins built last; -1: outside the box
void sh_point_bins(long long n, const double *x, long long *bin) {
  for (long long k = 0; k < n; k++) bin[k] = cfdh_sample::point_bin(g_bins.g, x + (size_t)g_bins.g.D * k);
}
}
