// extern "C" face of csrc/cfdh_traction_host.hpp for test_traction_host.py (g++, ctypes).  th_build keeps the list it built; th_get
// copies it into arrays the caller sized from th_build's `sizes` (rows, pairs, slices, pair columns of the sliced layout).
#include <cstdio>
#include <cstring>

#include "cfdh_traction_host.hpp"

namespace T = cfdh_traction;

static T::WorkList g_list;

template <class V>
static void put(const std::vector<V> &v, V *out) {
  if (!v.empty()) memcpy(out, v.data(), v.size() * sizeof(V));
}

extern "C" {

int th_build(int D, int nv, int nc, const int *cells, int nfac, const int *fcell, const int *flocal, const int *fmarker, int nb, const int *markers,
             unsigned tangential, const int *vptr, const int *vcol, int *sizes, char *msg, int len) {
  std::string why;
  if (!T::build_worklist(D, nv, nc, cells, nfac, fcell, flocal, fmarker, nb, markers, tangential, vptr, vcol, g_list, why)) {
    snprintf(msg, len, "%s", why.c_str());
    return -1;
  }
  sizes[0] = g_list.nrows; sizes[1] = g_list.npairs; sizes[2] = g_list.nslices; sizes[3] = g_list.sptr.empty() ? 0 : g_list.sptr.back();
  return 0;
}
void th_get(int *row, int *rptr, int *pcell, int *pmeta, int *pslot, int *sptr, int *dcell, int *dmeta, int *dslot) {
  put(g_list.row, row); put(g_list.rptr, rptr); put(g_list.pcell, pcell); put(g_list.pmeta, pmeta); put(g_list.pslot, pslot);
  put(g_list.sptr, sptr); put(g_list.dcell, dcell); put(g_list.dmeta, dmeta); put(g_list.dslot, dslot);
}
int th_check(int n, int nmax, const int32_t *markers, const double *values, double beta_nitsche, const double *beta_backflow, char *msg, int len) {
  std::string why;
  if (T::check_boundaries(n, nmax, markers, values, beta_nitsche, beta_backflow, why)) return 0;
  snprintf(msg, len, "%s", why.c_str());
  return -1;
}
int th_slice() { return T::SLICE; }

}  // extern "C"
