// extern "C" wrappers around csrc/cfdh_section_host.hpp for tests/test_section_twin.py (g++, loaded with ctypes).
#include <cstring>

#include "cfdh_section_host.hpp"

namespace {
cfdh_section::Cut g_cut;
}

extern "C" {

// builds the cut and keeps it; sizes[0..1] = entries in all, the longest list; max_entries <= 0: the limit of the header;
// -1 with the reason in msg
int sc_build(int D, int nv, int nc, const double *coords, const int *cells, const int *caller_index, const unsigned char *flipped, int K,
             const double *planes, long long max_entries, long long *sizes, char *msg, int nmsg) {
  std::string why;
  if (!cfdh_section::build_cut(D, nv, nc, cells, coords, caller_index, flipped, K, planes, g_cut, why,
                               max_entries > 0 ? max_entries : cfdh_section::MAX_ENTRIES)) {
    if (msg && nmsg > 0) { std::strncpy(msg, why.c_str(), (size_t)nmsg - 1); msg[nmsg - 1] = 0; }
    return -1;
  }
  sizes[0] = g_cut.total;
  sizes[1] = g_cut.maxlen;
  return 0;
}

// copies of the cut built last: ptr [K + 1], cell / code [total], t [total][np], meas [total][nt], straddling [K], normal [K][3]
void sc_get(long long *ptr, int *cell, int *code, double *t, double *meas, int *straddling, double *normal) {
  std::memcpy(ptr, g_cut.ptr.data(), sizeof(long long) * g_cut.ptr.size());
  if (g_cut.total) {
    std::memcpy(cell, g_cut.cell.data(), sizeof(int) * g_cut.cell.size());
    std::memcpy(code, g_cut.code.data(), sizeof(int) * g_cut.code.size());
    std::memcpy(t, g_cut.t.data(), sizeof(double) * g_cut.t.size());
    std::memcpy(meas, g_cut.meas.data(), sizeof(double) * g_cut.meas.size());
  }
  if (g_cut.K) {
    std::memcpy(straddling, g_cut.straddling.data(), sizeof(int) * g_cut.straddling.size());
    std::memcpy(normal, g_cut.normal.data(), sizeof(double) * g_cut.normal.size());
  }
}

// out [K][10] of the cut built last: the kernel's arithmetic per entry, on the host
void sc_eval(const int *cells, const double *u, const double *p, double rho, double *out) { cfdh_section::eval_rows(g_cut, cells, u, p, rho, out); }
}
