// extern "C" wrappers around csrc/cfdh_flow_host.hpp for tests/test_flow_twin.py (g++, loaded with ctypes).
#include <cstring>

#include "cfdh_flow_host.hpp"

namespace {
cfdh_flow::CellIndex g_index;
}

extern "C" {

// builds the index and keeps it; sizes[0..4] = ninc, nslices, maxlen, columns of all slices; -1 with the reason in msg
int fh_build(int D, int nv, int nc, const int *cells, const int *visit, int *sizes, char *msg, int nmsg) {
  std::string why;
  if (!cfdh_flow::build_index(D, nv, nc, cells, visit, g_index, why)) {
    if (msg && nmsg > 0) { std::strncpy(msg, why.c_str(), (size_t)nmsg - 1); msg[nmsg - 1] = 0; }
    return -1;
  }
  sizes[0] = g_index.ninc; sizes[1] = g_index.nslices; sizes[2] = g_index.maxlen; sizes[3] = g_index.sptr.empty() ? 0 : g_index.sptr.back();
  return 0;
}

// copies of the index built last: rptr [nv + 1], inc [ninc], sptr [nslices + 1], dinc [columns * 64]
void fh_get(int *rptr, int *inc, int *sptr, int *dinc) {
  std::memcpy(rptr, g_index.rptr.data(), sizeof(int) * g_index.rptr.size());
  if (!g_index.inc.empty()) std::memcpy(inc, g_index.inc.data(), sizeof(int) * g_index.inc.size());
  std::memcpy(sptr, g_index.sptr.data(), sizeof(int) * g_index.sptr.size());
  if (!g_index.dinc.empty()) std::memcpy(dinc, g_index.dinc.data(), sizeof(int) * g_index.dinc.size());
}

int fh_field_width(int D, int which) { return cfdh_flow::field_width(D, which); }
int fh_slice() { return cfdh_flow::SLICE; }
}
