// extern "C" face of csrc/cfdh_mesh_host.hpp for test_mesh_host.py (g++, ctypes): one wrapper per step, raw arrays in and out.
// Output arrays are allocated by the caller; a refusal returns -1 with the reason in msg.
#include <cstring>

#include "cfdh_mesh_host.hpp"

namespace M = cfdh_mesh;

static int refuse(const std::string &why, char *msg, int len) {
  snprintf(msg, len, "%s", why.c_str());
  return -1;
}
template <class T>
static void put(const std::vector<T> &v, T *out) {
  if (!v.empty()) memcpy(out, v.data(), v.size() * sizeof(T));
}

extern "C" {

int mh_check_sizes(int64_t nv, int64_t nvo, int64_t nc, int NL, const int32_t *cells, int64_t nv_max, int64_t nc_max, char *msg, int len) {
  std::string why;
  return M::check_sizes(nv, nvo, nc, NL, cells, nv_max, nc_max, M::Wording(), why) ? 0 : refuse(why, msg, len);
}
int mh_check_facets(int64_t nfac, const int32_t *fcell, const int32_t *flocal, int64_t nc, int NF, char *msg, int len) {
  std::string why;
  return M::check_facets(nfac, fcell, flocal, nc, NF, M::Wording(), why) ? 0 : refuse(why, msg, len);
}
int mh_morton(int D, int bits, int renumber, int nv, int nvo, const double *coords, int *perm, int *iperm, double *xout, char *msg, int len) {
  std::string why;
  return M::morton_numbering(D, bits, renumber != 0, nv, nvo, coords, perm, iperm, xout, why) ? 0 : refuse(why, msg, len);
}
// h_cells [NL ncu], cell_user [ncu], cmap [ncu]; returns the number of cells kept
int mh_select_cells(int NL, int ncu, int nvo, const int32_t *cells, const int *perm, int *h_cells, int *cell_user, int *cmap) {
  std::vector<int> hc, cu, cm;
  M::select_cells(NL, ncu, nvo, cells, perm, hc, cu, cm);
  put(hc, h_cells); put(cu, cell_user); put(cm, cmap);
  return (int)cu.size();
}
// iptr, vptr [nvo + 1], vdiag [nvo], inc [NL nc], vcol [NL NL nc]; returns the number of graph entries
int mh_node_graph(int NL, int nc, int nvo, const int *h_cells, const int *iperm, int *iptr, int *inc, int *vptr, int *vcol, int *vdiag, char *msg,
                  int len) {
  std::vector<int> ip, in, vp, vc, vd;
  std::string why;
  if (!M::node_graph(NL, nc, nvo, h_cells, iperm, ip, in, vp, vc, vd, M::Wording(), why)) return refuse(why, msg, len);
  put(ip, iptr); put(in, inc); put(vp, vptr); put(vc, vcol); put(vd, vdiag);
  return (int)vc.size();
}
void mh_graph_slots(int NL, int nc, int nvo, const int *h_cells, const int *vptr, const int *vcol, int *slot) {
  std::vector<int> s;
  M::graph_slots(NL, nc, nvo, h_cells, vptr, vcol, s);
  put(s, slot);
}
// slot [nc NL NL] in (graph slots) and out (staging positions); eptr [nnz + 1], fptr [nvo + 1], fdst [nc NL fper]
void mh_staging_order(int NL, int nc, int nvo, int nnz, const int *h_cells, int fper, int *slot, int *eptr, int *fptr, int *fdst) {
  std::vector<int> s(slot, slot + (size_t)nc * NL * NL), ep, fp, fd;
  M::staging_order(NL, nc, nvo, nnz, h_cells, fper, s, ep, fp, fd);
  put(s, slot); put(ep, eptr); put(fp, fptr); put(fd, fdst);
}
// per-cell matrices K [nc][NL][NL], Md [nc][NL], measures [nc] -> Lval [nnz], Ml [nv]
void mh_scatter(int NL, int nc, int nv, const int *h_cells, const int *slot, int nnz, const double *K, const double *Md, const double *meas, double *Lval,
                double *Ml) {
  const std::vector<int> s(slot, slot + (size_t)nc * NL * NL);
  std::vector<double> L, m;
  M::scatter_stiffness_mass(NL, nc, nv, h_cells, s, nnz, [&](int e, double *Ke, double *Mde) {
    memcpy(Ke, K + (size_t)e * NL * NL, sizeof(double) * NL * NL);
    memcpy(Mde, Md + (size_t)e * NL, sizeof(double) * NL);
    return meas[e];
  }, L, m);
  put(L, Lval); put(m, Ml);
}
// rowptr [nv + 1], col / val [2 nv]; returns the number of vertex nodes
int mh_p1_subspace(int NL, int NV, const int *edges, int nc, int nv, const int *h_cells, int *rowptr, int *col, double *val) {
  std::vector<int> rp, cl;
  std::vector<double> vl;
  const int nvert = M::p1_subspace(NL, NV, reinterpret_cast<const int(*)[2]>(edges), nc, nv, h_cells, rp, cl, vl);
  put(rp, rowptr); put(cl, col); put(vl, val);
  return nvert;
}
double mh_tri_det(const double *X, const int *v) { return M::tri_det(X, v); }
int mh_is_parallelogram(const double *X, const int *v, double adet) { return M::is_parallelogram(X, v, adet) ? 1 : 0; }
int mh_is_parallelepiped(const double *X, const int *v, double adet) { return M::is_parallelepiped(X, v, adet) ? 1 : 0; }
int mh_p2_bent_edge(int D, const int *edges, const double *X, const int *v, double adet) {
  return M::p2_bent_edge(D, reinterpret_cast<const int(*)[2]>(edges), X, v, adet);
}
void mh_lcg(int64_t n, double *out) { put(M::lcg_vector((size_t)n), out); }

}  // extern "C"
