// extern "C" face of csrc/cfdh_ipcs_host.hpp for test_ipcs_host.py (g++, ctypes).  ih_create walks the steps of cfdh_ipcs_create
// and of the ipcs_midpoint build in their order and keeps every array; ih_size / ih_get hand them out by name.  Output arrays are
// allocated by the caller; a refusal returns -1 (the builder's CFDH_E_ARG) or a null handle with the reason in msg.
#include <cstring>

#include "cfdh_ipcs_host.hpp"

namespace H = cfdh_ipcs_host;

struct Built {
  H::IpRef R;
  H::IpOps O;
  H::IpMid Q;
  std::vector<double> geo;
};

static int refuse(const std::string &why, char *msg, int len) {
  snprintf(msg, len, "%s", why.c_str());
  return -1;
}
static const std::vector<int> *ints(const Built *b, const char *n) {
  const struct { const char *name; const std::vector<int> *v; } t[] = {
      {"ptr2", &b->O.ptr2}, {"col2", &b->O.col2}, {"ptr1", &b->O.ptr1}, {"col1", &b->O.col1}, {"gptr", &b->O.gptr}, {"gcol", &b->O.gcol},
      {"bptr", &b->O.bptr}, {"bcol", &b->O.bcol}, {"eptr", &b->O.eptr}, {"elist", &b->O.elist}, {"nptr", &b->Q.nptr}, {"nlist", &b->Q.nlist}};
  for (const auto &e : t)
    if (!strcmp(e.name, n)) return e.v;
  return nullptr;
}
static const std::vector<double> *doubles(const Built *b, const char *n) {
  const struct { const char *name; const std::vector<double> *v; } t[] = {
      {"rM", &b->R.M}, {"rK", &b->R.K}, {"rT2", &b->R.T2}, {"rB", &b->R.B}, {"rG", &b->R.G}, {"rMP", &b->R.MP}, {"geo", &b->geo},
      {"M", &b->O.M}, {"K", &b->O.K}, {"L", &b->O.L}, {"Mp", &b->O.Mp}, {"G", &b->O.G}, {"BT", &b->O.BT}, {"B", &b->O.B}, {"m1", &b->O.m1},
      {"ES", &b->Q.ES}, {"Pn", &b->Q.Pn}, {"BTP", &b->Q.BTP}};
  for (const auto &e : t)
    if (!strcmp(e.name, n)) return e.v;
  return nullptr;
}

extern "C" {

int ih_check_mesh(int D, int64_t nn, int64_t nvert, int64_t nc, const int32_t *cells, char *msg, int len) {
  std::string why;
  return H::ip_check_mesh(D, nn, nvert, nc, cells, why) ? 0 : refuse(why, msg, len);
}
void *ih_create(int D, int nn, int nvert, int nc, const int32_t *cells, const double *coords, int nfac, const int32_t *fcell, const int32_t *flocal,
                char *msg, int len) {
  std::string why;
  Built *b = new Built();
  if (!H::ip_check_mesh(D, nn, nvert, nc, cells, why) || !H::ip_geometry(D, nc, cells, coords, b->geo, why)) {
    refuse(why, msg, len);
    delete b;
    return nullptr;
  }
  H::ip_reference(D, b->R);
  H::ip_constant_operators(b->R, nn, nvert, nc, cells, b->geo.data(), b->O);
  H::ip_midpoint_constants(b->R, b->O, nn, nc, cells, b->geo.data(), (size_t)nfac, fcell, flocal, b->Q);
  return b;
}
void ih_free(void *h) { delete static_cast<Built *>(h); }
int64_t ih_size(const void *h, const char *name) {
  const Built *b = static_cast<const Built *>(h);
  if (const auto *v = ints(b, name)) return (int64_t)v->size();
  if (const auto *v = doubles(b, name)) return (int64_t)v->size();
  return -1;
}
void ih_get(const void *h, const char *name, void *out) {
  const Built *b = static_cast<const Built *>(h);
  if (const auto *v = ints(b, name)) { if (!v->empty()) memcpy(out, v->data(), v->size() * sizeof(int)); }
  else if (const auto *w = doubles(b, name)) { if (!w->empty()) memcpy(out, w->data(), w->size() * sizeof(double)); }
}
// Lc [nnz1], aptr [nvert + 1], acol / aval [nnz1], lift / fix [nvert]; returns the number of entries of the stripped matrix and
// sets *singular
int ih_dirichlet(const void *h, const unsigned char *flag, const double *cnt, const double *val, double *Lc, int *aptr, int *acol, double *aval,
                 int *singular, double *lift, double *fix) {
  const Built *b = static_cast<const Built *>(h);
  const size_t nv = b->O.ptr1.size() - 1;
  const std::vector<unsigned char> f(flag, flag + nv);
  const std::vector<double> c(cnt, cnt + nv), v(val, val + nv);
  std::vector<double> lc, av, li, fx;
  std::vector<int> ap, ac;
  bool sing;
  H::ip_constrain_laplacian(b->O, f, c, lc, ap, ac, av, sing);
  H::ip_lifting(b->O, f, c, v, li, fx);
  memcpy(Lc, lc.data(), lc.size() * sizeof(double));
  memcpy(aptr, ap.data(), ap.size() * sizeof(int));
  if (!ac.empty()) { memcpy(acol, ac.data(), ac.size() * sizeof(int)); memcpy(aval, av.data(), av.size() * sizeof(double)); }
  memcpy(lift, li.data(), nv * sizeof(double));
  memcpy(fix, fx.data(), nv * sizeof(double));
  *singular = sing ? 1 : 0;
  return (int)ac.size();
}
// rm [nnz2], dinv [nn]
void ih_rho_mass(const void *h, double rho, double *rm, double *dinv) {
  const Built *b = static_cast<const Built *>(h);
  std::vector<double> r, d;
  H::ip_rho_mass(b->O, rho, r, d);
  memcpy(rm, r.data(), r.size() * sizeof(double));
  memcpy(dinv, d.data(), d.size() * sizeof(double));
}

}  // extern "C"
