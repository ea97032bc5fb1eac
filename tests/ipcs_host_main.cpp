// Stand-alone walk through every step of csrc/cfdh_ipcs_host.hpp on one mesh, built by test_ipcs_host.py with
// -fsanitize=address,undefined and run as a child process: index arithmetic that reads or writes out of bounds ends it.
// Input file: int32 header {D, nn, nvert, nc, nfac}, then cells [nc][NL], fcell [nfac], flocal [nfac], the pressure Dirichlet
// flags [nvert] (int32), coords [nn][D], the object counts [nvert] and values [nvert] (double).
#include <cstdio>
#include <cstdlib>

#include "cfdh_ipcs_host.hpp"

namespace H = cfdh_ipcs_host;

template <class T>
static std::vector<T> rd(FILE *f, size_t n) {
  std::vector<T> v(n);
  if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input file\n"); exit(2); }
  return v;
}
static void need(bool ok, const char *what, const std::string &why) {
  if (!ok) { fprintf(stderr, "%s refused: %s\n", what, why.c_str()); exit(3); }
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  const std::vector<int32_t> h = rd<int32_t>(f, 5);
  const int D = h[0], nn = h[1], nvert = h[2], nc = h[3], nfac = h[4], NL = D == 2 ? 6 : 10;
  const std::vector<int32_t> cells = rd<int32_t>(f, (size_t)NL * nc), fcell = rd<int32_t>(f, nfac), flocal = rd<int32_t>(f, nfac), fl = rd<int32_t>(f, nvert);
  const std::vector<double> coords = rd<double>(f, (size_t)D * nn), cnt = rd<double>(f, nvert), val = rd<double>(f, nvert);
  fclose(f);
  std::string why;
  need(H::ip_check_mesh(D, nn, nvert, nc, cells.data(), why), "ip_check_mesh", why);
  std::vector<double> geo;
  need(H::ip_geometry(D, nc, cells.data(), coords.data(), geo, why), "ip_geometry", why);
  H::IpRef R;
  H::ip_reference(D, R);
  H::IpOps O;
  H::ip_constant_operators(R, nn, nvert, nc, cells.data(), geo.data(), O);
  H::IpMid Q;
  H::ip_midpoint_constants(R, O, nn, nc, cells.data(), geo.data(), (size_t)nfac, fcell.data(), flocal.data(), Q);
  long long sum = (long long)O.elist.size() + O.eptr.back() + Q.nptr.back() + (long long)Q.nlist.size();
  double acc = 0.0;
  for (const auto *v : {&O.M, &O.K, &O.L, &O.Mp, &O.G, &O.BT, &O.B, &O.m1, &Q.ES, &Q.Pn, &Q.BTP})
    for (double x : *v) acc += x;
  // the Dirichlet treatment: without an object, with the file's objects, with every vertex constrained
  const std::vector<unsigned char> flag(fl.begin(), fl.end());
  for (int pass = 0; pass < 3; pass++) {
    const std::vector<unsigned char> fp = pass == 1 ? flag : std::vector<unsigned char>(nvert, pass == 0 ? 0 : 1);
    const std::vector<double> cp = pass == 1 ? cnt : std::vector<double>(nvert, pass == 0 ? 0.0 : 1.0);
    std::vector<double> Lc, aval, lift, fix;
    std::vector<int> aptr, acol;
    bool singular;
    H::ip_constrain_laplacian(O, fp, cp, Lc, aptr, acol, aval, singular);
    H::ip_lifting(O, fp, cp, val, lift, fix);
    sum += aptr.back() + (singular ? 1 : 0) + (long long)Lc.size();
    for (int i = 0; i < nvert; i++) acc += lift[i] + fix[i];
  }
  std::vector<double> rm, dinv;
  H::ip_rho_mass(O, 1.06, rm, dinv);
  for (double x : dinv) acc += x;
  printf("ok %lld %.17g\n", sum + (long long)rm.size(), acc);
  return 0;
}
