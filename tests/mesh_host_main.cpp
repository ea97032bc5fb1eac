// Stand-alone walk through every step of csrc/cfdh_mesh_host.hpp on one mesh, built by test_mesh_host.py with
// -fsanitize=address,undefined and run as a child process: index arithmetic that reads or writes out of bounds ends it.
// Input file: int32 header {D, NL, NV, NF, bits, nv, nvo, nc, nfac, nedges}, then cells [nc][NL], fcell [nfac], flocal [nfac],
// edges [nedges][2] (int32), coords [nv][D] (double).  NL == D + 1: the closed-form steps run too; nedges > 0: a P2 space.
#include <cstdio>
#include <cstdlib>

#include "cfdh_mesh_host.hpp"

namespace M = cfdh_mesh;

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
  const std::vector<int32_t> h = rd<int32_t>(f, 10);
  const int D = h[0], NL = h[1], NV = h[2], NF = h[3], bits = h[4], nv = h[5], nvo = h[6], ncu = h[7], nfac = h[8], ned = h[9];
  const std::vector<int32_t> cells = rd<int32_t>(f, (size_t)NL * ncu), fcell = rd<int32_t>(f, nfac), flocal = rd<int32_t>(f, nfac), edges = rd<int32_t>(f, 2 * (size_t)ned);
  const std::vector<double> coords = rd<double>(f, (size_t)D * nv);
  fclose(f);
  const M::Wording W;
  std::string why;
  need(M::check_sizes(nv, nvo, ncu, NL, cells.data(), 1ll << 28, 1ll << 24, W, why), "check_sizes", why);
  need(M::check_facets(nfac, fcell.data(), flocal.data(), ncu, NF, W, why), "check_facets", why);
  long long sum = 0;
  for (int renumber = 0; renumber < 2; renumber++) {
    std::vector<int> perm(nv), iperm(nv);
    std::vector<double> X((size_t)D * nv);
    need(M::morton_numbering(D, bits, renumber != 0, nv, nvo, coords.data(), perm.data(), iperm.data(), X.data(), why), "morton_numbering", why);
    // cells of the context: the closed forms select and sort them, the generic builders keep them all
    std::vector<int> h_cells((size_t)NL * ncu), cell_user, cmap;
    for (size_t t = 0; t < h_cells.size(); t++) h_cells[t] = perm[cells[t]];
    if (NL == D + 1) M::select_cells(NL, ncu, nvo, cells.data(), perm.data(), h_cells, cell_user, cmap);
    const int nc = (int)(h_cells.size() / NL);
    std::vector<int> iptr, inc, vptr, vcol, vdiag, slot, eptr, fptr, fdst;
    need(M::node_graph(NL, nc, nvo, h_cells.data(), iperm.data(), iptr, inc, vptr, vcol, vdiag, W, why), "node_graph", why);
    const int nnz = (int)vcol.size();
    for (int v = 0; v < nvo; v++) sum += vcol[vdiag[v]] - v + M::graph_slot(vptr.data(), vcol.data(), v, v) - vdiag[v];
    M::graph_slots(NL, nc, nvo, h_cells.data(), vptr.data(), vcol.data(), slot);
    std::vector<double> Lval, Ml;
    M::scatter_stiffness_mass(NL, nc, nv, h_cells.data(), slot, nnz, [&](int e, double *K, double *Md) {
      for (int a = 0; a < NL; a++) { Md[a] = 1.0 + a; for (int b = 0; b < NL; b++) K[a * NL + b] = a == b ? NL - 1.0 : -1.0; }
      return 1.0 + e % 3;
    }, Lval, Ml);
    for (int fper : {1, NL}) {
      std::vector<int> st = slot;
      M::staging_order(NL, nc, nvo, nnz, h_cells.data(), fper, st, eptr, fptr, fdst);
      sum += eptr[nnz] + fptr[nvo] + (long long)fdst.size();
    }
    if (ned) {
      std::vector<int> rp, cl;
      std::vector<double> vl;
      sum += M::p1_subspace(NL, NV, reinterpret_cast<const int(*)[2]>(edges.data()), nc, nv, h_cells.data(), rp, cl, vl) + rp[nv];
    }
    for (int e = 0; e < nc; e++) {
      const int *v = &h_cells[(size_t)NL * e];
      if (ned) sum += M::p2_bent_edge(D, reinterpret_cast<const int(*)[2]>(edges.data()), X.data(), v, 1.0);
      if (D == 2) sum += M::tri_det(X.data(), v) != 0.0;
      if (NL == 4 && D == 2) sum += M::is_parallelogram(X.data(), v, 1.0);
      if (NL == 8) sum += M::is_parallelepiped(X.data(), v, 1.0);
    }
    sum += (long long)Lval.size() + (long long)Ml.size();
  }
  sum += (long long)(M::lcg_vector((size_t)D * nv)[0] * 1e6);
  printf("ok %lld\n", sum);
  return 0;
}
