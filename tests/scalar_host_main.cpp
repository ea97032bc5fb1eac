// Stand-alone run of csrc/cfdh_scalar_host.hpp for test_scalar_twin.py: built with -fsanitize=address,undefined and started as a
// child process.  Input file: int32 header {D, nv, nc, nnz}, then cells [nc][D + 1], vptr [nv + 1], vcol [nnz].  Builds the list,
// walks every entry of both layouts against the cells and the graph, repeats with a graph that lacks every column and with a
// vertex out of range, runs the argument checks, and prints "ok <rows> <incidences> <slices> <widest slice>".
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "cfdh_scalar_host.hpp"

namespace T = cfdh_scalar;

static std::vector<int> take(FILE *f, size_t n) {
  std::vector<int> v(n);
  if (n && fread(v.data(), sizeof(int), n, f) != n) { fprintf(stderr, "short file\n"); exit(2); }
  return v;
}
#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "failed: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  const std::vector<int> h = take(f, 4);
  const int D = h[0], nv = h[1], nc = h[2], n1 = D + 1;
  std::vector<int> cells = take(f, (size_t)n1 * nc);
  const std::vector<int> vptr = take(f, (size_t)nv + 1), vcol = take(f, h[3]);
  fclose(f);
  T::WorkList w;
  std::string why;
  REQUIRE(T::build_worklist(D, nv, nc, cells.data(), vptr.data(), vcol.data(), w, why));
  REQUIRE(w.nrows == nv && (int)w.rptr.size() == nv + 1 && w.rptr.back() == w.ninc && w.ninc == n1 * nc);
  REQUIRE(w.nslices == (nv + T::SLICE - 1) / T::SLICE && (int)w.sptr.size() == w.nslices + 1);
  REQUIRE(w.dinc.size() == (size_t)w.sptr[w.nslices] * T::SLICE && w.dslot.size() == w.dinc.size());
  int widest = 0;
  std::vector<int> seen((size_t)n1 * nc, 0);
  for (int r = 0; r < nv; r++) {
    const int s = r / T::SLICE, l = r % T::SLICE;
    widest = std::max(widest, w.sptr[s + 1] - w.sptr[s]);
    REQUIRE(w.rptr[r + 1] - w.rptr[r] <= w.sptr[s + 1] - w.sptr[s]);
    for (int c = w.sptr[s]; c < w.sptr[s + 1]; c++) {
      const size_t k = (size_t)c * T::SLICE + l;
      const int j = w.rptr[r] + (c - w.sptr[s]);
      if (j >= w.rptr[r + 1]) { REQUIRE(w.dinc[k] == -1); continue; }
      const int e = w.dinc[k] >> 2, a = w.dinc[k] & 3;
      REQUIRE(w.dinc[k] == w.inc[j] && w.dslot[k] == w.slot[j] && e >= 0 && e < nc && a <= D);
      REQUIRE(j == w.rptr[r] || w.inc[j] > w.inc[j - 1]);  // ascending cells inside a row
      REQUIRE(cells[(size_t)n1 * e + a] == r);
      seen[(size_t)n1 * e + a]++;
      for (int b = 0; b < n1; b++) {
        const int pos = (int)((w.dslot[k] >> (8 * b)) & 0xffu);
        REQUIRE(pos < vptr[r + 1] - vptr[r] && vcol[vptr[r] + pos] == cells[(size_t)n1 * e + b]);
      }
    }
  }
  for (int v : seen) REQUIRE(v == 1);  // every (cell, local vertex) exactly once
  REQUIRE(w.nslices > 0);
  for (size_t k = (size_t)w.sptr[w.nslices - 1] * T::SLICE; k < w.dinc.size(); k++)  // the lanes behind the last row hold no incidence
    if ((int)(k % T::SLICE) + (w.nslices - 1) * T::SLICE >= nv) REQUIRE(w.dinc[k] == -1);
  {  // a graph whose rows are empty lacks every column: refused with a message, nothing read out of range
    const std::vector<int> none((size_t)nv + 1, 0);
    T::WorkList bad;
    REQUIRE(!T::build_worklist(D, nv, nc, cells.data(), none.data(), vcol.data(), bad, why) && !why.empty());
  }
  {
    T::WorkList bad;
    const int keep = cells[0];
    cells[0] = nv;
    REQUIRE(!T::build_worklist(D, nv, nc, cells.data(), vptr.data(), vcol.data(), bad, why) && why.find("out of range") != std::string::npos);
    cells[0] = -1;
    REQUIRE(!T::build_worklist(D, nv, nc, cells.data(), vptr.data(), vcol.data(), bad, why));
    cells[0] = keep;
    REQUIRE(!T::build_worklist(4, nv, nc, cells.data(), vptr.data(), vcol.data(), bad, why));
  }
  const double inf = INFINITY, nan = NAN;
  REQUIRE(T::check_params(0.0, -3.0, 1.0, why) && T::check_params(1e-3, 1.0, 0.5, why));
  REQUIRE(!T::check_params(-1e-9, 0.0, 0.5, why) && !T::check_params(inf, 0.0, 0.5, why) && !T::check_params(nan, 0.0, 0.5, why));
  REQUIRE(!T::check_params(0.0, inf, 0.5, why) && !T::check_params(0.0, nan, 0.5, why));
  REQUIRE(!T::check_params(0.0, 0.0, 0.0, why) && !T::check_params(0.0, 0.0, 1.0 + 1e-12, why) && !T::check_params(0.0, 0.0, nan, why));
  const int32_t nodes[3] = {0, nv - 1, 0};
  const double vals[3] = {1.0, 2.0, 3.0}, badv[3] = {1.0, nan, 3.0};
  const int32_t far[1] = {nv}, neg[1] = {-1};
  REQUIRE(T::check_dirichlet(3, nv, nodes, vals, why) && T::check_dirichlet(0, nv, nullptr, nullptr, why));
  REQUIRE(!T::check_dirichlet(3, nv, nodes, badv, why) && !T::check_dirichlet(1, nv, far, vals, why) && !T::check_dirichlet(1, nv, neg, vals, why));
  REQUIRE(!T::check_dirichlet(-1, nv, nodes, vals, why) && !T::check_dirichlet(2, nv, nullptr, vals, why) && !T::check_dirichlet(2, nv, nodes, nullptr, why));
  printf("ok %d %d %d %d\n", w.nrows, w.ninc, w.nslices, widest);
  return 0;
}
