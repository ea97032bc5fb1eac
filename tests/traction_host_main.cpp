// Stand-alone run of csrc/cfdh_traction_host.hpp for test_traction_host.py: built with -fsanitize=address,undefined and started as a
// child process.  Input file: int32 header {D, nv, nc, nfac, nb, tangential, nnz}, then cells [nc][D + 1], fcell, flocal, fmarker
// [nfac], markers [nb], vptr [nv + 1], vcol [nnz].  Builds the list, walks every entry of both layouts against the graph, repeats
// with no boundary and with a graph that lacks a column, and prints "ok <rows> <pairs> <slices>".
#include <cstdio>
#include <cstdlib>

#include "cfdh_traction_host.hpp"

namespace T = cfdh_traction;

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
  const std::vector<int> h = take(f, 7);
  const int D = h[0], nv = h[1], nc = h[2], nfac = h[3], nb = h[4], n1 = D + 1;
  const unsigned tang = (unsigned)h[5];
  const std::vector<int> cells = take(f, (size_t)n1 * nc), fcell = take(f, nfac), flocal = take(f, nfac), fmarker = take(f, nfac), markers = take(f, nb),
                         vptr = take(f, (size_t)nv + 1), vcol = take(f, h[6]);
  fclose(f);
  T::WorkList w;
  std::string why;
  REQUIRE(T::build_worklist(D, nv, nc, cells.data(), nfac, fcell.data(), flocal.data(), fmarker.data(), nb, markers.data(), tang, vptr.data(),
                            vcol.data(), w, why));
  REQUIRE((int)w.row.size() == w.nrows && (int)w.rptr.size() == w.nrows + 1 && w.rptr.back() == w.npairs);
  for (int r = 0; r < w.nrows; r++) {
    const int s = r / T::SLICE, l = r % T::SLICE;
    REQUIRE(r == 0 || w.row[r] > w.row[r - 1]);
    REQUIRE(w.rptr[r + 1] - w.rptr[r] >= 1 && w.rptr[r + 1] - w.rptr[r] <= w.sptr[s + 1] - w.sptr[s]);
    for (int c = w.sptr[s]; c < w.sptr[s + 1]; c++) {
      const size_t k = (size_t)c * T::SLICE + l;
      const int j = w.rptr[r] + (c - w.sptr[s]);
      if (j >= w.rptr[r + 1]) { REQUIRE(w.dcell[k] == -1); continue; }
      const int e = w.dcell[k], a = w.dmeta[k] & 3, fl = (w.dmeta[k] >> 2) & 3, b = w.dmeta[k] >> 4;
      REQUIRE(e == w.pcell[j] && w.dmeta[k] == w.pmeta[j] && e >= 0 && e < nc && a <= D && fl <= D && b < nb);
      REQUIRE(cells[(size_t)n1 * e + a] == w.row[r]);
      for (int q = 0; q < n1; q++) {
        const int slot = w.dslot[((size_t)c * n1 + q) * T::SLICE + l];
        REQUIRE(slot == w.pslot[(size_t)n1 * j + q] && slot >= vptr[w.row[r]] && slot < vptr[w.row[r] + 1] && vcol[slot] == cells[(size_t)n1 * e + q]);
      }
    }
  }
  T::WorkList e0;
  REQUIRE(T::build_worklist(D, nv, nc, cells.data(), nfac, fcell.data(), flocal.data(), fmarker.data(), 0, nullptr, 0u, vptr.data(), vcol.data(), e0, why));
  REQUIRE(e0.nrows == 0 && e0.npairs == 0 && e0.nslices == 0 && e0.dcell.empty() && e0.sptr.size() == 1);
  if (w.npairs) {  // a graph whose rows are empty lacks every column: refused with a message, nothing read out of range
    const std::vector<int> none((size_t)nv + 1, 0);
    T::WorkList bad;
    REQUIRE(!T::build_worklist(D, nv, nc, cells.data(), nfac, fcell.data(), flocal.data(), fmarker.data(), nb, markers.data(), tang, none.data(),
                               vcol.data(), bad, why) && !why.empty());
  }
  const int32_t mk[2] = {3, 3};
  const double vals[2] = {1.0, 2.0}, bf[2] = {0.0, -1.0};
  REQUIRE(!T::check_boundaries(2, 8, mk, vals, 1.0, nullptr, why) && !T::check_boundaries(9, 8, mk, vals, 1.0, nullptr, why));
  REQUIRE(!T::check_boundaries(1, 8, mk, vals, 1.0, bf + 1, why) && T::check_boundaries(1, 8, mk, vals, 1.0, bf, why) && T::check_boundaries(0, 8, nullptr, nullptr, 0.0, nullptr, why));
  printf("ok %d %d %d\n", w.nrows, w.npairs, w.nslices);
  return 0;
}
