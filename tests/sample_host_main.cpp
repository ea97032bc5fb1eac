// Stand-alone run of csrc/cfdh_sample_host.hpp for tests/test_sample_twin.py, built with -fsanitize=address,undefined: reads a mesh
// (header of int32: D nv nc; then coords as float64 and cells as int32), builds the bins in the given order and in a reversed
// visiting order at two tolerances, checks them against their definition, looks points up (the vertices, the corners of the box,
// points outside) and runs the refusals; prints "ok ..." and returns 0, or says what failed.
#include <cstdio>
#include <cstdlib>

#include "cfdh_sample_host.hpp"

static int die(const char *what, const std::string &why = "") {
  std::printf("FAILED %s %s\n", what, why.c_str());
  return 1;
}

// shape and size of the lists, and every vertex of a cell in a bin that lists the cell
static const char *check(int D, int nv, int nc, const std::vector<double> &x, const std::vector<int> &cells, const std::vector<int> &rank,
                         const cfdh_sample::Bins &B) {
  const int n1 = D + 1;
  if ((long long)B.ptr.size() != B.nbins + 1 || B.ptr[0] != 0 || B.ptr[B.nbins] != B.total || (long long)B.list.size() != B.total) return "sizes";
  if (B.nbins != (long long)B.g.nb[0] * B.g.nb[1] * B.g.nb[2]) return "bins per axis";
  if (B.total > (long long)cfdh_sample::LIST_FACTOR * nc) return "more than 16 nc entries";
  int maxlen = 0;
  std::vector<int> hits((size_t)nc, 0);
  for (long long b = 0; b < B.nbins; b++) {
    if (B.ptr[b + 1] < B.ptr[b]) return "ptr not monotone";
    maxlen = std::max(maxlen, B.ptr[b + 1] - B.ptr[b]);
    for (int k = B.ptr[b]; k < B.ptr[b + 1]; k++) {
      const int e = B.list[k];
      if (e < 0 || e >= nc) return "cell out of range";
      if (k > B.ptr[b] && rank[B.list[k - 1]] >= rank[e]) return "not ascending, or a cell twice";
      hits[e]++;
    }
  }
  if (maxlen != B.maxlen) return "maxlen";
  for (int e = 0; e < nc; e++) {
    if (hits[e] < 1) return "a cell is in no bin";
    for (int a = 0; a < n1; a++) {
      const long long b = cfdh_sample::point_bin(B.g, &x[(size_t)D * cells[(size_t)n1 * e + a]]);
      if (b < 0 || b >= B.nbins) return "a vertex is outside the box";
      bool listed = false;
      for (int k = B.ptr[b]; k < B.ptr[b + 1]; k++) listed = listed || B.list[k] == e;
      if (!listed) return "the bin of a vertex does not list its cell";
    }
  }
  double far[3] = {0, 0, 0}, corner[3];
  for (int i = 0; i < D; i++) { far[i] = B.g.hi[i] + 1.0; corner[i] = B.g.hi[i]; }
  if (cfdh_sample::point_bin(B.g, far) != -1) return "a point beyond the box has a bin";
  if (nc > 0 && cfdh_sample::point_bin(B.g, corner) != B.nbins - 1) return "the upper corner is not in the last bin";
  for (int i = 0; i < D; i++) corner[i] = B.g.lo[i];
  if (nc > 0 && cfdh_sample::point_bin(B.g, corner) != 0) return "the lower corner is not in the first bin";
  corner[0] = std::nan("");
  if (cfdh_sample::point_bin(B.g, corner) != -1) return "a NaN has a bin";
  (void)nv;
  return nullptr;
}

int main(int argc, char **argv) {
  if (argc < 2) return die("usage");
  std::FILE *f = std::fopen(argv[1], "rb");
  if (!f) return die("open");
  int hd[3];
  if (std::fread(hd, sizeof(int), 3, f) != 3) return die("header");
  const int D = hd[0], nv = hd[1], nc = hd[2], n1 = D + 1;
  std::vector<double> x((size_t)nv * D);
  std::vector<int> cells((size_t)nc * n1);
  if (!x.empty() && std::fread(x.data(), sizeof(double), x.size(), f) != x.size()) return die("read coords");
  if (!cells.empty() && std::fread(cells.data(), sizeof(int), cells.size(), f) != cells.size()) return die("read cells");
  std::fclose(f);

  std::string why;
  cfdh_sample::Bins B;
  std::vector<int> rank((size_t)nc), visit((size_t)nc);
  long long total = 0, nbins = 0;
  int maxlen = 0;
  for (double tol : {1e-9, 0.0, 1e-3}) {
    for (int e = 0; e < nc; e++) rank[e] = e;
    if (!cfdh_sample::build_bins(D, nv, nc, x.data(), cells.data(), nullptr, tol, B, why)) return die("bins", why);
    if (const char *bad = check(D, nv, nc, x, cells, rank, B)) return die("identity order:", bad);
    if (tol == 1e-9) { total = B.total; nbins = B.nbins; maxlen = B.maxlen; }
    for (int k = 0; k < nc; k++) { visit[k] = nc - 1 - k; rank[nc - 1 - k] = k; }
    if (!cfdh_sample::build_bins(D, nv, nc, x.data(), cells.data(), visit.data(), tol, B, why)) return die("bins, reversed", why);
    if (const char *bad = check(D, nv, nc, x, cells, rank, B)) return die("reversed order:", bad);
  }

  // refusals: a vertex out of range, a visiting order that is no permutation, a bad dimension, a bad tol, a NaN coordinate
  if (nc > 0) {
    std::vector<int> broken(cells);
    broken[broken.size() / 2] = nv;
    if (cfdh_sample::build_bins(D, nv, nc, x.data(), broken.data(), nullptr, 0.0, B, why)) return die("vertex out of range accepted");
    broken = cells;
    broken[0] = -1;
    if (cfdh_sample::build_bins(D, nv, nc, x.data(), broken.data(), nullptr, 0.0, B, why)) return die("negative vertex accepted");
    std::vector<double> xn(x);
    xn[(size_t)D * cells[0]] = std::nan("");
    if (cfdh_sample::build_bins(D, nv, nc, xn.data(), cells.data(), nullptr, 0.0, B, why)) return die("NaN coordinate accepted");
  }
  if (nc > 1) {
    visit[0] = visit[1];
    if (cfdh_sample::build_bins(D, nv, nc, x.data(), cells.data(), visit.data(), 0.0, B, why)) return die("doubled cell in the visiting order accepted");
    visit[0] = nc;
    if (cfdh_sample::build_bins(D, nv, nc, x.data(), cells.data(), visit.data(), 0.0, B, why)) return die("cell out of range in the visiting order accepted");
  }
  if (cfdh_sample::build_bins(4, nv, nc, x.data(), cells.data(), nullptr, 0.0, B, why)) return die("D = 4 accepted");
  if (cfdh_sample::build_bins(D, nv, (1 << 27) + 1, x.data(), cells.data(), nullptr, 0.0, B, why)) return die("more cells than the 32-bit offsets of the lists allow accepted");
  if (cfdh_sample::build_bins(D, nv, nc, x.data(), cells.data(), nullptr, 2e-3, B, why)) return die("tol above 1e-3 accepted");
  if (cfdh_sample::build_bins(D, nv, nc, x.data(), cells.data(), nullptr, -1e-9, B, why)) return die("negative tol accepted");
  if (cfdh_sample::build_bins(D, nv, nc, x.data(), cells.data(), nullptr, std::nan(""), B, why)) return die("NaN tol accepted");
  if (!cfdh_sample::build_bins(D, 0, 0, nullptr, nullptr, nullptr, 0.0, B, why) || B.total != 0 || B.nbins != 1 || !B.list.empty()) return die("empty mesh", why);
  std::printf("ok %lld entries in %lld bins, longest list %d\n", total, nbins, maxlen);
  return 0;
}
