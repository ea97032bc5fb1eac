// Stand-alone run of csrc/cfdh_flow_host.hpp for tests/test_flow_twin.py, built with -fsanitize=address,undefined: reads a mesh
// (header of int32: D nv nc; then cells as int32), builds the inverted index in the given order and in a reversed visiting order,
// checks both against their definition and runs the refusals; prints "ok ..." and returns 0, or says what failed.
#include <cstdio>
#include <cstdlib>

#include "cfdh_flow_host.hpp"

static int die(const char *what, const std::string &why = "") {
  std::printf("FAILED %s %s\n", what, why.c_str());
  return 1;
}

// every incidence exactly once, in visiting order per vertex, and the slice layout equal to the by-row layout
static const char *check(int D, int nv, int nc, const std::vector<int> &cells, const std::vector<int> &rank, const cfdh_flow::CellIndex &w) {
  const int n1 = D + 1, S = cfdh_flow::SLICE;
  if ((int)w.rptr.size() != nv + 1 || w.rptr[0] != 0 || w.rptr[nv] != w.ninc || w.ninc != nc * n1) return "sizes";
  std::vector<int> hits((size_t)nc, 0);
  int maxlen = 0;
  for (int v = 0; v < nv; v++) {
    if (w.rptr[v + 1] < w.rptr[v]) return "rptr not monotone";
    maxlen = std::max(maxlen, w.rptr[v + 1] - w.rptr[v]);
    for (int j = w.rptr[v]; j < w.rptr[v + 1]; j++) {
      const int e = w.inc[j];
      if (e < 0 || e >= nc) return "cell out of range";
      bool holds = false;
      for (int a = 0; a < n1; a++) holds = holds || cells[(size_t)e * n1 + a] == v;
      if (!holds) return "the cell does not hold the vertex";
      if (j > w.rptr[v] && rank[w.inc[j - 1]] >= rank[e]) return "not ascending";
      hits[e]++;
    }
  }
  for (int e = 0; e < nc; e++)
    if (hits[e] != n1) return "an incidence is missing or doubled";
  if (maxlen != w.maxlen) return "maxlen";
  if (w.nslices != (nv + S - 1) / S || (int)w.sptr.size() != w.nslices + 1 || w.dinc.size() != (size_t)w.sptr[w.nslices] * S) return "slice sizes";
  long long filled = 0;
  for (int s = 0; s < w.nslices; s++) {
    int width = 0;
    for (int l = 0; l < S; l++) {
      const int v = s * S + l, len = v < nv ? w.rptr[v + 1] - w.rptr[v] : 0;
      width = std::max(width, len);
      for (int k = 0; k < w.sptr[s + 1] - w.sptr[s]; k++) {
        const int got = w.dinc[((size_t)w.sptr[s] + k) * S + l];
        if (got != (k < len ? w.inc[w.rptr[v] + k] : -1)) return "slice layout differs from the by-row layout";
        filled += got >= 0;
      }
    }
    if (width != w.sptr[s + 1] - w.sptr[s]) return "slice width";
  }
  return filled == w.ninc ? nullptr : "slice fill";
}

int main(int argc, char **argv) {
  if (argc < 2) return die("usage");
  std::FILE *f = std::fopen(argv[1], "rb");
  if (!f) return die("open");
  int hd[3];
  if (std::fread(hd, sizeof(int), 3, f) != 3) return die("header");
  const int D = hd[0], nv = hd[1], nc = hd[2], n1 = D + 1;
  std::vector<int> cells((size_t)nc * n1);
  if (!cells.empty() && std::fread(cells.data(), sizeof(int), cells.size(), f) != cells.size()) return die("read");
  std::fclose(f);

  std::string why;
  cfdh_flow::CellIndex w;
  std::vector<int> rank((size_t)nc), visit((size_t)nc);
  for (int e = 0; e < nc; e++) rank[e] = e;
  if (!cfdh_flow::build_index(D, nv, nc, cells.data(), nullptr, w, why)) return die("index", why);
  if (const char *bad = check(D, nv, nc, cells, rank, w)) return die("identity order:", bad);
  const int ninc = w.ninc, maxlen = w.maxlen;
  for (int k = 0; k < nc; k++) { visit[k] = nc - 1 - k; rank[nc - 1 - k] = k; }
  if (!cfdh_flow::build_index(D, nv, nc, cells.data(), visit.data(), w, why)) return die("index, reversed", why);
  if (const char *bad = check(D, nv, nc, cells, rank, w)) return die("reversed order:", bad);

  // refusals: a vertex out of range, a visiting order that is no permutation, a bad dimension
  if (nc > 0) {
    std::vector<int> broken(cells);
    broken[broken.size() / 2] = nv;
    if (cfdh_flow::build_index(D, nv, nc, broken.data(), nullptr, w, why)) return die("vertex out of range accepted");
    broken = cells;
    broken[0] = -1;
    if (cfdh_flow::build_index(D, nv, nc, broken.data(), nullptr, w, why)) return die("negative vertex accepted");
  }
  if (nc > 1) {
    visit[0] = visit[1];
    if (cfdh_flow::build_index(D, nv, nc, cells.data(), visit.data(), w, why)) return die("doubled cell in the visiting order accepted");
    visit[0] = nc;
    if (cfdh_flow::build_index(D, nv, nc, cells.data(), visit.data(), w, why)) return die("cell out of range in the visiting order accepted");
  }
  if (cfdh_flow::build_index(4, nv, nc, cells.data(), nullptr, w, why)) return die("D = 4 accepted");
  if (!cfdh_flow::build_index(D, 0, 0, nullptr, nullptr, w, why) || w.ninc != 0 || w.nslices != 0 || !w.dinc.empty()) return die("empty mesh", why);
  std::printf("ok %d incidences, valence up to %d\n", ninc, maxlen);
  return 0;
}
