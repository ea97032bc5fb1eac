// Stand-alone run of csrc/cfdh_section_host.hpp for tests/test_section_twin.py, built with -fsanitize=address,undefined: reads a
// mesh (header of int32: D nv nc; then coords as float64 and cells as int32), cuts it with planes through its centre, through
// vertices, outside its box and with clip balls, in the given order and in a reversed, re-oriented storage, checks the lists
// against their definition, evaluates a field and runs the refusals; prints "ok ..." and returns 0, or says what failed.
#include <cstdio>
#include <cstdlib>

#include "cfdh_section_host.hpp"

static int die(const char *what, const std::string &why = "") {
  std::printf("FAILED %s %s\n", what, why.c_str());
  return 1;
}

// shape of the lists and of every entry
static const char *check(int D, int nc, const std::vector<int> &user_of, const cfdh_section::Cut &C) {
  const int NP = cfdh_section::np_of(D), NT = cfdh_section::nt_of(D);
  if ((int)C.ptr.size() != C.K + 1 || C.ptr[0] != 0 || C.ptr[C.K] != C.total) return "ptr";
  if ((long long)C.cell.size() != C.total || (long long)C.code.size() != C.total || (long long)C.t.size() != C.total * NP ||
      (long long)C.meas.size() != C.total * NT || (int)C.straddling.size() != C.K || (int)C.normal.size() != 3 * C.K)
    return "sizes";
  long long maxlen = 0;
  for (int k = 0; k < C.K; k++) {
    if (C.ptr[k + 1] < C.ptr[k]) return "ptr not monotone";
    maxlen = std::max(maxlen, C.ptr[k + 1] - C.ptr[k]);
    double len = 0.0;
    for (int i = 0; i < 3; i++) len += C.normal[3 * k + i] * C.normal[3 * k + i];
    if (std::fabs(len - 1.0) > 1e-14) return "normal is not a unit vector";
    for (long long i = C.ptr[k]; i < C.ptr[k + 1]; i++) {
      if (C.cell[i] < 0 || C.cell[i] >= nc) return "cell out of range";
      if (i > C.ptr[k] && user_of[C.cell[i - 1]] >= user_of[C.cell[i]]) return "not ascending in the caller's index, or a cell twice";
      const int npoly = cfdh_section::code_n(C.code[i]);
      if (npoly != (D == 2 ? 2 : 3) && !(D == 3 && npoly == 4)) return "number of polygon vertices";
      for (int j = 0; j < NP; j++) {
        const int a = cfdh_section::code_a(C.code[i], j), b = cfdh_section::code_b(C.code[i], j);
        if (a > D || b > D || a == b) return "local edge";
        const double t = C.t[(size_t)NP * i + j];
        if (!(t >= 0.0 && t <= 1.0)) return "t outside [0, 1]";
      }
      for (int j = 0; j < NT; j++)
        if (!(C.meas[(size_t)NT * i + j] >= 0.0)) return "negative measure";
      if (D == 3 && npoly == 3 && C.meas[(size_t)NT * i + 1] != 0.0) return "a triangle with a second measure";
    }
  }
  if (maxlen != C.maxlen) return "maxlen";
  return nullptr;
}

int main(int argc, char **argv) {
  if (argc < 2) return die("usage");
  std::FILE *f = std::fopen(argv[1], "rb");
  if (!f) return die("open");
  int hd[3];
  if (std::fread(hd, sizeof(int), 3, f) != 3) return die("header");
  const int D = hd[0], nv = hd[1], nc = hd[2], n1 = D + 1, stride = 2 * D + 1;
  std::vector<double> x((size_t)nv * D);
  std::vector<int> cells((size_t)nc * n1);
  if (!x.empty() && std::fread(x.data(), sizeof(double), x.size(), f) != x.size()) return die("read coords");
  if (!cells.empty() && std::fread(cells.data(), sizeof(int), cells.size(), f) != cells.size()) return die("read cells");
  std::fclose(f);
  if (nv < 1 || nc < 1) return die("empty mesh");

  double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}, mid[3], diag = 0.0;
  for (int v = 0; v < nv; v++)
    for (int i = 0; i < D; i++) {
      const double xi = x[(size_t)D * v + i];
      if (v == 0 || xi < lo[i]) lo[i] = xi;
      if (v == 0 || xi > hi[i]) hi[i] = xi;
    }
  for (int i = 0; i < D; i++) { mid[i] = 0.5 * (lo[i] + hi[i]); diag += (hi[i] - lo[i]) * (hi[i] - lo[i]); }
  diag = std::sqrt(diag);

  // planes: per axis through the centre, unbounded and with a small and a large ball; the diagonal through vertex 0; one through
  // the last vertex; one outside the box
  std::vector<double> planes;
  auto plane = [&](const double *o, const double *n, double r) {
    for (int i = 0; i < D; i++) planes.push_back(o[i]);
    for (int i = 0; i < D; i++) planes.push_back(n[i]);
    planes.push_back(r);
  };
  for (int a = 0; a < D; a++) {
    double n[3] = {0, 0, 0};
    n[a] = 2.5;
    plane(mid, n, 0.0);
    plane(mid, n, 0.05 * diag);
    plane(mid, n, 10.0 * diag);
    n[a] = -1.0;
    plane(mid, n, -1.0);
  }
  const double ones[3] = {1.0, 1.0, 1.0};
  plane(&x[0], ones, 0.0);
  plane(&x[(size_t)D * (nv - 1)], ones, 0.0);
  double far[3];
  for (int i = 0; i < D; i++) far[i] = hi[i] + diag;
  plane(far, ones, 0.0);
  const int K = (int)(planes.size() / stride);

  std::string why;
  cfdh_section::Cut C, R;
  std::vector<int> user_of((size_t)nc);
  for (int e = 0; e < nc; e++) user_of[e] = e;
  if (!cfdh_section::build_cut(D, nv, nc, cells.data(), x.data(), nullptr, nullptr, K, planes.data(), C, why)) return die("cut", why);
  if (const char *bad = check(D, nc, user_of, C)) return die("identity order:", bad);
  if (C.ptr[K] != C.ptr[K - 1]) return die("a plane outside the box cuts cells");
  for (int a = 0; a < D; a++) {
    const long long *p = &C.ptr[4 * a];
    if (p[1] - p[0] < 1) return die("a plane through the centre cuts nothing");
    if (p[3] - p[2] != p[1] - p[0] || C.straddling[4 * a + 2] != 0) return die("a ball around the whole mesh drops cells");
    if (p[2] - p[1] > p[1] - p[0]) return die("a small ball takes more than the plane");
  }

  // the same mesh stored in reverse order with the last two vertices of every second cell swapped
  std::vector<int> stored((size_t)nc * n1);
  std::vector<unsigned char> flipped((size_t)nc);
  for (int e = 0; e < nc; e++) {
    const int old = nc - 1 - e;
    user_of[e] = old;
    for (int a = 0; a < n1; a++) stored[(size_t)n1 * e + a] = cells[(size_t)n1 * old + a];
    flipped[e] = (unsigned char)(old & 1);
    if (flipped[e]) std::swap(stored[(size_t)n1 * e + n1 - 2], stored[(size_t)n1 * e + n1 - 1]);
  }
  if (!cfdh_section::build_cut(D, nv, nc, stored.data(), x.data(), user_of.data(), flipped.data(), K, planes.data(), R, why)) return die("cut, reversed", why);
  if (const char *bad = check(D, nc, user_of, R)) return die("reversed order:", bad);
  if (R.ptr != C.ptr || R.straddling != C.straddling) return die("the lists depend on the storage");
  const int NP = cfdh_section::np_of(D), NT = cfdh_section::nt_of(D);
  for (long long i = 0; i < C.total; i++) {
    if (user_of[R.cell[i]] != C.cell[i]) return die("the cells depend on the storage");
    for (int j = 0; j < NP; j++)
      if (R.t[(size_t)NP * i + j] != C.t[(size_t)NP * i + j]) return die("t depends on the storage");
    for (int j = 0; j < NT; j++)
      if (R.meas[(size_t)NT * i + j] != C.meas[(size_t)NT * i + j]) return die("the measures depend on the storage");
  }

  // a field, evaluated on both storages
  std::vector<double> u((size_t)nv * D), p((size_t)nv), rows((size_t)K * cfdh_section::NQ), rows_r(rows.size());
  for (int v = 0; v < nv; v++) {
    for (int i = 0; i < D; i++) u[(size_t)D * v + i] = std::sin(1.0 + 3.0 * v + i);
    p[v] = std::cos(0.5 * v);
  }
  cfdh_section::eval_rows(C, cells.data(), u.data(), p.data(), 1.06, rows.data());
  cfdh_section::eval_rows(R, stored.data(), u.data(), p.data(), 1.06, rows_r.data());
  for (size_t j = 0; j < rows.size(); j++) {
    const double scale = std::fabs(rows[cfdh_section::NQ * (j / cfdh_section::NQ)]) * 2.0 + 1e-300;  // 2 A bounds every slot of |u|, |p| <= 1, rho ~ 1
    if (!(std::fabs(rows[j] - rows_r[j]) <= 1e-12 * scale)) return die("the rows depend on the storage");
  }
  for (int s = 0; s < cfdh_section::NQ; s++)
    if (rows[(size_t)cfdh_section::NQ * (K - 1) + s] != 0.0 || std::signbit(rows[(size_t)cfdh_section::NQ * (K - 1) + s])) return die("an empty section is not +0.0");

  // refusals
  std::vector<double> bad(planes);
  if (cfdh_section::build_cut(D, nv, nc, cells.data(), x.data(), nullptr, nullptr, 257, planes.data(), R, why)) return die("K = 257 accepted");
  if (cfdh_section::build_cut(D, nv, nc, cells.data(), x.data(), nullptr, nullptr, -1, planes.data(), R, why)) return die("K = -1 accepted");
  for (int i = 0; i < stride; i++) {
    for (double v : {std::nan(""), HUGE_VAL}) {
      bad = planes;
      bad[stride + i] = v;
      if (cfdh_section::build_cut(D, nv, nc, cells.data(), x.data(), nullptr, nullptr, K, bad.data(), R, why)) return die("a non-finite entry accepted");
    }
  }
  bad = planes;
  for (int i = 0; i < D; i++) bad[D + i] = 0.0;
  if (cfdh_section::build_cut(D, nv, nc, cells.data(), x.data(), nullptr, nullptr, K, bad.data(), R, why)) return die("a zero normal accepted");
  if (cfdh_section::build_cut(D, nv, nc, cells.data(), x.data(), nullptr, nullptr, K, planes.data(), R, why, C.total - 1)) return die("more entries than the limit accepted");
  if (!cfdh_section::build_cut(D, nv, nc, cells.data(), x.data(), nullptr, nullptr, K, planes.data(), R, why, C.total)) return die("the limit itself refused", why);
  std::vector<int> broken(cells);
  broken[broken.size() / 2] = nv;
  if (cfdh_section::build_cut(D, nv, nc, broken.data(), x.data(), nullptr, nullptr, K, planes.data(), R, why)) return die("vertex out of range accepted");
  if (nc > 1) {
    std::vector<int> twice(user_of);
    twice[0] = twice[1];
    if (cfdh_section::build_cut(D, nv, nc, cells.data(), x.data(), twice.data(), nullptr, K, planes.data(), R, why)) return die("doubled caller's index accepted");
  }
  if (cfdh_section::build_cut(4, nv, nc, cells.data(), x.data(), nullptr, nullptr, K, planes.data(), R, why)) return die("D = 4 accepted");
  if (!cfdh_section::build_cut(D, nv, nc, cells.data(), x.data(), nullptr, nullptr, 0, nullptr, R, why) || R.total != 0 || R.ptr.size() != 1) return die("K = 0", why);
  std::printf("ok %lld entries in %d sections, longest list %lld\n", C.total, K, C.maxlen);
  return 0;
}
