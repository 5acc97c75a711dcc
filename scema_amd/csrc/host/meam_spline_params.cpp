// meam_spline_params.cpp -- reader of LAMMPS spline-MEAM files (host/meam_spline_params.h) and its faces in the C ABI
#include "meam_spline_params.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <fstream>
#include <sstream>

#include "scema_md.h"
#include "triplet_file.h"

namespace scema {

namespace {

struct RawSpline {
  int n = 0, line_slopes = 0, line_last = 0;
  double d0 = 0.0, dn = 0.0;
  std::vector<double> x, y;
};

std::vector<std::string> words_of(const std::string &line) {
  std::istringstream ss(line);
  std::vector<std::string> w;
  for (std::string s; ss >> s;) w.push_back(s);
  return w;
}

// second derivatives of the clamped cubic spline through (x, y) with end slopes d0, dn: the tridiagonal system, forward sweep and back
// substitution
void clamped_second_derivatives(int n, const double *x, const double *y, double d0, double dn, double *y2) {
  std::vector<double> u(n);
  y2[0] = -0.5;
  u[0] = (3.0 / (x[1] - x[0])) * ((y[1] - y[0]) / (x[1] - x[0]) - d0);
  for (int i = 1; i < n - 1; i++) {
    const double sig = (x[i] - x[i - 1]) / (x[i + 1] - x[i - 1]);
    const double p = sig * y2[i - 1] + 2.0;
    y2[i] = (sig - 1.0) / p;
    const double dd = (y[i + 1] - y[i]) / (x[i + 1] - x[i]) - (y[i] - y[i - 1]) / (x[i] - x[i - 1]);
    u[i] = (6.0 * dd / (x[i + 1] - x[i - 1]) - sig * u[i - 1]) / p;
  }
  const double un = (3.0 / (x[n - 1] - x[n - 2])) * (dn - (y[n - 1] - y[n - 2]) / (x[n - 1] - x[n - 2]));
  y2[n - 1] = (un - 0.5 * u[n - 2]) / (0.5 * y2[n - 2] + 1.0);
  for (int k = n - 2; k >= 0; k--) y2[k] = y2[k] * y2[k + 1] + u[k];
}

void fill_fn(const RawSpline &R, double scale, MsFn &F) {
  std::memset(&F, 0, sizeof F);
  F.n = R.n;
  F.d0 = R.d0 * scale;
  F.dn = R.dn * scale;
  for (int k = 0; k < R.n; k++) { F.x[k] = R.x[k]; F.y[k] = R.y[k] * scale; }
  clamped_second_derivatives(R.n, F.x, F.y, F.d0, F.dn, F.y2);
  // (a spline whose solve overflows -- knots a rounding apart -- stays finite only by luck; the reader's callers check)
  const double h = (F.x[R.n - 1] - F.x[0]) / (R.n - 1);
  bool uniform = true;
  for (int k = 0; k + 1 < R.n; k++) uniform = uniform && std::fabs((F.x[k + 1] - F.x[k]) - h) <= 1e-9 * h;
  F.uniform = uniform ? 1 : 0;
  F.ih = uniform ? 1.0 / h : 0.0;
}

}  // namespace

bool read_meam_spline(const std::string &path, const std::vector<std::string> &elements, int energy_unit, MsTable &T, std::vector<int> &type_map,
                      std::string &err) {
  auto bad = [&](const std::string &m) { err = path + ": " + m; return false; };
  if (energy_unit != 0 && energy_unit != 1) return bad("energy unit " + std::to_string(energy_unit) + " (0: phi and U in eV, 1: in kcal/mol)");
  if (elements.empty()) return bad("no elements named");
  for (const std::string &s : elements)
    if (s.empty()) return bad("empty element name");
  std::ifstream in(path);
  if (!in) return bad("cannot open");
  std::vector<std::string> lines;
  for (std::string s; std::getline(in, s);) lines.push_back(s);
  size_t at = 0;   // lines consumed: the next one is line at + 1
  auto L = [&](size_t k) { return "line " + std::to_string(k); };
  auto take = [&](const char *what, std::vector<std::string> &w) {
    if (at >= lines.size()) { bad("truncated: " + L(at + 1) + " (" + what + ") is missing"); return false; }
    w = words_of(lines[at++]);
    return true;
  };
  std::vector<std::string> w;
  if (!take("the comment", w)) return false;
  // the header of the new format, or the first spline of the old one
  std::vector<std::string> file_el;
  bool fresh = false;
  if (at < lines.size()) {
    const std::vector<std::string> h = words_of(lines[at]);
    if (!h.empty() && h[0] == "meam/spline") {
      fresh = true;
      at++;
      double v = 0.0;
      if (h.size() < 2 || !word_number(h[1], v) || v != std::floor(v) || v < 1.0 || v > 16.0)
        return bad(L(at) + ": expected `meam/spline <number of elements, 1 to 16> <element> ...`");
      if ((size_t)v != h.size() - 2)
        return bad(L(at) + ": the header announces " + show_word(h[1]) + " elements and names " + std::to_string(h.size() - 2));
      file_el.assign(h.begin() + 2, h.end());
    }
  }
  const int nf = fresh ? (int)file_el.size() : 1, npf = nf * (nf + 1) / 2;
  // the elements kept and where each stands in the file
  std::vector<std::string> el;
  std::vector<int> file_of;
  type_map.assign(elements.size(), 0);
  for (size_t k = 0; k < elements.size(); k++) {
    if (!fresh) continue;   // (the old format names no element: every type is its one element)
    size_t m = 0;
    while (m < el.size() && el[m] != elements[k]) m++;
    if (m == el.size()) {
      const auto it = std::find(file_el.begin(), file_el.end(), elements[k]);
      if (it == file_el.end()) return bad("element " + show_word(elements[k]) + " is not among the elements of " + L(2));
      el.push_back(elements[k]);
      file_of.push_back((int)(it - file_el.begin()));
    }
    type_map[k] = (int)m;
  }
  if (!fresh) file_of.push_back(0);
  const int ne = (int)file_of.size();
  if (ne > MS_MAXEL) return bad("more than " + std::to_string(MS_MAXEL) + " distinct elements (MS_MAXEL)");
  // every spline of the file, in its order: phi (npf), rho, U, f (nf each), g (npf)
  const int total = 2 * npf + 3 * nf;
  std::vector<RawSpline> raw(total);
  for (int s = 0; s < total; s++) {
    RawSpline &R = raw[s];
    const std::string which = "spline " + std::to_string(s + 1) + " of " + std::to_string(total);
    if (fresh) {
      if (!take("`spline3eq`", w)) return false;
      if (w.size() != 1 || w[0] != "spline3eq") return bad(L(at) + ": expected `spline3eq` before " + which);
    }
    if (!take("a number of knots", w)) return false;
    double v = 0.0;
    if (w.size() != 1 || !word_number(w[0], v) || v != std::floor(v)) return bad(L(at) + ": expected the number of knots of " + which);
    if (v < 2.0) return bad(L(at) + ": " + which + " has fewer than 2 knots");
    if (v > (double)MS_MAXKNOT) return bad(L(at) + ": " + which + " has more than " + std::to_string(MS_MAXKNOT) + " knots (MS_MAXKNOT)");
    R.n = (int)v;
    if (!take("the end slopes", w)) return false;
    if (w.size() != 2 || !word_number(w[0], R.d0) || !word_number(w[1], R.dn)) return bad(L(at) + ": expected the two end slopes of " + which + " as finite numbers");
    R.line_slopes = (int)at;
    if (!fresh && !take("the line after the end slopes", w)) return false;
    R.x.resize(R.n);
    R.y.resize(R.n);
    for (int k = 0; k < R.n; k++) {
      if (!take("a knot", w)) return false;
      double y2 = 0.0;
      if (w.size() != 3 || !word_number(w[0], R.x[k]) || !word_number(w[1], R.y[k]) || !word_number(w[2], y2))
        return bad(L(at) + ": expected `x y y2` as three finite numbers (knot " + std::to_string(k + 1) + " of " + which + ")");
      if (k > 0 && !(R.x[k] > R.x[k - 1])) return bad(L(at) + ": the knots of " + which + " are not strictly ascending");
    }
    R.line_last = (int)at;
    const bool ranged = s < npf + nf || (s >= npf + 2 * nf && s < npf + 3 * nf);   // phi, rho, f
    if (ranged && R.y[R.n - 1] != 0.0) return bad(L(R.line_last) + ": " + which + " (phi, rho or f) does not end with the value 0: the energy would jump at its cutoff");
    if (ranged && R.dn != 0.0) return bad(L(R.line_slopes) + ": " + which + " (phi, rho or f) does not end with the slope 0: the force would jump at its cutoff");
  }
  std::memset(&T, 0, sizeof T);
  const int np = ne * (ne + 1) / 2;
  T.nelem = ne;
  T.nfn = 2 * np + 3 * ne;
  T.off_phi = 0; T.off_rho = np; T.off_u = np + ne; T.off_f = np + 2 * ne; T.off_g = np + 3 * ne;
  const double es = energy_unit == 0 ? MS_EV_TO_KCALMOL : 1.0;
  for (int a = 0; a < ne; a++) {
    const int fa = file_of[a];
    fill_fn(raw[npf + fa], 1.0, T.fn[T.off_rho + a]);
    fill_fn(raw[npf + nf + fa], es, T.fn[T.off_u + a]);
    fill_fn(raw[npf + 2 * nf + fa], 1.0, T.fn[T.off_f + a]);
    for (int b = a; b < ne; b++) {
      const int fp = ms_pair_index(nf, fa, file_of[b]), kp = ms_pair_index(ne, a, b);
      fill_fn(raw[fp], es, T.fn[T.off_phi + kp]);
      fill_fn(raw[npf + 3 * nf + fp], 1.0, T.fn[T.off_g + kp]);
    }
  }
  for (int k = 0; k < T.nfn; k++)
    for (int q = 0; q < T.fn[k].n; q++)
      if (!std::isfinite(T.fn[k].y2[q])) return bad("the second derivatives of function " + std::to_string(k + 1) + " of the elements kept are not finite (knots too close; the file ends on " + L(lines.size()) + ")");
  for (int a = 0; a < ne; a++) {
    double dy;
    T.u0[a] = ms_eval(T.fn[T.off_u + a], 0.0, &dy);
    const MsFn &R = T.fn[T.off_rho + a], &F = T.fn[T.off_f + a];
    T.cutmax = std::max(T.cutmax, std::max(R.x[R.n - 1], F.x[F.n - 1]));
    for (int b = 0; b < ne; b++) T.cut_f[b][a] = F.x[F.n - 1];
    for (int b = a; b < ne; b++) {
      const MsFn &P = T.fn[T.off_phi + ms_pair_index(ne, a, b)];
      T.cutmax = std::max(T.cutmax, P.x[P.n - 1]);
    }
  }
  if (!(T.cutmax > 0.0)) return bad("no positive range: the last knots of phi, rho and f are all <= 0 (" + L(lines.size()) + ")");
  return true;
}

}  // namespace scema

namespace {
void say_into(char *errbuf, int32_t errcap, const std::string &m) {
  if (errbuf && errcap > 0) { std::strncpy(errbuf, m.c_str(), (size_t)errcap - 1); errbuf[errcap - 1] = 0; }
}
bool read_for_capi(const char *path, const char *const *elements, int32_t n_elements, int32_t energy_unit, MsTable &T, std::vector<int> &map, char *errbuf,
                   int32_t errcap, int *rc) {
  say_into(errbuf, errcap, "");
  if (!path || !elements || n_elements <= 0) { say_into(errbuf, errcap, "bad arguments"); *rc = SCEMA_MD_ERR_ARG; return false; }
  std::vector<std::string> el;
  for (int k = 0; k < n_elements; k++) el.push_back(elements[k] ? elements[k] : "");
  std::string err;
  if (!scema::read_meam_spline(path, el, energy_unit, T, map, err)) { say_into(errbuf, errcap, err); *rc = SCEMA_MD_ERR_IO; return false; }
  return true;
}
}  // namespace

extern "C" int scema_md_meam_spline_read_params(const char *path, const char *const *elements, int32_t n_elements, int32_t energy_unit, int32_t *n_kept,
                                                int32_t *type_map, int32_t *knots, double *head, double *values, char *errbuf, int32_t errcap) {
  MsTable T;
  std::vector<int> map;
  int rc = SCEMA_MD_OK;
  if (!read_for_capi(path, elements, n_elements, energy_unit, T, map, errbuf, errcap, &rc)) return rc;
  if (n_kept) *n_kept = T.nelem;
  if (type_map) for (int k = 0; k < n_elements; k++) type_map[k] = map[k];
  if (knots) for (int k = 0; k < MS_NFN; k++) knots[k] = k < T.nfn ? T.fn[k].n : 0;
  if (head) {
    head[0] = T.cutmax; head[1] = T.nfn;
    for (int a = 0; a < MS_MAXEL; a++) {
      head[2 + a] = T.u0[a];
      for (int b = 0; b < MS_MAXEL; b++) head[2 + MS_MAXEL + a * MS_MAXEL + b] = T.cut_f[a][b];
    }
  }
  if (values)
    for (int k = 0; k < MS_NFN; k++) {
      double *v = values + (size_t)k * (4 + 3 * MS_MAXKNOT);
      const MsFn &F = T.fn[k];
      v[0] = F.d0; v[1] = F.dn; v[2] = F.uniform; v[3] = F.ih;
      std::memcpy(v + 4, F.x, sizeof F.x);
      std::memcpy(v + 4 + MS_MAXKNOT, F.y, sizeof F.y);
      std::memcpy(v + 4 + 2 * MS_MAXKNOT, F.y2, sizeof F.y2);
    }
  return SCEMA_MD_OK;
}

extern "C" int scema_md_meam_spline_eval(const char *path, const char *const *elements, int32_t n_elements, int32_t energy_unit, int32_t fn, int32_t mode,
                                         const double *x, int32_t n, double *y, double *dy, char *errbuf, int32_t errcap) {
  MsTable T;
  std::vector<int> map;
  int rc = SCEMA_MD_OK;
  if (!read_for_capi(path, elements, n_elements, energy_unit, T, map, errbuf, errcap, &rc)) return rc;
  if (fn < 0 || fn >= T.nfn || (mode != 0 && mode != 1) || n < 0 || (n > 0 && (!x || !y || !dy))) {
    say_into(errbuf, errcap, "bad arguments: function " + std::to_string(fn) + " of " + std::to_string(T.nfn) + ", mode " + std::to_string(mode));
    return SCEMA_MD_ERR_ARG;
  }
  for (int k = 0; k < n; k++) y[k] = ms_eval_by(T.fn[fn], x[k], &dy[k], mode == 1);
  return SCEMA_MD_OK;
}
