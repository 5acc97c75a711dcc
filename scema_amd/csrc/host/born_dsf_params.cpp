// born_dsf_params.cpp -- reader of the script lines of `pair_style born/coul/dsf` (host/born_dsf_params.h) and its faces in the C ABI
#include "born_dsf_params.h"

#include "ionic_script.h"
#include "scema_md.h"

namespace scema {

using namespace ionic_script;

bool read_born_dsf_params(const std::string &path, int energy_unit, BdTable &T, std::vector<int> &type_map, std::string &err, std::vector<double> *raw,
                          bool *has_style) {
  if (has_style) *has_style = false;
  auto fail = [&](int ln, const std::string &why) {
    err = path + " line " + std::to_string(ln) + ": " + why;
    return false;
  };
  std::vector<std::vector<Line>> lines;
  if (!read_lines(path, energy_unit, {"pair_style", "pair_coeff", "units"}, lines, err)) return false;
  const std::vector<Line> &styles = lines[0], &coeffs = lines[1], &units = lines[2];
  std::string why;
  // the style
  for (const Line &L : styles)
    if (L.w.size() < 2 || L.w[1] != "born/coul/dsf") return fail(L.ln, "pair_style " + (L.w.size() > 1 ? L.w[1] : std::string("(none)")) + " is not born/coul/dsf");
  if (styles.empty()) return fail(0, "no `pair_style born/coul/dsf <alpha> <cut_lj> [<cut_coul>]` line");
  if (has_style) *has_style = true;
  if (styles.size() > 1) return fail(styles[1].ln, "a second pair_style line");
  const Line &S = styles[0];
  if (S.w.size() < 4 || S.w.size() > 5) return fail(S.ln, "expected `pair_style born/coul/dsf <alpha> <cut_lj> [<cut_coul>]`");
  double sv[3] = {0.0, 0.0, 0.0};
  if (!numbers(S, 2, sv, why)) return fail(S.ln, why);
  const double alpha = sv[0], cut_lj = sv[1], cut_coul = S.w.size() == 5 ? sv[2] : cut_lj;
  if (!(alpha > 0.0)) return fail(S.ln, "alpha must be positive");
  if (!(cut_lj > 0.0) || !(cut_coul > 0.0)) return fail(S.ln, "a cutoff must be positive");
  // the units
  int unit, uln = 0;
  if (!resolve_units(units, energy_unit, unit, uln, why)) return fail(uln, why);
  // the coefficients
  std::vector<Coeff> cs;
  int ntypes = 0;
  for (const Line &L : coeffs) {
    if (L.w.size() < 8 || L.w.size() > 9) return fail(L.ln, "expected `pair_coeff I J A rho sigma C D [cut_lj]`");
    Coeff c;
    c.v[5] = cut_lj;
    if (!coeff_words(L, c, c.v, why) || !coeff_add(c, cs, ntypes, why)) return fail(L.ln, why);
  }
  std::memset(&T, 0, sizeof T);
  std::vector<double> vals;
  if (!expand(cs, ntypes, unit, cut_coul, "born/coul/dsf", T, vals, type_map, why)) return fail(S.ln, why);
  T.alpha = alpha;
  bd_shift(alpha, cut_coul, &T.e_s, &T.f_s);
  if (raw) *raw = vals;
  return true;
}

}  // namespace scema

using scema::ionic_script::say;

extern "C" int scema_md_born_dsf_read_params(const char *path, int32_t energy_unit, int32_t *n_types, double *head, double *values, char *errbuf,
                                             int32_t errcap) {
  say(errbuf, errcap, "");
  if (!path || (energy_unit != 0 && energy_unit != 1)) { say(errbuf, errcap, "bad arguments"); return SCEMA_MD_ERR_ARG; }
  BdTable T;
  std::vector<int> map;
  std::vector<double> raw;
  std::string err;
  if (!scema::read_born_dsf_params(path, energy_unit, T, map, err, &raw)) { say(errbuf, errcap, err); return SCEMA_MD_ERR_IO; }
  if (n_types) *n_types = T.ntypes;
  if (head) { head[0] = T.alpha; head[1] = T.cut_coul; head[2] = T.e_s; head[3] = T.f_s; head[4] = T.k; head[5] = T.cutmax; }
  if (values) std::memcpy(values, raw.data(), raw.size() * sizeof(double));
  return SCEMA_MD_OK;
}

extern "C" int scema_md_born_dsf_eval(const char *path, int32_t energy_unit, int32_t ti, int32_t tj, double qi, double qj, const double *r, int32_t n,
                                      double *out, double *e_self, char *errbuf, int32_t errcap) {
  say(errbuf, errcap, "");
  if (!path || (energy_unit != 0 && energy_unit != 1) || n < 0 || (n > 0 && (!r || !out))) { say(errbuf, errcap, "bad arguments"); return SCEMA_MD_ERR_ARG; }
  BdTable T;
  std::vector<int> map;
  std::string err;
  if (!scema::read_born_dsf_params(path, energy_unit, T, map, err)) { say(errbuf, errcap, err); return SCEMA_MD_ERR_IO; }
  if (ti < 0 || tj < 0 || ti >= T.ntypes || tj >= T.ntypes) { say(errbuf, errcap, "a type beyond the file's"); return SCEMA_MD_ERR_ARG; }
  for (int k = 0; k < n; k++) bd_pair(T, T.pair[ti * BD_MAXEL + tj], qi, qj, r[k] * r[k], &out[4 * k], &out[4 * k + 1], &out[4 * k + 2], &out[4 * k + 3]);
  if (e_self) { e_self[0] = bd_self(T, qi); e_self[1] = bd_self(T, qj); }
  return SCEMA_MD_OK;
}
