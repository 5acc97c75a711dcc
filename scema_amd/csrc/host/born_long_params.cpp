// born_long_params.cpp -- reader of the script lines of `pair_style born/coul/long` and `buck/coul/long` (host/born_long_params.h) and
// its faces in the C ABI
#include "born_long_params.h"

#include "ionic_script.h"
#include "scema_md.h"

namespace scema {

using namespace ionic_script;

static bool long_style(const std::string &s) { return s == "born/coul/long" || s == "buck/coul/long"; }

bool read_born_long_params(const std::string &path, int energy_unit, BlTable &T, std::vector<int> &type_map, std::string &err, std::vector<double> *raw,
                           bool *has_style) {
  if (has_style) *has_style = false;
  auto fail = [&](int ln, const std::string &why) {
    err = path + " line " + std::to_string(ln) + ": " + why;
    return false;
  };
  std::vector<std::vector<Line>> lines;
  if (!read_lines(path, energy_unit, {"pair_style", "pair_coeff", "units", "kspace_style", "kspace_modify"}, lines, err)) return false;
  const std::vector<Line> &styles = lines[0], &coeffs = lines[1], &units = lines[2], &kstyles = lines[3], &kmods = lines[4];
  std::string why;
  // the style
  for (const Line &L : styles)
    if (L.w.size() < 2 || !long_style(L.w[1]))
      return fail(L.ln, "pair_style " + (L.w.size() > 1 ? L.w[1] : std::string("(none)")) + " is neither born/coul/long nor buck/coul/long");
  if (styles.empty()) return fail(0, "no `pair_style born/coul/long <cut_lj> [<cut_coul>]` or `pair_style buck/coul/long ...` line");
  if (has_style) *has_style = true;
  if (styles.size() > 1) return fail(styles[1].ln, "a second pair_style line");
  const Line &S = styles[0];
  const bool buck = S.w[1] == "buck/coul/long";
  if (S.w.size() < 3 || S.w.size() > 4) return fail(S.ln, "expected `pair_style " + S.w[1] + " <cut_lj> [<cut_coul>]`");
  double sv[2] = {0.0, 0.0};
  if (!numbers(S, 2, sv, why)) return fail(S.ln, why);
  const double cut_lj = sv[0], cut_coul = S.w.size() == 4 ? sv[1] : cut_lj;
  if (!(cut_lj > 0.0) || !(cut_coul > 0.0)) return fail(S.ln, "a cutoff must be positive");
  // the solver
  if (!kmods.empty()) return fail(kmods[0].ln, "a kspace_modify line: none of its options is honoured");
  if (kstyles.empty()) return fail(0, "no `kspace_style ewald|pppm <accuracy>` line (" + S.w[1] + " needs a long-range solver)");
  if (kstyles.size() > 1) return fail(kstyles[1].ln, "a second kspace_style line");
  const Line &Ks = kstyles[0];
  if (Ks.w.size() < 2 || (Ks.w[1] != "ewald" && Ks.w[1] != "pppm"))
    return fail(Ks.ln, "kspace_style " + (Ks.w.size() > 1 ? Ks.w[1] : std::string("(none)")) + " is neither ewald nor pppm");
  if (Ks.w.size() != 3) return fail(Ks.ln, "expected `kspace_style " + Ks.w[1] + " <accuracy>`");
  double accuracy = 0.0;
  if (!number(Ks.w[2], accuracy)) return fail(Ks.ln, "`" + Ks.w[2] + "` is not a finite number");
  if (!(accuracy > 0.0) || !(accuracy < 1.0)) return fail(Ks.ln, "the accuracy must be above 0 and below 1");
  // the units
  int unit, uln = 0;
  if (!resolve_units(units, energy_unit, unit, uln, why)) return fail(uln, why);
  // the coefficients
  std::vector<Coeff> cs;
  int ntypes = 0;
  const size_t nw = buck ? 6 : 8;   // words of a pair_coeff line without its own cutoff
  for (const Line &L : coeffs) {
    if (L.w.size() < nw || L.w.size() > nw + 1)
      return fail(L.ln, buck ? "expected `pair_coeff I J A rho C [cut_lj]` (buck/coul/long)" : "expected `pair_coeff I J A rho sigma C D [cut_lj]` (born/coul/long)");
    Coeff c;
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, cut_lj};
    if (!coeff_words(L, c, v, why)) return fail(L.ln, why);
    if (buck) {   // A rho C [cut]: sigma = 0, D = 0
      c.v[0] = v[0]; c.v[1] = v[1]; c.v[2] = 0.0; c.v[3] = v[2]; c.v[4] = 0.0; c.v[5] = L.w.size() == nw + 1 ? v[3] : cut_lj;
    } else {
      for (int k = 0; k < 6; k++) c.v[k] = v[k];
    }
    if (!coeff_add(c, cs, ntypes, why)) return fail(L.ln, why);
  }
  std::memset(&T, 0, sizeof T);
  std::vector<double> vals;
  if (!expand(cs, ntypes, unit, cut_coul, S.w[1], T.bd, vals, type_map, why)) return fail(S.ln, why);
  T.accuracy = accuracy;
  T.pppm = Ks.w[1] == "pppm" ? 1 : 0;
  T.buck = buck ? 1 : 0;
  if (raw) *raw = vals;
  return true;
}

}  // namespace scema

using scema::ionic_script::say;

extern "C" int scema_md_born_long_read_params(const char *path, int32_t energy_unit, int32_t *n_types, double *head, double *values, char *errbuf,
                                              int32_t errcap) {
  say(errbuf, errcap, "");
  if (!path || (energy_unit != 0 && energy_unit != 1)) { say(errbuf, errcap, "bad arguments"); return SCEMA_MD_ERR_ARG; }
  BlTable T;
  std::vector<int> map;
  std::vector<double> raw;
  std::string err;
  if (!scema::read_born_long_params(path, energy_unit, T, map, err, &raw)) { say(errbuf, errcap, err); return SCEMA_MD_ERR_IO; }
  if (n_types) *n_types = T.bd.ntypes;
  if (head) { head[0] = T.bd.cut_coul; head[1] = T.accuracy; head[2] = T.pppm; head[3] = T.bd.k; head[4] = T.bd.cutmax; head[5] = T.buck; }
  if (values) std::memcpy(values, raw.data(), raw.size() * sizeof(double));
  return SCEMA_MD_OK;
}

extern "C" int scema_md_born_long_eval(const char *path, int32_t energy_unit, double g_ewald, int32_t ti, int32_t tj, double qi, double qj, const double *r,
                                       int32_t n, double *out, char *errbuf, int32_t errcap) {
  say(errbuf, errcap, "");
  if (!path || (energy_unit != 0 && energy_unit != 1) || n < 0 || (n > 0 && (!r || !out)) || !(g_ewald >= 0.0)) { say(errbuf, errcap, "bad arguments"); return SCEMA_MD_ERR_ARG; }
  BlTable T;
  std::vector<int> map;
  std::string err;
  if (!scema::read_born_long_params(path, energy_unit, T, map, err)) { say(errbuf, errcap, err); return SCEMA_MD_ERR_IO; }
  if (ti < 0 || tj < 0 || ti >= T.bd.ntypes || tj >= T.bd.ntypes) { say(errbuf, errcap, "a type beyond the file's"); return SCEMA_MD_ERR_ARG; }
  for (int k = 0; k < n; k++) bl_pair(T, T.bd.pair[ti * BD_MAXEL + tj], g_ewald, qi, qj, r[k] * r[k], &out[4 * k], &out[4 * k + 1], &out[4 * k + 2], &out[4 * k + 3]);
  return SCEMA_MD_OK;
}
