// eam_coul_params.cpp -- reader of the script lines of `pair_style hybrid/overlay coul/long <cut_coul> eam/alloy`, the builder of the
// stage's table block (host/eam_coul_params.h) and their face in the C ABI
#include "eam_coul_params.h"

#include "eam_setfl.h"
#include "ionic_script.h"
#include "scema_md.h"

namespace scema {

using namespace ionic_script;

bool read_eam_coul_script(const std::string &path, int energy_unit, EamCoulParams &P, std::string &err, bool *has_style) {
  if (has_style) *has_style = false;
  auto fail = [&](int ln, const std::string &why) {
    err = path + " line " + std::to_string(ln) + ": " + why;
    return false;
  };
  std::vector<std::vector<Line>> lines;
  if (!read_lines(path, energy_unit, {"pair_style", "pair_coeff", "units", "kspace_style", "kspace_modify"}, lines, err)) return false;
  const std::vector<Line> &styles = lines[0], &coeffs = lines[1], &units = lines[2], &kstyles = lines[3], &kmods = lines[4];
  std::string why;
  // the style: its two sub-styles in either order
  for (const Line &L : styles)
    if (L.w.size() < 2 || L.w[1] != "hybrid/overlay")
      return fail(L.ln, "pair_style " + (L.w.size() > 1 ? L.w[1] : std::string("(none)")) + " is not hybrid/overlay");
  if (styles.empty()) return fail(0, "no `pair_style hybrid/overlay coul/long <cut_coul> eam/alloy` line");
  if (has_style) *has_style = true;
  if (styles.size() > 1) return fail(styles[1].ln, "a second pair_style line");
  const Line &S = styles[0];
  bool has_coul = false, has_eam = false;
  double cut_coul = 0.0;
  for (size_t k = 2; k < S.w.size(); k++) {
    const std::string &s = S.w[k];
    if (s == "coul/long") {
      if (has_coul) return fail(S.ln, "sub-style coul/long given twice");
      if (k + 1 >= S.w.size()) return fail(S.ln, "expected `coul/long <cut_coul>`");
      if (!number(S.w[k + 1], cut_coul)) return fail(S.ln, "`" + S.w[k + 1] + "` is not a finite number (cut_coul)");
      has_coul = true;
      k++;
    } else if (s == "eam/alloy") {
      if (has_eam) return fail(S.ln, "sub-style eam/alloy given twice");
      has_eam = true;
    } else if (has_coul && has_eam) {
      return fail(S.ln, "a third sub-style `" + s + "`: hybrid/overlay is taken with coul/long and eam/alloy alone");
    } else {
      return fail(S.ln, "sub-style `" + s + "` is neither coul/long nor eam/alloy");
    }
  }
  if (!has_coul || !has_eam) return fail(S.ln, "expected `pair_style hybrid/overlay coul/long <cut_coul> eam/alloy`");
  if (!(cut_coul > 0.0)) return fail(S.ln, "cut_coul must be positive");
  // the solver
  if (!kmods.empty()) return fail(kmods[0].ln, "a kspace_modify line: none of its options is honoured");
  if (kstyles.empty()) return fail(0, "no `kspace_style ewald|pppm <accuracy>` line (coul/long needs a long-range solver)");
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
  // the two pair_coeff lines
  const Line *ccoul = nullptr, *ceam = nullptr;
  for (const Line &L : coeffs) {
    if (L.w.size() < 4 || L.w[1] != "*" || L.w[2] != "*") return fail(L.ln, "expected `pair_coeff * * coul/long` or `pair_coeff * * eam/alloy <file> <element> ...`");
    if (L.w[3] == "coul/long") {
      if (ccoul) return fail(L.ln, "a second `pair_coeff * * coul/long` line");
      if (L.w.size() != 4) return fail(L.ln, "`pair_coeff * * coul/long` takes no further word");
      ccoul = &L;
    } else if (L.w[3] == "eam/alloy") {
      if (ceam) return fail(L.ln, "a second `pair_coeff * * eam/alloy` line");
      if (L.w.size() < 6) return fail(L.ln, "expected `pair_coeff * * eam/alloy <file> <element> ...` (one element per atom type)");
      for (size_t k = 5; k < L.w.size(); k++)
        if (L.w[k] == "NULL") return fail(L.ln, "NULL as an element: every atom type takes both sub-styles");
      ceam = &L;
    } else {
      return fail(L.ln, "pair_coeff for sub-style `" + L.w[3] + "`, which is neither coul/long nor eam/alloy");
    }
  }
  if (!ccoul) return fail(0, "no `pair_coeff * * coul/long` line");
  if (!ceam) return fail(0, "no `pair_coeff * * eam/alloy <file> <element> ...` line");
  // the file: ${locs}/ and relative names from the script's own folder
  const size_t slash = path.find_last_of('/');
  const std::string folder = slash == std::string::npos ? std::string(".") : (slash == 0 ? std::string("/") : path.substr(0, slash));
  const std::string locs = "${locs}/";
  std::string file = ceam->w[4];
  if (file.compare(0, locs.size(), locs) == 0) file = file.substr(locs.size());
  if (file.empty()) return fail(ceam->ln, "an empty file name");
  P = EamCoulParams();
  P.setfl = file[0] == '/' ? file : folder + "/" + file;
  P.elements.assign(ceam->w.begin() + 5, ceam->w.end());
  P.cut_coul = cut_coul;
  P.accuracy = accuracy;
  P.pppm = Ks.w[1] == "pppm" ? 1 : 0;
  P.unit = unit;
  P.k = unit == 0 ? BD_COULOMB_EV * BD_EV_TO_KCALMOL : BD_COULOMB_KCALMOL;
  return true;
}

bool build_eam_coul_block(const std::string &path, int energy_unit, std::vector<double> &block, std::vector<int> &type_map, EamCoulParams &P, std::string &err,
                          bool *has_style) {
  if (!read_eam_coul_script(path, energy_unit, P, err, has_style)) return false;
  std::vector<double> eam;
  if (!read_eam_setfl(P.setfl, P.elements, P.unit, eam, type_map, err)) return false;
  const EamHead &H = eam_head(eam);
  BlTable T;
  std::memset(&T, 0, sizeof T);   // (every Born pair zero, cut_lj2 = 0 included: no distance is inside it)
  T.bd.ntypes = H.nelem;
  T.bd.cut_coul = P.cut_coul;
  T.bd.k = P.k;
  T.bd.cutmax = std::max(H.cutoff, P.cut_coul);
  T.accuracy = P.accuracy;
  T.pppm = P.pppm;
  block.assign((size_t)EC_EAM_OFF + eam.size(), 0.0);
  std::memcpy(block.data(), &T, sizeof T);
  std::memcpy(block.data() + EC_EAM_OFF, eam.data(), eam.size() * sizeof(double));
  return true;
}

}  // namespace scema

extern "C" int scema_md_eam_coul_read_params(const char *path, int32_t energy_unit, double *head, int32_t *n_types, int32_t *type_map, int32_t type_cap,
                                             char *setfl_path, int32_t setfl_cap, char *errbuf, int32_t errcap) {
  using scema::ionic_script::say;
  say(errbuf, errcap, "");
  if (!path || energy_unit < -1 || energy_unit > 1 || type_cap < 0 || setfl_cap < 0) { say(errbuf, errcap, "bad arguments"); return SCEMA_MD_ERR_ARG; }
  std::vector<double> block;
  std::vector<int> map;
  scema::EamCoulParams P;
  std::string err;
  if (!scema::build_eam_coul_block(path, energy_unit, block, map, P, err)) { say(errbuf, errcap, err); return SCEMA_MD_ERR_IO; }
  const BlTable &T = scema::eam_coul_table(block);
  const EamHead &H = scema::eam_coul_head(block);
  if (head) { head[0] = T.bd.cut_coul; head[1] = T.accuracy; head[2] = T.pppm; head[3] = T.bd.k; head[4] = T.bd.cutmax; head[5] = H.cutoff; }
  if (n_types) *n_types = (int32_t)map.size();
  if (type_map)
    for (int k = 0; k < (int)map.size() && k < type_cap; k++) type_map[k] = map[k];
  if (setfl_path) say(setfl_path, setfl_cap, P.setfl);
  return SCEMA_MD_OK;
}
