"""The reader of the `pair_style born/coul/long` and `buck/coul/long` script lines (scema_amd/csrc/host/born_long_params.cpp) through its
pure-host faces in the library (scema_md_born_long_read_params, scema_md_born_long_eval: no GPU, no engine): what it takes from the two
fixtures against the independent parser of tests/born_long_numpy.py, bl_pair of the kernel against the numpy pair functions, and every
refusal with the line it names.
"""
import os

import numpy as np
import pytest

import born_long_numpy as bl
from scema_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NACL = os.path.join(ROOT, "tests", "golden", "NaCl.born_long")
MGO = os.path.join(ROOT, "tests", "golden", "MgO.buck_long")

GOOD = ["units metal", "pair_style born/coul/long 10.0", "pair_coeff 1 1 0.2637 0.317 2.340 1.05 -0.499", "pair_coeff 1 2 0.2110 0.317 2.755 6.99 -8.676",
        "pair_coeff 2 2 0.1582 0.317 3.170 72.40 -145.427", "kspace_style ewald 1.0e-5"]
BUCK = ["units metal", "pair_style buck/coul/long 8.0 9.0", "pair_coeff 1 1 0.0 0.3 0.0", "pair_coeff 1 2 1284.38 0.2997 0.0 7.0", "pair_coeff 2 2 9547.96 0.2192 32.0",
        "kspace_style pppm 1.0e-4"]


def _write(tmp_path, lines, name="frag.born_long"):
    p = tmp_path / name
    p.write_text("\n".join(lines) + "\n")
    return str(p)


@pytest.mark.parametrize("path", [NACL, MGO])
def test_fixtures_against_the_numpy_parser(path):
    got, ref = capi.born_long_read_params(path), bl.read_born_long(path)
    assert got["n"] == ref["n"] == 2
    assert (got["cut_coul"], got["K"], got["cutmax"]) == (ref["cut_coul"], ref["K"], bl.BornLong(ref).cutmax)
    assert (got["accuracy"], got["solver"], got["style"]) == (ref["accuracy"], ref["solver"], ref["style"])
    for k, name in enumerate(capi.BORN_DSF_FIELDS):
        assert np.array_equal(got["values"][:, :, k], ref[name]), name
    assert np.array_equal(got["values"], got["values"].transpose(1, 0, 2))
    if path == MGO:      # the Buckingham form: sigma = 0, D = 0; a per-pair cutoff; cut_coul beyond cut_lj; pppm at 1e-4
        assert not got["values"][:, :, 2].any() and not got["values"][:, :, 4].any()
        assert got["values"][:, :, 5].tolist() == [[8.0, 7.0], [7.0, 8.0]] and got["cut_coul"] == got["cutmax"] == 9.0
        assert (got["accuracy"], got["solver"], got["style"]) == (1e-4, "pppm", "buck")
        assert got["values"][1, 1, 3] == 32.0 * bl.EV_TO_KCALMOL
    else:
        assert (got["accuracy"], got["solver"], got["style"], got["cut_coul"]) == (1e-5, "ewald", "born", 10.0)


@pytest.mark.parametrize("path,pair,qq", [(NACL, (0, 1), (1.0, -1.0)), (NACL, (1, 1), (-1.0, -1.0)), (MGO, (0, 1), (1.2, -1.2)), (MGO, (1, 1), (-1.2, -1.2)),
                                          (MGO, (0, 0), (1.2, 0.0))])
def test_the_kernels_pair_function_against_numpy(path, pair, qq):
    """bl_pair on the host at distances across both cutoffs: energies and dE/dr = -f r to 1e-13 of the largest term, exact zeros beyond"""
    ref = bl.BornLong(bl.read_born_long(path))
    cut, g = ref.p["cut_lj"][pair], 0.3082
    r = np.concatenate([np.linspace(1.8, 11.0, 93), [cut - 1e-9, cut, ref.rc - 1e-9, ref.rc, ref.rc + 1e-9]])
    eb, ec, fb, fc = capi.born_long_eval(path, g, pair[0], pair[1], qq[0], qq[1], r)
    reb, rdeb = ref.born(pair[0], pair[1], r)
    rec, rdec = ref.real(g, qq[0] * qq[1], r)
    for got, want in ((eb, reb), (ec, rec), (-fb * r, rdeb), (-fc * r, rdec)):
        assert np.abs(got - want).max() <= 1e-13 * max(np.abs(want).max(), 1e-300)
    assert not eb[r >= cut].any() and not fb[r >= cut].any() and not ec[r >= ref.rc].any() and not fc[r >= ref.rc].any()
    if qq[0] * qq[1] != 0.0:      # neither term is shifted: just inside its cutoff it is its full value
        assert ec[r < ref.rc].all() and fc[r < ref.rc].all()


def test_both_energy_units(tmp_path):
    p = _write(tmp_path, GOOD[1:])      # no units line: the caller's energy unit decides
    metal, real = capi.born_long_read_params(p, 0), capi.born_long_read_params(p, 1)
    assert metal["K"] == bl.K_EV * bl.EV_TO_KCALMOL and real["K"] == bl.K_KCALMOL
    assert np.array_equal(metal["values"][:, :, [0, 3, 4]], real["values"][:, :, [0, 3, 4]] * bl.EV_TO_KCALMOL)
    assert np.array_equal(metal["values"][:, :, [1, 2, 5]], real["values"][:, :, [1, 2, 5]])
    assert capi.born_long_read_params(_write(tmp_path, ["units real"] + GOOD[1:]), 1)["K"] == bl.K_KCALMOL


def test_what_is_taken(tmp_path):
    """comments, other commands, a second cutoff word, a per-pair cutoff, `*` for either type, a later line overriding an earlier one, the
    kspace_style line anywhere, pppm for ewald"""
    p = _write(tmp_path, ["# a comment", "kspace_style pppm 1e-6", "variable a equal 1 # pair_style sw", "pair_style born/coul/long 6.0 9.5 # style",
                          "pair_coeff * * 1 0.3 2 3 4", "pair_coeff 1 * 2 0.31 2 3 4 7.5", "pair_coeff * 3 5 0.32 2 3 4", "pair_coeff 2 2 6 0.33 2 3 4 12.0", "run 100"])
    got = capi.born_long_read_params(p, 1)
    assert got["n"] == 3 and got["cut_coul"] == 9.5 and got["cutmax"] == 12.0 and (got["solver"], got["accuracy"]) == ("pppm", 1e-6)
    assert got["values"][:, :, 0].tolist() == [[2.0, 2.0, 5.0], [2.0, 6.0, 5.0], [5.0, 5.0, 5.0]]
    assert got["values"][:, :, 5].tolist() == [[7.5, 7.5, 6.0], [7.5, 12.0, 6.0], [6.0, 6.0, 6.0]]
    only_star = capi.born_long_read_params(_write(tmp_path, ["pair_style buck/coul/long 6.0", "pair_coeff * * 1 0.3 2", "kspace_style ewald 1e-4"]), 1)
    assert only_star["n"] == capi.BD_MAXEL and (only_star["values"][:, :, 0] == 1.0).all() and (only_star["values"][:, :, 3] == 2.0).all()


def _with(k, line, base=GOOD):
    out = list(base)
    out[k] = line
    return out


REFUSALS = [
    ("no pair_style line", [GOOD[0]] + GOOD[2:], r"line 0: no `pair_style born/coul/long"),
    ("two pair_style lines", GOOD + ["pair_style born/coul/long 10.0"], r"line 7: a second pair_style line"),
    ("another pair style", _with(1, "pair_style born/coul/dsf 0.25 10.0"), r"line 2: pair_style born/coul/dsf is neither born/coul/long nor buck/coul/long"),
    ("another pair style beside it", GOOD + ["pair_style sw"], r"line 7: pair_style sw is neither born/coul/long nor buck/coul/long"),
    ("a bare pair_style", _with(1, "pair_style"), r"line 2: pair_style \(none\) is neither"),
    ("cut_lj zero", _with(1, "pair_style born/coul/long 0.0"), r"line 2: a cutoff must be positive"),
    ("cut_coul negative", _with(1, "pair_style born/coul/long 10.0 -9.0"), r"line 2: a cutoff must be positive"),
    ("a pair's cutoff zero", _with(3, GOOD[3] + " 0.0"), r"line 4: a cutoff must be positive"),
    ("rho zero", _with(2, "pair_coeff 1 1 0.2637 0.0 2.340 1.05 -0.499"), r"line 3: rho must be positive"),
    ("rho negative", _with(4, "pair_coeff 2 2 0.1582 -0.317 3.170 72.40 -145.427"), r"line 5: rho must be positive"),
    ("a word that is no number", _with(3, "pair_coeff 1 2 0.2110 0.317 2.755 6.99 abc"), r"line 4: `abc` is not a finite number"),
    ("nan", _with(2, "pair_coeff 1 1 nan 0.317 2.340 1.05 -0.499"), r"line 3: `nan` is not a finite number"),
    ("inf", _with(1, "pair_style born/coul/long inf"), r"line 2: `inf` is not a finite number"),
    ("a LAMMPS variable", _with(1, "pair_style born/coul/long ${rc}"), r"line 2: `\$\{rc\}` is not a finite number"),
    ("a missing word", _with(3, "pair_coeff 1 2 0.2110 0.317 2.755 6.99"), r"line 4: expected `pair_coeff I J A rho sigma C D \[cut_lj\]` \(born/coul/long\)"),
    ("a surplus word", _with(3, GOOD[3] + " 9.0 1.0"), r"line 4: expected `pair_coeff I J A rho sigma C D \[cut_lj\]`"),
    ("a Buckingham line under born", _with(3, "pair_coeff 1 2 1284.38 0.2997 0.0"), r"line 4: expected `pair_coeff I J A rho sigma C D \[cut_lj\]` \(born/coul/long\)"),
    ("a Born line under buck", _with(3, GOOD[3], BUCK), r"line 4: expected `pair_coeff I J A rho C \[cut_lj\]` \(buck/coul/long\)"),
    ("a short Buckingham line", _with(2, "pair_coeff 1 1 0.0 0.3", BUCK), r"line 3: expected `pair_coeff I J A rho C \[cut_lj\]`"),
    ("a short pair_style", _with(1, "pair_style born/coul/long"), r"line 2: expected `pair_style born/coul/long <cut_lj> \[<cut_coul>\]`"),
    ("a long pair_style", _with(1, "pair_style buck/coul/long 10 10 10", BUCK), r"line 2: expected `pair_style buck/coul/long <cut_lj>"),
    ("I > J", _with(3, "pair_coeff 2 1 0.2110 0.317 2.755 6.99 -8.676"), r"line 4: pair_coeff I J needs I <= J"),
    ("a range", _with(3, "pair_coeff 1*2 2 0.2110 0.317 2.755 6.99 -8.676"), r"line 4: a type range `1\*2` is not taken"),
    ("a type above the limit", GOOD + ["pair_coeff 1 5 0.2110 0.317 2.755 6.99 -8.676"], r"line 7: atom type 5 is above the 4 types"),
    ("type zero", _with(2, "pair_coeff 0 1 0.2637 0.317 2.340 1.05 -0.499"), r"line 3: atom types count from 1"),
    ("a type that is no number", _with(2, "pair_coeff Na 1 0.2637 0.317 2.340 1.05 -0.499"), r"line 3: `Na` is not an atom type"),
    ("a pair never set", GOOD[:3] + GOOD[4:], r"line 2: no pair_coeff line sets the pair 1 2 \(born/coul/long has no mixing rule\)"),
    ("no pair_coeff at all", GOOD[:2] + GOOD[5:], r"line 2: no pair_coeff line sets the pair 1 1"),
    ("other units", _with(0, "units lj"), r"line 1: units must be real or metal"),
    ("units against the energy unit", _with(0, "units real"), r"line 1: units real contradicts energy unit 0"),
    ("no kspace_style line", GOOD[:5], r"line 0: no `kspace_style ewald\|pppm <accuracy>` line \(born/coul/long needs a long-range solver\)"),
    ("two kspace_style lines", GOOD + ["kspace_style pppm 1e-4"], r"line 7: a second kspace_style line"),
    ("another solver", _with(5, "kspace_style msm 1.0e-5"), r"line 6: kspace_style msm is neither ewald nor pppm"),
    ("a bare kspace_style", _with(5, "kspace_style"), r"line 6: kspace_style \(none\) is neither ewald nor pppm"),
    ("no accuracy", _with(5, "kspace_style ewald"), r"line 6: expected `kspace_style ewald <accuracy>`"),
    ("a surplus solver word", _with(5, "kspace_style pppm 1e-4 5"), r"line 6: expected `kspace_style pppm <accuracy>`"),
    ("accuracy zero", _with(5, "kspace_style ewald 0.0"), r"line 6: the accuracy must be above 0 and below 1"),
    ("accuracy negative", _with(5, "kspace_style ewald -1e-5"), r"line 6: the accuracy must be above 0 and below 1"),
    ("accuracy one", _with(5, "kspace_style ewald 1.0"), r"line 6: the accuracy must be above 0 and below 1"),
    ("an accuracy that is no number", _with(5, "kspace_style ewald fine"), r"line 6: `fine` is not a finite number"),
    ("a kspace_modify line", GOOD + ["kspace_modify gewald 0.3"], r"line 7: a kspace_modify line: none of its options is honoured"),
]


@pytest.mark.parametrize("what,lines,message", REFUSALS, ids=[r[0].replace(" ", "_") for r in REFUSALS])
def test_refusals_name_their_line(tmp_path, what, lines, message):
    p = _write(tmp_path, lines)
    with pytest.raises(IOError, match=r"rc=5: .*frag\.born_long " + message):
        capi.born_long_read_params(p, 0)
    with pytest.raises(IOError, match=message):
        capi.born_long_eval(p, 0.3, 0, 0, 1.0, 1.0, [2.0])
    with pytest.raises(IOError, match=message):
        capi.born_long_kvectors(p, [0, 0, 0, 12, 12, 12, 0, 0, 0], 8, 8.0)


def test_other_refusals(tmp_path):
    with pytest.raises(IOError, match=r"nowhere\.born_long: cannot open"):
        capi.born_long_read_params(str(tmp_path / "nowhere.born_long"))
    with pytest.raises(IOError, match="bad arguments"):
        capi.born_long_read_params(NACL, 2)
    with pytest.raises(IOError, match="a type beyond the file's"):
        capi.born_long_eval(NACL, 0.3, 0, 2, 1.0, 1.0, [2.0])
    with pytest.raises(IOError, match="bad arguments"):
        capi.born_long_kvectors(NACL, [0, 0, 0, 12, 12, 12, 0, 0, 0], 0, 8.0)
    assert capi.born_long_read_params(_write(tmp_path, GOOD))["n"] == 2 and capi.born_long_read_params(_write(tmp_path, BUCK))["style"] == "buck"
    # the DSF reader still refuses these lines under its own name, and this reader the DSF lines: a script configures one of the two
    with pytest.raises(IOError, match=r"line 2: pair_style born/coul/long is not born/coul/dsf"):
        capi.born_dsf_read_params(_write(tmp_path, GOOD))
