"""The reader of the `pair_style born/coul/dsf` script lines (scema_amd/csrc/host/born_dsf_params.cpp) through its pure-host faces in the
library (scema_md_born_dsf_read_params, scema_md_born_dsf_eval: no GPU, no engine): what it takes from the two fixtures against the
independent parser of tests/born_dsf_numpy.py, the shift constants, bd_pair of the kernel against the numpy pair functions, and every
refusal with the line it names.
"""
import math
import os

import numpy as np
import pytest

import born_dsf_numpy as bn
from scema_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NACL = os.path.join(ROOT, "tests", "golden", "NaCl.born_dsf")
KNACL = os.path.join(ROOT, "tests", "golden", "KNaCl.born_dsf")

GOOD = ["units metal", "pair_style born/coul/dsf 0.25 10.0", "pair_coeff 1 1 0.2637 0.317 2.340 1.05 -0.499", "pair_coeff 1 2 0.2110 0.317 2.755 6.99 -8.676",
        "pair_coeff 2 2 0.1582 0.317 3.170 72.40 -145.427"]


def _write(tmp_path, lines, name="frag.born_dsf"):
    p = tmp_path / name
    p.write_text("\n".join(lines) + "\n")
    return str(p)


@pytest.mark.parametrize("path", [NACL, KNACL])
def test_fixtures_against_the_numpy_parser(path):
    got, ref = capi.born_dsf_read_params(path), bn.read_born_dsf(path)
    bd = bn.BornDsf(ref)
    assert got["n"] == ref["n"] == (2 if path == NACL else 3)
    assert (got["alpha"], got["cut_coul"], got["K"], got["cutmax"]) == (ref["alpha"], ref["cut_coul"], ref["K"], bd.cutmax)
    assert abs(got["e_s"] - bd.e_s) <= 1e-15 * bd.e_s and abs(got["f_s"] - bd.f_s) <= 1e-15 * bd.f_s
    for k, name in enumerate(capi.BORN_DSF_FIELDS):
        assert np.array_equal(got["values"][:, :, k], ref[name]), name
    assert np.array_equal(got["values"], got["values"].transpose(1, 0, 2))
    if path == KNACL:      # per-pair cutoffs, the `*` line for the pair 2 3 alone, cut_coul beyond every cut_lj
        assert got["values"][:, :, 5].tolist() == [[7.0, 8.0, 9.0], [8.0, 9.0, 8.0], [9.0, 8.0, 7.0]]
        assert got["values"][1, 2, 0] == 0.2 * bn.EV_TO_KCALMOL and got["cut_coul"] == got["cutmax"] == 10.0


def test_the_shift_constants():
    got = capi.born_dsf_read_params(NACL)
    a, rc = 0.25, 10.0
    f_s = math.erfc(a * rc) / rc ** 2 + 2.0 * a / math.sqrt(math.pi) * math.exp(-a * a * rc * rc) / rc
    assert abs(got["f_s"] - f_s) <= 1e-15 * f_s and abs(got["e_s"] - (math.erfc(a * rc) / rc + f_s * rc)) <= 1e-15 * got["e_s"]


@pytest.mark.parametrize("path,pair,qq", [(NACL, (0, 1), (1.0, -1.0)), (NACL, (1, 1), (-1.0, -1.0)), (KNACL, (0, 0), (1.0, 1.0)), (KNACL, (0, 2), (1.0, 2.0)),
                                          (KNACL, (1, 2), (-1.0, 0.0))])
def test_the_kernels_pair_function_against_numpy(path, pair, qq):
    """bd_pair on the host at distances across both cutoffs: energies and dE/dr = -f r to 1e-13 of the largest term, exact zeros beyond"""
    bd = bn.BornDsf(bn.read_born_dsf(path))
    cut = bd.p["cut_lj"][pair]
    r = np.concatenate([np.linspace(1.8, 11.0, 93), [cut - 1e-9, cut, bd.rc - 1e-9, bd.rc, bd.rc + 1e-9]])
    eb, ec, fb, fc, eself = capi.born_dsf_eval(path, pair[0], pair[1], qq[0], qq[1], r)
    reb, rdeb = bd.born(pair[0], pair[1], r)
    rec, rdec = bd.coul(qq[0] * qq[1], r)
    for got, ref in ((eb, reb), (ec, rec), (-fb * r, rdeb), (-fc * r, rdec)):
        assert np.abs(got - ref).max() <= 1e-13 * max(np.abs(ref).max(), 1e-300)
    assert not eb[r >= cut].any() and not fb[r >= cut].any() and not ec[r >= bd.rc].any() and not fc[r >= bd.rc].any()
    # (1e-9 A inside rc the Coulomb energy is (1e-9)^2 E''/2, below the rounding of its terms: it may round to 0 there)
    assert eb[r < cut].all() and fb[r < cut].all() and (qq[0] * qq[1] == 0.0 or (ec[r < bd.rc - 1e-3].all() and fc[r < bd.rc - 1e-3].all()))
    assert abs(eself[0] - bd.self_energy([qq[0]])) <= 1e-15 * abs(eself[0]) and abs(eself[1] - bd.self_energy([qq[1]])) <= 1e-15 * max(abs(eself[1]), 1e-300)


def test_both_energy_units(tmp_path):
    p = _write(tmp_path, GOOD[1:])      # no units line: the caller's energy unit decides
    metal, real = capi.born_dsf_read_params(p, 0), capi.born_dsf_read_params(p, 1)
    assert metal["K"] == bn.K_EV * bn.EV_TO_KCALMOL and real["K"] == bn.K_KCALMOL
    assert np.array_equal(metal["values"][:, :, [0, 3, 4]], real["values"][:, :, [0, 3, 4]] * bn.EV_TO_KCALMOL)
    assert np.array_equal(metal["values"][:, :, [1, 2, 5]], real["values"][:, :, [1, 2, 5]])
    assert capi.born_dsf_read_params(_write(tmp_path, ["units real"] + GOOD[1:]), 1)["K"] == bn.K_KCALMOL


def test_what_is_taken(tmp_path):
    """comments, other commands, a third cutoff word, a per-pair cutoff, `*` for either type, a later line overriding an earlier one"""
    p = _write(tmp_path, ["# a comment", "variable a equal 1 # pair_style sw", "pair_style born/coul/dsf 0.3 6.0 9.5 # style", "pair_coeff * * 1 0.3 2 3 4",
                          "pair_coeff 1 * 2 0.31 2 3 4 7.5", "pair_coeff * 3 5 0.32 2 3 4", "pair_coeff 2 2 6 0.33 2 3 4 12.0   # beyond cut_coul", "run 100"])
    got = capi.born_dsf_read_params(p, 1)
    assert got["n"] == 3 and got["alpha"] == 0.3 and got["cut_coul"] == 9.5 and got["cutmax"] == 12.0
    assert got["values"][:, :, 0].tolist() == [[2.0, 2.0, 5.0], [2.0, 6.0, 5.0], [5.0, 5.0, 5.0]]
    assert got["values"][:, :, 5].tolist() == [[7.5, 7.5, 6.0], [7.5, 12.0, 6.0], [6.0, 6.0, 6.0]]
    only_star = capi.born_dsf_read_params(_write(tmp_path, ["pair_style born/coul/dsf 0.3 6.0", "pair_coeff * * 1 0.3 2 3 4"]), 1)
    assert only_star["n"] == capi.BD_MAXEL and (only_star["values"][:, :, 0] == 1.0).all()


def _with(k, line):
    out = list(GOOD)
    out[k] = line
    return out


REFUSALS = [
    ("no pair_style line", [GOOD[0]] + GOOD[2:], r"line 0: no `pair_style born/coul/dsf"),
    ("two pair_style lines", GOOD + ["pair_style born/coul/dsf 0.25 10.0"], r"line 6: a second pair_style line"),
    ("another pair style", _with(1, "pair_style born/coul/wolf 0.25 10.0"), r"line 2: pair_style born/coul/wolf is not born/coul/dsf"),
    ("another pair style beside it", GOOD + ["pair_style sw"], r"line 6: pair_style sw is not born/coul/dsf"),
    ("a bare pair_style", _with(1, "pair_style"), r"line 2: pair_style \(none\) is not born/coul/dsf"),
    ("alpha zero", _with(1, "pair_style born/coul/dsf 0.0 10.0"), r"line 2: alpha must be positive"),
    ("alpha negative", _with(1, "pair_style born/coul/dsf -0.25 10.0"), r"line 2: alpha must be positive"),
    ("cut_lj zero", _with(1, "pair_style born/coul/dsf 0.25 0.0"), r"line 2: a cutoff must be positive"),
    ("cut_coul negative", _with(1, "pair_style born/coul/dsf 0.25 10.0 -9.0"), r"line 2: a cutoff must be positive"),
    ("a pair's cutoff zero", _with(3, GOOD[3] + " 0.0"), r"line 4: a cutoff must be positive"),
    ("rho zero", _with(2, "pair_coeff 1 1 0.2637 0.0 2.340 1.05 -0.499"), r"line 3: rho must be positive"),
    ("rho negative", _with(4, "pair_coeff 2 2 0.1582 -0.317 3.170 72.40 -145.427"), r"line 5: rho must be positive"),
    ("a word that is no number", _with(3, "pair_coeff 1 2 0.2110 0.317 2.755 6.99 abc"), r"line 4: `abc` is not a finite number"),
    ("a number with a tail", _with(3, "pair_coeff 1 2 0.2110x 0.317 2.755 6.99 -8.676"), r"line 4: `0.2110x` is not a finite number"),
    ("nan", _with(2, "pair_coeff 1 1 nan 0.317 2.340 1.05 -0.499"), r"line 3: `nan` is not a finite number"),
    ("inf", _with(1, "pair_style born/coul/dsf 0.25 inf"), r"line 2: `inf` is not a finite number"),
    ("an overflowing number", _with(2, "pair_coeff 1 1 1e999 0.317 2.340 1.05 -0.499"), r"line 3: `1e999` is not a finite number"),
    ("a LAMMPS variable", _with(1, "pair_style born/coul/dsf ${alpha} 10.0"), r"line 2: `\$\{alpha\}` is not a finite number"),
    ("a missing word", _with(3, "pair_coeff 1 2 0.2110 0.317 2.755 6.99"), r"line 4: expected `pair_coeff I J A rho sigma C D \[cut_lj\]`"),
    ("a surplus word", _with(3, GOOD[3] + " 9.0 1.0"), r"line 4: expected `pair_coeff I J A rho sigma C D \[cut_lj\]`"),
    ("a short pair_style", _with(1, "pair_style born/coul/dsf 0.25"), r"line 2: expected `pair_style born/coul/dsf <alpha> <cut_lj> \[<cut_coul>\]`"),
    ("a long pair_style", _with(1, "pair_style born/coul/dsf 0.25 10 10 10"), r"line 2: expected `pair_style born/coul/dsf"),
    ("I > J", _with(3, "pair_coeff 2 1 0.2110 0.317 2.755 6.99 -8.676"), r"line 4: pair_coeff I J needs I <= J"),
    ("a range", _with(3, "pair_coeff 1*2 2 0.2110 0.317 2.755 6.99 -8.676"), r"line 4: a type range `1\*2` is not taken"),
    ("an open range", _with(3, "pair_coeff 1 2* 0.2110 0.317 2.755 6.99 -8.676"), r"line 4: a type range `2\*` is not taken"),
    ("a type above the limit", GOOD + ["pair_coeff 1 5 0.2110 0.317 2.755 6.99 -8.676"], r"line 6: atom type 5 is above the 4 types"),
    ("type zero", _with(2, "pair_coeff 0 1 0.2637 0.317 2.340 1.05 -0.499"), r"line 3: atom types count from 1"),
    ("a type that is no number", _with(2, "pair_coeff Na 1 0.2637 0.317 2.340 1.05 -0.499"), r"line 3: `Na` is not an atom type"),
    ("a pair never set", GOOD[:3] + GOOD[4:], r"line 2: no pair_coeff line sets the pair 1 2 \(born/coul/dsf has no mixing rule\)"),
    ("a diagonal pair never set", GOOD[:4], r"line 2: no pair_coeff line sets the pair 2 2"),
    ("no pair_coeff at all", GOOD[:2], r"line 2: no pair_coeff line sets the pair 1 1"),
    ("other units", _with(0, "units lj"), r"line 1: units must be real or metal"),
    ("units against the energy unit", _with(0, "units real"), r"line 1: units real contradicts energy unit 0"),
]


@pytest.mark.parametrize("what,lines,message", REFUSALS, ids=[r[0].replace(" ", "_") for r in REFUSALS])
def test_refusals_name_their_line(tmp_path, what, lines, message):
    p = _write(tmp_path, lines)
    with pytest.raises(IOError, match=r"rc=5: .*frag\.born_dsf " + message):
        capi.born_dsf_read_params(p, 0)
    with pytest.raises(IOError, match=message):
        capi.born_dsf_eval(p, 0, 0, 1.0, 1.0, [2.0])


def test_other_refusals(tmp_path):
    with pytest.raises(IOError, match=r"nowhere\.born_dsf: cannot open"):
        capi.born_dsf_read_params(str(tmp_path / "nowhere.born_dsf"))
    with pytest.raises(IOError, match="bad arguments"):
        capi.born_dsf_read_params(NACL, 2)
    with pytest.raises(IOError, match="a type beyond the file's"):
        capi.born_dsf_eval(NACL, 0, 2, 1.0, 1.0, [2.0])
    assert capi.born_dsf_read_params(_write(tmp_path, GOOD))["n"] == 2      # (the lines every refusal above changes one of)
