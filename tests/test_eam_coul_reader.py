"""The reader of `pair_style hybrid/overlay coul/long <cut_coul> eam/alloy` script lines (scema_md_eam_coul_read_params, a pure host
function, no GPU): both sub-style orders, the three forms of the setfl path, the units, and every refusal with its line number.  The
numpy restatement's own parser (tests/eam_coul_numpy.py) reads the same fixtures and must agree."""
import os
import re
import shutil

import pytest

import eam_coul_numpy as ec
from scema_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LONG, SHORT, SETFL = (os.path.join(GOLDEN, n) for n in ("UO2.eam_coul", "UO2_short.eam_coul", "UO2.eam.alloy"))
K_METAL, K_REAL = 14.399645 * 23.060549, 332.06371

GOOD = ["units metal", "pair_style hybrid/overlay coul/long 9.0 eam/alloy", "pair_coeff * * coul/long", "pair_coeff * * eam/alloy UO2.eam.alloy O U",
        "kspace_style ewald 1.0e-5"]


def _folder(tmp_path, lines, name="in.strain.lammps", with_setfl=True):
    tmp_path.mkdir(exist_ok=True)
    if with_setfl:
        shutil.copy(SETFL, tmp_path / "UO2.eam.alloy")
    p = tmp_path / name
    p.write_text("\n".join(lines) + "\n")
    return str(p)


def test_the_two_fixtures_in_either_sub_style_order():
    a, b = capi.eam_coul_read_params(LONG), capi.eam_coul_read_params(SHORT)
    assert (a["cut_coul"], a["accuracy"], a["solver"], a["cutmax"], a["cutoff"]) == (9.0, 1e-5, "ewald", 9.0, 7.0)
    assert (b["cut_coul"], b["accuracy"], b["solver"], b["cutmax"], b["cutoff"]) == (6.0, 1e-4, "pppm", 7.0, 7.0)
    assert a["type_map"] == b["type_map"] == [0, 1] and a["setfl"] == b["setfl"] == SETFL
    assert abs(a["K"] - K_METAL) < 1e-9 and abs(b["K"] - K_METAL) < 1e-9
    for path, got in ((LONG, a), (SHORT, b)):
        p = ec.read_eam_coul(path)
        assert (p["cut_coul"], p["accuracy"], p["solver"], p["setfl"], p["K"]) == (got["cut_coul"], got["accuracy"], got["solver"], got["setfl"], got["K"])


def test_the_three_forms_of_the_setfl_path(tmp_path):
    rel = _folder(tmp_path / "rel", GOOD)
    locs = _folder(tmp_path / "locs", [s.replace("UO2.eam.alloy", "${locs}/UO2.eam.alloy") for s in GOOD])
    absolute = _folder(tmp_path / "abs", [s.replace("UO2.eam.alloy", SETFL) for s in GOOD], with_setfl=False)
    assert capi.eam_coul_read_params(rel)["setfl"] == str(tmp_path / "rel" / "UO2.eam.alloy")
    assert capi.eam_coul_read_params(locs)["setfl"] == str(tmp_path / "locs" / "UO2.eam.alloy")
    assert capi.eam_coul_read_params(absolute)["setfl"] == SETFL
    # an element order of the script's own, a repeat: the type map follows the order of first appearance
    swapped = _folder(tmp_path / "swap", [s.replace("O U", "U O U") for s in GOOD])
    assert capi.eam_coul_read_params(swapped)["type_map"] == [0, 1, 0]


def test_units(tmp_path):
    real = _folder(tmp_path / "real", ["units real"] + GOOD[1:])
    silent = _folder(tmp_path / "silent", GOOD[1:])
    assert abs(capi.eam_coul_read_params(real, energy_unit=1)["K"] - K_REAL) < 1e-12
    assert abs(capi.eam_coul_read_params(real, energy_unit=-1)["K"] - K_REAL) < 1e-12
    assert abs(capi.eam_coul_read_params(silent, energy_unit=-1)["K"] - K_METAL) < 1e-9
    assert abs(capi.eam_coul_read_params(silent, energy_unit=1)["K"] - K_REAL) < 1e-12
    with pytest.raises(IOError, match=r"line 1: units real contradicts energy unit 0"):
        capi.eam_coul_read_params(real, energy_unit=0)
    with pytest.raises(IOError, match=r"line 4: units metal contradicts energy unit 1"):
        capi.eam_coul_read_params(LONG, energy_unit=1)


def _edit(k, new):
    """GOOD with line k (from 1) replaced by the lines `new`"""
    return GOOD[:k - 1] + list(new) + GOOD[k:]


REFUSALS = [
    ("third sub-style", _edit(2, ["pair_style hybrid/overlay coul/long 9.0 eam/alloy zbl 3.0 4.0"]), r"line 2: a third sub-style `zbl`"),
    ("another sub-style", _edit(2, ["pair_style hybrid/overlay lj/cut 9.0 eam/alloy"]), r"line 2: sub-style `lj/cut` is neither coul/long nor eam/alloy"),
    ("another style", _edit(2, ["pair_style eam/alloy"]), r"line 2: pair_style eam/alloy is not hybrid/overlay"),
    ("no style", _edit(2, []), r"line 0: no `pair_style hybrid/overlay"),
    ("two styles", GOOD + [GOOD[1]], r"line 6: a second pair_style line"),
    ("one sub-style", _edit(2, ["pair_style hybrid/overlay coul/long 9.0"]), r"line 2: expected `pair_style hybrid/overlay coul/long <cut_coul> eam/alloy`"),
    ("sub-style twice", _edit(2, ["pair_style hybrid/overlay eam/alloy eam/alloy coul/long 9.0"]), r"line 2: sub-style eam/alloy given twice"),
    ("no cut_coul", _edit(2, ["pair_style hybrid/overlay eam/alloy coul/long"]), r"line 2: expected `coul/long <cut_coul>`"),
    ("cut_coul no number", _edit(2, ["pair_style hybrid/overlay coul/long eam/alloy"]), r"line 2: `eam/alloy` is not a finite number"),
    ("cut_coul zero", _edit(2, ["pair_style hybrid/overlay coul/long 0.0 eam/alloy"]), r"line 2: cut_coul must be positive"),
    ("cut_coul negative", _edit(2, ["pair_style hybrid/overlay coul/long -9.0 eam/alloy"]), r"line 2: cut_coul must be positive"),
    ("coul coeff missing", _edit(3, []), r"line 0: no `pair_coeff \* \* coul/long` line"),
    ("coul coeff twice", GOOD + [GOOD[2]], r"line 6: a second `pair_coeff \* \* coul/long` line"),
    ("coul coeff with words", _edit(3, ["pair_coeff * * coul/long 9.0"]), r"line 3: `pair_coeff \* \* coul/long` takes no further word"),
    ("eam coeff missing", _edit(4, []), r"line 0: no `pair_coeff \* \* eam/alloy"),
    ("eam coeff twice", GOOD + [GOOD[3]], r"line 6: a second `pair_coeff \* \* eam/alloy` line"),
    ("eam coeff without element", _edit(4, ["pair_coeff * * eam/alloy UO2.eam.alloy"]), r"line 4: expected `pair_coeff \* \* eam/alloy <file> <element> \.\.\.`"),
    ("NULL element", _edit(4, ["pair_coeff * * eam/alloy UO2.eam.alloy O NULL"]), r"line 4: NULL as an element"),
    ("typed coeff", _edit(3, ["pair_coeff 1 2 coul/long"]), r"line 3: expected `pair_coeff \* \* coul/long`"),
    ("coeff of another sub-style", GOOD + ["pair_coeff * * zbl 3.0"], r"line 6: pair_coeff for sub-style `zbl`"),
    ("no kspace", _edit(5, []), r"line 0: no `kspace_style ewald\|pppm <accuracy>` line"),
    ("two kspace", GOOD + ["kspace_style pppm 1e-4"], r"line 6: a second kspace_style line"),
    ("kspace msm", _edit(5, ["kspace_style msm 1e-5"]), r"line 5: kspace_style msm is neither ewald nor pppm"),
    ("kspace without accuracy", _edit(5, ["kspace_style ewald"]), r"line 5: expected `kspace_style ewald <accuracy>`"),
    ("kspace_modify", GOOD + ["kspace_modify mesh 16 16 16"], r"line 6: a kspace_modify line: none of its options is honoured"),
    ("accuracy zero", _edit(5, ["kspace_style ewald 0.0"]), r"line 5: the accuracy must be above 0 and below 1"),
    ("accuracy one", _edit(5, ["kspace_style ewald 1.0"]), r"line 5: the accuracy must be above 0 and below 1"),
    ("accuracy nan", _edit(5, ["kspace_style ewald nan"]), r"line 5: `nan` is not a finite number"),
    ("units", _edit(1, ["units lj"]), r"line 1: units must be real or metal"),
]


@pytest.mark.parametrize("what,lines,match", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_name_the_line(tmp_path, what, lines, match):
    path = _folder(tmp_path / "s", lines)
    with pytest.raises(IOError, match=r"rc=5: " + re.escape(path) + " " + match):
        capi.eam_coul_read_params(path)


def test_a_comment_hides_the_rest_of_a_line_and_other_commands_are_ignored(tmp_path):
    lines = ["# pair_style born/coul/long 10.0", "timestep 1.0", "fix 1 all nvt temp 300 300 100"] + GOOD + ["run 100  # kspace_modify gewald 0.3"]
    got = capi.eam_coul_read_params(_folder(tmp_path / "s", lines))
    assert got["cut_coul"] == 9.0 and got["solver"] == "ewald"


def test_the_refusals_of_the_setfl_reader_are_passed_on(tmp_path):
    """everything scema_md_eam_read_setfl refuses, with its own message: a missing file, an element the file lacks, a truncated file, more
    than four elements, a word that is no number"""
    missing = _folder(tmp_path / "missing", GOOD, with_setfl=False)
    with pytest.raises(IOError, match=r"rc=5: .*missing/UO2\.eam\.alloy: cannot open"):
        capi.eam_coul_read_params(missing)
    lacks = _folder(tmp_path / "lacks", [s.replace("O U", "O Pu") for s in GOOD])
    with pytest.raises(IOError, match=r"UO2\.eam\.alloy: element Pu is not in the file"):
        capi.eam_coul_read_params(lacks)
    data = open(SETFL).read()
    cut = _folder(tmp_path / "cut", GOOD)
    (tmp_path / "cut" / "UO2.eam.alloy").write_text(data[:len(data) // 2])
    with pytest.raises(IOError, match=r"UO2\.eam\.alloy: truncated file"):
        capi.eam_coul_read_params(cut)
    junk = _folder(tmp_path / "junk", GOOD)
    (tmp_path / "junk" / "UO2.eam.alloy").write_text(data.replace("500 ", "5x0 ", 1))
    with pytest.raises(IOError, match=r"UO2\.eam\.alloy: '5x0' on line 5 is not a number"):
        capi.eam_coul_read_params(junk)
    for path in (missing, lacks, cut, junk):
        try:
            capi.eam_coul_read_params(path)
        except IOError as err:
            assert str(err).split(": ", 1)[1] == _setfl_message(path)


def _setfl_message(script):
    """the message of scema_md_eam_read_setfl itself on the file the script names, with the script's elements"""
    p = ec.read_eam_coul(script)
    try:
        capi.eam_read_setfl(p["setfl"], p["elements"])
    except IOError as err:
        return str(err).split(": ", 1)[1]
    return None
