"""The reader of LAMMPS Stillinger-Weber files (scema_amd/csrc/host/sw_params.cpp through scema_md_sw_read_params: a pure host function, no
GPU): the reference's Si.sw, the [i][j][k] mapping of a two-element file, entries over several lines, comments, and files that must be
refused with a message instead of crashing."""
import os

import numpy as np
import pytest

import sw_numpy as swn
from scema_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SI_SW = os.path.join(ROOT, "tests", "golden", "Si.sw")
SI = [2.1683, 2.0951, 1.80, 21.0, 1.20, -0.333333333333, 7.049556277, 0.6022245584, 4.0, 0.0, 0.0]


def test_si_sw_eleven_numbers():
    n, tmap, v = capi.sw_read_params(SI_SW, ["Si"], energy_unit=1)
    assert n == 1 and list(tmap) == [0] and v.shape == (1, 1, 1, 11)
    assert list(v[0, 0, 0]) == SI                      # as written: every digit of the file
    assert capi.SW_FIELDS == swn.FIELDS


def test_energy_unit():
    _, _, ev = capi.sw_read_params(SI_SW, ["Si"], energy_unit=0)
    assert ev[0, 0, 0, 0] == SI[0] * 23.060549          # eV -> kcal/mol
    assert list(ev[0, 0, 0, 1:]) == SI[1:]
    with pytest.raises(IOError, match="energy unit"):
        capi.sw_read_params(SI_SW, ["Si"], energy_unit=2)


def test_every_type_may_name_the_same_element():
    n, tmap, v = capi.sw_read_params(SI_SW, ["Si", "Si", "Si"], energy_unit=1)      # pair_coeff * * Si.sw Si Si Si
    assert n == 1 and list(tmap) == [0, 0, 0] and v.shape == (1, 1, 1, 11)


def test_two_element_mapping(tmp_path):
    p = tmp_path / "two.sw"
    p.write_text(swn.TWO_ELEMENT_SW)
    ref, _ = swn.read_sw(str(p), ["Si", "X"], energy_unit=1)
    n, tmap, v = capi.sw_read_params(str(p), ["Si", "X"], energy_unit=1)
    assert n == 2 and list(tmap) == [0, 1]
    for (i, j, k), d in ref.items():
        assert list(v[i, j, k]) == [d[f] for f in swn.FIELDS], (i, j, k)
    assert len(ref) == 8
    # the order of the element list decides the indices: X first
    n, tmap, w = capi.sw_read_params(str(p), ["X", "Si", "X"], energy_unit=1)
    assert n == 2 and list(tmap) == [0, 1, 0]
    for i, j, k in np.ndindex(2, 2, 2):
        assert list(w[i, j, k]) == list(v[1 - i, 1 - j, 1 - k])
    # the entries of elements that are not named are skipped: Si alone reads the Si Si Si entry
    n, _, s = capi.sw_read_params(str(p), ["Si"], energy_unit=1)
    assert n == 1 and list(s[0, 0, 0]) == SI


def test_missing_triplet_is_refused(tmp_path):
    lines = swn.TWO_ELEMENT_SW.splitlines()
    for drop in range(1, 9):
        p = tmp_path / f"drop{drop}.sw"
        p.write_text("\n".join(l for n, l in enumerate(lines) if n != drop) + "\n")
        with pytest.raises(IOError, match="no entry for the triplet"):
            capi.sw_read_params(str(p), ["Si", "X"])
        missing = lines[drop].split()[:3]
        if missing != ["Si", "Si", "Si"]:
            assert capi.sw_read_params(str(p), ["Si"], energy_unit=1)[0] == 1      # ... but not needed for Si alone


def test_multi_line_entries_and_comments(tmp_path):
    p = tmp_path / "ml.sw"
    p.write_text("# header\n\n   # indented comment\nSi Si   # names end here\n Si 2.1683\n\n 2.0951  1.80  21.0 # mid-entry comment 9 9 9\n"
                 "1.20  -0.333333333333\n\t7.049556277  0.6022245584  4.0  0.0 0.0 # tail\n# Si Si Si 1 1 1 1 1 1 1 1 1 1 1\n")
    _, _, v = capi.sw_read_params(str(p), ["Si"], energy_unit=1)
    assert list(v[0, 0, 0]) == SI


def test_duplicate_entry_is_refused(tmp_path):
    p = tmp_path / "dup.sw"
    p.write_text(open(SI_SW).read() + "Si Si Si 1 2 1.8 21 1.2 -0.3 7 0.6 4 0 0\n")
    with pytest.raises(IOError, match="duplicate"):
        capi.sw_read_params(str(p), ["Si"])


def test_too_many_elements():
    with pytest.raises(IOError, match="distinct elements"):
        capi.sw_read_params(SI_SW, ["A", "B", "C", "D", "E"])
