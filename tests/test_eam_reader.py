"""The setfl reader of the library (host/eam_setfl.cpp through scema_md_eam_read_setfl, a pure host function: no GPU) against the numpy
restatement tests/eam_numpy.py: the header's numbers, the elements named in any order and with repeats, the seven spline coefficients of
every knot of every function, the energy unit."""
import os

import numpy as np
import pytest

import eam_numpy as en
from scema_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUAG = os.path.join(ROOT, "tests", "golden", "CuAg.eam.alloy")


def _records(s):
    """the library's two records of a knot from the numpy coefficients s0..s6"""
    val = s[:, 3:7]
    der = np.concatenate([s[:, 0:3], np.zeros((len(s), 1))], axis=1)
    return val, der


def _close(got, want, tol=1e-13):
    for g, w in zip(got, _records(want)):
        assert g.shape == w.shape and np.abs(g - w).max() <= tol * np.abs(w).max()


def test_fixture_header_and_size():
    out = capi.eam_read_setfl(CUAG, ["Cu", "Ag"])
    assert out["n"] == 2 and list(out["type_map"]) == [0, 1] and out["nrho"] == out["nr"] == 500
    assert out["cutoff"] == 5.5 and out["dr"] == 0.0112 and out["cutoff"] <= (out["nr"] - 1) * out["dr"]
    assert out["rhomax"] == (out["nrho"] - 1) * out["drho"]
    assert list(out["masses"]) == [en.CU_MASS, en.AG_MASS]
    assert os.path.getsize(CUAG) < 216 * 1024
    # with the default skin the 4-atom cell stays inside the two-image limit of the row driver: box width >= (cutoff + skin) / 2
    assert en.A_CU >= (out["cutoff"] + 1.0) / 2.0
    head = open(CUAG).read().split("\n")[:3]
    assert "Johnson" in head[0] and "not from LAMMPS" in head[2]


@pytest.mark.parametrize("elements", [["Cu"], ["Ag"], ["Cu", "Ag"], ["Ag", "Cu"], ["Ag", "Cu", "Ag", "Ag"]])
def test_spline_tables_match_numpy(elements):
    """every coefficient of every kept function, the elements out of file order and repeated"""
    out = capi.eam_read_setfl(CUAG, elements)
    tab, tmap = en.read_setfl(CUAG, elements)
    assert out["n"] == tab["n"] == len(set(elements)) and list(out["type_map"]) == tmap
    assert list(out["masses"]) == tab["masses"]
    for i in range(out["n"]):
        _close(out["F"][i], en.spline(tab["F"][i], tab["drho"]))
        _close(out["rho"][i], en.spline(tab["rho"][i], tab["dr"]))
        for j in range(i + 1):
            _close(out["z"][(i, j)], en.spline(tab["z"][i][j], tab["dr"]))
    if elements == ["Ag", "Cu"]:            # the pair table of (Ag, Cu) is the file's (Cu, Ag); the elements' own tables follow their names
        other = capi.eam_read_setfl(CUAG, ["Cu", "Ag"])
        assert np.array_equal(out["z"][(1, 0)][0], other["z"][(1, 0)][0])
        assert np.array_equal(out["F"][0][0], other["F"][1][0]) and np.array_equal(out["rho"][1][1], other["rho"][0][1])
        assert np.array_equal(out["z"][(0, 0)][0], other["z"][(1, 1)][0])


def test_energy_unit_scales_f_and_rphi_only():
    a, b = capi.eam_read_setfl(CUAG, ["Cu"], energy_unit=0), capi.eam_read_setfl(CUAG, ["Cu"], energy_unit=1)
    assert np.array_equal(a["rho"][0][0], b["rho"][0][0]) and np.array_equal(a["rho"][0][1], b["rho"][0][1])
    for key in ("F", "z"):
        x, y = (a[key][0], b[key][0]) if key == "F" else (a[key][(0, 0)], b[key][(0, 0)])
        assert np.abs(x[0] - 23.060549 * y[0]).max() <= 1e-14 * np.abs(x[0]).max()
    with pytest.raises(IOError, match="energy unit 2"):
        capi.eam_read_setfl(CUAG, ["Cu"], energy_unit=2)


def test_end_formulae_on_a_short_table(tmp_path):
    """Nr = Nrho = 5, the least the end formulae allow: knots 0, 1, 3 and 4 take the one-sided and three-point slopes, knot 2 the
    five-point one"""
    f = np.array([1.0, 3.0, 2.0, 5.0, 4.0])
    path = str(tmp_path / "five.eam.alloy")
    en.write_setfl(path, ["X"], [1], [10.0], [3.0], 5, 0.5, 5, 0.25, 1.0, [f], [f[::-1].copy()], {(0, 0): f * 0.5}, ["a", "b", "c"])
    out = capi.eam_read_setfl(path, ["X"], energy_unit=1)
    s5 = out["F"][0][0][:, 2]
    assert list(s5) == [2.0, 0.5, ((1.0 - 4.0) + 8.0 * (5.0 - 3.0)) / 12.0, 1.0, -1.0]
    _close(out["F"][0], en.spline(f, 0.5), tol=1e-15)
    assert not out["F"][0][0][4, :2].any() and not out["F"][0][1][4, :2].any()      # s3 = s4 = 0 and with them s0 = s1 at the last knot
