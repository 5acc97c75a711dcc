"""The reader of LAMMPS Vashishta files (scema_amd/csrc/host/vashishta_params.cpp through scema_md_vashishta_read_params: a pure host
function, no GPU): the fixture tests/golden/SiC.vashishta value by value, both energy units, comments and entries over several lines,
element selection, and every refusal with its message."""
import os

import numpy as np
import pytest

import vashishta_numpy as vn
from scema_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIC = os.path.join(ROOT, "tests", "golden", "SiC.vashishta")
EV = 23.060549
#        H          eta  Zi      Zj      l1   D        l4   W        rc
SISI = [23.67291,  7.0, 1.201,  1.201,  5.0, 15.575,  3.0, 0.0,     7.35]
CC = [471.74538,   7.0, -1.201, -1.201, 5.0, 0.0,     3.0, 0.0,     7.35]
SIC_ = [447.09026, 9.0, 1.201,  -1.201, 5.0, 7.7874,  3.0, 61.4694, 7.35]
CSI = SIC_[:2] + [-1.201, 1.201] + SIC_[4:]
THREE = [9.003, 1.0, 2.90, 5.0, -0.333333333333]


def test_fixture_numbers():
    n, tmap, v = capi.vashishta_read_params(SIC, ["Si", "C"], energy_unit=1)
    assert n == 2 and list(tmap) == [0, 1] and v.shape == (2, 2, 2, 14)
    assert capi.VASHISHTA_FIELDS == vn.FIELDS
    assert list(v[0, 0, 0]) == SISI + [0.0] * 5 and list(v[1, 1, 1]) == CC + [0.0] * 5          # as written: every digit of the file
    assert list(v[0, 1, 1]) == SIC_ + THREE and list(v[1, 0, 0]) == CSI + THREE
    for ijk in ((0, 0, 1), (0, 1, 0), (1, 0, 1), (1, 1, 0)):
        assert not v[ijk].any()
    ref, rmap, K = vn.read_vashishta(SIC, ["Si", "C"], energy_unit=1)
    assert rmap == [0, 1] and K == 332.06371
    for (i, j, k), d in ref.items():
        assert list(v[i, j, k]) == [d[f] for f in vn.FIELDS]


def test_fixture_is_what_its_generator_writes():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_vashishta_fixture", os.path.join(ROOT, "tests", "golden", "make_vashishta_fixture.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert open(SIC).read() == "\n".join(mod.lines()) + "\n"


def test_energy_unit():
    _, _, ev = capi.vashishta_read_params(SIC, ["Si", "C"], energy_unit=0)
    _, _, kc = capi.vashishta_read_params(SIC, ["Si", "C"], energy_unit=1)
    scaled = [0, 5, 7, 9]                                         # H, D, W, B: eV -> kcal/mol
    for ijk in np.ndindex(2, 2, 2):
        for f in range(14):
            assert ev[ijk][f] == (kc[ijk][f] * EV if f in scaled else kc[ijk][f])
    ref, _, K = vn.read_vashishta(SIC, ["Si", "C"], energy_unit=0)
    assert K == 14.399645 * EV and ev[0, 1, 1, 0] == ref[(0, 1, 1)]["H"] and ev[0, 1, 1, 9] == ref[(0, 1, 1)]["B"]
    with pytest.raises(IOError, match="energy unit"):
        capi.vashishta_read_params(SIC, ["Si"], energy_unit=2)


def test_element_selection_and_order():
    _, _, v = capi.vashishta_read_params(SIC, ["Si", "C"], energy_unit=1)
    n, tmap, w = capi.vashishta_read_params(SIC, ["C", "Si", "C"], energy_unit=1)       # the order of the list decides the indices
    assert n == 2 and list(tmap) == [0, 1, 0]
    for i, j, k in np.ndindex(2, 2, 2):
        assert list(w[i, j, k]) == list(v[1 - i, 1 - j, 1 - k])
    n, tmap, s = capi.vashishta_read_params(SIC, ["C", "C"], energy_unit=1)              # entries of elements not named are skipped
    assert n == 1 and list(tmap) == [0, 0] and list(s[0, 0, 0]) == CC + [0.0] * 5
    with pytest.raises(IOError, match="no entry for the triplet Si Si Ge"):
        capi.vashishta_read_params(SIC, ["Si", "Ge"])
    with pytest.raises(IOError, match="more than 4 distinct elements"):
        capi.vashishta_read_params(SIC, ["Si", "C", "A", "B", "D"])


def test_comments_and_wrapped_entries(tmp_path):
    body = []
    for l in vn.SYNTH.split("\n"):
        w = l.split("#")[0].split()
        body.append("  ".join(w[:5]) + "   # a comment in the middle of an entry\n# a whole line\n\n" + " ".join(w[5:11]) + "\n\t" + " ".join(w[11:]) if w else l)
    p = tmp_path / "wrapped.vashishta"
    p.write_text("\n".join(body) + "\n")
    q = tmp_path / "plain.vashishta"
    q.write_text(vn.SYNTH + "Ge Ge Ge 1 2 3 4 5 6 7 8 9 10 11 12 13 14\nX Ge Ge 1 2 3 4 5 6 7 8 -9 10 11 12 13 14\n")      # (entries of unnamed elements, skipped unjudged)
    a, b = capi.vashishta_read_params(str(p), ["X", "Y"]), capi.vashishta_read_params(str(q), ["X", "Y"])
    assert a[0] == b[0] == 2 and np.array_equal(a[2], b[2]) and a[2][0, 0, 0, 1] == 7.5 and a[2][1, 1, 1, 4] == 0.0


def _with(tmp_path, name, edit):
    """the synthetic file with one entry's numbers changed: edit = {(El1, El2, El3): {field: value}}"""
    lines = []
    for l in vn.SYNTH.split("\n"):
        w = l.split("#")[0].split()
        if w and tuple(w[:3]) in edit:
            for f, val in edit[tuple(w[:3])].items():
                w[3 + vn.FIELDS.index(f)] = repr(val)
            l = " ".join(w)
        lines.append(l)
    p = tmp_path / name
    p.write_text("\n".join(lines))
    return str(p)


REFUSALS = [
    ("rc0", {("X", "X", "X"): {"rc": 0.0, "r0": 0.0}}, "rc of a pair entry .i j j. must be positive"),
    ("rcneg", {("Y", "Y", "Y"): {"rc": -1.0, "r0": 0.0}}, "rc of a pair entry .i j j. must be positive"),
    ("eta0", {("X", "X", "X"): {"eta": 0.0}}, "eta of a pair entry .i j j. with H != 0 must be positive"),
    ("etaneg", {("X", "X", "X"): {"eta": -7.0}}, "eta of a pair entry .i j j. with H != 0 must be positive"),
    ("l1", {("X", "X", "X"): {"lambda1": -1.0}}, "lambda1, lambda4, gamma and r0 must not be negative"),
    ("l4", {("X", "X", "X"): {"lambda4": -1.0}}, "lambda1, lambda4, gamma and r0 must not be negative"),
    ("gamma", {("Y", "Y", "Y"): {"gamma": -0.1}}, "lambda1, lambda4, gamma and r0 must not be negative"),
    ("r0neg", {("Y", "Y", "Y"): {"r0": -0.1}}, "lambda1, lambda4, gamma and r0 must not be negative"),
    ("cneg", {("X", "X", "X"): {"C": -1.0}}, "C must not be negative"),
    ("cneg3", {("X", "Y", "X"): {"C": -1.0}}, "C must not be negative"),
    ("r0rc", {("X", "X", "X"): {"r0": 6.5}}, "r0 of a pair entry .i j j. must not exceed its rc"),
    ("rcdiff", {("X", "Y", "Y"): {"rc": 6.6}}, "entries X Y Y and Y X X differ in rc or r0"),
    ("r0diff", {("Y", "X", "X"): {"r0": 2.8}}, "entries X Y Y and Y X X differ in rc or r0"),
]


@pytest.mark.parametrize("name,edit,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_of_the_numbers(tmp_path, name, edit, message):
    with pytest.raises(IOError, match=message):
        capi.vashishta_read_params(_with(tmp_path, name + ".vashishta", edit), ["X", "Y"])


def test_what_is_not_refused(tmp_path):
    """eta = 0 with H = 0 (a pair without repulsion), a pair entry i j k (j != k) with any numbers in its pair fields, r0 = rc"""
    ok = _with(tmp_path, "ok.vashishta", {("Y", "Y", "Y"): {"H": 0.0, "eta": 0.0}, ("X", "X", "Y"): {"rc": -3.0, "eta": -1.0, "H": 4.0, "r0": 9.0},
                                          ("X", "X", "X"): {"r0": 6.0}})
    n, _, v = capi.vashishta_read_params(ok, ["X", "Y"])
    assert n == 2 and v[1, 1, 1, 0] == 0.0 and v[0, 0, 1, 8] == -3.0 and v[0, 0, 0, 11] == v[0, 0, 0, 8] == 6.0


def test_refusals_of_the_triplet_reader(tmp_path):
    """what host/triplet_file.h refuses, through this reader: a short entry, a non-numeric field, a number where a name belongs, a
    duplicate, a missing triplet, an unreadable file, no element"""
    words = vn.SYNTH.split()
    cases = {"short": (vn.SYNTH.rstrip()[:-6], "short entry"), "nan": (vn.SYNTH.replace("7.5", "7.5x"), "'7.5x' on line 2 is not a number"),
             "name": (vn.SYNTH.replace("Y Y Y", "Y 3 Y"), "'3' on line 3 where an element name is expected"),
             "dup": (vn.SYNTH + vn.SYNTH.split("\n")[1] + "\n", "duplicate entry X X X"),
             "missing": ("\n".join(vn.SYNTH.split("\n")[:-2]) + "\n", "no entry for the triplet Y X Y")}
    assert len(words) > 8 * 17
    for name, (text, message) in cases.items():
        p = tmp_path / (name + ".vashishta")
        p.write_text(text)
        with pytest.raises(IOError, match=message):
            capi.vashishta_read_params(str(p), ["X", "Y"])
    with pytest.raises(IOError, match="cannot open"):
        capi.vashishta_read_params(str(tmp_path / "none.vashishta"), ["X", "Y"])
    with pytest.raises(IOError, match="empty element name"):
        capi.vashishta_read_params(SIC, ["Si", ""])


def test_reader_under_host_sanitizers(tmp_path):
    """the reader and the arithmetic as a stand-alone program (tests/vashishta_host_driver.cpp) built with AddressSanitizer and UBSan: the
    fixture, and copies of it cut at every 97th byte -- each run ends with the program's own status (0, or 1 with the reader's message)
    and without a sanitizer report"""
    import subprocess
    exe = str(tmp_path / "vashishta_driver_san")
    srcs = [os.path.join(ROOT, "tests", "vashishta_host_driver.cpp"), os.path.join(ROOT, "scema_amd", "csrc", "host", "vashishta_params.cpp")]
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-std=c++17",
                           "-I", os.path.join(ROOT, "include"), "-o", exe] + srcs)
    dimer = "2\n0 0 0 30 30 30 0 0 0\n0 0 10 10\n1 2 10 10\n"
    text = open(SIC).read()
    seen = set()
    for cut in [len(text)] + list(range(0, len(text), 97)):
        p = tmp_path / "cut.vashishta"
        p.write_text(text[:cut])
        r = subprocess.run([exe, str(p), "0", "Si", "C"], input=dimer, capture_output=True, text=True)
        assert r.returncode in (0, 1) and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (cut, r.returncode, r.stderr[-400:])
        seen.add(r.returncode)
        if r.returncode == 1:
            assert str(p) in r.stderr
    assert seen == {0, 1}
