"""The reader of LAMMPS EDIP files (scema_amd/csrc/host/edip_params.cpp through scema_md_edip_read_params: a pure host function, no GPU):
the fixtures tests/golden/Si.edip and tests/golden/SiC.edip value by value, both energy units, comments and entries over several lines,
element selection, and every refusal with its message."""
import importlib.util
import os
import subprocess

import numpy as np
import pytest

import edip_numpy as en
from scema_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SI = os.path.join(ROOT, "tests", "golden", "Si.edip")
SIC = os.path.join(ROOT, "tests", "golden", "SiC.edip")
EV = 23.060549
#          A          B          cutoffA    cutoffC    alpha      beta       eta        gamma      lambda     mu         rho        sigma      Q0           u1         u2      u3        u4
SI_ROW = [7.9821730, 1.5075463, 3.1213820, 2.5609104, 3.1083847, 0.0070975, 0.2523244, 1.1247945, 1.4533108, 0.6966326, 1.2085196, 0.5774108, 312.1341346, -0.165799, 32.557, 0.286198, 0.66]
SCALED = [0, 8]      # A, lambda: eV -> kcal/mol


def _generator():
    spec = importlib.util.spec_from_file_location("make_edip_fixture", os.path.join(ROOT, "tests", "golden", "make_edip_fixture.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_silicon_fixture_numbers():
    """the published constants, every digit, in both units"""
    assert capi.EDIP_FIELDS == en.FIELDS
    n, tmap, v = capi.edip_read_params(SI, ["Si"], energy_unit=1)
    assert n == 1 and list(tmap) == [0] and v.shape == (1, 1, 1, 17)
    assert list(v[0, 0, 0]) == SI_ROW
    _, _, ev = capi.edip_read_params(SI, ["Si", "Si"], energy_unit=0)
    assert list(ev[0, 0, 0]) == [x * EV if k in SCALED else x for k, x in enumerate(SI_ROW)]
    ref, rmap = en.read_edip(SI, ["Si"], energy_unit=0)
    assert rmap == [0] and list(ev[0, 0, 0]) == [ref[(0, 0, 0)][f] for f in en.FIELDS]


def test_synthetic_fixture_numbers():
    """every entry of the two-element file against the generator's own tables, in both units; its two symmetry rules; its comment"""
    gen = _generator()
    names = ["Si", "C"]
    for unit in (1, 0):
        n, tmap, v = capi.edip_read_params(SIC, names, energy_unit=unit)
        assert n == 2 and list(tmap) == [0, 1] and v.shape == (2, 2, 2, 17)
        ref, _ = en.read_edip(SIC, names, energy_unit=unit)
        for i, j, k in np.ndindex(2, 2, 2):
            want = dict.fromkeys(gen.ORDER, 0.0)
            if j == k:
                want.update(gen.PAIR[(names[i], names[j])])
            want.update(gen.TRIP[(names[i], "".join(sorted((names[j], names[k]))))])
            row = [want[f] * (EV if unit == 0 and q in SCALED else 1.0) for q, f in enumerate(gen.ORDER)]
            assert list(v[i, j, k]) == row == [ref[(i, j, k)][f] for f in en.FIELDS], (i, j, k)
    _, _, v = capi.edip_read_params(SIC, names, energy_unit=1)
    trip = [en.FIELDS.index(f) for f in ("eta", "lambda", "mu", "Q0", "u1", "u2", "u3", "u4")]
    for i in range(2):
        assert list(v[i, 0, 1][trip]) == list(v[i, 1, 0][trip])
    assert v[0, 1, 1, 2] == v[1, 0, 0, 2]
    # numbers of their own: no two pairs and no two unordered triplets agree in any number that is read
    pair = [en.FIELDS.index(f) for f in ("A", "B", "cutoffC", "alpha", "beta", "gamma", "rho", "sigma")]
    rows = [v[0, 0, 0], v[0, 1, 1], v[1, 0, 0], v[1, 1, 1]]
    for a in range(4):
        for b in range(a + 1, 4):
            assert (rows[a][pair] != rows[b][pair]).all()
    trips = [v[0, 0, 0], v[0, 0, 1], v[0, 1, 1], v[1, 0, 0], v[1, 0, 1], v[1, 1, 1]]
    for a in range(6):
        for b in range(a + 1, 6):
            assert (trips[a][trip] != trips[b][trip]).all()
    head = open(SIC).read().split("\n")[0]
    assert "SYNTHETIC" in head and "neither from the reference nor from LAMMPS" in head


def test_fixtures_are_what_their_generator_writes():
    gen = _generator()
    assert open(SI).read() == "\n".join(gen.si_lines()) + "\n"
    assert open(SIC).read() == "\n".join(gen.sic_lines()) + "\n"


def test_energy_unit_refused():
    with pytest.raises(IOError, match="energy unit"):
        capi.edip_read_params(SI, ["Si"], energy_unit=2)


def test_element_selection_and_order():
    _, _, v = capi.edip_read_params(SIC, ["Si", "C"], energy_unit=1)
    n, tmap, w = capi.edip_read_params(SIC, ["C", "Si", "C"], energy_unit=1)       # the order of the list decides the indices
    assert n == 2 and list(tmap) == [0, 1, 0]
    for i, j, k in np.ndindex(2, 2, 2):
        assert list(w[i, j, k]) == list(v[1 - i, 1 - j, 1 - k])
    n, tmap, s = capi.edip_read_params(SIC, ["C", "C"], energy_unit=1)              # entries of elements not named are skipped
    assert n == 1 and list(tmap) == [0, 0] and list(s[0, 0, 0]) == list(v[1, 1, 1])
    with pytest.raises(IOError, match="no entry for the triplet Si Si Ge"):
        capi.edip_read_params(SIC, ["Si", "Ge"])
    with pytest.raises(IOError, match="more than 4 distinct elements"):
        capi.edip_read_params(SIC, ["Si", "C", "A", "B", "D"])


def _body():
    return [l for l in open(SIC).read().split("\n") if l and not l.startswith("#")]


def test_comments_and_wrapped_entries(tmp_path):
    body = []
    for l in _body():
        w = l.split()
        body.append("  ".join(w[:5]) + "   # a comment in the middle of an entry\n# a whole line\n\n" + " ".join(w[5:11]) + "\n\t" + " ".join(w[11:]))
    p = tmp_path / "wrapped.edip"
    p.write_text("\n".join(body) + "\n")
    q = tmp_path / "plain.edip"
    q.write_text("\n".join(_body()) + "\nGe Ge Ge " + " ".join(str(k) for k in range(1, 18)) + "\nSi Ge Ge " + " ".join(str(-k) for k in range(1, 18)) + "\n")      # (entries of unnamed elements, skipped unjudged)
    a, b, c = capi.edip_read_params(str(p), ["Si", "C"]), capi.edip_read_params(str(q), ["Si", "C"]), capi.edip_read_params(SIC, ["Si", "C"])
    assert a[0] == b[0] == 2 and np.array_equal(a[2], b[2]) and np.array_equal(a[2], c[2])


def _with(tmp_path, name, edit):
    """the synthetic file with some entries' numbers changed: edit = {(El1, El2, El3): {field: value}}"""
    lines = []
    for l in _body():
        w = l.split()
        if tuple(w[:3]) in edit:
            for f, val in edit[tuple(w[:3])].items():
                w[3 + en.FIELDS.index(f)] = repr(val)
            l = " ".join(w)
        lines.append(l)
    p = tmp_path / name
    p.write_text("\n".join(lines) + "\n")
    return str(p)


REFUSALS = [
    ("a0", {("Si", "Si", "Si"): {"cutoffA": 0.0}}, "cutoffA of a pair entry .i j j. must be positive"),
    ("aneg", {("C", "C", "C"): {"cutoffA": -1.0}}, "cutoffA of a pair entry .i j j. must be positive"),
    ("cneg", {("Si", "Si", "Si"): {"cutoffC": -0.1}}, "cutoffC of a pair entry .i j j. must not be negative"),
    ("c_eq_a", {("Si", "Si", "Si"): {"cutoffC": 3.12}}, "cutoffC of a pair entry .i j j. must lie below its cutoffA"),
    ("c_gt_a", {("C", "C", "C"): {"cutoffC": 3.5}}, "cutoffC of a pair entry .i j j. must lie below its cutoffA"),
    ("alpha", {("Si", "Si", "Si"): {"alpha": -1.0}}, "alpha of a pair entry .i j j. must not be negative"),
    ("sigma", {("Si", "C", "C"): {"sigma": -0.5}}, "sigma of a pair entry .i j j. must not be negative"),
    ("gamma", {("C", "Si", "Si"): {"gamma": -0.1}}, "gamma of a pair entry .i j j. must not be negative"),
    ("rho", {("C", "C", "C"): {"rho": -1.2}}, "rho of a pair entry .i j j. must not be negative"),
    ("b0", {("Si", "Si", "Si"): {"B": 0.0}}, "B of a pair entry .i j j. with A != 0 must be positive"),
    ("bneg", {("Si", "Si", "Si"): {"B": -1.5}}, "B of a pair entry .i j j. with A != 0 must be positive"),
    ("adiff", {("Si", "C", "C"): {"cutoffA": 3.06}}, "entries Si C C and C Si Si differ in cutoffA"),
    ("tripdiff", {("Si", "Si", "C"): {"u3": 0.281}}, "entries Si Si C and Si C Si differ in eta, lambda, mu, Q0 or u1..u4"),
    ("tripdiff2", {("C", "C", "Si"): {"lambda": 1.76}}, "entries C Si C and C C Si differ in eta, lambda, mu, Q0 or u1..u4"),
]


@pytest.mark.parametrize("name,edit,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_of_the_numbers(tmp_path, name, edit, message):
    with pytest.raises(IOError, match=message):
        capi.edip_read_params(_with(tmp_path, name + ".edip", edit), ["Si", "C"])


def test_what_is_not_refused(tmp_path):
    """B = 0 with A = 0 (a pair without a pair term), an entry i j k (j != k) with any numbers in its pair fields, c = 0, cutoffC that
    differs between i j j and j i i (only a must agree)"""
    ok = _with(tmp_path, "ok.edip", {("C", "C", "C"): {"A": 0.0, "B": 0.0, "cutoffC": 0.0}, ("Si", "Si", "C"): {"cutoffA": -3.0, "alpha": -1.0, "B": -4.0},
                                     ("Si", "C", "Si"): {"rho": -2.0}})
    n, _, v = capi.edip_read_params(ok, ["Si", "C"])
    assert n == 2 and v[1, 1, 1, 0] == 0.0 and v[0, 0, 1, 2] == -3.0 and v[0, 1, 1, 3] != v[1, 0, 0, 3]


def test_refusals_of_the_triplet_reader(tmp_path):
    """what host/triplet_file.h refuses, through this reader: a short entry, a non-numeric field, a number where a name belongs, a
    duplicate, a missing triplet, an unreadable file, no element"""
    text = "\n".join(_body()) + "\n"
    cases = {"short": (text.rstrip()[:-4], "short entry"), "nan": (text.replace("0.0071", "0.0071x"), "'0.0071x' on line 1 is not a number"),
             "name": (text.replace("Si C  C ", "Si 3  C "), "'3' on line 4 where an element name is expected"),
             "dup": (text + _body()[0] + "\n", "duplicate entry Si Si Si"),
             "missing": ("\n".join(_body()[:-2]) + "\n", "no entry for the triplet C C Si")}
    for name, (body, message) in cases.items():
        p = tmp_path / (name + ".edip")
        p.write_text(body)
        with pytest.raises(IOError, match=message):
            capi.edip_read_params(str(p), ["Si", "C"])
    with pytest.raises(IOError, match="cannot open"):
        capi.edip_read_params(str(tmp_path / "none.edip"), ["Si", "C"])
    with pytest.raises(IOError, match="empty element name"):
        capi.edip_read_params(SIC, ["Si", ""])


def test_reader_under_host_sanitizers(tmp_path):
    """the reader and the arithmetic as a stand-alone program (tests/edip_host_driver.cpp) built with AddressSanitizer and UBSan: the
    synthetic fixture, and copies of it cut at every 61st byte -- each run ends with the program's own status (0, or 1 with the reader's
    message) and without a sanitizer report"""
    exe = str(tmp_path / "edip_driver_san")
    srcs = [os.path.join(ROOT, "tests", "edip_host_driver.cpp"), os.path.join(ROOT, "scema_amd", "csrc", "host", "edip_params.cpp")]
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-std=c++17",
                           "-I", os.path.join(ROOT, "include"), "-o", exe] + srcs)
    trimer = "3\n0 0 0 30 30 30 0 0 0\n0 10 10 10\n1 12.4 10 10\n1 9.5 12.7 10\n"
    text = open(SIC).read()
    seen = set()
    for cut in [len(text)] + list(range(0, len(text), 61)):
        p = tmp_path / "cut.edip"
        p.write_text(text[:cut])
        r = subprocess.run([exe, str(p), "0", "Si", "C"], input=trimer, capture_output=True, text=True)
        assert r.returncode in (0, 1) and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (cut, r.returncode, r.stderr[-400:])
        seen.add(r.returncode)
        if r.returncode == 1:
            assert str(p) in r.stderr
    assert seen == {0, 1}
