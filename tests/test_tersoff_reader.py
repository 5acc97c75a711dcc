"""The reader of LAMMPS Tersoff files (scema_amd/csrc/host/tersoff_params.cpp through scema_md_tersoff_read_params: a pure host function,
no GPU): the fixture tests/golden/SiC.tersoff, comments and entries over several lines, element selection and order, which entry feeds
which slot of the kernels' tables (through tests/tersoff_host_driver.cpp), and every refusal with its message."""
import ctypes as C
import os

import numpy as np
import pytest

import tersoff_numpy as tsn
from scema_amd import capi
from test_tersoff_host import driver_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIC = os.path.join(ROOT, "tests", "golden", "SiC.tersoff")
SI = [3, 1, 0, 100390, 16.217, -0.59825, 0.78734, 1.1e-6, 1.7322, 471.18, 2.85, 0.15, 2.4799, 1830.8]
CC = [3, 1, 0, 38049, 4.3484, -0.57058, 0.72751, 1.5724e-7, 2.2119, 346.74, 1.95, 0.15, 3.4879, 1393.6]
MIX = [1.97205, 395.1451, 2.36, 0.15, 2.9839, 1597.3111]


def test_fixture_numbers():
    n, tmap, v = capi.tersoff_read_params(SIC, ["Si", "C"], energy_unit=1)
    assert n == 2 and list(tmap) == [0, 1] and v.shape == (2, 2, 2, 14)
    assert capi.TERSOFF_FIELDS == tsn.FIELDS
    assert list(v[0, 0, 0]) == SI and list(v[1, 1, 1]) == CC          # as written: every digit of the file
    assert list(v[0, 1, 1]) == SI[:8] + MIX and list(v[1, 0, 0]) == CC[:8] + MIX
    # the entries that carry three-body numbers only: those of their first element, zeros for the pair fields, R D of the third atom
    for (i, j, k), rd in {(0, 0, 1): [2.36, 0.15], (0, 1, 0): [2.85, 0.15], (1, 1, 0): [2.36, 0.15], (1, 0, 1): [1.95, 0.15]}.items():
        assert list(v[i, j, k]) == (SI if i == 0 else CC)[:6] + [0, 0, 0, 0] + rd + [0, 0]
    ref, _ = tsn.read_tersoff(SIC, ["Si", "C"], energy_unit=1)
    for (i, j, k), d in ref.items():
        assert list(v[i, j, k]) == [d[f] for f in tsn.FIELDS]


def test_energy_unit():
    _, _, ev = capi.tersoff_read_params(SIC, ["Si"], energy_unit=0)
    assert ev[0, 0, 0, 13] == SI[13] * 23.060549 and ev[0, 0, 0, 9] == SI[9] * 23.060549          # A and B: eV -> kcal/mol
    assert list(ev[0, 0, 0, :9]) == SI[:9] and list(ev[0, 0, 0, 10:13]) == SI[10:13]
    with pytest.raises(IOError, match="energy unit"):
        capi.tersoff_read_params(SIC, ["Si"], energy_unit=2)


def test_element_selection_and_order():
    _, _, v = capi.tersoff_read_params(SIC, ["Si", "C"], energy_unit=1)
    n, tmap, w = capi.tersoff_read_params(SIC, ["C", "Si", "C"], energy_unit=1)       # the order of the list decides the indices
    assert n == 2 and list(tmap) == [0, 1, 0]
    for i, j, k in np.ndindex(2, 2, 2):
        assert list(w[i, j, k]) == list(v[1 - i, 1 - j, 1 - k])
    n, tmap, s = capi.tersoff_read_params(SIC, ["C", "C"], energy_unit=1)              # entries of elements not named are skipped
    assert n == 1 and list(tmap) == [0, 0] and list(s[0, 0, 0]) == CC
    with pytest.raises(IOError, match="no entry for the triplet Si Si Ge"):
        capi.tersoff_read_params(SIC, ["Si", "Ge"])
    with pytest.raises(IOError, match="more than 4 distinct elements"):
        capi.tersoff_read_params(SIC, ["Si", "C", "A", "B", "D"])


def test_comments_and_wrapped_entries(tmp_path):
    words = tsn.SYNTH.split("\n")
    p = tmp_path / "wrapped.tersoff"
    body = []
    for l in words:
        w = l.split("#")[0].split()
        body.append("  ".join(w[:5]) + "   # a comment in the middle of an entry\n# a whole line\n\n" + " ".join(w[5:11]) + "\n\t" + " ".join(w[11:]) if w else l)
    p.write_text("\n".join(body) + "\n")
    q = tmp_path / "plain.tersoff"
    q.write_text(tsn.SYNTH)
    a, b = capi.tersoff_read_params(str(p), ["X", "Y"]), capi.tersoff_read_params(str(q), ["X", "Y"])
    assert a[0] == b[0] == 2 and np.array_equal(a[2], b[2]) and a[2][0, 0, 1, 10] == 2.6


def test_which_entry_feeds_which_table_slot(tmp_path):
    """pair [i][j]: A B lambda1 lambda2 beta n R D of entry i j j; triplet [i][j][k]: gamma lambda3 c d costheta0 m AND R D of entry i j k"""
    L = driver_lib()
    L.tsh_create.restype = C.c_void_p
    # a file in which every number of every entry is distinct: entry number e (1-based) field f holds e + f / 100 (m stays 1 or 3)
    names = [(a, b, c) for a in "PQ" for b in "PQ" for c in "PQ"]
    lines = []
    for e, nm in enumerate(names, 1):
        v = [e + f / 100.0 for f in range(14)]
        v[0] = 3 if e % 2 else 1
        v[11] = 0.5 + e / 100.0          # D <= R
        lines.append(" ".join(nm) + " " + " ".join(repr(x) for x in v))
    p = tmp_path / "distinct.tersoff"
    p.write_text("\n".join(lines) + "\n")
    arr = (C.c_char_p * 2)(b"P", b"Q")
    h = L.tsh_create(str(p).encode(), arr, 2, 1, 0)
    assert h
    val = lambda nm, f: (3.0 if (names.index(nm) + 1) % 2 else 1.0) if f == 0 else (0.5 + (names.index(nm) + 1) / 100.0 if f == 11 else names.index(nm) + 1 + f / 100.0)
    F = {n: k for k, n in enumerate(tsn.FIELDS)}
    for i, j, k in np.ndindex(2, 2, 2):
        out = np.zeros(16)
        L.tsh_slot(h, i, j, k, out.ctypes.data_as(C.c_void_p))
        ijj, ijk = ("PQ"[i], "PQ"[j], "PQ"[j]), ("PQ"[i], "PQ"[j], "PQ"[k])
        assert list(out[:8]) == [val(ijj, F[f]) for f in ("A", "B", "lambda1", "lambda2", "beta", "n", "R", "D")]
        want = [val(ijk, F["gamma"]), val(ijk, F["lambda3"]), val(ijk, F["c"]) ** 2, val(ijk, F["d"]) ** 2, val(ijk, F["costheta0"]), val(ijk, F["R"]),
                val(ijk, F["D"]), val(ijk, F["m"])]
        assert list(out[8:]) == want, (i, j, k)
    L.tsh_destroy(C.c_void_p(h))


ENTRY = "Si Si Si 3 1 0 100390 16.217 -0.59825 0.78734 1.1e-6 1.7322 471.18 2.85 0.15 2.4799 1830.8\n"


def _refused(tmp_path, text, match, elements=("Si",)):
    p = tmp_path / "bad.tersoff"
    p.write_text(text)
    with pytest.raises(IOError, match=match):
        capi.tersoff_read_params(str(p), list(elements))


@pytest.mark.parametrize("field", ["c", "d", "n", "beta", "lambda2", "B", "R", "D", "lambda1", "A", "gamma"])
def test_negative_value_is_refused(tmp_path, field):
    w = ENTRY.split()
    w[3 + tsn.FIELDS.index(field)] = "-" + w[3 + tsn.FIELDS.index(field)]
    _refused(tmp_path, " ".join(w) + "\n", "must not be negative")


def test_other_refusals(tmp_path):
    w = ENTRY.split()
    _refused(tmp_path, " ".join(w[:13] + ["2.85", "2.86"] + w[15:]) + "\n", "D must not exceed R")
    for m in ("2", "0", "1.5", "-3"):
        _refused(tmp_path, " ".join(w[:3] + [m] + w[4:]) + "\n", "m must be 1 or 3")
    for m in ("1", "3", "1.0", "3e0"):
        q = tmp_path / "m.tersoff"
        q.write_text(" ".join(w[:3] + [m] + w[4:]) + "\n")
        assert capi.tersoff_read_params(str(q), ["Si"])[0] == 1
    _refused(tmp_path, ENTRY + ENTRY, "duplicate entry Si Si Si")
    _refused(tmp_path, " ".join(w[:16]) + "\n", "short entry: 16 of 17 words")
    _refused(tmp_path, " ".join(w[:9] + ["n.a."] + w[10:]) + "\n", "'n.a.' on line 1 is not a number")
    _refused(tmp_path, " ".join(w[:9] + ["0"] + w[10:]) + "\n", "n of a pair entry")
    _refused(tmp_path, "# nothing but a comment\n", "no entry for the triplet Si Si Si")
    lines = open(SIC).read().splitlines()
    entries = [n for n, l in enumerate(lines) if l and not l.startswith("#")]
    assert len(entries) == 8
    for drop in entries:                      # each of the eight triplets is needed once both elements are named
        _refused(tmp_path, "\n".join(l for n, l in enumerate(lines) if n != drop) + "\n", "no entry for the triplet", elements=("Si", "C"))
    # a negative lambda3 or costheta0 is no refusal (LAMMPS has none)
    q = tmp_path / "neg.tersoff"
    q.write_text(" ".join(w[:5] + ["-1.3"] + w[6:]) + "\n")
    assert capi.tersoff_read_params(str(q), ["Si"], energy_unit=1)[2][0, 0, 0, 2] == -1.3
