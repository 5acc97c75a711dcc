"""The readers of the Tersoff forms' parameter files (scema_amd/csrc/host/tersoff_params.cpp through scema_md_tersoff_mod_read_params and
scema_md_tersoff_zbl_read_params: pure host functions, no GPU) against the numpy readers of tests/tersoff_forms_numpy.py field by field:
both file shapes of the mod form (17 columns: tersoff/mod, c0 = 0 filled in; 18: tersoff/mod/c), entries spread over several lines,
comments, the energy unit, and every refusal with its message."""
import os

import numpy as np
import pytest

import tersoff_forms_numpy as tf
from scema_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MOD, MODC, ZBL = (os.path.join(GOLD, n) for n in ("Si.tersoff.mod", "Si.tersoff.modc", "SiC.tersoff.zbl"))
KUMAGAI = [1.0, 2.3890327, -0.365, 1.0, 1.0, 1.345797, 121.00047, 3.0, 0.3, 3.2300135, 3281.5905, 0.93810551, 0.20173476, 730418.72, 1000000.0, 1.0, 26.0]


def test_field_names():
    assert capi.TERSOFF_MOD_FIELDS == tf.MOD_FIELDS and capi.TERSOFF_ZBL_FIELDS == tf.ZBL_FIELDS and len(tf.MOD_FIELDS) == len(tf.ZBL_FIELDS) == 18


def test_both_shapes_of_the_mod_file():
    n, tmap, v = capi.tersoff_mod_read_params(MOD, ["Si"], energy_unit=1)
    assert n == 1 and list(tmap) == [0] and v.shape == (1, 1, 1, 18) and list(v[0, 0, 0]) == KUMAGAI + [0.0]          # 17 columns: c0 = 0
    n, tmap, c = capi.tersoff_mod_read_params(MODC, ["Si", "Si"], energy_unit=1)
    assert n == 1 and list(tmap) == [0, 0] and list(c[0, 0, 0]) == KUMAGAI + [-0.0251]
    for path, ncol in ((MOD, 17), (MODC, 18)):
        for unit in (0, 1):
            ref, rmap, rcol = tf.read_mod(path, ["Si"], energy_unit=unit)
            got = capi.tersoff_mod_read_params(path, ["Si"], energy_unit=unit)[2]
            assert rcol == ncol and list(got[0, 0, 0]) == [ref[(0, 0, 0)][f] for f in tf.MOD_FIELDS]
    ev = capi.tersoff_mod_read_params(MODC, ["Si"], energy_unit=0)[2][0, 0, 0]
    F = tf.MOD_FIELDS.index
    assert ev[F("A")] == 3281.5905 * 23.060549 and ev[F("B")] == 121.00047 * 23.060549 and ev[F("c0")] == -0.0251 * 23.060549          # A, B and c0
    assert [x for k, x in enumerate(ev) if k not in (F("A"), F("B"), F("c0"))] == [x for k, x in enumerate(KUMAGAI + [0.0]) if k not in (F("A"), F("B"), F("c0"))]
    with pytest.raises(IOError, match="energy unit"):
        capi.tersoff_mod_read_params(MOD, ["Si"], energy_unit=2)


def test_synthetic_mod_file_wrapped_and_commented(tmp_path):
    """the two-element file as written, and with every entry spread over four lines with comments between: the same numbers, those of the
    numpy reader; element selection and order as for the plain reader"""
    p, q = tmp_path / "plain.tersoff.modc", tmp_path / "wrapped.tersoff.modc"
    p.write_text(tf.SYNTH_MOD)
    body = []
    for l in tf.SYNTH_MOD.split("\n"):
        w = l.split("#")[0].split()
        body.append("  ".join(w[:5]) + "   # a comment in the middle of an entry\n# a whole line\n\n" + " ".join(w[5:12]) + "\n\t" + " ".join(w[12:]) if w else l)
    q.write_text("\n".join(body) + "\n")
    a, b = capi.tersoff_mod_read_params(str(p), ["X", "Y"]), capi.tersoff_mod_read_params(str(q), ["X", "Y"])
    assert a[0] == b[0] == 2 and np.array_equal(a[2], b[2])
    ref = tf.read_mod(str(p), ["X", "Y"])[0]
    for (i, j, k), d in ref.items():
        assert list(a[2][i, j, k]) == [d[f] for f in tf.MOD_FIELDS], (i, j, k)
    assert a[2][1, 0, 1, tf.MOD_FIELDS.index("c4")] == 0.0 and a[2][0, 0, 1, tf.MOD_FIELDS.index("R")] == 2.6
    n, tmap, w = capi.tersoff_mod_read_params(str(p), ["Y", "X", "Y"])
    assert n == 2 and list(tmap) == [0, 1, 0]
    for i, j, k in np.ndindex(2, 2, 2):
        assert list(w[i, j, k]) == list(a[2][1 - i, 1 - j, 1 - k])
    assert capi.tersoff_mod_read_params(str(p), ["Y"])[0] == 1
    with pytest.raises(IOError, match="no entry for the triplet X X Ge"):
        capi.tersoff_mod_read_params(str(p), ["X", "Ge"])


def test_zbl_fixture_numbers(tmp_path):
    for unit in (0, 1):
        n, tmap, v = capi.tersoff_zbl_read_params(ZBL, ["Si", "C"], energy_unit=unit)
        ref = tf.read_zbl(ZBL, ["Si", "C"], energy_unit=unit)[0]
        assert n == 2 and list(tmap) == [0, 1] and v.shape == (2, 2, 2, 18) and len(ref) == 8
        for (i, j, k), d in ref.items():
            assert list(v[i, j, k]) == [d[f] for f in tf.ZBL_FIELDS], (i, j, k)
    assert list(v[0, 1, 1, 14:]) == [14.0, 6.0, 0.95, 14.0] and list(v[1, 0, 0, 14:]) == [6.0, 14.0, 0.95, 14.0]
    # the fourteen plain numbers are those of the plain reader on tests/golden/SiC.tersoff
    plain = capi.tersoff_read_params(os.path.join(GOLD, "SiC.tersoff"), ["Si", "C"], energy_unit=1)[2]
    assert np.array_equal(v[..., :14], plain)
    words = open(ZBL).read().split("\n")
    q = tmp_path / "wrapped.tersoff.zbl"
    q.write_text("\n".join((" ".join(l.split()[:9]) + " # comment\n" + " ".join(l.split()[9:])) if l and not l.startswith("#") else l for l in words) + "\n")
    assert np.array_equal(capi.tersoff_zbl_read_params(str(q), ["Si", "C"], energy_unit=1)[2], v)


MOD_ENTRY = "Si Si Si " + " ".join(repr(x) for x in KUMAGAI)
ZBL_ENTRY = "Si Si Si 3 1 0 100390 16.217 -0.59825 0.78734 1.1e-6 1.7322 471.18 2.85 0.15 2.4799 1830.8 14 14 0.95 14.0"


def _refused(tmp_path, reader, text, match, elements=("Si",)):
    p = tmp_path / "bad.file"
    p.write_text(text)
    with pytest.raises(IOError, match=match):
        reader(str(p), list(elements))


def _with(entry, fields, **kw):
    w = entry.split()
    for f, val in kw.items():
        w[3 + fields.index(f)] = str(val)
    return " ".join(w) + "\n"


@pytest.mark.parametrize("field", ["alpha", "eta", "lambda2", "B", "R", "D", "lambda1", "A", "n", "c2", "c3", "c4", "c5"])
def test_negative_value_is_refused_mod(tmp_path, field):
    _refused(tmp_path, capi.tersoff_mod_read_params, _with(MOD_ENTRY, tf.MOD_FIELDS, **{field: "-" + MOD_ENTRY.split()[3 + tf.MOD_FIELDS.index(field)]}),
             "alpha, eta, lambda2, B, R, D, lambda1, A, n, c2, c3, c4 and c5 must not be negative")


def test_other_refusals_mod(tmp_path):
    R = lambda text, match, **k: _refused(tmp_path, capi.tersoff_mod_read_params, text, match, **k)
    W = lambda **kw: _with(MOD_ENTRY, tf.MOD_FIELDS, **kw)
    for b in ("0.9", "2", "0"):
        R(W(beta_ters=b), r"beta_ters must be 1 \(entry that starts on line 1\)")
    for b in ("2", "0", "1.5", "-3"):
        R(W(beta=b), "beta must be 1 or 3")
    for b in ("1", "3", "3e0"):
        q = tmp_path / "ok.mod"
        q.write_text(W(beta=b))
        assert capi.tersoff_mod_read_params(str(q), ["Si"])[0] == 1
    R(W(D="3.01"), "D must not exceed R")
    R(W(n="0"), "n of a pair entry")
    R(W(eta="0"), "eta of a pair entry")
    # c3 = 0: refused where cos theta can reach h (the rule: -1 <= h <= 1), let through otherwise; a negative c1 or h is no refusal
    R(W(c3="0"), "c3 must be positive where cos theta can reach h")
    R(W(c3="0", h="1.0"), "c3 must be positive")
    q = tmp_path / "ok.mod"
    q.write_text(W(c3="0", h="-1.5", c1="-0.1"))
    v = capi.tersoff_mod_read_params(str(q), ["Si"], energy_unit=1)[2][0, 0, 0]
    assert v[tf.MOD_FIELDS.index("c3")] == 0.0 and v[tf.MOD_FIELDS.index("h")] == -1.5 and v[tf.MOD_FIELDS.index("c1")] == -0.1
    R(MOD_ENTRY + "\n" + MOD_ENTRY + "\n", "duplicate entry Si Si Si")
    R(" ".join(MOD_ENTRY.split()[:19]) + "\n", "short entry: 19 of 20 words")
    R(MOD_ENTRY + " -0.02\n" + " ".join(MOD_ENTRY.split()[:20]) + "\n", "short entry: 20 of 21 words")          # a mod/c file whose second entry lacks c0
    R(W(h="n.a."), "'n.a.' on line 1 is not a number")
    R("# nothing but a comment\n", "no entry for the triplet Si Si Si")
    R(MOD_ENTRY + "\n", "no entry for the triplet Si Si C", elements=("Si", "C"))
    # the plain Tersoff fixture handed to this reader: a column-count message, no table
    with pytest.raises(IOError, match="where an element name is expected|short entry|is not a number"):
        capi.tersoff_mod_read_params(os.path.join(GOLD, "SiC.tersoff"), ["Si"])


@pytest.mark.parametrize("field", ["c", "d", "n", "beta", "lambda2", "B", "R", "D", "lambda1", "A", "gamma"])
def test_negative_value_is_refused_zbl(tmp_path, field):
    _refused(tmp_path, capi.tersoff_zbl_read_params, _with(ZBL_ENTRY, tf.ZBL_FIELDS, **{field: "-" + ZBL_ENTRY.split()[3 + tf.ZBL_FIELDS.index(field)]}),
             "must not be negative")


def test_other_refusals_zbl(tmp_path):
    R = lambda text, match, **k: _refused(tmp_path, capi.tersoff_zbl_read_params, text, match, **k)
    W = lambda **kw: _with(ZBL_ENTRY, tf.ZBL_FIELDS, **kw)
    R(W(Z_i="0"), "Z_i and Z_j must be positive")
    R(W(Z_j="-6"), "Z_i and Z_j must be positive")
    R(W(ZBLcut="-0.1"), "ZBLcut and ZBLexpscale must not be negative")
    R(W(ZBLexpscale="-14"), "ZBLcut and ZBLexpscale must not be negative")
    R(W(D="2.86"), "D must not exceed R")
    R(W(m="2"), "m must be 1 or 3")
    R(W(n="0"), "n of a pair entry")
    R(ZBL_ENTRY + "\n" + ZBL_ENTRY + "\n", "duplicate entry Si Si Si")
    R(" ".join(ZBL_ENTRY.split()[:17]) + "\n", "short entry: 17 of 21 words")          # a plain Tersoff entry
    R(W(ZBLcut="x"), "'x' on line 1 is not a number")
    lines = open(ZBL).read().splitlines()
    entries = [n for n, l in enumerate(lines) if l and not l.startswith("#")]
    assert len(entries) == 8
    for drop in entries:
        R("\n".join(l for n, l in enumerate(lines) if n != drop) + "\n", "no entry for the triplet", elements=("Si", "C"))
    q = tmp_path / "ok.zbl"
    q.write_text(W(ZBLcut="0", ZBLexpscale="0"))          # zero is allowed
    assert capi.tersoff_zbl_read_params(str(q), ["Si"])[0] == 1
