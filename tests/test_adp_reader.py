"""The reader of extended setfl files (pair_style adp; host/eam_setfl.cpp through scema_md_adp_read_setfl, a pure host function: no GPU):
the fixture value by value against the formulae of its generator, the spline records of every kept function against
tests/adp_numpy.py, both energy units, every refusal with its message -- those of the embedded-atom reader, and a file that ends inside
its u or its w tables -- and the reader as a stand-alone program under AddressSanitizer and UBSan on the fixture and truncated copies."""
import math
import os
import subprocess

import numpy as np
import pytest

import adp_numpy as an
import eam_numpy as en
from scema_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUAG = os.path.join(ROOT, "tests", "golden", "CuAg.adp")
CUAG_EAM = os.path.join(ROOT, "tests", "golden", "CuAg.eam.alloy")
NWORDS = 2 * (4 + an.NRHO + an.NR) + 9 * an.NR          # after the line of counts: 3 488


def _records(s):
    """the library's two records of a knot from the numpy coefficients s0..s6"""
    return s[:, 3:7], np.concatenate([s[:, 0:3], np.zeros((len(s), 1))], axis=1)


def _close(got, want, tol=1e-13):
    for g, w in zip(got, _records(want)):
        assert g.shape == w.shape and np.abs(g - w).max() <= tol * np.abs(w).max()


@pytest.fixture(scope="module")
def good():
    return open(CUAG).read().split("\n")


def _write(tmp_path, lines, name="bad.adp"):
    p = tmp_path / name
    p.write_text("\n".join(lines))
    return str(p)


def _header(lines, text):
    out = list(lines)
    out[4] = text
    return out


def test_fixture_header_and_size():
    out = capi.adp_read_setfl(CUAG, ["Cu", "Ag"])
    assert out["n"] == 2 and list(out["type_map"]) == [0, 1] and out["nrho"] == an.NRHO == 200 and out["nr"] == an.NR == 280
    assert out["cutoff"] == 5.5 and out["dr"] == an.DR == 0.02 and out["cutoff"] <= (out["nr"] - 1) * out["dr"]
    assert out["rhomax"] == (out["nrho"] - 1) * out["drho"]
    assert list(out["masses"]) == [en.CU_MASS, en.AG_MASS]
    assert os.path.getsize(CUAG) <= os.path.getsize(CUAG_EAM)                 # no larger than the embedded-atom fixture
    head = open(CUAG).read().split("\n")[:3]
    assert "Analytic ADP" in head[0] and "not from LAMMPS" in head[2]
    assert NWORDS == 3488 and len(" ".join(open(CUAG).read().split("\n")[5:]).split()) == NWORDS


def test_fixture_value_by_value_against_the_generator():
    """the file's numbers against the analytic functions: F, rho, r phi of Johnson's form (eam_numpy.johnson_tables on this grid), u and w
    of adp_numpy.u_of / w_of, to the 17 digits the file keeps; as the library's reader returns them (s6 of a knot is the tabulated value)"""
    out = capi.adp_read_setfl(CUAG, ["Cu", "Ag"], energy_unit=1)
    names = ["Cu", "Ag"]
    nrho, drho, nr, dr, cutoff, F, rho, z = en.johnson_tables(names, nrho=an.NRHO, nr=an.NR, dr=an.DR)
    assert out["drho"] == float("%.17g" % drho)
    r = np.arange(nr) * dr
    same = lambda got, want: np.abs(got - want).max() <= 1e-15 * np.abs(want).max()
    for i in range(2):
        assert same(out["F"][i][0][:, 3], F[i]) and same(out["rho"][i][0][:, 3], rho[i])
        for j in range(i + 1):
            assert same(out["z"][(i, j)][0][:, 3], z[(i, j)])
            assert same(out["u"][(i, j)][0][:, 3], an.u_of(names[i], names[j], r)) and same(out["w"][(i, j)][0][:, 3], an.w_of(names[i], names[j], r))
    # each pair has an amplitude of its own, of either sign, and u, w end at zero with the switch
    amps = [(out["u"][p][0][100, 3], out["w"][p][0][100, 3]) for p in ((0, 0), (1, 0), (1, 1))]
    assert len({round(abs(a), 6) for a, _ in amps}) == 3 and len({round(abs(b), 6) for _, b in amps}) == 3
    assert amps[0][0] > 0 > amps[1][0] and amps[0][1] < 0 < amps[1][1]
    for p in ((0, 0), (1, 0), (1, 1)):
        assert abs(out["u"][p][0][275:, 3]).max() == 0.0 and abs(out["w"][p][0][275:, 3]).max() == 0.0           # from 5.5 A on


@pytest.mark.parametrize("elements", [["Cu"], ["Ag"], ["Cu", "Ag"], ["Ag", "Cu"], ["Ag", "Cu", "Ag", "Ag"]])
def test_spline_tables_match_numpy(elements):
    """every coefficient of every kept function, the elements out of file order and repeated"""
    out = capi.adp_read_setfl(CUAG, elements)
    tab, tmap = an.read_adp(CUAG, elements)
    assert out["n"] == tab["n"] == len(set(elements)) and list(out["type_map"]) == tmap
    for i in range(out["n"]):
        _close(out["F"][i], en.spline(tab["F"][i], tab["drho"]))
        _close(out["rho"][i], en.spline(tab["rho"][i], tab["dr"]))
        for j in range(i + 1):
            for key in ("z", "u", "w"):
                _close(out[key][(i, j)], en.spline(tab[key][i][j], tab["dr"]))
    if elements == ["Ag", "Cu"]:            # the pair tables follow the names: (Ag, Ag) is the file's third pair, not its first
        other = capi.adp_read_setfl(CUAG, ["Cu", "Ag"])
        for key in ("z", "u", "w"):
            assert np.array_equal(out[key][(1, 0)][0], other[key][(1, 0)][0]) and np.array_equal(out[key][(0, 0)][0], other[key][(1, 1)][0])
            assert np.array_equal(out[key][(1, 1)][1], other[key][(0, 0)][1])
    if elements == ["Ag"]:
        other = capi.adp_read_setfl(CUAG, ["Cu", "Ag"])
        assert np.array_equal(out["u"][(0, 0)][0], other["u"][(1, 1)][0]) and np.array_equal(out["w"][(0, 0)][0], other["w"][(1, 1)][0])


def test_the_eam_part_is_the_eam_readers(tmp_path):
    """the same F, rho and r phi through both readers: the embedded-atom reader takes the ADP file (it stops after r phi), and the two agree to the bit"""
    a, b = capi.adp_read_setfl(CUAG, ["Cu", "Ag"]), capi.eam_read_setfl(CUAG, ["Cu", "Ag"])
    for i in range(2):
        assert np.array_equal(a["F"][i][0], b["F"][i][0]) and np.array_equal(a["rho"][i][1], b["rho"][i][1])
        for j in range(i + 1):
            assert np.array_equal(a["z"][(i, j)][0], b["z"][(i, j)][0]) and np.array_equal(a["z"][(i, j)][1], b["z"][(i, j)][1])


def test_energy_units():
    """unit 0: F and r phi times 23.060549, u and w times its square root; the density has no unit; unit 1: as written"""
    a, b = capi.adp_read_setfl(CUAG, ["Cu", "Ag"], energy_unit=0), capi.adp_read_setfl(CUAG, ["Cu", "Ag"], energy_unit=1)
    assert np.array_equal(a["rho"][0][0], b["rho"][0][0]) and np.array_equal(a["rho"][1][1], b["rho"][1][1])
    for key, scale in (("F", 23.060549), ("z", 23.060549), ("u", math.sqrt(23.060549)), ("w", math.sqrt(23.060549))):
        for x, y in ((a[key][0], b[key][0]),) if key == "F" else ((a[key][p], b[key][p]) for p in ((0, 0), (1, 0), (1, 1))):
            # a tabulated value is rounded once after scaling (1.1e-16 relative); a coefficient of the value record is a sum of up to six
            # of them with weights of at most 3, one of the derivative record that times at most 3 / delta
            delta = a["drho"] if key == "F" else a["dr"]
            for rec, weight in ((0, 1.0), (1, 3.0 / delta)):
                assert np.abs(x[rec]).max() > 0.0 and np.abs(x[rec] - scale * y[rec]).max() <= 2e-15 * weight * np.abs(x[0]).max(), key
    with pytest.raises(IOError, match="energy unit 2"):
        capi.adp_read_setfl(CUAG, ["Cu"], energy_unit=2)


def test_files_cut_inside_u_and_inside_w(tmp_path, good):
    """lines 367 to 534 hold u, 535 to 702 hold w (five numbers a line): the refusal says in which block the file ends"""
    assert len(good) == 704 and good[-1] == ""
    for keep, block in ((367, "u"), (400, "u"), (534, "u"), (535, "w"), (600, "w"), (702, "w")):
        with pytest.raises(IOError, match=f"truncated file: it ends inside the {block} tables of an ADP file .*its counts announce 3488 numbers, it holds {5 * keep - 27}$"):
            capi.adp_read_setfl(_write(tmp_path, good[:keep]), ["Cu", "Ag"])
    # one number short at the very end, and one number short of the end of u
    with pytest.raises(IOError, match="it ends inside the w tables.*announce 3488 numbers, it holds 3487"):
        capi.adp_read_setfl(_write(tmp_path, good[:-2] + [" ".join(good[-2].split()[:-1])]), ["Cu"])
    with pytest.raises(IOError, match="it ends inside the u tables.*it holds 2647"):
        capi.adp_read_setfl(_write(tmp_path, good[:534] + [" ".join(good[534].split()[:-1])]), ["Cu"])
    # a plain eam/alloy file has neither
    with pytest.raises(IOError, match="CuAg.eam.alloy: truncated file: it ends inside the u tables of an ADP file"):
        capi.adp_read_setfl(CUAG_EAM, ["Cu"])
    # whole: the reader takes it, and numbers after the last table are not its business
    assert capi.adp_read_setfl(_write(tmp_path, good), ["Cu"])["n"] == 1


def test_refusals_of_the_setfl_reader(tmp_path, good):
    """the refusals of the embedded-atom reader, through this one, with their messages"""
    with pytest.raises(IOError, match="nothing.adp: cannot open"):
        capi.adp_read_setfl(str(tmp_path / "nothing.adp"), ["Cu"])
    for keep, what in ((300, "announce 3488 numbers, it holds"), (100, "announce 3488 numbers, it holds"), (4, "it ends where Nrho is expected"),
                       (3, "it ends where the number of elements is expected")):
        with pytest.raises(IOError, match="truncated file.*" + what):
            capi.adp_read_setfl(_write(tmp_path, good[:keep]), ["Cu"])
    with pytest.raises(IOError, match="truncated file: 2 element names announced, 1 words left"):
        capi.adp_read_setfl(_write(tmp_path, good[:3] + ["2 Cu"]), ["Cu"])
    bad = list(good)
    w = bad[600].split()
    w[2] = "1.0e+0x"
    bad[600] = " ".join(w)
    with pytest.raises(IOError, match=r"'1.0e\+0x' on line 601 is not a number \(w\(r\)\)"):
        capi.adp_read_setfl(_write(tmp_path, bad), ["Cu", "Ag"])
    bad = list(good)
    bad[400] = bad[400].replace(bad[400].split()[0], "u?", 1)
    with pytest.raises(IOError, match=r"'u\?' on line 401 is not a number \(u\(r\)\)"):
        capi.adp_read_setfl(_write(tmp_path, bad), ["Cu", "Ag"])
    with pytest.raises(IOError, match=r"'nan' on line 5 is not a number \(drho\)"):
        capi.adp_read_setfl(_write(tmp_path, _header(good, "200 nan 280 0.02 5.5")), ["Cu"])
    with pytest.raises(IOError, match="'Cu' on line 4 is not a number"):
        capi.adp_read_setfl(_write(tmp_path, good[:3] + ["Cu 2 Ag"] + good[4:]), ["Cu"])
    with pytest.raises(IOError, match="Nrho = 200.5 on line 5: a whole number"):
        capi.adp_read_setfl(_write(tmp_path, _header(good, "200.5 0.02 280 0.02 5.5")), ["Cu"])
    for text, what in (("4 0.02 280 0.02 5.5", "Nrho"), ("200 0.02 4 0.02 0.05", "Nr")):
        with pytest.raises(IOError, match=what + " = 4 on line 5: a whole number of at least 5"):
            capi.adp_read_setfl(_write(tmp_path, _header(good, text)), ["Cu"])
    for text in ("200 0.0 280 0.02 5.5", "200 0.02 280 -0.02 5.5", "200 0.02 280 0.02 0"):
        with pytest.raises(IOError, match="drho, dr and the cutoff must be positive"):
            capi.adp_read_setfl(_write(tmp_path, _header(good, text)), ["Cu"])
    with pytest.raises(IOError, match=r"the cutoff 5.6\d* lies beyond the last knot \(Nr - 1\) dr = 5.58"):
        capi.adp_read_setfl(_write(tmp_path, _header(good, "200 0.02 280 0.02 5.6")), ["Cu"])
    with pytest.raises(IOError, match="element Au is not in the file"):
        capi.adp_read_setfl(CUAG, ["Cu", "Au"])
    with pytest.raises(IOError, match="empty element name"):
        capi.adp_read_setfl(CUAG, ["Cu", ""])
    with pytest.raises(IOError, match="more than 4 distinct elements"):
        capi.adp_read_setfl(_write(tmp_path, good[:3] + ["5 A B C D E"] + good[4:]), ["A", "B", "C", "D", "E"])
    bad = list(good)
    bad[5] = "29 -63.5 3.615 fcc"
    with pytest.raises(IOError, match="the mass of Cu must be positive"):
        capi.adp_read_setfl(_write(tmp_path, bad), ["Ag"])
    # counts the file cannot hold: refused from the word count, before any table is sized by them
    for text, nums in (("1000000000 0.02 280 0.02 5.5", "2000003088"), ("200 0.02 900000000 0.0000000112 5.5", "9900000408")):
        with pytest.raises(IOError, match="truncated file: its counts .* announce " + nums + " numbers, it holds 3488"):
            capi.adp_read_setfl(_write(tmp_path, _header(good, text)), ["Cu"])
    # an Nr one larger than the file's: the EAM part and the u tables would fit, the w tables do not
    with pytest.raises(IOError, match="it ends inside the w tables.*announce 3499 numbers, it holds 3488"):
        capi.adp_read_setfl(_write(tmp_path, _header(good, "200 0.02 281 0.02 5.5")), ["Cu"])


def test_reader_under_host_sanitizers(tmp_path):
    """the reader and the arithmetic as a stand-alone program (tests/adp_host_driver.cpp) built with AddressSanitizer and UBSan: the
    fixture and ten truncated copies, three of them cut inside u and three inside w -- each run ends with the program's own status (0, or
    1 with the reader's message) and without a sanitizer report"""
    exe = str(tmp_path / "adp_driver_san")
    srcs = [os.path.join(ROOT, "tests", "adp_host_driver.cpp"), os.path.join(ROOT, "scema_amd", "csrc", "host", "eam_setfl.cpp")]
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-std=c++17",
                           "-I", os.path.join(ROOT, "include"), "-o", exe] + srcs)
    x, box, t = an.case_trimer((0, 1, 0))
    text_in = "3\n%s\n" % " ".join("%g" % b for b in box) + "".join("%d %.17g %.17g %.17g\n" % (k, *p) for k, p in zip(t, x))
    text = open(CUAG).read()
    u0, w0 = len("\n".join(text.split("\n")[:367])), len("\n".join(text.split("\n")[:535]))          # where the u and the w tables start
    cuts = [0, 150, 600, 20011, u0 + 1, u0 + 5003, w0 - 30, w0 + 3, w0 + 9001, len(text) - 30]
    assert len(cuts) == 10 and sorted(cuts) == cuts and cuts[-1] > w0
    seen = []
    for cut in [len(text)] + cuts:
        p = tmp_path / "cut.adp"
        p.write_text(text[:cut])
        r = subprocess.run([exe, str(p), "0", "0", "Cu", "Ag"], input=text_in, capture_output=True, text=True)
        assert r.returncode in (0, 1) and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (cut, r.returncode, r.stderr[-400:])
        seen.append(r.returncode)
        if r.returncode == 1:
            assert str(p) in r.stderr
            if cut > u0:
                assert ("inside the u tables" if cut <= w0 else "inside the w tables") in r.stderr, (cut, r.stderr)
    assert seen == [0] + [1] * 10
