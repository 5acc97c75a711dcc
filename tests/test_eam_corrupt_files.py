"""What the setfl reader refuses (host/eam_setfl.cpp through scema_md_eam_read_setfl, no GPU): each with a message that says what is wrong,
none with a crash or an allocation sized by a number the file merely claims."""
import os

import numpy as np
import pytest

import eam_numpy as en
from scema_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUAG = os.path.join(ROOT, "tests", "golden", "CuAg.eam.alloy")


@pytest.fixture(scope="module")
def good():
    return open(CUAG).read().split("\n")


def _write(tmp_path, lines, name="bad.eam.alloy"):
    p = tmp_path / name
    p.write_text("\n".join(lines))
    return str(p)


def _header(lines, text):
    """the file with its line `Nrho drho Nr dr cutoff` replaced"""
    out = list(lines)
    out[4] = text
    return out


def test_missing_file(tmp_path):
    with pytest.raises(IOError, match="nothing.eam.alloy: cannot open"):
        capi.eam_read_setfl(str(tmp_path / "nothing.eam.alloy"), ["Cu"])


def test_truncated_files(tmp_path, good):
    # cut in the middle of the last table, in the middle of an element's block, inside the header, after the comments
    for keep, what in ((len(good) - 40, "announce 3508 numbers, it holds"), (300, "announce 3508 numbers, it holds"), (4, "it ends where Nrho is expected"),
                       (3, "it ends where the number of elements is expected")):
        with pytest.raises(IOError, match="truncated file.*" + what):
            capi.eam_read_setfl(_write(tmp_path, good[:keep]), ["Cu"])
    with pytest.raises(IOError, match="truncated file: 2 element names announced, 1 words left"):
        capi.eam_read_setfl(_write(tmp_path, good[:3] + ["2 Cu"]), ["Cu"])
    # one number short at the very end
    last = good[:-2] + [" ".join(good[-2].split()[:-1])]
    with pytest.raises(IOError, match="truncated file.*announce 3508 numbers, it holds 3507"):
        capi.eam_read_setfl(_write(tmp_path, last), ["Cu"])


def test_non_numeric_fields(tmp_path, good):
    bad = list(good)
    w = bad[200].split()
    w[2] = "1.0e+0x"
    bad[200] = " ".join(w)
    with pytest.raises(IOError, match=r"'1.0e\+0x' on line 201 is not a number"):
        capi.eam_read_setfl(_write(tmp_path, bad), ["Cu", "Ag"])
    with pytest.raises(IOError, match=r"'nan' on line 5 is not a number \(drho\)"):
        capi.eam_read_setfl(_write(tmp_path, _header(good, "500 nan 500 0.0112 5.5")), ["Cu"])
    with pytest.raises(IOError, match="'Cu' on line 4 is not a number"):
        capi.eam_read_setfl(_write(tmp_path, good[:3] + ["Cu 2 Ag"] + good[4:]), ["Cu"])
    with pytest.raises(IOError, match="Nrho = 500.5 on line 5: a whole number"):
        capi.eam_read_setfl(_write(tmp_path, _header(good, "500.5 0.02 500 0.0112 5.5")), ["Cu"])


def test_too_few_knots(tmp_path):
    f4, f5 = np.arange(4.0), np.arange(5.0)
    for nrho, nr, what in ((4, 5, "Nrho"), (5, 4, "Nr")):
        path = str(tmp_path / f"few_{what}.eam.alloy")
        en.write_setfl(path, ["X"], [1], [10.0], [3.0], nrho, 0.5, nr, 0.25, 0.5, [f4 if nrho == 4 else f5], [f4 if nr == 4 else f5],
                       {(0, 0): f4 if nr == 4 else f5}, ["a", "b", "c"])
        with pytest.raises(IOError, match=what + " = 4 on line 5: a whole number of at least 5"):
            capi.eam_read_setfl(path, ["X"])


def test_spacings_and_cutoff(tmp_path, good):
    for text in ("500 0.0 500 0.0112 5.5", "500 0.02 500 -0.0112 5.5", "500 0.02 500 0.0112 0"):
        with pytest.raises(IOError, match="drho, dr and the cutoff must be positive"):
            capi.eam_read_setfl(_write(tmp_path, _header(good, text)), ["Cu"])
    with pytest.raises(IOError, match=r"the cutoff 5.6\d* lies beyond the last knot \(Nr - 1\) dr = 5.588"):
        capi.eam_read_setfl(_write(tmp_path, _header(good, "500 0.02 500 0.0112 5.6")), ["Cu"])


def test_elements(tmp_path, good):
    with pytest.raises(IOError, match="element Au is not in the file"):
        capi.eam_read_setfl(CUAG, ["Cu", "Au"])
    with pytest.raises(IOError, match="empty element name"):
        capi.eam_read_setfl(CUAG, ["Cu", ""])
    five = _write(tmp_path, good[:3] + ["5 A B C D E"] + good[4:])
    with pytest.raises(IOError, match="more than 4 distinct elements"):
        capi.eam_read_setfl(five, ["A", "B", "C", "D", "E"])
    bad = list(good)
    bad[5] = "29 -63.5 3.615 fcc"
    with pytest.raises(IOError, match="the mass of Cu must be positive"):
        capi.eam_read_setfl(_write(tmp_path, bad), ["Ag"])


def test_counts_the_file_cannot_hold(tmp_path, good):
    """Nrho of a thousand million in a file of 82 kB: refused from the word count, before any table is sized by it"""
    for text, nums in (("1000000000 0.02 500 0.0112 5.5", "2000002508"), ("500 0.02 900000000 0.0000000112 5.5", "4500001008")):
        with pytest.raises(IOError, match="truncated file: its counts .* announce " + nums + " numbers, it holds 3508"):
            capi.eam_read_setfl(_write(tmp_path, _header(good, text)), ["Cu"])
    with pytest.raises(IOError, match="Nr = 1e\\+30 on line 5: a whole number"):
        capi.eam_read_setfl(_write(tmp_path, _header(good, "500 0.02 1e+30 0.0112 5.5")), ["Cu"])
    many = _write(tmp_path, good[:3] + ["70000 " + " ".join("E%d" % k for k in range(70000))] + good[4:])
    with pytest.raises(IOError, match="truncated file: its counts"):
        capi.eam_read_setfl(many, ["E1"])
