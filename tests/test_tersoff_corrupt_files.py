"""Corrupt Tersoff parameter files (the idea of tests/test_sw_corrupt_files.py for scema_md_tersoff_read_params): truncations and garbage
are refused with a message; nothing crashes."""
import os

import numpy as np
import pytest

from scema_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIC = os.path.join(ROOT, "tests", "golden", "SiC.tersoff")
ENTRY = "Si Si Si 3 1 0 100390 16.217 -0.59825 0.78734 1.1e-6 1.7322 471.18 2.85 0.15 2.4799 1830.8\n"


def _refused(path, match=None):
    with pytest.raises(IOError, match=match):
        capi.tersoff_read_params(str(path), ["Si"])


def test_every_truncation_of_the_fixture(tmp_path):
    """cut anywhere, the file is refused with a message or holds a whole Si Si Si entry (the last number may have lost digits that still
    leave a number; a cut inside a later entry leaves a short one)"""
    raw = open(SIC, "rb").read()
    start = raw.index(b"\nSi Si Si") + 1
    p = tmp_path / "cut.tersoff"
    whole = 0
    for cut in range(0, len(raw) + 1, 3):
        p.write_bytes(raw[:cut])
        words = raw[start:cut].split() if cut > start else []
        try:
            capi.tersoff_read_params(str(p), ["Si"], energy_unit=1)
        except IOError as err:
            assert len(words) % 17 != 0 or len(words) == 0 or b"#" in raw[start:cut], (cut, err)
            assert str(err).strip(), cut
            continue
        assert len(words) >= 17 and len(words) % 17 == 0, cut
        whole += 1
    assert whole >= 1


@pytest.mark.parametrize("bad", ["x", "1.2.3", "nan", "inf", "1e999", "0x", "--1", "1,5"])
def test_non_numeric_field(tmp_path, bad):
    for k in range(3, 17):
        w = ENTRY.split()
        w[k] = bad
        p = tmp_path / "bad.tersoff"
        p.write_text(" ".join(w) + "\n")
        _refused(p, "not a number")


def test_short_entry_and_shifted_words(tmp_path):
    w = ENTRY.split()
    p = tmp_path / "short.tersoff"
    p.write_text(" ".join(w[:16]) + "\n")
    _refused(p, "short entry")
    p.write_text(" ".join(w[:16]) + "\n" + ENTRY)            # a short entry in front shifts a name into a number's place
    _refused(p, "not a number")
    p.write_text(ENTRY + "Si Si\n")
    _refused(p, "short entry")
    p.write_text("Si Si 2.0 " + " ".join(w[3:]) + " 0.0\n")    # a number where the third name belongs
    _refused(p, "element name")


def test_garbage(tmp_path):
    rng = np.random.default_rng(5)
    p = tmp_path / "g.tersoff"
    for n in (0, 1, 16, 17, 200, 5000):
        p.write_bytes(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        _refused(p)
    p.write_bytes(b"\x00" * 64)
    _refused(p)
    p.write_bytes(("Si " * 5000).encode())
    _refused(p)
    p.write_bytes(b"Si Si Si 3 " + b"9" * 100000 + b" 1 1 1 1 1 1 1 1 1 1 1 1\n")     # a number of 100 000 digits overflows to infinity
    _refused(p, "not a number")
    _refused(os.path.join(ROOT, "tests", "golden", "lammps_17Nov16_init.sic_1.bin"))   # a binary restart is no parameter file
    _refused(os.path.join(ROOT, "tests", "golden", "Si.sw"))                           # nor is a Stillinger-Weber file (14-word entries)
    _refused(tmp_path)                                          # a directory
    _refused(tmp_path / "does_not_exist.tersoff", "cannot open")


def test_bad_arguments():
    import ctypes as C
    L = capi.lib()
    L.scema_md_tersoff_read_params.restype = C.c_int
    err = C.create_string_buffer(64)
    assert L.scema_md_tersoff_read_params(None, None, C.c_int32(0), C.c_int32(0), None, None, None, err, C.c_int32(64)) == 1
    arr = (C.c_char_p * 1)(b"Si")
    # outputs are optional, a small error buffer truncates the message
    assert L.scema_md_tersoff_read_params(SIC.encode(), arr, C.c_int32(1), C.c_int32(0), None, None, None, None, C.c_int32(0)) == 0
    small = C.create_string_buffer(8)
    assert L.scema_md_tersoff_read_params(b"/nonexistent/x.tersoff", arr, C.c_int32(1), C.c_int32(0), None, None, None, small, C.c_int32(8)) == 5
    assert len(small.value) == 7
    with pytest.raises(IOError, match="empty element"):
        capi.tersoff_read_params(SIC, [""])
