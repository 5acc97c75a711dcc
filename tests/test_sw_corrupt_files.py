"""Corrupt Stillinger-Weber parameter files (the idea of tests/test_corrupt_files.py for scema_md_sw_read_params): truncations and
garbage are refused with a message; nothing crashes."""
import os

import numpy as np
import pytest

from scema_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SI_SW = os.path.join(ROOT, "tests", "golden", "Si.sw")
ENTRY = "Si Si Si 2.1683 2.0951 1.80 21.0 1.20 -0.333333333333 7.049556277 0.6022245584 4.0 0.0 0.0\n"


def _refused(path, match=None):
    with pytest.raises(IOError, match=match):
        capi.sw_read_params(str(path), ["Si"])


def test_every_truncation_of_the_reference_file(tmp_path):
    raw = open(SI_SW, "rb").read()
    start = raw.index(b"\nSi Si Si") + 1
    p = tmp_path / "cut.sw"
    whole = 0
    for cut in range(0, len(raw) + 1):
        p.write_bytes(raw[:cut])
        words = raw[start:cut].split() if cut > start else []
        try:
            _, _, v = capi.sw_read_params(str(p), ["Si"], energy_unit=1)
        except IOError as err:
            assert len(words) < 14 or cut < start, (cut, err)
            assert str(err).strip(), cut
            continue
        # accepted: all fourteen words are there (the last number may have lost digits that still leave a number)
        assert len(words) == 14, cut
        whole += 1
    assert whole >= 1


@pytest.mark.parametrize("bad", ["x", "1.2.3", "nan", "inf", "1e999", "0x", "--1", "1,5"])
def test_non_numeric_field(tmp_path, bad):
    for k in range(3, 14):
        w = ENTRY.split()
        w[k] = bad
        p = tmp_path / "bad.sw"
        p.write_text(" ".join(w) + "\n")
        _refused(p, "not a number")


def test_short_entry_and_shifted_words(tmp_path):
    w = ENTRY.split()
    p = tmp_path / "short.sw"
    p.write_text(" ".join(w[:13]) + "\n")
    _refused(p, "short entry")
    p.write_text(" ".join(w[:13]) + "\n" + ENTRY)            # a short entry in front shifts a name into a number's place
    _refused(p, "not a number")
    p.write_text(ENTRY + "Si Si\n")
    _refused(p, "short entry")
    p.write_text("Si Si 2.0 " + " ".join(w[3:]) + " 0.0\n")    # a number where the third name belongs
    _refused(p, "element name")


def test_negative_or_zero_lengths(tmp_path):
    p = tmp_path / "neg.sw"
    for k, val in [(4, "-2.0951"), (4, "0.0"), (5, "0"), (5, "-1.8"), (3, "-1"), (11, "-4")]:
        w = ENTRY.split()
        w[k] = val
        p.write_text(" ".join(w) + "\n")
        _refused(p)


def test_garbage(tmp_path):
    rng = np.random.default_rng(5)
    p = tmp_path / "g.sw"
    for n in (0, 1, 13, 14, 200, 5000):
        p.write_bytes(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        _refused(p)
    p.write_bytes(b"\x00" * 64)
    _refused(p)
    p.write_bytes(("Si " * 5000).encode())
    _refused(p)
    p.write_bytes(b"Si Si Si " + b"9" * 100000 + b" 1 1 1 1 1 1 1 1 1 1\n")     # a number of 100 000 digits overflows to infinity
    _refused(p, "not a number")
    _refused(os.path.join(ROOT, "tests", "golden", "lammps_17Nov16_init.sic_1.bin"))   # a binary restart is no parameter file
    _refused(tmp_path)                                          # a directory
    _refused(tmp_path / "does_not_exist.sw", "cannot open")


def test_bad_arguments():
    import ctypes as C
    L = capi.lib()
    L.scema_md_sw_read_params.restype = C.c_int
    err = C.create_string_buffer(64)
    assert L.scema_md_sw_read_params(None, None, C.c_int32(0), C.c_int32(0), None, None, None, err, C.c_int32(64)) == 1
    arr = (C.c_char_p * 1)(b"Si")
    # outputs are optional, a small error buffer truncates the message
    assert L.scema_md_sw_read_params(SI_SW.encode(), arr, C.c_int32(1), C.c_int32(0), None, None, None, None, C.c_int32(0)) == 0
    small = C.create_string_buffer(8)
    assert L.scema_md_sw_read_params(b"/nonexistent/x.sw", arr, C.c_int32(1), C.c_int32(0), None, None, None, small, C.c_int32(8)) == 5
    assert len(small.value) == 7
    with pytest.raises(IOError, match="empty element"):
        capi.sw_read_params(SI_SW, [""])
