"""The core both many-body parameter readers stand on (scema_amd/csrc/host/triplet_file.h), driven through scema_md_sw_read_params and
scema_md_tersoff_read_params (pure host functions, no GPU): the same file shapes in both formats -- an entry split over lines, a comment in
mid-entry, an entry of an element not named, a duplicate, a short tail, a number where a name belongs -- give the same values or the same
message, word count apart."""
import numpy as np
import pytest

from scema_amd import capi

SW = "2.1683 2.0951 1.80 21.0 1.20 -0.333333333333 7.049556277 0.6022245584 4.0 0.0 0.0".split()
TS = "3 1 0 100390 16.217 -0.59825 0.78734 1.1e-6 1.7322 471.18 2.85 0.15 2.4799 1830.8".split()
FORMATS = {"sw": (capi.sw_read_params, SW), "tersoff": (capi.tersoff_read_params, TS)}


def _entry(numbers, names=("Si", "Si", "Si")):
    return " ".join(list(names) + numbers) + "\n"


def _read(fmt, tmp_path, text, elements=("Si",)):
    p = tmp_path / ("case." + fmt)
    p.write_text(text)
    return FORMATS[fmt][0](str(p), list(elements), energy_unit=1)


def _message(fmt, tmp_path, text, elements=("Si",)):
    """the reader's message without return code and path"""
    with pytest.raises(IOError) as ei:
        _read(fmt, tmp_path, text, elements)
    head = f"{tmp_path / ('case.' + fmt)}: "
    assert head in str(ei.value)
    return str(ei.value).split(head, 1)[1]


@pytest.mark.parametrize("fmt", FORMATS)
def test_split_entry_with_comments(fmt, tmp_path):
    num = FORMATS[fmt][1]
    n, tmap, plain = _read(fmt, tmp_path, _entry(num))
    w = ["Si", "Si", "Si"] + num
    text = "# header\n" + " ".join(w[:2]) + "   # a comment in mid-entry\n\n# a whole line\n\t" + " ".join(w[2:7]) + "\n" + " ".join(w[7:]) + " # the end\n"
    m, tmap2, split = _read(fmt, tmp_path, text)
    assert n == m == 1 and list(tmap) == list(tmap2) == [0]
    assert np.array_equal(plain, split) and list(plain[0, 0, 0]) == [float(x) for x in num]


@pytest.mark.parametrize("fmt", FORMATS)
def test_entry_of_an_element_not_named_is_skipped(fmt, tmp_path):
    num = FORMATS[fmt][1]
    other = ["-" + x.lstrip("-") for x in num]          # numbers the format's own checks would refuse: a skipped entry never reaches them
    text = _entry(other, ("Ge", "Si", "Si")) + _entry(num) + _entry(other, ("Si", "Si", "Ge")) + _entry(other, ("Ge", "Ge", "Ge")) * 2
    n, _, v = _read(fmt, tmp_path, text)
    assert n == 1 and list(v[0, 0, 0]) == [float(x) for x in num]


def test_refusals_read_alike(tmp_path):
    got = {}
    for fmt, (_, num) in FORMATS.items():
        nw = 3 + len(num)
        good = _entry(num)
        cases = {
            "duplicate": ("# one\n" + good + "\n" + good, "duplicate entry Si Si Si (entry that starts on line 4)"),
            "short tail": (good + "Si Si\n" + " ".join(num[:3]) + "\n", f"short entry: 5 of {nw} words (entry that starts on line 2)"),
            "short only": ("Si\n", f"short entry: 1 of {nw} words (entry that starts on line 1)"),
            "number for a name": (good + "Si 14 Si\n" + " ".join(num) + "\n", "'14' on line 2 where an element name is expected (entry that starts on line 2)"),
            "name for a number": ("Si Si Si\n" + " ".join(num[:4] + ["Si"] + num[5:]) + "\n", "'Si' on line 2 is not a number (entry that starts on line 1)"),
            "shifted by a lost word": (_entry(num[:-1]) + good, None),
            "nothing": ("# nothing but a comment\n", "no entry for the triplet Si Si Si"),
        }
        for name, (text, want) in cases.items():
            msg = _message(fmt, tmp_path, text)
            if want is not None:
                assert msg == want, (fmt, name)
            got.setdefault(name, {})[fmt] = msg.replace(f"of {nw} words", "of NW words")
    for name, by in got.items():
        assert by["sw"] == by["tersoff"], name
    # the entry after a lost word starts one word early: its first "name" is the last number of the entry before
    assert got["shifted by a lost word"]["sw"] == "'Si' on line 2 is not a number (entry that starts on line 1)"


def test_element_list_refusals_read_alike(tmp_path):
    for fmt, (_, num) in FORMATS.items():
        assert _message(fmt, tmp_path, _entry(num), elements=("Si", "")) == "empty element name"
        assert _message(fmt, tmp_path, _entry(num), elements=("Si", "A", "B", "C", "D")) == "more than 4 distinct elements"
        assert _message(fmt, tmp_path, _entry(num), elements=("Si", "C")) == "no entry for the triplet Si Si C"
