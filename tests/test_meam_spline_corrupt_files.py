"""A corpus of truncated and bit-flipped meam/spline files through the reader (scema_md_meam_spline_read_params and
scema_md_meam_spline_eval, no GPU): it never crashes, a file it takes yields finite splines, and every refusal names a line.  The same
corpus goes through the stand-alone driver built with the address and undefined-behaviour sanitizers (tests/meam_spline_host_driver.cpp
--read): nothing of it is loaded into Python."""
import os
import re
import subprocess

import numpy as np
import pytest

from scema_amd import capi
from test_meam_spline_host import driver_exe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = {"Ti": (os.path.join(ROOT, "tests", "golden", "Ti.meam.spline"), ["Ti"]), "TiO": (os.path.join(ROOT, "tests", "golden", "TiO.meam.spline"), ["Ti", "O"])}


def corpus(which):
    """(name, bytes): the file cut at 60 places, and with one bit flipped at 240 places (seeded)"""
    path, _ = FILES[which]
    data = open(path, "rb").read()
    rng = np.random.default_rng(17 if which == "Ti" else 18)
    out = []
    for cut in sorted(set(int(c) for c in np.concatenate([np.arange(0, 40), rng.integers(0, len(data), 40), [len(data) - 1, len(data) - 2]]))):
        out.append((f"cut{cut}", data[:cut]))
    first = data.index(b"\n") + 1
    for k in range(240):
        pos = int(rng.integers(first if k % 4 else 0, len(data)))
        b = bytearray(data)
        b[pos] ^= 1 << int(rng.integers(0, 8))
        out.append((f"flip{k}_{pos}", bytes(b)))
    return out


@pytest.mark.parametrize("which", ["Ti", "TiO"])
def test_the_reader_never_crashes_and_every_refusal_names_a_line(tmp_path, which):
    _, el = FILES[which]
    taken = refused = 0
    for name, data in corpus(which):
        p = tmp_path / (name + ".meam.spline")
        p.write_bytes(data)
        try:
            tab = capi.meam_spline_read_params(str(p), el)
        except IOError as err:
            refused += 1
            assert re.search(r"line \d+", str(err)), (name, str(err))
            continue
        taken += 1
        for k, fn in enumerate(tab["fn"]):
            assert 2 <= fn["n"] <= 32 and np.isfinite(fn["y2"]).all() and (np.diff(fn["x"]) > 0.0).all(), (name, k)
            xs = np.linspace(fn["x"][0] - 1.0, fn["x"][-1] + 1.0, 33)
            a, b = capi.meam_spline_eval(str(p), el, k, xs), capi.meam_spline_eval(str(p), el, k, xs, search=True)
            assert np.isfinite(a[0]).all() and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (name, k)
    print(f"{which}: {taken} files taken, {refused} refused")
    assert refused > 60 and taken > 10      # (a flipped bit in a mantissa or in the ignored third column leaves a readable file)


def test_the_corpus_through_the_sanitized_driver(tmp_path):
    """the stand-alone program with -fsanitize=address,undefined over both fixtures and the corpus: exit status 0 (taken) or 1 (refused),
    never a sanitizer report (which ends the program with another status and text on stderr)"""
    exe = driver_exe(("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"), "_asan")
    n = 0
    for which, (path, el) in FILES.items():
        items = [("good", open(path, "rb").read())] + corpus(which)[::3]
        for name, data in items:
            p = tmp_path / (which + name + ".meam.spline")
            p.write_bytes(data)
            r = subprocess.run([exe, "--read", str(p), "0"] + el, capture_output=True, text=True)
            assert r.returncode in (0, 1) and r.stderr == "", (which, name, r.returncode, r.stderr[-2000:])
            assert (r.returncode == 0) == r.stdout.startswith("ok "), (which, name, r.stdout)
            n += 1
        assert subprocess.run([exe, "--read", path, "0"] + el, capture_output=True, text=True).returncode == 0
    assert n > 200
