"""A corpus of truncated and bit-flipped born/coul/long and buck/coul/long fragments through the reader (scema_md_born_long_read_params and
scema_md_born_long_eval, no GPU): it never crashes, a fragment it takes yields a finite table and finite pair terms, and every refusal
names a line.  The same corpus goes through the stand-alone driver built with the address and undefined-behaviour sanitizers
(tests/born_long_host_driver.cpp --read): nothing of it is loaded into Python."""
import os
import re
import subprocess

import numpy as np
import pytest

from scema_amd import capi
from test_born_long_host import driver_exe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = {"NaCl": os.path.join(ROOT, "tests", "golden", "NaCl.born_long"), "MgO": os.path.join(ROOT, "tests", "golden", "MgO.buck_long")}


def corpus(which):
    """(name, bytes): the fragment cut at some 80 places, and with one bit flipped at 240 places (seeded), three quarters of them in
    the lines that are read"""
    data = open(FILES[which], "rb").read()
    rng = np.random.default_rng(31 if which == "NaCl" else 32)
    out = []
    for cut in sorted(set(int(c) for c in np.concatenate([np.arange(0, 40), rng.integers(0, len(data), 40), [len(data) - 1, len(data) - 2]]))):
        out.append((f"cut{cut}", data[:cut]))
    first = data.index(b"units")
    for k in range(240):
        pos = int(rng.integers(first if k % 4 else 0, len(data)))
        b = bytearray(data)
        b[pos] ^= 1 << int(rng.integers(0, 8))
        out.append((f"flip{k}_{pos}", bytes(b)))
    return out


@pytest.mark.parametrize("which", sorted(FILES))
def test_the_reader_never_crashes_and_every_refusal_names_a_line(tmp_path, which):
    taken = refused = 0
    for name, data in corpus(which):
        p = tmp_path / (name + ".born_long")
        p.write_bytes(data)
        try:
            tab = capi.born_long_read_params(str(p))
        except IOError as err:
            refused += 1
            assert re.search(r"line \d+: ", str(err)), (name, str(err))
            continue
        taken += 1
        n = tab["n"]
        assert 1 <= n <= capi.BD_MAXEL and np.isfinite(tab["values"]).all() and (tab["values"][:, :, 1] > 0.0).all() and (tab["values"][:, :, 5] > 0.0).all(), name
        assert tab["cut_coul"] > 0.0 and tab["cutmax"] >= tab["cut_coul"] and 0.0 < tab["accuracy"] < 1.0, name
        r = np.array([0.9 * tab["cutmax"], tab["cutmax"], 1.1 * tab["cutmax"]])
        for ti in range(n):
            eb, ec, fb, fc = capi.born_long_eval(str(p), 0.3, ti, n - 1, 1.0, -1.0, r)
            assert np.isfinite(np.concatenate([eb, ec, fb, fc])).all() and not eb[1:].any() and not ec[1:].any(), (name, ti)
    print(f"{which}: {taken} fragments taken, {refused} refused")
    assert refused > 60 and taken > 10      # (a flipped bit in a digit or in a comment leaves a readable fragment)


def test_the_corpus_through_the_sanitized_driver(tmp_path):
    """the stand-alone program with -fsanitize=address,undefined over both fixtures and the corpus: exit status 0 (taken) or 1 (refused
    with the reader's message), never a sanitizer report (which ends the program with another status and its own text on stderr)"""
    exe = driver_exe(0, ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"), "_asan")
    n = 0
    for which, path in FILES.items():
        items = [("good", open(path, "rb").read())] + corpus(which)[::3]
        for name, data in items:
            p = tmp_path / (which + name + ".born_long")
            p.write_bytes(data)
            r = subprocess.run([exe, str(p), "0", "--read"], capture_output=True, text=True, errors="replace")
            assert r.returncode in (0, 1) and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (which, name, r.returncode, r.stderr[-2000:])
            assert (r.returncode == 0) == r.stdout.startswith("ok ") and (r.returncode == 1) == bool(re.search(r"line \d+: ", r.stderr)), (which, name, r.stdout, r.stderr)
            n += 1
        assert subprocess.run([exe, path, "0", "--read"], capture_output=True, text=True).returncode == 0
    assert n > 200
