"""A corpus of truncated and bit-flipped `hybrid/overlay coul/long eam/alloy` scripts, and of truncated and garbled copies of the setfl
file they name, through the reader (scema_md_eam_coul_read_params, no GPU): it never crashes, a script it takes yields a sane head, and
every refusal of a script names a line while every refusal of the setfl file carries the setfl reader's own message.  The same corpus
goes through the stand-alone driver (tests/eam_coul_host_driver.cpp), which also holds the block's BlTable prefix and EAM offsets
against what the kernels assume."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import hostdrv
from scema_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SETFL = os.path.join(GOLDEN, "UO2.eam.alloy")
FILES = {"long": os.path.join(GOLDEN, "UO2.eam_coul"), "short": os.path.join(GOLDEN, "UO2_short.eam_coul")}


def driver_exe():
    return hostdrv.build("eam_coul_host_driver", ["tests/eam_coul_host_driver.cpp", "scema_amd/csrc/host/eam_coul_params.cpp", "scema_amd/csrc/host/eam_setfl.cpp"],
                         shared=False)


def script_corpus(which):
    """(name, bytes): the script cut at some 80 places, and with one bit flipped at 240 places (seeded), three quarters of them in the
    lines that are read"""
    data = open(FILES[which], "rb").read()
    rng = np.random.default_rng(41 if which == "long" else 42)
    out = []
    for cut in sorted(set(int(c) for c in np.concatenate([np.arange(0, 40), rng.integers(0, len(data), 40), [len(data) - 1, len(data) - 2]]))):
        out.append((f"cut{cut}", data[:cut]))
    first = data.index(b"pair_style") if which == "short" else data.index(b"units")
    for k in range(240):
        pos = int(rng.integers(first if k % 4 else 0, len(data)))
        b = bytearray(data)
        b[pos] ^= 1 << int(rng.integers(0, 8))
        out.append((f"flip{k}_{pos}", bytes(b)))
    return out


def setfl_corpus():
    """(name, bytes): the setfl file cut at 40 places (in its head, in F, in rho, in r phi), with a word replaced by garbage at 30
    places, and with a count of its head changed"""
    data = open(SETFL, "rb").read()
    rng = np.random.default_rng(43)
    out = [(f"cut{c}", data[:c]) for c in sorted(set(int(c) for c in np.concatenate([np.arange(0, 600, 60), rng.integers(0, len(data), 30)])))]
    head = data.index(b"2 O U")
    for k in range(30):
        pos = int(rng.integers(head, len(data) - 8))
        out.append((f"junk{k}_{pos}", data[:pos] + b" x?\xff " + data[pos + 4:]))
    for k, (a, b) in enumerate([(b"500 ", b"5000000 "), (b"500 ", b"4 "), (b"2 O U", b"9 O U"), (b" 7\n", b" 70\n"), (b"500 ", b"-500 ")]):
        assert a in data
        out.append((f"head{k}", data.replace(a, b, 1)))
    return out


def _sane(tab):
    return tab["cut_coul"] > 0.0 and tab["cutmax"] >= max(tab["cut_coul"], tab["cutoff"]) and 0.0 < tab["accuracy"] < 1.0 and tab["K"] > 0.0 and \
        all(0 <= t < 4 for t in tab["type_map"])


@pytest.mark.parametrize("which", sorted(FILES))
def test_the_script_reader_never_crashes_and_every_refusal_names_a_line(tmp_path, which):
    shutil.copy(SETFL, tmp_path / "UO2.eam.alloy")
    taken = refused = 0
    for name, data in script_corpus(which):
        p = tmp_path / (name + ".eam_coul")
        p.write_bytes(data)
        try:
            tab = capi.eam_coul_read_params(str(p))
        except IOError as err:
            refused += 1
            # (a flipped bit in the file name or an element: the setfl reader's message, which names the file and not a line)
            assert re.search(r"line \d+: ", str(err)) or re.search(r"(cannot open|is not in the file)", str(err)), (name, str(err))
            continue
        taken += 1
        assert _sane(tab), (name, tab)
    print(f"{which}: {taken} scripts taken, {refused} refused")
    assert refused > 60 and taken > 10      # (a flipped bit in a digit or in a comment leaves a readable script)


def test_a_corrupt_setfl_file_is_refused_with_the_setfl_readers_message(tmp_path):
    shutil.copy(FILES["long"], tmp_path / "UO2.eam_coul")
    taken = refused = 0
    for name, data in setfl_corpus():
        (tmp_path / "UO2.eam.alloy").write_bytes(data)
        try:
            tab = capi.eam_coul_read_params(str(tmp_path / "UO2.eam_coul"))
        except IOError as err:
            refused += 1
            assert "UO2.eam.alloy: " in str(err), (name, str(err))
            with pytest.raises(IOError) as own:
                capi.eam_read_setfl(str(tmp_path / "UO2.eam.alloy"), ["O", "U"])
            assert str(own.value) == str(err), name
            continue
        taken += 1
        assert _sane(tab) and name.startswith("junk"), (name, tab)      # (garbage that fell into the three comment lines or a lattice name)
    print(f"setfl: {taken} files taken, {refused} refused")
    assert refused > 60


def test_the_corpus_through_the_stand_alone_driver(tmp_path):
    """the stand-alone program over both fixtures and the corpus: exit status 0 (taken: the block is what the kernels assume) or 1 (refused
    with the reader's message), never 3 (a block that is not what the kernels assume) and never a crash"""
    exe = driver_exe()
    shutil.copy(SETFL, tmp_path / "UO2.eam.alloy")
    n = 0
    for which, path in FILES.items():
        r = subprocess.run([exe, path, "0"], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.startswith("ok 2 "), (r.stdout, r.stderr)
        w = r.stdout.split()
        assert (float(w[2]), float(w[3]), float(w[4])) == ((9.0, 9.0, 7.0) if which == "long" else (6.0, 7.0, 7.0)) and int(w[5]) % 4 == 0
        for name, data in script_corpus(which)[::3]:
            p = tmp_path / (which + name + ".eam_coul")
            p.write_bytes(data)
            r = subprocess.run([exe, str(p), "0"], capture_output=True, text=True, errors="replace")
            assert r.returncode in (0, 1), (which, name, r.returncode, r.stderr[-2000:])
            assert (r.returncode == 0) == r.stdout.startswith("ok ") and (r.returncode == 1) == bool(r.stderr.strip()), (which, name, r.stdout, r.stderr)
            n += 1
    shutil.copy(FILES["long"], tmp_path / "UO2.eam_coul")
    for name, data in setfl_corpus():
        (tmp_path / "UO2.eam.alloy").write_bytes(data)
        r = subprocess.run([exe, str(tmp_path / "UO2.eam_coul"), "0"], capture_output=True, text=True, errors="replace")
        assert r.returncode in (0, 1) and ((r.returncode == 1) == ("UO2.eam.alloy: " in r.stderr)), (name, r.returncode, r.stdout, r.stderr[-2000:])
        n += 1
    assert n > 250
