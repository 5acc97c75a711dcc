"""The builder of the host drivers (tests/*_host_driver.cpp, each compiled together with the product's reader of its potential) and the
comparison that the stand-alone drivers share.  A plain module, imported like the numpy restatements.

build() decides staleness from what the compiler says it read, not from a list typed by hand: a header that a driver includes but
nobody listed used to leave a stale driver in tests/_build, and the test then pinned old arithmetic.
"""
import os
import shlex
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "_build")
FLAGS = ["-O2", "-ffp-contract=off", "-std=c++17"]


def _stale(out, cmdline):
    dep, rec = out + ".d", out + ".cmd"
    if not (os.path.exists(out) and os.path.exists(dep) and os.path.exists(rec)) or open(rec).read() != cmdline:
        return True
    built = os.path.getmtime(out)
    names = [w for w in open(dep).read().replace("\\\n", " ").split() if not w.endswith(":")]
    return any(not os.path.exists(n) or os.path.getmtime(n) > built for n in names)


def build(name, sources, *, shared, defines=(), flags=()):
    """Compile `sources` (paths below the repository root) into tests/_build/<name> -- a library for ctypes when `shared`, a program
    otherwise -- and return its path.  defines: -D switches of the driver (`VSH_WRONG=2`); flags: further compiler flags of one driver.
    Rebuilt when the output, its dependency file or its recorded command line is missing, when the command line differs from the
    recorded one, or when any file the compiler read is newer than the output.  The dependency file comes from a -MM pass over all
    sources with the same flags (-MMD -MF on the compiling command itself records the last source only when there are several)"""
    os.makedirs(OUT, exist_ok=True)
    out = os.path.join(OUT, name)
    srcs = [os.path.join(ROOT, s) for s in sources]
    common = ["g++"] + FLAGS + [f"-D{d}" for d in defines] + list(flags) + ["-I", os.path.join(ROOT, "include")]
    cmd = common + (["-fPIC", "-shared"] if shared else []) + ["-o", out] + srcs
    cmdline = shlex.join(cmd)
    if _stale(out, cmdline):
        subprocess.check_call(cmd)
        deps = subprocess.run(common + ["-MM"] + srcs, capture_output=True, text=True, check=True).stdout
        with open(out + ".d", "w") as f:
            f.write(deps)
        with open(out + ".cmd", "w") as f:
            f.write(cmdline)
    return out


def mismatch(got, ref, *, counters, energies, tol, scale=None, energy_scale=(), energy_scale_of_scale=False, virial_parts=()):
    """What differs beyond tol between a driver's result and the reference's: a list out of "counts", "forces", "energy", "virial".
    counters are compared exactly; forces, each of `energies` and the virial relative to the largest force component, energy term and
    virial component of ref, or, for forces and virial, of `scale` (a perfect cell, whose forces and virial cancel, is measured on its
    jittered twin).  energy_scale: the keys whose largest sets the energy scale where they are not `energies` (a key that a result lacks
    counts as zero); energy_scale_of_scale: take that scale from `scale` too; virial_parts: keys of `scale` whose largest sets the virial
    scale where `scale` has them (a virial that is a difference of large parts is held on the scale of the parts)"""
    bad = []
    scale = scale or ref
    if tuple(got[k] for k in counters) != tuple(ref[k] for k in counters):
        bad.append("counts")
    if not np.abs(got["f"] - ref["f"]).max() <= tol * max(np.abs(scale["f"]).max(), 1e-300):
        bad.append("forces")
    src = scale if energy_scale_of_scale else ref
    es = max([abs(src.get(k, 0.0)) for k in (energy_scale or energies)] + [1e-300])
    if not all(abs(got[k] - ref[k]) <= tol * es for k in energies):
        bad.append("energy")
    ws = max(np.abs(scale[k]).max() for k in virial_parts) if virial_parts and virial_parts[0] in scale else np.abs(scale["w"]).max()
    if not np.abs(got["w"] - ref["w"]).max() <= tol * max(ws, 1e-300):
        bad.append("virial")
    return bad
