"""Writes tests/golden/Si.edip and tests/golden/SiC.edip next to itself, in the format of LAMMPS `pair_style edip` / `edip/multi`: three
element names, then A B cutoffA cutoffC alpha beta eta gamma lambda mu rho sigma Q0 u1 u2 u3 u4; units metal (eV, A).

Provenance.  Si.edip holds the constants published in J. F. Justo, M. Z. Bazant, E. Kaxiras, V. V. Bulatov and S. Yip, "Interatomic
potential for silicon defects and disordered phases", Phys. Rev. B 58, 2539 (1998), table I.  The check that a slip would show in: with
these numbers the diamond lattice has -4.649953 eV per atom at 5.430 A, its minimum between 5.42 and 5.44 A and C11 = 172.04 GPa
(tests/edip_numpy.py, pinned by tests/test_edip_host.py); the paper gives -4.650 eV, 5.430 A and 172 GPa.

SiC.edip is SYNTHETIC: no material.  It comes neither from the reference nor from LAMMPS nor from any paper; its numbers were made up
for the tests around those of silicon so that every pair (Si Si, C C, Si C, C Si) and every unordered triplet has numbers of its own and a
wrong index shows.  It obeys the two rules the reader demands: entries i j k and i k j agree in their eight triplet numbers, and entries
i j j and j i i agree in cutoffA.  The pair numbers of an entry i j k with j != k are never read and stand as zeros.

  python tests/golden/make_edip_fixture.py
"""
import os

ORDER = ["A", "B", "cutoffA", "cutoffC", "alpha", "beta", "eta", "gamma", "lambda", "mu", "rho", "sigma", "Q0", "u1", "u2", "u3", "u4"]
SI = "7.9821730 1.5075463 3.1213820 2.5609104 3.1083847 0.0070975 0.2523244 1.1247945 1.4533108 0.6966326 1.2085196 0.5774108 312.1341346 -0.165799 32.557 0.286198 0.66"

# the synthetic file: pair numbers per (i, j), triplet numbers per (i, {j, k})
PAIR = {("Si", "Si"): dict(A=7.98, B=1.51, cutoffA=3.12, cutoffC=2.56, alpha=3.11, beta=0.0071, gamma=1.12, rho=1.21, sigma=0.58),
        ("C", "C"): dict(A=9.5, B=1.30, cutoffA=2.95, cutoffC=2.30, alpha=2.6, beta=0.012, gamma=0.95, rho=1.45, sigma=0.47),
        ("Si", "C"): dict(A=8.7, B=1.40, cutoffA=3.05, cutoffC=2.45, alpha=2.9, beta=0.009, gamma=1.05, rho=1.30, sigma=0.52),
        ("C", "Si"): dict(A=8.2, B=1.45, cutoffA=3.05, cutoffC=2.40, alpha=3.3, beta=0.010, gamma=1.00, rho=1.25, sigma=0.55)}
TRIP = {("Si", "SiSi"): dict(eta=0.25, Q0=312.0, mu=0.70, u1=-0.166, u2=32.5, u3=0.286, u4=0.66, **{"lambda": 1.45}),
        ("Si", "CSi"): dict(eta=0.27, Q0=290.0, mu=0.60, u1=-0.160, u2=30.0, u3=0.280, u4=0.67, **{"lambda": 1.55}),
        ("Si", "CC"): dict(eta=0.28, Q0=280.0, mu=0.62, u1=-0.150, u2=29.0, u3=0.290, u4=0.68, **{"lambda": 1.70}),
        ("C", "SiSi"): dict(eta=0.22, Q0=300.0, mu=0.66, u1=-0.140, u2=31.0, u3=0.270, u4=0.64, **{"lambda": 1.60}),
        ("C", "CSi"): dict(eta=0.24, Q0=270.0, mu=0.58, u1=-0.130, u2=27.0, u3=0.295, u4=0.69, **{"lambda": 1.75}),
        ("C", "CC"): dict(eta=0.31, Q0=250.0, mu=0.55, u1=-0.120, u2=25.0, u3=0.300, u4=0.70, **{"lambda": 1.90})}


def si_lines():
    return ["# EDIP for silicon: Justo, Bazant, Kaxiras, Bulatov, Yip, Phys. Rev. B 58, 2539 (1998), table I",
            "# written by tests/golden/make_edip_fixture.py from the published numbers; units metal (eV, A)",
            "# el1 el2 el3  " + " ".join(ORDER),
            "Si Si Si  " + SI]


def sic_lines():
    out = ["# SYNTHETIC two-element EDIP file for the tests: no material.  It comes neither from the reference nor from LAMMPS nor from a paper;",
           "# every pair and every unordered triplet has made-up numbers of its own.  Written by tests/golden/make_edip_fixture.py; units metal",
           "# el1 el2 el3  " + " ".join(ORDER)]
    for i in ("Si", "C"):
        for j in ("Si", "C"):
            for k in ("Si", "C"):
                v = dict.fromkeys(ORDER, 0.0)
                if j == k:
                    v.update(PAIR[(i, j)])
                v.update(TRIP[(i, "".join(sorted((j, k))))])
                out.append(f"{i:2s} {j:2s} {k:2s}  " + " ".join(f"{v[n]:g}" for n in ORDER))
    return out


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    for name, lines in (("Si.edip", si_lines()), ("SiC.edip", sic_lines())):
        with open(os.path.join(here, name), "w") as f:
            f.write("\n".join(lines) + "\n")
        print(os.path.join(here, name))
