"""Writes tests/golden/SiC.vashishta next to itself: the eight entries of the Vashishta potential for silicon carbide in the format of
LAMMPS `pair_style vashishta` (three element names, then H eta Zi Zj lambda1 D lambda4 W rc B gamma r0 C costheta0; units metal).

Provenance.  The numbers are those published in P. Vashishta, R. K. Kalia, A. Nakano and J. P. Rino, "Interaction potential for silicon
carbide: a molecular dynamics study of elastic constants and vibrational density of states for crystalline and amorphous silicon
carbide", J. Appl. Phys. 101, 103515 (2007), table I, written down from memory of the paper; the file was composed here and copied
neither from LAMMPS nor from any other program.  The check that a slip would show in: with these numbers zincblende SiC at a = 4.3581 A
has -6.34014 eV per atom (tests/vashishta_numpy.py, pinned by tests/test_vashishta_host.py), the paper's cohesive energy of 6.34 eV.

  python tests/golden/make_vashishta_fixture.py
"""
import os

Z = {"Si": 1.201, "C": -1.201}
LAMBDA1, LAMBDA4, RC = 5.0, 3.0, 7.35
# pair -> H (eV A^eta), eta, D (eV A^4), W (eV A^6)
PAIR = {("Si", "Si"): (23.67291, 7, 15.575, 0.0), ("C", "C"): (471.74538, 7, 0.0, 0.0), ("Si", "C"): (447.09026, 9, 7.7874, 61.4694)}
# the two live triplets: B (eV), gamma (A), r0 (A), C, cos(theta0)
THREE = (9.003, 1.0, 2.90, 5.0, -1.0 / 3.0)


def lines():
    out = ["# Vashishta potential for SiC: Vashishta, Kalia, Nakano, Rino, J. Appl. Phys. 101, 103515 (2007), table I",
           "# written by tests/golden/make_vashishta_fixture.py from the published numbers; units metal (eV, A)",
           "# el1 el2 el3  H eta Zi Zj lambda1 D lambda4 W rc  B gamma r0 C costheta0"]
    for i in ("Si", "C"):
        for j in ("Si", "C"):
            for k in ("Si", "C"):
                if j == k:
                    h, eta, d, w = PAIR[(i, j)] if (i, j) in PAIR else PAIR[(j, i)]
                    two = f"{h:.5f} {eta:d} {Z[i]:.3f} {Z[j]:.3f} {LAMBDA1:.1f} {d:.4f} {LAMBDA4:.1f} {w:.4f} {RC:.2f}"
                else:
                    two = "0.0 0 0.0 0.0 0.0 0.0 0.0 0.0 0.0"
                if j == k and i != j:
                    b, g, r0, c, c0 = THREE
                    three = f"{b:.3f} {g:.1f} {r0:.2f} {c:.1f} {c0:.12f}"
                else:
                    three = "0.0 0.0 0.0 0.0 0.0"
                out.append(f"{i:2s} {j:2s} {k:2s}  {two}  {three}")
    return out


if __name__ == "__main__":
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "SiC.vashishta")
    with open(path, "w") as f:
        f.write("\n".join(lines()) + "\n")
    print(path)
