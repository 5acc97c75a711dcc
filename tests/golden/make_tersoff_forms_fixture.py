"""Writes the parameter files of the Tersoff forms' tests next to itself: Si.tersoff.mod, Si.tersoff.modc and SiC.tersoff.zbl.  None comes
from LAMMPS or from the project this one was modelled on, and physical accuracy is not what the tests pin.

  Si.tersoff.mod   the silicon numbers of Kumagai, Izumi, Hara, Sakai (Comp. Mater. Sci. 39, 457 (2007)) as remembered: diamond at
                   5.429 A gives -4.630 eV per atom, the paper's cohesive energy
  Si.tersoff.modc  the same entry with an 18th number, c0 = -0.0251 eV (an arbitrary non-zero shift)
  SiC.tersoff.zbl  the eight entries of SiC.tersoff, each extended by Z_i Z_j ZBLcut ZBLexpscale = Z Z 0.95 14.0 (Z = 14 for Si, 6 for C)

Run from anywhere: python tests/golden/make_tersoff_forms_fixture.py
"""
import os

HERE = os.path.dirname(os.path.abspath(__file__))
KUMAGAI = "1.0 2.3890327 -0.365 1.0 1.0 1.345797 121.00047 3.0 0.3 3.2300135 3281.5905 0.93810551 0.20173476 730418.72 1000000.0 1.0 26.0"
COLUMNS = "# El El El  beta alpha h eta beta_ters lambda2 B R D lambda1 A n c1 c2 c3 c4 c5"
Z = {"Si": "14", "C": "6"}


def main():
    with open(os.path.join(HERE, "Si.tersoff.mod"), "w") as f:
        f.write("# tersoff/mod fixture of the tests: silicon, the numbers of Kumagai et al. (2007) as remembered; energies in eV\n")
        f.write(COLUMNS + "\nSi Si Si " + KUMAGAI + "\n")
    with open(os.path.join(HERE, "Si.tersoff.modc"), "w") as f:
        f.write("# tersoff/mod/c fixture of the tests: Si.tersoff.mod with an arbitrary c0; energies in eV\n")
        f.write(COLUMNS + " c0\nSi Si Si " + KUMAGAI + " -0.0251\n")
    words = []
    for line in open(os.path.join(HERE, "SiC.tersoff")):
        words += line.split("#")[0].split()
    assert len(words) == 8 * 17
    with open(os.path.join(HERE, "SiC.tersoff.zbl"), "w") as f:
        f.write("# tersoff/zbl fixture of the tests: the entries of SiC.tersoff, each extended by Z_i Z_j ZBLcut ZBLexpscale\n")
        for t in range(0, len(words), 17):
            e = words[t:t + 17]
            f.write(" ".join(e + [Z[e[0]], Z[e[1]], "0.95", "14.0"]) + "\n")


if __name__ == "__main__":
    main()
