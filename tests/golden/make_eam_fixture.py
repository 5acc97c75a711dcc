"""Writes tests/golden/CuAg.eam.alloy, the DYNAMO setfl file of the embedded-atom tests: two elements, Nrho = Nr = 500, cutoff 5.5 A.

The functions are Johnson's analytic nearest-neighbour EAM (R. A. Johnson, Phys. Rev. B 37, 3924 (1988); alloy pair term: Phys. Rev. B
39, 12554 (1989)) as tests/eam_numpy.py states it (JOHNSON, johnson_tables), carried out to the cutoff and multiplied by a switching
function that takes value and slope to zero there.  Written for this project: the file comes neither from the project this one was
modelled on nor from LAMMPS, and physical accuracy is not what the tests pin.

    python tests/golden/make_eam_fixture.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import eam_numpy as en  # noqa: E402


def main():
    names = ["Cu", "Ag"]
    pars = "; ".join("%s: " % a + " ".join("%s=%g" % (k, en.JOHNSON[a][k]) for k in ("a", "Ec", "fe", "phie", "alpha", "beta", "gamma")) for a in names)
    header = ["Analytic EAM of the Johnson form (Phys. Rev. B 37, 3924 (1988); alloys 39, 12554 (1989)), switched off between %.1f and %.1f A by 1 - 3t^2 + 2t^3"
              % (en.SWITCH_ON, en.CUTOFF),
              pars,
              "written by tests/golden/make_eam_fixture.py for this project's tests: not from LAMMPS, not from any other project; units metal (eV, A)"]
    en.write_johnson(os.path.join(HERE, "CuAg.eam.alloy"), names, header)


if __name__ == "__main__":
    main()
