"""Writes tests/golden/CuAg.adp, the extended setfl file of the angular-dependent-potential tests: two elements, Nrho = 200, Nr = 280,
cutoff 5.5 A.

The embedded-atom part is Johnson's analytic EAM as tests/eam_numpy.py states it (the functions behind CuAg.eam.alloy, on a coarser
grid so that this file is no larger than that one); u and w are decaying exponentials times the same switching function, with an
amplitude of its own for every pair (tests/adp_numpy.py: ANGULAR, u_of, w_of).  Written for this project: the file comes neither from
the project this one was modelled on nor from LAMMPS, and physical accuracy is not what the tests pin.

    python tests/golden/make_adp_fixture.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import adp_numpy as an  # noqa: E402


def main():
    names = ["Cu", "Ag"]
    amps = "; ".join("%s-%s: U=%g W=%g" % (a, b, *an.ANGULAR[(a, b)]) for a, b in sorted(an.ANGULAR))
    header = ["Analytic ADP: EAM of the Johnson form (Phys. Rev. B 37, 3924 (1988); 39, 12554 (1989)) plus u = U exp(-%g (r/2.7 - 1)), w = W exp(-%g (r/2.7 - 1)), "
              "all switched off between %.1f and %.1f A by 1 - 3t^2 + 2t^3" % (an.U_DECAY, an.W_DECAY, an.en.SWITCH_ON, an.CUTOFF),
              amps,
              "written by tests/golden/make_adp_fixture.py for this project's tests: not from LAMMPS, not from any other project; units metal (eV, A)"]
    an.write_fixture(os.path.join(HERE, "CuAg.adp"), names, header)


if __name__ == "__main__":
    main()
