"""Writes the fixtures of the EAM + long-range Coulomb stage (`pair_style hybrid/overlay coul/long <cut_coul> eam/alloy`) next to itself:

  UO2.eam.alloy ........ a DYNAMO setfl file of two elements, O and U, Nrho = Nr = 500 (the sizes of CuAg.eam.alloy), setfl cutoff 7.0 A:
                         analytic functions in the SHAPE of the many-body oxide models of Cooper, Rushton and Grimes (J. Phys.: Condens.
                         Matter 26, 105401 (2014)) as tests/eam_coul_numpy.py states them (CRG, crg_tables): phi = Buckingham + Morse,
                         rho(r) = n / r^8 with an erf switch at short range, F = -G sqrt(rho), every function evaluated no closer than
                         0.6 A and taken smoothly to value 0 and slope 0 at the cutoff (1 - 3t^2 + 2t^3 from 6.0 A on)
  UO2.eam_coul ......... script lines with `coul/long 9.0`, larger than the setfl cutoff, `kspace_style ewald 1.0e-5`, `units metal`
  UO2_short.eam_coul ... `coul/long 6.0`, smaller than the setfl cutoff, `kspace_style pppm 1.0e-4`, the sub-styles in the other order

Provenance.  All three were written for this project and are SYNTHETIC: nothing comes from LAMMPS or from the reference, the constants
are WRITTEN FROM MEMORY and pin nothing physical.  The charges belong to the replica: U +2.2208, O -1.1104.

    python tests/golden/make_eam_coul_fixture.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import eam_coul_numpy as ec  # noqa: E402
import eam_numpy as en  # noqa: E402

LONG = """# UO2.eam_coul -- SYNTHETIC script lines of pair_style hybrid/overlay coul/long eam/alloy for the tests: type 1 O (-1.1104), type 2 U (+2.2208)
# written for this project by tests/golden/make_eam_coul_fixture.py: neither from LAMMPS nor from the reference; constants WRITTEN FROM
# MEMORY, they pin nothing physical
units metal
pair_style hybrid/overlay coul/long 9.0 eam/alloy     # cut_coul above the setfl cutoff of 7.0 A
pair_coeff * * coul/long
pair_coeff * * eam/alloy UO2.eam.alloy O U
kspace_style ewald 1.0e-5
"""

SHORT = """# UO2_short.eam_coul -- SYNTHETIC script lines of pair_style hybrid/overlay eam/alloy coul/long for the tests: type 1 O, type 2 U
# written for this project by tests/golden/make_eam_coul_fixture.py: neither from LAMMPS nor from the reference; constants WRITTEN FROM
# MEMORY, they pin nothing physical
pair_style hybrid/overlay eam/alloy coul/long 6.0     # cut_coul below the setfl cutoff of 7.0 A; the sub-styles in the other order
pair_coeff * * eam/alloy ${locs}/UO2.eam.alloy O U
pair_coeff * * coul/long
kspace_style pppm 1.0e-4
timestep 1.0                                          # (any other command is ignored)
"""


def main():
    names = ["O", "U"]
    header = ["SYNTHETIC many-body oxide tables in the shape of Cooper, Rushton and Grimes (2014): phi = Buckingham + Morse, rho = n/r^8 with an erf switch, F = -G sqrt(rho)",
              "evaluated no closer than %.1f A, switched off between %.1f and %.1f A by 1 - 3t^2 + 2t^3; constants WRITTEN FROM MEMORY, they pin nothing physical"
              % (ec.R_FLOOR, ec.SWITCH_ON, ec.CUTOFF),
              "written by tests/golden/make_eam_coul_fixture.py for this project's tests: not from LAMMPS, not from any other project; units metal (eV, A)"]
    en.write_setfl(os.path.join(HERE, "UO2.eam.alloy"), names, [ec.CRG["Z"][a] for a in names], [ec.CRG["mass"][a] for a in names], [ec.A_UO2] * 2,
                   *ec.crg_tables(names), header)
    for name, text in (("UO2.eam_coul", LONG), ("UO2_short.eam_coul", SHORT)):
        with open(os.path.join(HERE, name), "w") as f:
            f.write(text)
    print("wrote UO2.eam.alloy, UO2.eam_coul, UO2_short.eam_coul")


if __name__ == "__main__":
    main()
