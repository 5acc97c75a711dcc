"""Writes tests/golden/NaCl.born_long and tests/golden/MgO.buck_long next to itself: script fragments of LAMMPS `pair_style born/coul/long`
and `pair_style buck/coul/long` with their `kspace_style` line (the styles have no parameter file: the parameters are the script lines
themselves).

Provenance.  Both files were written for this project; neither comes from LAMMPS or from the reference.

  NaCl.born_long .. the constants of NaCl.born_dsf (Born-Mayer-Huggins in the Tosi-Fumi form for sodium chloride, type 1 Na, type 2 Cl,
                    WRITTEN FROM MEMORY, pinning nothing physical) under `pair_style born/coul/long 10.0` and `kspace_style ewald 1.0e-5`;
                    charges +1 and -1 belong to the replica, not to the file.
  MgO.buck_long ... SYNTHETIC, no material: `buck/coul/long` in the Buckingham form `pair_coeff I J A rho C [cut_lj]` with a per-pair
                    cut_lj below the style's, cut_coul 9 A while cut_lj is 8 A, `kspace_style pppm 1.0e-4` (honoured as the Ewald sum at
                    that accuracy), `units metal`; the replica supplies charges of +1.2 and -1.2.

  python tests/golden/make_born_long_fixture.py
"""
import os

HERE = os.path.dirname(os.path.abspath(__file__))

NACL = """# NaCl.born_long -- pair_style born/coul/long for sodium chloride, type 1 Na (+1), type 2 Cl (-1)
# written for this project by tests/golden/make_born_long_fixture.py: the constants of NaCl.born_dsf, Tosi-Fumi (Born-Mayer-Huggins)
# WRITTEN FROM MEMORY, neither from LAMMPS nor from the reference; they pin nothing physical
units metal
pair_style born/coul/long 10.0
kspace_style ewald 1.0e-5
#          I J  A (eV)  rho (A)  sigma (A)  C (eV A^6)  D (eV A^8)
pair_coeff 1 1  0.2637  0.317    2.340      1.05        -0.499
pair_coeff 1 2  0.2110  0.317    2.755      6.99        -8.676
pair_coeff 2 2  0.1582  0.317    3.170      72.40       -145.427
"""

MGO = """# MgO.buck_long -- SYNTHETIC fragment of pair_style buck/coul/long for the tests (no material): type 1 Mg (+1.2), type 2 O (-1.2)
# written for this project by tests/golden/make_born_long_fixture.py: neither from LAMMPS nor from the reference, not physically accurate
units metal
pair_style buck/coul/long 8.0 9.0     # cut_lj, cut_coul
kspace_style pppm 1.0e-4              # (honoured as the Ewald sum at this accuracy)
#          I J  A (eV)    rho (A)  C (eV A^6)  [cut_lj]
pair_coeff 1 1  0.0       0.3000   0.0
pair_coeff 1 2  1284.38   0.2997   0.0         7.0
pair_coeff 2 2  9547.96   0.2192   32.0
timestep 1.0                          # (any other command is ignored)
"""

if __name__ == "__main__":
    for name, text in (("NaCl.born_long", NACL), ("MgO.buck_long", MGO)):
        with open(os.path.join(HERE, name), "w") as f:
            f.write(text)
        print("wrote", name)
