"""Writes tests/golden/NaCl.born_dsf and tests/golden/KNaCl.born_dsf next to itself: script fragments of LAMMPS `pair_style born/coul/dsf`
(the style has no parameter file: the parameters are the script lines themselves).

Provenance.  Both files were written for this project; neither comes from LAMMPS or from the reference.

  NaCl.born_dsf ... `units metal`, `pair_style born/coul/dsf 0.25 10.0`, and Born-Mayer-Huggins constants in the Tosi-Fumi form for sodium
                    chloride (type 1 Na, type 2 Cl; charges +1 and -1 belong to the replica, not to the file).  The constants are WRITTEN
                    FROM MEMORY and pin nothing physical; with them numpy gives a rock-salt minimum at a = 5.62-5.64 A, -185.7 kcal/mol
                    per ion pair there, and a Madelung constant -E_coul (a/2)/K of 1.74710 at a = 5.64 A (exact: 1.747565).
  KNaCl.born_dsf .. SYNTHETIC, no material: a third type, per-pair cut_lj of 7, 8 and 9 A, cut_coul 10 A while pair_style says cut_lj 8,
                    a `*` line that later lines override, so that the tests reach every path of the reader and the kernel.

  python tests/golden/make_born_dsf_fixture.py
"""
import os

HERE = os.path.dirname(os.path.abspath(__file__))

NACL = """# NaCl.born_dsf -- pair_style born/coul/dsf for sodium chloride, type 1 Na (+1), type 2 Cl (-1)
# written for this project by tests/golden/make_born_dsf_fixture.py: Tosi-Fumi (Born-Mayer-Huggins) constants WRITTEN FROM MEMORY,
# neither from LAMMPS nor from the reference; they pin nothing physical
units metal
pair_style born/coul/dsf 0.25 10.0
#          I J  A (eV)  rho (A)  sigma (A)  C (eV A^6)  D (eV A^8)
pair_coeff 1 1  0.2637  0.317    2.340      1.05        -0.499
pair_coeff 1 2  0.2110  0.317    2.755      6.99        -8.676
pair_coeff 2 2  0.1582  0.317    3.170      72.40       -145.427
"""

KNACL = """# KNaCl.born_dsf -- SYNTHETIC three-type fragment of pair_style born/coul/dsf for the tests (no material)
# written for this project by tests/golden/make_born_dsf_fixture.py: neither from LAMMPS nor from the reference, not physically accurate
units metal
pair_style born/coul/dsf 0.20 8.0 10.0   # alpha, cut_lj, cut_coul
pair_coeff * * 0.2000 0.330 2.900 10.00 -12.000        # every pair, at the style's cut_lj of 8; the lines below override
pair_coeff 1 1 0.2637 0.317 2.340 1.05 -0.499 7.0
pair_coeff 1 2 0.2110 0.317 2.755 6.99 -8.676          # cut_lj 8
pair_coeff 2 2 0.1582 0.317 3.170 72.40 -145.427 9.0
pair_coeff 1 3 0.2300 0.335 2.800 3.10 -2.400 9.0
pair_coeff 3 3 0.2110 0.337 3.260 24.30 -24.000 7.0
timestep 1.0                                           # (any other command is ignored)
"""

if __name__ == "__main__":
    for name, text in (("NaCl.born_dsf", NACL), ("KNaCl.born_dsf", KNACL)):
        with open(os.path.join(HERE, name), "w") as f:
            f.write(text)
        print("wrote", name)
