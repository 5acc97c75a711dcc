"""Writes tests/golden/Ti.meam.spline and tests/golden/TiO.meam.spline next to itself, in the two formats of LAMMPS `pair_style meam/spline`
(units metal: eV, A), from the analytic shapes stated in tests/meam_spline_numpy.py.

Provenance.  Both files are SYNTHETIC and were written for this project.  They come neither from LAMMPS nor from the reference nor from any
paper, and they are not physically accurate: smooth made-up shapes sampled at 8 to 16 knots, chosen so that the tests reach every path.

  Ti.meam.spline ... the old format: a comment line, then phi, rho, U, f, g, each as `N`, `d0 dN`, one line that is skipped, N lines
                     `x y y2`.  phi, f and g have non-uniform knots, rho and U uniform ones.
  TiO.meam.spline .. the new format: a comment line, `meam/spline 2 Ti O`, then phi (TiTi TiO OO), rho (Ti O), U (Ti O), f (Ti O), g (TiTi
                     TiO OO), each spline as `spline3eq`, `N`, `d0 dN`, N lines `x y y2`; every function has an amplitude of its own so
                     that a swapped index shows.

phi, rho and f end with value 0 and slope 0 (a factor (rc - r)^3); f's range (3.4 and 3.0 A) is clearly shorter than phi's (5.5 A).  U's
first knot lies below zero density, its first interior knot above the density of a distant pair and its last knot below that of a
compressed lattice.  g spans [-1, 1].  The third column holds the second derivatives of the clamped spline (readers here ignore it).

  python tests/golden/make_meam_spline_fixture.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import meam_spline_numpy as mn  # noqa: E402

NOTE = "SYNTHETIC, written for this project by tests/golden/make_meam_spline_fixture.py: neither from LAMMPS nor from the reference, not physically accurate"


def spline_lines(knots, shape, fresh):
    val, der = shape
    y = np.array([float(val(x)) for x in knots]) + 0.0      # (+ 0.0: no negative zero in the file)
    d0, dn = float(der(knots[0])) + 0.0, float(der(knots[-1])) + 0.0
    m = mn.Spline(knots, y, d0, dn).m
    out = (["spline3eq"] if fresh else []) + [str(len(knots)), f"{d0!r} {dn!r}"] + ([] if fresh else ["1 0 1 0"])
    return out + [f"{float(x)!r} {float(v)!r} {float(c)!r}" for x, v, c in zip(knots, y, m)]


def ti_lines():
    out = ["# Ti, old one-element format.  " + NOTE]
    for _, knots, shape in mn.TI_FUNCTIONS:
        out += spline_lines(knots, shape, False)
    return out


def tio_lines():
    out = ["# Ti-O, multi-element format.  " + NOTE, "meam/spline %d %s" % (len(mn.TIO_ELEMENTS), " ".join(mn.TIO_ELEMENTS))]
    for _, knots, shape in mn.TIO_FUNCTIONS:
        out += spline_lines(knots, shape, True)
    return out


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    for name, lines in (("Ti.meam.spline", ti_lines()), ("TiO.meam.spline", tio_lines())):
        with open(os.path.join(here, name), "w") as f:
            f.write("\n".join(lines) + "\n")
        print(os.path.join(here, name))
