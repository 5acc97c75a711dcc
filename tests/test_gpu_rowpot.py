"""What the three potentials on full neighbour rows (Stillinger-Weber, Tersoff, eam/alloy) share on the host side: the order in which an
update that mixes their materials is refused.  The refusal names the kind that comes first in the order Stillinger-Weber, Tersoff, EAM,
whatever the order of the simulations in the list, with that kind's count.
"""
import os
import re

import numpy as np
import pytest

import eam_numpy as en
import tersoff_numpy as tsn
from scema_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUAG = os.path.join(ROOT, "tests", "golden", "CuAg.eam.alloy")
SIC = os.path.join(ROOT, "tests", "golden", "SiC.tersoff")
SI_SW = os.path.join(ROOT, "tests", "golden", "Si.sw")


def test_mixed_kinds_are_refused_in_table_order():
    """three materials on one engine (the 8-atom diamond cell under Si.sw and under SiC.tersoff, the 4-atom fcc cell under CuAg.eam.alloy,
    each as a cluster in the 30 A box); the three pairs of kinds in both orders of the list; no state after a refusal; each alone runs"""
    xs = tsn.diamond(1, 1, 1, tsn.A_SI)[0] + 12.0
    xc = en.fcc(1, 1, 1, en.A_CU)[0] + 12.0
    box = tsn.BIG_BOX.copy()
    e = capi.Engine(capi.default_params())
    try:
        e.sw_configure("sw", SI_SW)
        e.tersoff_configure("ts", SIC)
        e.eam_configure("cu", CUAG)
        e.register_replica("sw", 1, capi.bare_system(tsn.zeros(8), xs, box))
        e.register_replica("ts", 1, capi.bare_system(tsn.zeros(8), xs, box))
        e.register_replica("cu", 1, capi.bare_system(en.zeros(4), xc, box, masses=(en.CU_MASS,)))
        s = np.array([1e-3 * 30.0, 0.0, 0.0, 0.0, 0.0, 0.0])
        mk = lambda q, m: capi.make_sim(q, m, 1, s, nss=10, most_recent=capi.QP_NONE)
        expect = {("sw", "ts"): "Stillinger-Weber", ("sw", "cu"): "Stillinger-Weber", ("ts", "cu"): "Tersoff"}
        for (a, b), name in expect.items():
            msg = f"one update mixes {name} materials (1 of 2 simulations) with others"
            for first, second in ((a, b), (b, a)):
                with pytest.raises(capi.EngineError, match="rc=1.*" + re.escape(msg)) as info:
                    e.strain_batch([mk(0, first), mk(1, second)])
                print(f"{first} + {second}: {info.value}")
                assert not e.has_state(0, first, 1) and not e.has_state(1, second, 1)
        for q, m in enumerate(("sw", "ts", "cu")):
            assert e.strain_batch([mk(q, m)])[0].stress_updated == 1
            assert e.has_state(q, m, 1)
    finally:
        e.close()
