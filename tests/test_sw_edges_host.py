"""The numpy Stillinger-Weber reference (tests/sw_numpy.py) on the inputs of tests/test_gpu_sw_edges.py, where it does what no earlier case asked
of it: boxes narrower than one cutoff, in which an atom is its own neighbour and both arms of a triplet may be images of one atom; boxes
tilted close to lx / 2; clusters at the kernel's limit of 32 neighbours.  No GPU needed.

  * supercell identity: the cell repeated 3 x 3 x 3 is a box above two list radii in which no atom meets an image of itself, and is the
    same crystal -- E / 27, W / 27 and the forces on the first n atoms must equal the single cell's to 1e-12.  This licenses the reference
    where it lists self images (measured on N1 to N3: energy 1e-15, forces 6e-15, virial 2e-14);
  * forces against central differences of the reference's own energy, as tests/test_sw_host.py does for its cases;
  * the counts the GPU tests rely on, pinned;
  * the host-compiled sw_core.h (tests/sw_host_driver.cpp) on the narrow boxes at 1e-12: sw_owns with j == i on the CPU.
"""

import numpy as np
import pytest

import sw_numpy as swn
from test_sw_host import SI_SW, Driver, driver_lib, same

NARROW = ["N1", "N2", "N3", "N4", "N5"]
# pairs, triplets, most neighbours inside the cutoff, row entries that name the row's own atom (summed over the atoms)
COUNTS = {"N1": (148, 1716, 17, 48), "N2": (31, 357, 13, 20), "N3": (21, 202, 12, 24), "N4": (3, 15, 6, 6), "N5": (125, 1213, 14, 48),
          "T3": (996, 8209, 11, 0), "T2": (294, 2412, 10, 0)}


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    p = tmp_path_factory.mktemp("sw_edges") / "two.sw"
    p.write_text(swn.TWO_ELEMENT_SW)
    return swn.SW(swn.read_sw(SI_SW, ["Si"])[0]), swn.SW(swn.read_sw(str(p), ["Si", "X"])[0]), str(p)


def _case(name):
    return swn.tilted(3) if name == "T3" else swn.tilted(2) if name == "T2" else swn.narrow(name)


def _self_entries(ref, x, box, t):
    return [sum(1 for j, _, _ in row if j == i) for i, row in enumerate(ref.neighbours(x, box, t))]


def test_conditions_on_the_boxes(refs):
    """what the generators assert from the box, and the widths the GPU tests count on: N1 two images deep in x alone, N2 in y and z, N3 in
    x and y; the 3 x 3 x 3 tilted box above two list radii (minimum image), the 2 x 2 x 2 one between one and two (one image deep)"""
    assert abs(swn.SI_CUT - refs[0].cutmax) < 1e-15 and refs[1].cutmax == refs[0].cutmax
    deep = lambda box: [0 if (swn.widths(box) >= 2 * swn.SI_RLIST).all() else int(np.ceil(swn.SI_RLIST / w)) for w in swn.widths(box)]
    want = {"N1": [2, 1, 1], "N2": [1, 2, 2], "N3": [2, 2, 1], "N4": [2, 2, 2], "N5": [2, 1, 1], "T3": [0, 0, 0], "T2": [1, 1, 1]}
    for name, m in want.items():
        x, box, t = _case(name)
        w = swn.check_box(box)
        assert deep(box) == m, (name, w)
    assert np.allclose(swn.widths(swn.narrow("N2")[1]), [8.02, 2.92, 3.40], atol=0.01)
    assert np.allclose(swn.widths(swn.tilted(3)[1]), [12.77, 14.86, 16.29], atol=0.01)
    assert np.allclose(swn.widths(swn.tilted(2)[1]), [8.51, 9.91, 10.86], atol=0.01)
    with pytest.raises(AssertionError):
        swn.check_box(np.array([0.0, 0.0, 0.0, 2.38, 3.3, 3.4, 0.0, 0.0, 0.0]))


def _second_image_entries(ref, x, box, t):
    """neighbours inside the cutoff that sit two box vectors from the partner as wrapped into the box: what a search one image deep misses"""
    Hi = np.linalg.inv(swn.h_matrix(box))
    s = (x - box[:3]) @ Hi
    assert (s >= 0.0).all() and (s < 1.0).all()
    count = 0
    for i, row in enumerate(ref.neighbours(x, box, t)):
        for j, _, d in row:
            shift = np.rint(d @ Hi - (s[j] - s[i]))
            assert np.abs(shift).max() <= 2
            count += int(np.abs(shift).max() == 2)
    return count


def test_second_image_neighbours(refs):
    """N2 and N3 each hold a pair inside the cutoff two box vectors deep (listed at both ends), so a row build that stops at the first image
    gives other forces.  N1 cannot: across 3.2 A with every image at least 2.1 A away, an atom's partner next to the opposite face has its
    nearest image at rho >= sqrt(2.1^2 - e^2) off the axis, e < 0.57 A, and the next one at sqrt((3.2 + e)^2 + rho^2) >= 3.83 A, beyond the
    cutoff of 3.77 A; there the second images only fill the skin of the rows (N4 likewise: its own images at 6.4 A and more)"""
    want = {"N1": 0, "N2": 2, "N3": 2, "N4": 0}
    for name, n2 in want.items():
        x, box, t = swn.narrow(name)
        assert _second_image_entries(refs[0], x, box, t) == n2, name


def test_gas_keeps_its_distance_to_every_image():
    for name in ("N1", "N2", "N3"):
        x, box, _ = swn.narrow(name)
        xs, _, _ = swn.supercell(x, box, np.zeros(len(x), int), 5)
        d = np.linalg.norm(xs[:, None, :] - xs[None, :, :], axis=2)
        d[np.diag_indices(len(xs))] = np.inf
        assert d.min() >= 2.1, (name, d.min())
        x2, _, _ = swn.narrow(name)
        assert np.array_equal(x, x2)          # deterministic


@pytest.mark.parametrize("name", NARROW + ["T2", "T3"])
def test_supercell_identity(refs, name):
    ref = refs[1] if name == "N5" else refs[0]
    x, box, t = _case(name)
    one = ref.compute(x, box, t)
    assert (one["npairs"], one["ntriplets"], one["maxin"], sum(_self_entries(ref, x, box, t))) == COUNTS[name]
    assert one["maxin"] <= 32
    xs, bs, ts = swn.supercell(x, box, t)
    assert (swn.widths(bs) >= 2 * ref.cutmax).all()      # no atom of the supercell is within the cutoff of an image of itself
    big = ref.compute(xs, bs, ts)
    n = len(x)
    assert big["npairs"] == 27 * one["npairs"] and big["ntriplets"] == 27 * one["ntriplets"] and big["maxin"] == one["maxin"]
    es = max(abs(one["e2"]), abs(one["e3"]))
    de = max(abs(big["e2"] / 27 - one["e2"]), abs(big["e3"] / 27 - one["e3"])) / es
    dw = np.abs(big["w"] / 27 - one["w"]).max() / np.abs(one["w"]).max()
    # (N4: the net force on the one atom is zero by symmetry; the scale is the largest single pair term)
    fs = max(np.abs(one["f"]).max(), largest_force_term(ref, x, box, t) if name == "N4" else 0.0)
    df = np.abs(big["f"][:n] - one["f"]).max() / fs
    print(f"sw supercell {name}: energy {de:.1e}, forces {df:.1e}, virial {dw:.1e}")
    assert de <= 1e-12 and df <= 1e-12 and dw <= 1e-12


def largest_force_term(ref, x, box, t):
    """the largest two-body force among the pairs of a configuration (silicon): the size of the terms that cancel in a symmetric one"""
    P = ref.pair(0, 0)
    r = np.array([np.linalg.norm(d) for row in ref.neighbours(x, box, t) for _, _, d in row])
    ex = np.exp(P["sigma"] / (r - P["a"] * P["sigma"]))
    poly = P["B"] * (P["sigma"] / r) ** P["p"] - (P["sigma"] / r) ** P["q"]
    dpoly = -P["p"] * P["B"] * P["sigma"] ** P["p"] * r ** (-P["p"] - 1) + P["q"] * P["sigma"] ** P["q"] * r ** (-P["q"] - 1)
    return float(np.abs(P["A"] * P["epsilon"] * ex * (dpoly - poly * P["sigma"] / (r - P["a"] * P["sigma"]) ** 2)).max())


@pytest.mark.parametrize("name", ["N1", "N4"])
def test_forces_are_the_gradient_of_the_energy_in_narrow_boxes(refs, name):
    """central differences, h = 1e-5 A, as tests/test_sw_host.py: truncation h^2 f''' / 6 ~ 1e-10 f, rounding 1e-16 E / h.  Moving an atom moves
    its images with it: in N4 every direction is a rigid translation, so the energy must not change and the force is zero"""
    ref = refs[0]
    x, box, t = swn.narrow(name)
    f = ref.compute(x, box, t)["f"]
    scale = max(np.abs(f).max(), largest_force_term(ref, x, box, t))
    rng = np.random.default_rng(3)
    h = 1e-5
    for _ in range(6):
        u = rng.normal(size=x.shape)
        u /= np.linalg.norm(u)
        num = -(ref.energy(x + h * u, box, t) - ref.energy(x - h * u, box, t)) / (2 * h)
        assert abs(num - np.sum(f * u)) < 1e-6 * scale, name
    if name == "N4":
        assert np.abs(f).max() < 1e-12 * scale


def test_pinned_counts(refs):
    ref = refs[0]
    c32, c33 = ref.compute(*swn.cluster(32)), ref.compute(*swn.cluster(33))
    assert (c32["maxin"], c32["npairs"], c32["ntriplets"]) == (32, 151, 1506)
    assert (c33["maxin"], c33["npairs"], c33["ntriplets"]) == (33, 162, 1672)
    x = swn.cluster(32)[0]
    d = np.linalg.norm(x[:, None, :] - x[None, :, :], axis=2)
    d[np.diag_indices(len(x))] = np.inf
    assert abs(d.min() - 1.91) < 0.005 and abs(np.abs(c32["f"]).max() - 281.0) < 1.0
    far = ref.compute(*swn.cluster(33, 3.9))          # the shell beyond the cutoff: the centre has no neighbour
    assert len(ref.neighbours(*swn.cluster(33, 3.9))[0]) == 0 and (far["maxin"], far["npairs"], far["ntriplets"]) == (8, 115, 690)
    assert ref.compute(*swn.case_a_compressed())["maxin"] == 33
    for name, least in (("N1", 2), ("N3", 6), ("N4", 6)):
        x, box, t = swn.narrow(name)
        assert min(_self_entries(ref, x, box, t)) == least >= 1
    one, two = ref.compute(*swn.lone(1)), ref.compute(*swn.lone(2))
    assert (one["npairs"], one["ntriplets"], one["e"], np.abs(one["f"]).max()) == (0, 0, 0.0, 0.0)
    assert (two["npairs"], two["ntriplets"]) == (1, 0) and two["e3"] == 0.0 and two["e2"] < 0.0
    want = {7: (7, 10), 9: (10, 18), 63: (101, 283), 65: (106, 301), 511: (1421, 7200), 513: (1426, 7225)}
    for n, (npairs, ntrip) in want.items():
        o = ref.compute(*swn.truncated(n))
        assert (o["npairs"], o["ntriplets"]) == (npairs, ntrip) and o["maxin"] <= 32
    x, box, t = swn.truncated(1025)
    xg, bg, _ = swn.case_g()
    assert np.array_equal(bg, box) and np.array_equal(xg[:1025], x)      # the block of case (g)


@pytest.mark.parametrize("name", NARROW)
def test_host_compiled_core_in_narrow_boxes(refs, name):
    """sw_core.h as the kernels run it, with sw_owns deciding an atom's pair with its own image, against the reference at 1e-12"""
    L = driver_lib()
    if name == "N5":
        ref, drivers = refs[1], [Driver(L, refs[2], ["Si", "X"])]
    else:
        ref, drivers = refs[0], [Driver(L, SI_SW, ["Si"]), Driver(L, SI_SW, ["Si"], general=True)]
    x, box, t = swn.narrow(name)
    want = ref.compute(x, box, t)
    for d in drivers:
        got = d(x, box, t)
        if name == "N4":      # zero net force: compare on the scale of the terms
            assert np.abs(got["f"]).max() <= 1e-12 * largest_force_term(ref, x, box, t)
            got["f"] = want["f"]
        same(got, want)
