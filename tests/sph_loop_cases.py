"""Inputs that take the Hsml loop of density() through every branch of density_check_neighbours (densitytree2.hpp:177-257), through
the wave and workgroup tiers of the device walk inside the loop, and to Hsml / Box of 1e-5, where the slack of the f32 pre-test of
the candidate scan decides which neighbours survive.  Shared by test_density_brute_cpu.py (oracle against the all-pairs sum of
density_brute.py) and test_gpu_sph_loop.py (device against both).

Every case: BOX 8, unequal masses a float holds exactly, normal velocities, entropies in [0.5, 2), zero kick factors,
update_hsml = 1, DoEgyDensity = 1.  A case is a Case record; `state(case)` makes the particle tables of the C ABI from it."""
import functools
from types import SimpleNamespace

import numpy as np

import orc
import common as cm
import density_brute as db

BOX = cm.BOX


def Case(name, pos, hsml, seed, kernel=1, dev=0.5, MinGasHsml=0.006, nbh=0, active=None, brute=True):
    """`nbh`: the last nbh particles are black holes (type 5, BlackHoleOn = 1, BlackHoleNgbFactor 2)"""
    n = len(pos)
    rng = np.random.default_rng(1000 + seed)
    c = SimpleNamespace(name=name, n=n, pos=np.ascontiguousarray(pos, dtype=np.float64), kernel=kernel, dev=dev, MinGasHsml=MinGasHsml,
                        nbh=nbh, brute=brute)
    c.mass = rng.uniform(0.5, 1.5, size=n).astype(np.float32)
    c.vel = rng.normal(size=(n, 3))
    c.entropy = rng.uniform(0.5, 2.0, size=n)             # by particle; black-hole rows unused
    c.hsml = np.broadcast_to(np.asarray(hsml, dtype=np.float64), (n,)).copy()
    c.type = np.zeros(n, dtype=np.uint8)
    if nbh:
        c.type[n - nbh:] = 5
    c.active = None if active is None else np.ascontiguousarray(active, dtype=np.int32)
    assert np.all((c.pos >= 0) & (c.pos < BOX))
    return c


def params(c):
    return cm.density_params(kernel=c.kernel, MaxNumNgbDeviation=c.dev, update_hsml=1, DoEgyDensity=1, BlackHoleOn=1 if c.nbh else 0,
                             MinGasHsml=c.MinGasHsml)


def state(c):
    """(pman, SphP, BhP) of a case, gas slots in particle order"""
    import shenqi_amd as sq
    ngas = c.n - c.nbh
    pman = sq.PartManager(c.n, BOX)
    P = pman.Base
    P["Pos"], P["Mass"], P["Vel"], P["Hsml"] = c.pos, c.mass, c.vel, c.hsml
    P["ID"] = np.arange(1, c.n + 1)
    P["Type"] = c.type
    P["PI"][:ngas] = np.arange(ngas)
    P["PI"][ngas:] = np.arange(c.nbh)
    SphP = np.zeros(max(ngas, 1), dtype=sq.SPH_DTYPE)[:ngas]
    SphP["Entropy"] = c.entropy[:ngas]
    SphP["Density"] = 1
    BhP = np.zeros(max(c.nbh, 2), dtype=sq.BH_SLOT_DTYPE)
    return pman, SphP, BhP


def _uniform(seed, n):
    return np.random.default_rng(seed).uniform(0, BOX, size=(n, 3))


def _random(seed, n):
    return cm.random_positions(orc.boost_mt19937_uniform(seed, 3 * n), n)


def _with_clump(seed, nbg, nclump, centre, sigma):
    rng = np.random.default_rng(seed)
    bg = rng.uniform(0, BOX, size=(nbg, 3))
    cl = np.mod(np.asarray(centre) + sigma * rng.normal(size=(nclump, 3)), BOX)
    cl[cl >= BOX] = 0.0                                    # -tiny mod Box rounds to Box
    return np.concatenate([bg, cl])


def alone(n):
    """fewer particles than any target count: grow by 1.26 until 1.26 Hsml > 0.99 Box, bisect against Right = Box, collapse at Box"""
    return Case("alone%d" % n, _uniform(11 + n, n), BOX / 4, seed=n)


def sparse(n):
    """Hsml ends between 0.39 and 0.75 Box: beyond Box / 2, where the minimum image stops the sums growing like a sphere's"""
    return Case("sparse%d" % n, _uniform(21 + n, n), BOX / 4, seed=20 + n)


def clump_floor():
    """200 particles within sigma 0.002 of a point 0.002 from two periodic faces: their bracket closes below MinGasHsml"""
    return Case("clump_floor", _with_clump(31, 824, 200, (0.002, BOX - 0.002, 4.0), 0.002), BOX / 10, seed=31)


def tiny_start():
    """from Hsml 1e-4 the sums hold the target's own term only for dozens of passes: DhsmlDensityFactor = 1 / 0, growth by 1.26"""
    return Case("tiny_start", _random(41, 1024), 1e-4, seed=41)


def huge_start():
    """from 0.6 Box every target meets all 1024 candidates (more than a lane's list holds): the wave tier inside the loop, left
    again as Hsml shrinks by the 1/3 clamp"""
    return Case("huge_start", _random(41, 1024), 0.6 * BOX, seed=42)


def kernel2():
    return Case("kernel2", _random(51, 512), BOX / 10, seed=51, kernel=2, dev=0.05)


def kernel4():
    return Case("kernel4", _random(52, 512), BOX / 10, seed=52, kernel=4, dev=0.05)


def bh():
    return Case("bh", _random(61, 1024), BOX / 10, seed=61, nbh=5)


def lattice():
    """whole shells of neighbours at equal distance, candidates on node faces; a narrow band"""
    return Case("lattice", cm.grid_positions(10), 1.5 * BOX / 10, seed=71, dev=0.01)


def dynrange():
    """a clump of sigma 2e-4 at 7.99 in every coordinate: final Hsml ~ 1e-5 Box beside coordinates whose f32 ulp is 4.8e-7"""
    return Case("dynrange", _with_clump(81, 112, 400, (7.99, 7.99, 7.99), 2e-4), 1e-3, seed=81, MinGasHsml=1e-6)


def dynrange_corner():
    """the same clump across three periodic faces: the f64 scan of the wrapping tiles beside the f32 scan of the others"""
    return Case("dynrange_corner", _with_clump(81, 112, 400, (7.9999, 0.0001, 7.9999), 2e-4), 1e-3, seed=82, MinGasHsml=1e-6)


def refloor(c, hsml_converged):
    """a second call from converged radii with MinGasHsml raised to their median: one pass, every target in band, the lower half
    raised to the floor (the in-band floor of density_check_neighbours), the upper half left as it is"""
    r = SimpleNamespace(**vars(c))
    r.name = c.name + "_refloor"
    r.hsml = np.array(hsml_converged, dtype=np.float64)
    r.MinGasHsml = float(np.median(r.hsml))
    return r


def ragged(nactive):
    """queue edges: 0, 1, 63, 65, 1001 unsorted entries"""
    n = 1024
    act = np.random.default_rng(90 + nactive).permutation(n)[:nactive].astype(np.int32)
    return Case("ragged%d" % nactive, _random(91, n), BOX / 10, seed=91, active=act, brute=False)


@functools.lru_cache(maxsize=None)
def _tiers_base():
    """26^3 particles with the radii a full density() call of the oracle converges to"""
    n = 26**3
    c = Case("tiers_base", _random(95, n), BOX / 26, seed=95, brute=False)
    st, _ = oracle_run(c)
    return c, st.hsml.copy()


def tiers_active():
    """three targets restarted at 0.9 Box (all 17576 candidates: beyond the 16384 of the wave tier, so the workgroup tier), 200
    restarted at 4 x their radius (the wave tier), 1000 as they are (done in one pass), in shuffled order; the others inactive"""
    base, h = _tiers_base()
    rng = np.random.default_rng(96)
    pick = rng.permutation(base.n)[:1203]
    c = SimpleNamespace(**vars(base))
    c.name = "tiers_active"
    c.hsml = h.copy()
    c.hsml[pick[:3]] = 0.9 * BOX
    c.hsml[pick[3:203]] *= 4.0
    c.active = np.ascontiguousarray(rng.permutation(pick), dtype=np.int32)
    c.giants, c.wave = pick[:3], pick[3:203]
    return c


BRUTE_CASES = {"alone1": lambda: alone(1), "alone2": lambda: alone(2), "sparse20": lambda: sparse(20), "sparse40": lambda: sparse(40),
               "clump_floor": clump_floor, "tiny_start": tiny_start, "huge_start": huge_start, "kernel2": kernel2, "kernel4": kernel4,
               "bh": bh, "lattice": lattice, "dynrange": dynrange, "dynrange_corner": dynrange_corner}
REFLOOR_BASE = "kernel2"            # ends with every target in band: a second call decides in one pass
ORACLE_CASES = {"tiers_active": tiers_active, **{"ragged%d" % k: (lambda k=k: ragged(k)) for k in (0, 1, 63, 65, 1001)}}

# what each case is there to reach, counted on the CPU (test_density_brute_cpu.py asserts these are non-zero)
CLAIMS = {"alone1": ("grow_clamp", "bisect_box", "bracket_collapse"), "alone2": ("grow_clamp", "bisect_box", "bracket_collapse"),
          "sparse20": ("grow_clamp", "bisect", "newton"), "sparse40": ("grow_clamp", "bisect", "newton"),
          "clump_floor": ("floor_R", "bisect", "grow_clamp", "shrink_clamp", "newton", "inband"),
          "tiny_start": ("grow_clamp",), "huge_start": ("shrink_clamp",), "kernel2": ("bisect", "inband"), "kernel4": ("bisect", "inband"),
          "bh": ("inband",), "lattice": ("bisect", "inband"), "dynrange": ("shrink_clamp", "inband"),
          "dynrange_corner": ("shrink_clamp", "inband"), "kernel2_refloor": ("floor_band", "inband")}


def brute_run(c):
    """the all-pairs reference of a case (density_brute.density)"""
    k = c.kernel
    return db.density(c.pos, c.type, c.mass, c.vel, c.entropy, c.hsml, BOX, k, db.desnumngb(k), 2.0 * db.desnumngb(k), c.dev,
                      c.MinGasHsml, BlackHoleOn=1 if c.nbh else 0, active=c.active)


def oracle_run(c, tree=None):
    """orc.density on a case.  `tree`: (nodes, firstnode, father) of the gas; built by the oracle when None.
    Returns (SphState with the results, SimpleNamespace(niter, evp, gradrho, nodes))."""
    pman, SphP, BhP = state(c)
    st = orc.SphState(pman.Base, SphP, BhP)
    if tree is None:
        gas = np.flatnonzero(c.type == 0).astype(np.int32)
        tree = orc.tree_build(c.pos, c.mass, BOX, idx=gas, numpart_total=c.n)
    nodes, first, father = tree
    nodes = nodes.copy()
    act = c.active if c.active is None or len(c.active) else np.zeros(1, dtype=np.int32)[:0]
    rc, evp, gr, niter, _ = orc.density(nodes, first, father, st, params(c), active=act, want_gradrho=True)
    assert rc == 0
    return st, SimpleNamespace(niter=niter, evp=evp, gradrho=gr, nodes=nodes)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(case, brute result) computed once per process and shared; treat both as read-only"""
    if name.endswith("_refloor"):
        base, ref = reference(name[:-len("_refloor")])
        c = refloor(base, ref["Hsml"])
    else:
        c = BRUTE_CASES[name]()
    return c, brute_run(c)
