"""Small inputs that take the black-hole accretion and feedback walks (csrc/sph_bh.hip; one-shot and emit / resolve / apply) through
every branch of their pair code and postprocess, through the queue lengths at which lanes, waves and 256-target tasks end, through a
flush of the per-lane neighbour list, the periodic wrap, and particles that changed after the tree was built.  Shared by
test_bh_brute_cpu.py (branches, margins, oracle/blackhole.py against the all-pairs reference of bh_brute.py) and
test_gpu_bh_brute.py (both device routes against the same reference).

Every case: BOX 8, gas on a jittered grid, some dark matter the walks must pass over, holes; rows and slots shuffled; hole IDs
5 k + 11 (no two consecutive); Ti_Current 2^18 with hydro bins 16 - 20, so bins 19 and 20 are inactive; slot and work rows of holes in no
queue hold sentinels.  A case may change particles AFTER the tree is built (`garbage`, `retype`, `negmass`, `swallowed`):
apply_changes().
"""
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np

import common as cm
import bh_brute as bb
from density_brute import min_image

BOX = cm.BOX
TI = 1 << 18
SENT = -7.25                 # what float work rows hold before a call
PARAMS = dict(BoxSize=BOX, ForceSoftening=0.35, SeedBHDynMass=0.0, atime=0.25, a3inv=64.0, hubble=0.3, GravInternal=43.0, BlackHoleAccretionFactor=100.0,
              BlackHoleEddingtonFactor=2.1, BlackHoleFeedbackFactor=0.05, EddingtonConst=14.3, UnitTime_in_s=3.0, HubbleParam=0.7, LightOverUnitVel=3.0e2,
              MaxThermalU=1.5e4, OmegaBaryon=0.05, Hubble=0.1, BHKE_EddingtonThrFactor=1.5, BHKE_EddingtonMFactor=0.002, BHKE_EddingtonMPivot=0.05,
              BHKE_EddingtonMIndex=2.0, BHKE_EffRhoFactor=0.05, BHKE_EffCap=0.05, BHKE_InjEnergyThr=1.0, BHKE_SfrCritOverDensity=57.7, DensityKernelType=1,
              WindsDecoupleSph=0, RepositionEnabled=1, MergeGravBound=1, BH_DRAG=0, BlackHoleKineticOn=0)
RMERGE = 2 * 0.35 / 2.8      # 0.25


def Case(name, seed, ngrid=10, nbh=36, nq=None, ndm=40, bh_hsml=(1.8, 2.6), gas_hsml=(1.2, 1.8), pairs=8, void=None, eeqos=True, Ti=TI, **prm):
    """the set as it is when the tree is built.  Holes are numbered 0 .. nbh - 1 (`c.bh[k]` is the row of hole k); holes 2 j and
    2 j + 1 for j < pairs lie within the merging radius of each other; the queue is the first nq holes, shuffled.
    void: (centre, radius) with no gas inside."""
    import shenqi_amd as sq
    from shenqi_amd import capi
    rng = np.random.default_rng(9000 + seed)
    sp = BOX / ngrid
    gas = np.mod(cm.grid_positions(ngrid) + rng.normal(size=(ngrid**3, 3)) * 0.25 * sp, BOX)
    if void is not None:
        gas = gas[np.linalg.norm(min_image(gas - np.asarray(void[0]), BOX), axis=1) > void[1]]
    ngas = len(gas)
    bh = rng.random((nbh, 3)) * BOX
    for j in range(min(pairs, nbh // 2)):
        bh[2 * j + 1] = np.mod(bh[2 * j] + rng.normal(size=3) * 0.05, BOX)
    pos = np.concatenate([gas, rng.random((ndm, 3)) * BOX, bh])
    pos[pos >= BOX] = 0.0
    n = len(pos)
    perm = rng.permutation(n)
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n)
    c = SimpleNamespace(name=name, n=n, ngas=ngas, nbh=nbh, Ti=Ti, sp=sp, rng=rng)
    c.gas, c.bh = inv[:ngas], inv[ngas + ndm:]
    P = np.zeros(n, dtype=sq.PartManager(1, BOX).Base.dtype)
    P["Pos"] = pos[perm]
    P["Type"] = np.concatenate([np.zeros(ngas, np.uint8), np.ones(ndm, np.uint8), np.full(nbh, 5, np.uint8)])[perm]
    P["Mass"] = rng.uniform(0.8, 1.2, n).astype(np.float32)
    P["ID"] = rng.permutation(n).astype(np.uint64) * 5 + 11
    P["Vel"] = rng.normal(size=(n, 3)) * 30
    P["FullTreeGravAccel"] = rng.normal(size=(n, 3)) * 50
    P["GravPM"] = rng.normal(size=(n, 3)) * 5
    P["TimeBinGravity"] = rng.integers(20, 24, n)
    P["TimeBinHydro"] = rng.integers(16, 21, n)
    P["Hsml"] = sp * rng.uniform(*gas_hsml, n)
    P["Hsml"][c.bh] = sp * rng.uniform(*bh_hsml, nbh)
    P["PI"][c.gas] = rng.permutation(ngas)
    P["PI"][c.bh] = rng.permutation(nbh)
    S = np.zeros(ngas, dtype=capi.SPH_DTYPE)
    S["ReverseLink"][P["PI"][c.gas]] = c.gas
    S["Entropy"] = rng.uniform(50, 150, ngas)
    S["Density"] = rng.uniform(0.5, 2.0, ngas) * ngas / BOX**3
    S["HydroAccel"] = rng.normal(size=(ngas, 3)) * 20
    S["DelayTime"] = np.where(rng.random(ngas) < 0.15, 0.5, 0.0)
    B = np.zeros(nbh, dtype=capi.BH_DTYPE)
    B["ReverseLink"][P["PI"][c.bh]] = c.bh
    B["Mass"] = rng.uniform(0.5, 8.0, nbh)
    B["Density"] = rng.uniform(0.6, 1.5, nbh) * ngas / BOX**3
    B["Mtrack"] = rng.uniform(0.2, 3.0, nbh)
    B["DFAccel"] = rng.normal(size=(nbh, 3)) * 3
    B["VDisp"] = rng.uniform(0, 40, nbh)
    B["KineticFdbkEnergy"] = rng.uniform(0, 4e4, nbh)
    B["CountProgs"] = rng.integers(1, 4, nbh)
    B["SwallowID"] = np.uint64(0xffffffffffffffff)
    B["SwallowTime"], B["Mdot"], B["DragAccel"] = SENT, SENT, SENT
    B["encounter"], B["minTimeBin"] = 7, 3
    c.P, c.S, c.B = P, S, B
    c.queue = np.ascontiguousarray(rng.permutation(c.bh[:nbh if nq is None else nq]), dtype=np.int32)
    c.prm_kw = dict(PARAMS, **prm)
    c.prm = SimpleNamespace(**c.prm_kw)
    c.rnd = rng.random(4099)
    c.eeqos = (np.arange(n) % 3 == 0).astype(np.uint8) if eeqos else None
    c.maxpart = n + 50
    c.garbage = c.retype = c.negmass = c.swallowed = np.zeros(0, dtype=np.int64)
    c.gravkicks = 1e-4 * (np.arange(47) - 10)
    c.hydrokicks = 5e-5 * (np.arange(47) - 8)
    c.dloga = np.where(np.arange(47) > 0, 1e-7 * 2.0 ** (np.arange(47) - 16), 0.0)
    c.FgravkickB = 2e-3
    return c


def slot(c, k):
    """BH slot of hole k"""
    return c.P["PI"][c.bh[k]]


def place(c, k, pos, hsml=None):
    c.P["Pos"][c.bh[k]] = np.mod(pos, BOX)
    if hsml is not None:
        c.P["Hsml"][c.bh[k]] = hsml


def set_ids(c, ks, order):
    """give holes `ks` the IDs they have now, reassigned so that their ranks follow `order` (0 = smallest)"""
    rows = c.bh[list(ks)]
    have = np.sort(c.P["ID"][rows])
    c.P["ID"][rows] = have[np.asarray(order)]


def kick_factors(c):
    import shenqi_amd as sq
    kf = sq.KickFactors()
    kf.FgravkickB = c.FgravkickB
    for b in range(47):
        kf.gravkicks[b], kf.hydrokicks[b], kf.dloga_for_bin[b] = c.gravkicks[b], c.hydrokicks[b], c.dloga[b]
    return kf


def params(c):
    from shenqi_amd import capi
    p = capi.BhParams()
    for k, v in c.prm_kw.items():
        setattr(p, k, v)
    return p


def state(c):
    """(pman, S, B, kf) of a case as it is when the tree is built: fresh copies"""
    import shenqi_amd as sq
    pman = sq.PartManager(c.n, BOX)
    pman.Base[:] = c.P
    return pman, c.S.copy(), c.B.copy(), kick_factors(c)


def in_tree(c):
    """what force_tree_rebuild_mask(GASMASK + BHMASK) takes in: gas and holes, no garbage, no swallowed hole (forcetree.cpp:805)"""
    t, f = c.P["Type"], c.P["Flags"]
    return ((t == 0) | (t == 5)) & ((f & 3) == 0)


def apply_changes(c, P):
    """what happens between the tree build and the call"""
    P["Flags"][c.garbage] |= 1
    P["Type"][c.retype] = 4
    P["Mass"][c.negmass] = -1.0
    P["Flags"][c.swallowed] |= 2


def work_arrays(c):
    """the BHPriv arrays with sentinels, KEflag 0 (the feedback postprocess reads it whether or not the kinetic mode is on)"""
    return bb.new_work(len(c.S), len(c.B), SENT)


def brute_run(c, flagged=True, drop_swallowed=False):
    """(accretion, feedback) of bh_brute on a case.  flagged=False: as if nothing had changed after the build; drop_swallowed: as if
    the walk passed over holes that were swallowed after the build"""
    P = c.P.copy()
    if flagged:
        apply_changes(c, P)
    kf = kick_factors(c)
    ids = np.ascontiguousarray(P["ID"])
    tree = in_tree(c)
    if drop_swallowed:
        tree = tree & ((P["Flags"] & 2) == 0)
    acc = bb.accretion(P, c.S, c.B, ids, c.queue, kf, c.prm, c.Ti, c.rnd, tree, work_arrays(c))
    fb = bb.feedback(acc, ids, c.queue, kf, c.prm, c.maxpart, c.rnd, c.eeqos, tree)
    return acc, fb


def oracle_run(c):
    """oracle/blackhole.py on a case, in the layout of compare()"""
    oracle = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle")
    if oracle not in sys.path:
        sys.path.insert(0, oracle)
    import blackhole as obh
    P, S, B, w = c.P.copy(), c.S.copy(), c.B.copy(), work_arrays(c)
    apply_changes(c, P)
    kf = kick_factors(c)
    ids = np.ascontiguousarray(P["ID"])
    obh.accretion(P, S, B, ids, c.queue, kf, c.prm, c.Ti, c.rnd, w, in_tree(c))
    acc = snapshot(P, S, B, w, None)
    counts = obh.feedback(P, S, B, ids, c.queue, kf, c.prm, c.maxpart, c.rnd, c.eeqos, w, in_tree(c))
    return dict(acc=acc, fb=snapshot(P, S, B, w, counts))


def snapshot(P, S, B, work, counts):
    return dict(P=P.copy(), S=S.copy(), B=B.copy(), work={k: v.copy() for k, v in work.items()}, counts=counts)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(case, accretion result, feedback result), computed once per process and shared; treat all three as read-only"""
    c = CASES[name]()
    acc, fb = brute_run(c)
    return c, acc, fb


# ---- the cases -----------------------------------------------------------------------------------------------------------------
def uniform():
    """700 holes in 14^3 gas: 11 waves, three 256-target tasks, a ragged last wave; random close pairs beside the placed ones"""
    return Case("uniform", 1, ngrid=14, nbh=700, bh_hsml=(1.2, 1.8), pairs=40)


def _qcase(nq, seed):
    c = Case("q%d" % nq if nq > 1 else "single", seed, ngrid=8, nbh=nq + 6, nq=nq, pairs=min(8, nq // 2 + 1), eeqos=bool(seed % 2))
    return c


def lonely():
    """five holes with Hsml 0.05 in a void of radius 1.3 that no gas kernel reaches: no neighbour but themselves.  The first at rest with
    Density > 0 (norm == 0), the second with Density == 0, the third with BlackHoleKineticOn off and nothing else special"""
    centre = np.array([4.0, 4.0, 4.0])
    c = Case("lonely", 3, ngrid=10, nbh=20, pairs=3, void=(centre, 1.3), gas_hsml=(0.7, 1.1), BH_DRAG=1)
    for k in range(5):
        place(c, 6 + k, centre + 0.3 * np.array([np.cos(k), np.sin(k), 0.2 * k - 0.4]), 0.05)
    c.P["Vel"][c.bh[6]] = 0
    c.B["Density"][slot(c, 7)] = 0
    return c


def tiny():
    """Hsml of 1e-5 Box: six holes each 0.3 Hsml away from a gas particle (one gas particle inside the kernel, every other neighbour
    through its own Hsml), beside ordinary holes"""
    c = Case("tiny", 4, ngrid=10, nbh=24, pairs=3)
    for k in range(6):
        g = c.gas[37 * k + 5]
        h = 1e-5 * BOX * (0.8 + 0.1 * k)
        u = np.array([0.6, -0.48, 0.64])
        place(c, 6 + k, c.P["Pos"][g] + 0.3 * h * u, h)
        c.B["Mass"][slot(c, 6 + k)] = 50.0
    return c


def wrap():
    """merging pairs across a face, an edge and the corner, a chain of three across a face, kernels reaching across faces"""
    c = Case("wrap", 5, ngrid=10, nbh=30, pairs=0)
    e = 0.03
    spots = [([e, 3.1, 5.2], [BOX - e, 3.11, 5.19]), ([2.2, BOX - e, 6.1], [2.21, e, 6.1]), ([5.5, 1.4, e], [5.49, 1.41, BOX - e]),
             ([e, e, 2.7], [BOX - e, BOX - 1.3 * e, 2.71]), ([BOX - e, 4.4, e], [e, 4.41, BOX - e]),
             ([e, e, e], [BOX - e, BOX - 1.2 * e, BOX - 0.8 * e])]
    for j, (a, b) in enumerate(spots):
        place(c, 2 * j, a)
        place(c, 2 * j + 1, b)
    place(c, 12, [BOX - 0.15, 6.6, 6.6])
    place(c, 13, [0.02, 6.6, 6.61])
    place(c, 14, [0.19, 6.61, 6.6])
    c.P["TimeBinHydro"][c.bh[:15]] = 17                                  # active: the larger ID of a pair swallows
    for k in range(15, 30):                                              # single holes within half a kernel of a face
        p = c.P["Pos"][c.bh[k]].copy()
        p[k % 3] = 0.2 if k % 2 else BOX - 0.2
        place(c, k, p)
    return c


def lanes():
    """66 holes in 14^3 gas in lane order, Hsml of 5.1 spacings beside 0.5: 400 - 700 accepted neighbours beside fewer than 20"""
    c = Case("lanes", 6, ngrid=14, nbh=66, pairs=0, gas_hsml=(0.9, 1.2), BH_DRAG=1)
    c.P["Hsml"][c.bh[0::2]] = 5.1 * c.sp * c.rng.uniform(0.97, 1.03, 33)
    c.P["Hsml"][c.bh[1::2]] = 0.5 * c.sp * c.rng.uniform(0.9, 1.1, 33)
    c.queue = np.ascontiguousarray(c.bh, dtype=np.int32)
    return c


def other_hsml():
    """pairs 0.2 apart (inside the merging radius 0.25): Hsml 0.05 beside 0.6, so the small one finds the large one only through the
    neighbour's Hsml; and both Hsml 0.1, so the two are no neighbours at all"""
    c = Case("other_hsml", 7, ngrid=10, nbh=28, pairs=0, Ti=TI)
    for j in range(6):
        a = c.P["Pos"][c.bh[2 * j]]
        place(c, 2 * j, a, 0.05 + 0.01 * j)
        place(c, 2 * j + 1, a + [0.12, 0.12, 0.1], 0.6 if j < 3 else 0.1)
    c.P["TimeBinHydro"][c.bh[:12]] = 17
    return c


def chain():
    """holes in reach of one another with active and inactive targets: a line X - Y - Z (0.2 apart: X and Z do not merge) where Y
    is marked and marks X; triangles and a square of mutual neighbours in every ID order with inactive members; heavy holes, so
    that gas is drawn by several holes at once"""
    c = Case("chain", 8, ngrid=10, nbh=40, pairs=0)
    hs = 1.6
    def group(ks, centre, offs, order, bins):
        for k, o in zip(ks, offs):
            place(c, k, np.asarray(centre) + o, hs)
        set_ids(c, ks, order)
        c.P["TimeBinHydro"][c.bh[list(ks)]] = bins
        for k in ks:
            c.B["Mass"][slot(c, k)] = 60.0
    line = [[0, 0, 0], [0.2, 0, 0], [0.4, 0, 0]]
    tri = [[0, 0, 0], [0.1, 0, 0], [0.05, 0.08, 0]]
    sq_ = [[0, 0, 0], [0.1, 0, 0], [0, 0.1, 0], [0.1, 0.1, 0.02]]
    group((0, 1, 2), [1.5, 1.5, 1.5], line, (0, 1, 2), 17)
    group((3, 4, 5), [5.5, 1.5, 2.5], tri, (0, 1, 2), 17)
    group((6, 7, 8), [1.5, 5.5, 3.5], tri, (1, 0, 2), (17, 19, 18))         # the smallest ID inactive
    group((9, 10, 11), [5.5, 5.5, 5.5], tri, (0, 2, 1), (20, 17, 19))       # the middle ID inactive: first mark from a smaller ID, replaced
    group((12, 13, 14), [2.5, 3.0, 6.5], tri, (2, 0, 1), (19, 20, 17))      # the largest ID inactive
    group((15, 16, 17, 18), [6.5, 3.0, 1.0], sq_, (3, 1, 0, 2), (17, 19, 18, 20))
    group((19, 20, 21, 22), [3.5, 6.8, 1.2], sq_, (1, 2, 3, 0), (20, 20, 17, 18))
    group((23, 24, 25), [6.8, 6.9, 3.1], line, (2, 0, 1), (19, 17, 18))
    return c


def _bound(name, seed, **kw):
    """pairs with nearly the same velocity and attracting accelerations (bound) beside random ones (unbound)"""
    c = Case(name, seed, ngrid=10, nbh=36, pairs=14, **kw)
    P = c.P
    for j in range(0, 14, 2):
        i, o = c.bh[2 * j], c.bh[2 * j + 1]
        P["Vel"][o] = P["Vel"][i] + 0.01
        P["FullTreeGravAccel"][o] = P["FullTreeGravAccel"][i] + 5000.0 * min_image(P["Pos"][i] - P["Pos"][o], BOX)
    return c


def bound():
    """check_grav_bound decides (RepositionEnabled 0, MergeGravBound 1); one hole of a pair in time bin 0"""
    c = _bound("bound", 9, RepositionEnabled=0, MergeGravBound=1)
    c.P["TimeBinHydro"][c.bh[1]] = 0
    c.P["TimeBinHydro"][c.bh[5]] = 0
    return c


def bound_off():
    """RepositionEnabled 0, MergeGravBound 0: every close pair merges"""
    return _bound("bound_off", 9, RepositionEnabled=0, MergeGravBound=0)


def bound_ti0():
    """RepositionEnabled 1, MergeGravBound 1, Ti_Current 0: every hole counts as active"""
    return _bound("bound_ti0", 9, RepositionEnabled=1, MergeGravBound=1, Ti=0)


def seed():
    """SeedBHDynMass 2 with Mtrack below and above it on the swallowing and the swallowed side; heavy holes, so that every hole
    swallows gas: the three branches of the feedback postprocess.  One swallower with Mtrack 0; one light swallower of a hole with
    Mtrack 0: black-hole mass accreted, no dynamical mass"""
    c = Case("seed", 10, ngrid=10, nbh=40, pairs=12, SeedBHDynMass=2.0, BH_DRAG=2)
    c.B["Mass"] = c.rng.uniform(20.0, 60.0, c.nbh)
    c.P["TimeBinHydro"][c.bh[:24]] = 17
    c.B["Mtrack"][slot(c, 3)] = 0.0
    c.B["Mtrack"][slot(c, 2)] = 0.7
    set_ids(c, (2, 3), (0, 1))                    # 3 swallows 2 with its own Mtrack 0
    set_ids(c, (4, 5), (0, 1))                    # 5, too light to draw gas, swallows 4, whose Mtrack is 0
    c.B["Mtrack"][slot(c, 4)] = 0.0
    c.B["Mtrack"][slot(c, 5)] = 1.0
    c.B["Mass"][slot(c, 5)] = 0.1
    set_ids(c, (6, 7), (0, 1))                    # 7, too light to draw gas, with Mtrack 0.3 swallows 6 with Mtrack 0.5: Mtrack grows to 0.8
    c.B["Mtrack"][slot(c, 6)], c.B["Mtrack"][slot(c, 7)], c.B["Mass"][slot(c, 7)] = 0.5, 0.3, 0.1
    return c


def eddington(drag):
    """the Bondi rate above and below the Eddington cap; BH_DRAG 0, 1, 2"""
    return Case("eddington_drag%d" % drag, 11 + drag, ngrid=10, nbh=36, BH_DRAG=drag, eeqos=bool(drag % 2))


def eddington_off():
    """BlackHoleEddingtonFactor 0: no cap (and a drag of zero with BH_DRAG 2)"""
    return Case("eddington_off", 14, ngrid=10, nbh=36, BlackHoleEddingtonFactor=0.0, BH_DRAG=2)


def kinetic():
    """BlackHoleKineticOn: KEflag 0, 1 and 2; lam_thresh = x and = ThrFactor; epsilon capped and free (Density 1e-7); VDisp == 0
    with energy above the threshold; a releasing hole with Density == 0; a hole that only accumulates"""
    c = Case("kinetic", 15, ngrid=10, nbh=48, BlackHoleKineticOn=1, DensityKernelType=2)
    for k in (16, 17, 18):
        c.B["Density"][slot(c, k)] = 1e-7
    c.B["KineticFdbkEnergy"][slot(c, 18)] = 0.0
    c.B["VDisp"][slot(c, 18)] = 35.0
    c.B["VDisp"][slot(c, 19)] = 0.0
    c.B["KineticFdbkEnergy"][slot(c, 19)] = 3e4
    c.B["Density"][slot(c, 20)] = 0.0
    c.B["VDisp"][slot(c, 20)] = 1.0
    c.B["KineticFdbkEnergy"][slot(c, 20)] = 3e4
    return c


def thermal():
    """thermal channel with overlapping kernels: the cap reached by one hole's heat, by the sum of two, and not at all; a hole with
    Density 0 (Mdot == 0: nothing to inject); gas of mass zero; a hole of Hsml 1e-4 whose only kernel gas has mass zero (weight 0)"""
    c = Case("thermal", 16, ngrid=10, nbh=60, bh_hsml=(1.8, 2.8), MaxThermalU=4.0e3)
    c.B["Density"][slot(c, 20)] = 0.0
    zero = c.gas[11::53]
    c.P["Mass"][zero] = 0.0
    g = zero[2]
    place(c, 21, c.P["Pos"][g] + [2e-5, -1e-5, 1e-5], 1e-4)
    c.B["Mass"][slot(c, 21)] = 0.1                # below its particle mass: it draws nothing
    # gas that two holes heat: its entropy put so that neither injection alone reaches the cap and their sum does (the injections
    # come from a first run; one particle's entropy moves a hole's Mdot by a per cent at most, the cap is missed by a quarter)
    _, fb = brute_run(c)
    by_slot = {}
    for row, _, kind, val, _ in fb.effects:
        if kind == 2:
            by_slot.setdefault(int(c.P["PI"][row]), []).append(val)
    cap, done = c.prm.MaxThermalU, 0
    for sl, v in sorted(by_slot.items()):
        if len(v) == 2 and max(v) < 0.5 * cap and min(v) > 0.2 * max(v) and done < 8:
            enttou = (c.S["Density"][sl] * c.prm.a3inv) ** (2.0 / 3) * 1.5
            c.S["Entropy"][sl] = (cap - max(v) - 0.5 * min(v)) / enttou
            done += 1
    assert done >= 3
    return c


def decoupled():
    """WindsDecoupleSph: the 15 % of the gas with DelayTime > 0 is passed over by both walks"""
    return Case("decoupled", 17, ngrid=10, nbh=36, WindsDecoupleSph=1, DensityKernelType=4, eeqos=False)


def flagged():
    """after the build: 5 % of the gas garbage, 5 % a star now, 5 % with Mass < 0, and six holes swallowed that are not in the queue
    and lie within the merging radius of queued holes"""
    c = Case("flagged", 18, ngrid=10, nbh=42, nq=36, pairs=0)
    r = c.rng.permutation(c.gas)
    m = len(r) // 20
    c.garbage, c.retype, c.negmass = np.sort(r[:m]), np.sort(r[m:2 * m]), np.sort(r[2 * m:3 * m])
    for k in range(6):
        place(c, 36 + k, c.P["Pos"][c.bh[k]] + [0.06, -0.05, 0.04])
        set_ids(c, (k, 36 + k), (1, 0) if k % 2 else (0, 1))
        c.P["TimeBinHydro"][c.bh[36 + k]] = 17 if k < 4 else 20
        c.B["SwallowID"][slot(c, 36 + k)] = 12345
        c.B["SwallowTime"][slot(c, 36 + k)] = 0.125
        c.B["encounter"][slot(c, 36 + k)] = 1
    c.swallowed = np.sort(c.bh[36:])
    return c


def template(kt):
    """every kernel template of both walks"""
    return Case("k%d" % kt, 20 + kt, ngrid=10, nbh=65, pairs=10, DensityKernelType=kt, eeqos=bool(kt % 2))


CASES = dict(uniform=uniform, single=functools.partial(_qcase, 1, 31), q63=functools.partial(_qcase, 63, 32), q64=functools.partial(_qcase, 64, 33),
             q65=functools.partial(_qcase, 65, 34), q257=functools.partial(_qcase, 257, 35), lonely=lonely, tiny=tiny, wrap=wrap, lanes=lanes,
             other_hsml=other_hsml, chain=chain, bound=bound, bound_off=bound_off, bound_ti0=bound_ti0, seed=seed,
             eddington_drag0=functools.partial(eddington, 0), eddington_drag1=functools.partial(eddington, 1),
             eddington_drag2=functools.partial(eddington, 2), eddington_off=eddington_off, kinetic=kinetic, thermal=thermal, decoupled=decoupled,
             flagged=flagged, k1=functools.partial(template, 1), k2=functools.partial(template, 2), k4=functools.partial(template, 4))
NAMES = list(CASES)


# ---- the bars, shared by the oracle check and the device checks ---------------------------------------------------------------------
SUM_BAR = 1e-11              # of the element's own scale (bh_brute), per element: the bar of ngbsums_cases.compare
EXACT = dict(P=("Flags", "Type", "PI", "TimeBinHydro", "TimeBinGravity", "Hsml", "Pos", "ID", "FullTreeGravAccel", "GravPM"),
             S=("ReverseLink", "Density", "DelayTime", "HydroAccel"),
             B=("ReverseLink", "minTimeBin", "encounter", "Density", "VDisp", "DFAccel", "SwallowTime", "SwallowID", "CountProgs"),
             work=("SPH_SwallowID", "BH_SwallowID", "KEflag"))
FLOAT = dict(P=("Vel",), S=("Entropy",), B=("Mdot", "Mass", "Mtrack", "KineticFdbkEnergy", "DragAccel"),
             work=("BH_FeedbackWeightSum", "BH_Entropy", "BH_SurroundingGasVel", "MgasEnc", "BH_accreted_Mass", "BH_accreted_BHMass",
                   "BH_accreted_momentum"))


def _worst(w, key, err, scale):
    ok = scale > 0
    w[key] = max(w.get(key, 0.0), float((err[ok] / scale[ok]).max()) / SUM_BAR if ok.any() else 0.0)


def compare_stage(c, ref, got, stage, w):
    """one snapshot (after the accretion call or after the feedback call) against the reference's state at that point"""
    for rec in ("P", "S", "B", "work"):
        for k in EXACT[rec]:
            a, b = got[rec][k], getattr(ref, rec)[k]
            assert np.array_equal(a, b), (c.name, stage, rec, k, np.flatnonzero(np.any(np.reshape(a != b, (len(a), -1)), axis=1))[:8])
        for k in FLOAT[rec]:
            a, b, s = got[rec][k], getattr(ref, rec)[k], ref.scale["%s.%s" % (rec, k)]
            err = np.abs(a - b)
            _worst(w, k, err, s)
            bad = ~(err <= SUM_BAR * s)                       # an element of scale 0 was not written: the same bits
            assert not bad.any(), (c.name, stage, rec, k, "element", np.argwhere(bad)[0], "off by", err[bad].max(), "scale", s[bad].max(),
                                   "worst in units of the bar", w[k])
    # the float particle mass: the float next to the reference's value, or its neighbour; untouched rows keep their bits
    a, b, exact = got["P"]["Mass"], ref.P["Mass"], ref.scale["P.Mass"]
    wr = exact != 0
    assert np.array_equal(a[~wr], b[~wr]), (c.name, stage, "Mass of particles nothing wrote to")
    f = exact[wr].astype(np.float32)
    assert np.all((a[wr] == f) | (a[wr] == np.nextafter(f, np.float32(np.inf))) | (a[wr] == np.nextafter(f, np.float32(-np.inf)))), (c.name, stage, "Mass")
    if got["counts"] is not None:
        assert tuple(got["counts"]) == tuple(ref.counts), (c.name, "swallow counts", got["counts"], ref.counts)


def compare(c, ref, got):
    """got: dict(acc=snapshot after the accretion call, fb=snapshot after the feedback call), ref: (accretion, feedback) of bh_brute.
    Integers, IDs, flag bytes and every field no call writes: equal.  Floats: within SUM_BAR of the element's own scale.  The float
    particle mass: the float rounding of the reference's value or its neighbour.  Returns the worst deviation of each quantity in
    units of the bar."""
    w = {}
    compare_stage(c, ref[0], got["acc"], "accretion", w)
    compare_stage(c, ref[1], got["fb"], "feedback", w)
    return w


def compare_records(c, ref, marks, effects):
    """the two emitted lists (capi.BH_MARK_DTYPE / BH_EFFECT_DTYPE, one rank) against the reference's, record by record; returns
    the worst deviation of the heat and kick values in units of the bar"""
    acc, fb = ref
    want = sorted((row, t, kind, i) for row, t, kind, i in acc.marks)
    have = sorted(zip(marks["part_index"].tolist(), marks["hole"].tolist(), marks["kind"].tolist(), marks["id"].tolist()))
    assert have == want, (c.name, "marks", len(have), len(want))
    assert np.all(marks["owner"] == 0)
    want = sorted(fb.effects)
    order = np.lexsort((effects["kind"], effects["hole"], effects["part_index"]))
    e = effects[order]
    assert [(r[0], r[1], r[2]) for r in want] == list(zip(e["part_index"].tolist(), e["hole"].tolist(), e["kind"].tolist())), (c.name, "effects")
    val, sc = np.array([r[3] for r in want]), np.array([r[4] for r in want])
    err = np.abs(e["value"] - val)
    assert np.all(err <= SUM_BAR * sc), (c.name, "effect values")
    w = {}
    for kind, key in ((2, "heat"), (3, "kick")):
        sel = e["kind"] == kind
        _worst(w, key, err[sel], sc[sel])
    return w


SHORT = {"KineticFdbkEnergy": "KFE", "DragAccel": "Drag", "BH_FeedbackWeightSum": "fws", "BH_Entropy": "bhEnt", "BH_SurroundingGasVel": "gasvel",
         "MgasEnc": "Mgas", "BH_accreted_Mass": "accM", "BH_accreted_BHMass": "accBH", "BH_accreted_momentum": "accmom"}


def line(c, w, who):
    """the worst deviations in units of the bar; quantities that are the reference's bits everywhere are left out"""
    return "%-16s %-8s %s" % (c.name, who, "  ".join("%s %.1e" % (SHORT.get(k, k), v) for k, v in w.items() if v > 0))
