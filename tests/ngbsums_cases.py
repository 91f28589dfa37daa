"""Small inputs that take shq_stellar_density, shq_wind_veldisp, shq_bh_veldisp and shq_bh_dynfric (csrc/sph_ngbsums.hip) through
every branch of their radius loops and exits, through a flush of the per-lane neighbour list in the middle of a walk, through ragged
queues in shuffled order, the periodic wrap, and the neighbour-side skip flags.  Shared by test_ngbsums_brute_cpu.py (oracle against
the all-pairs sums of ngbsums_brute.py) and test_gpu_ngbsums_brute.py (device against the same sums).

Every case: BOX 8; the neighbour-side particles come first, the targets after them, then five particles of the targets' type that
are in no queue (their output rows must stay as they were); output slots (P.PI) in a shuffled order; masses a float holds exactly; velocities,
accelerations, time bins and kick factors as in the oracle's own fixtures; every particle a distinct potential.  A case may mark
neighbour-side particles garbage or change their type AFTER the tree is built (`garbage`, `retype`): apply_changes().
"""
import functools
from types import SimpleNamespace

import numpy as np

import common as cm
import density_brute as db
import ngbsums_brute as nb

BOX = cm.BOX
GAS, DM, STAR, BH = 0, 1, 4, 5
OPS = ("stellar", "wind", "bhvd", "dynfric")
TARGET_TYPE = {"stellar": STAR, "wind": GAS, "bhvd": BH, "dynfric": BH}


def Case(name, op, nb_pos, nb_type, t_pos, t_hsml, seed, kernel=1, weighting=0, dev=2.0, method=0, Time=0.25, hubble=3.0,
         garbage_frac=0.0, retype_frac=0.0, retype_from=None, retype_to=None, still=False, bulk=0.0, extra_active=0, swallowed=0):
    rng = np.random.default_rng(7000 + seed)
    nn, nt = len(nb_pos), len(t_pos)
    nidle = 5                                            # particles of the targets' type that are in no queue: their rows stay
    n = nn + nt + nidle
    c = SimpleNamespace(name=name, op=op, n=n, nn=nn, nt=nt, kernel=kernel, weighting=weighting, dev=dev, method=method, Time=Time,
                        hubble=hubble)
    c.pos = np.ascontiguousarray(np.concatenate([nb_pos, t_pos, rng.uniform(0, BOX, size=(nidle, 3))]), dtype=np.float64)
    assert np.all((c.pos >= 0) & (c.pos < BOX)), name
    c.type0 = np.concatenate([np.broadcast_to(np.asarray(nb_type, dtype=np.uint8), (nn,)), np.full(nt + nidle, TARGET_TYPE[op], dtype=np.uint8)])
    t_hsml = np.concatenate([np.broadcast_to(np.asarray(t_hsml, dtype=np.float64), (nt,)), np.full(nidle, BOX / 16)])
    c.idle = np.arange(nn + nt, n)
    c.mass = rng.uniform(0.5, 1.5, size=n).astype(np.float32)
    c.vel = rng.normal(size=(n, 3)) * 100.0 + bulk
    c.treeacc = rng.normal(size=(n, 3)) * 1e3
    c.gravpm = rng.normal(size=(n, 3)) * 1e2
    c.bin_grav = rng.integers(20, 24, size=n).astype(np.uint8)
    if still:                                            # nothing moves: every relative velocity is exactly zero
        c.vel[:], c.treeacc[:], c.gravpm[:] = 0, 0, 0
    c.potential = rng.permutation(n) * 7.25 - 1e4 + rng.uniform(0, 1, size=n)          # distinct, gaps >= 6
    c.density = 1.0 + 3.0 * c.pos[:, 0] / BOX            # of the gas, by particle
    c.hsml = np.full(n, BOX / 16)
    c.hsml[nn:] = t_hsml
    c.slot = np.zeros(n, dtype=np.int32)                 # P.PI: gas by particle order, targets in a shuffled order
    gas0 = np.flatnonzero(c.type0 == GAS)
    if op != "wind":
        c.slot[gas0] = np.arange(len(gas0))
    c.slot[nn:] = rng.permutation(nt + nidle)
    c.nslots = nt + nidle
    c.queue = (nn + rng.permutation(nt)).astype(np.int32)            # shuffled: the lanes of a wave lie all over the box
    c.flags = np.zeros(n, dtype=np.uint8)
    c.garbage = np.sort(rng.permutation(nn)[:int(round(garbage_frac * nn))])
    c.retype = np.zeros(0, dtype=np.int64)
    c.retype_to = retype_to
    if retype_frac:
        pool = np.setdiff1d(np.flatnonzero(c.type0[:nn] == retype_from), c.garbage)
        c.retype = np.sort(rng.permutation(pool)[:int(round(retype_frac * len(pool)))])
    # bh_veldisp takes an active list that may hold swallowed holes and particles that are no holes: they get no work
    c.active = c.queue
    if op == "bhvd":
        c.swallowed = c.queue[:swallowed].copy()
        c.flags[c.swallowed] |= 2
        c.active = np.concatenate([c.queue, rng.permutation(nn)[:extra_active].astype(np.int32)])
        c.active = np.ascontiguousarray(rng.permutation(c.active), dtype=np.int32)
        c.queue = np.ascontiguousarray([i for i in c.active if c.type0[i] == BH and not c.flags[i] & 2], dtype=np.int32)
    c.gravkicks = np.zeros(47)
    c.gravkicks[20:24] = 1e-3 * (np.arange(20, 24) - 18)
    c.FgravkickB = 3e-3
    return c


def tree_mask(c):
    import shenqi_amd as sq
    if c.op == "stellar":
        return sq.GASMASK
    if c.op in ("wind", "bhvd"):
        return sq.DMMASK
    return {0: sq.ALLMASK, 1: sq.STARMASK + sq.BHMASK, 2: sq.STARMASK + sq.BHMASK + sq.DMMASK}[c.method]


def des_num_ngb(c):
    return db.desnumngb(c.kernel)


def state(c):
    """(pman, SphP, kf) of a case as it is when the tree is built"""
    import shenqi_amd as sq
    pman = sq.PartManager(c.n, BOX)
    P = pman.Base
    P["Pos"], P["Mass"], P["Vel"], P["Hsml"], P["Type"], P["PI"] = c.pos, c.mass, c.vel, c.hsml, c.type0, c.slot
    P["FullTreeGravAccel"], P["GravPM"], P["TimeBinGravity"], P["Potential"], P["Flags"] = c.treeacc, c.gravpm, c.bin_grav, c.potential, c.flags
    P["ID"] = np.arange(1, c.n + 1)
    gas0 = np.flatnonzero(c.type0 == GAS)
    SphP = np.zeros(max(len(gas0), 1), dtype=sq.SPH_DTYPE)
    if c.op == "stellar":
        SphP["Density"][c.slot[gas0]] = c.density[gas0]
        SphP["Entropy"] = 1.0
    kf = sq.KickFactors()
    kf.FgravkickB = c.FgravkickB
    for b in range(47):
        kf.gravkicks[b] = c.gravkicks[b]
    return pman, SphP, kf


def types_now(c):
    t = c.type0.copy()
    t[c.retype] = c.retype_to if len(c.retype) else 0
    return t


def flags_now(c):
    f = c.flags.copy()
    f[c.garbage] |= 1
    return f


def apply_changes(c, P):
    """what happens between the tree build and the call: some neighbour-side particles become garbage, some change type"""
    P["Flags"] = flags_now(c)
    P["Type"] = types_now(c)


def brute_run(c, flagged=True):
    """the all-pairs reference of a case.  flagged=False: as if nothing had been marked or retyped after the build"""
    t, f = (types_now(c), flags_now(c)) if flagged else (c.type0, c.flags)
    mass = c.mass.astype(np.float64)
    vp = nb.velpred(c.vel, c.treeacc, c.gravpm, c.bin_grav, c.gravkicks, c.FgravkickB)
    if c.op == "stellar":
        return nb.stellar_density(c.pos, t, f, mass, c.density, c.hsml, c.queue, BOX, c.kernel, des_num_ngb(c), c.dev, c.weighting)
    if c.op == "wind":
        return nb.wind_veldisp(c.pos, t, f, c.vel, vp, c.hsml, c.queue, BOX, c.Time, c.hubble)
    if c.op == "bhvd":
        return nb.bh_veldisp(c.pos, t, f, c.vel, vp, c.hsml, c.queue, BOX)
    mp, mpp, mpv = initial_minpot(c)
    return nb.bh_dynfric(c.pos, t, f, mass, c.vel, vp, c.potential, c.hsml, c.queue, c.slot[c.queue], BOX, c.kernel, c.method,
                         tree_mask(c), mp, mpp, mpv)


def initial_minpot(c):
    """blackhole_init_potential, bhdynfric.cpp:296-310: the hole's own potential and position; every other hole unbeatable"""
    mp, mpp, mpv = np.full(c.nslots, 1e29), np.zeros((c.nslots, 3)), np.zeros((c.nslots, 3))
    s = c.slot[c.queue]
    mp[s], mpp[s] = c.potential[c.queue], c.pos[c.queue]
    mp[s[::2]] = -1e30
    return mp, mpp, mpv


@functools.lru_cache(maxsize=None)
def reference(name):
    """(case, all-pairs result), computed once per process and shared; treat both as read-only"""
    c = CASES[name]()
    return c, brute_run(c)


# ---- positions ---------------------------------------------------------------------------------------------------------------
def _uniform(seed, n):
    return np.random.default_rng(seed).uniform(0, BOX, size=(n, 3))


def _clump(seed, nbg, nclump, centre, sigma):
    rng = np.random.default_rng(seed)
    cl = np.mod(np.asarray(centre) + sigma * rng.normal(size=(nclump, 3)), BOX)
    cl[cl >= BOX] = 0.0
    return np.concatenate([rng.uniform(0, BOX, size=(nbg, 3)), cl])


def _near_faces(seed, nt, reach):
    """thirds: within `reach` of a face, of an edge, of a corner"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0, BOX, size=(nt, 3))
    for i in range(nt):
        ncoord = 1 + (3 * i) // nt
        for k in rng.permutation(3)[:ncoord]:
            e = rng.uniform(0, reach)
            p[i, k] = e if rng.random() < 0.5 else BOX - e - 1e-9
    return p


def _nb_type(op, seed, n):
    """neighbour-side types: gas for the stellar density, dark matter for the dispersions, a mix for the friction"""
    if op == "stellar":
        return GAS
    if op in ("wind", "bhvd"):
        return DM
    return np.random.default_rng(seed).choice([GAS, DM, STAR], size=n, p=[0.2, 0.4, 0.4]).astype(np.uint8)


def _spread(seed, nt, lo, hi):
    return np.random.default_rng(seed).uniform(lo, hi, size=nt)


# ---- radius-loop cases (stellar, wind) -----------------------------------------------------------------------------------------
def uniform(op, nt=700, seed=1, **kw):
    """12^3 uniform background, start radii from 0.2 to 4.5 spacings; ~700 targets: three workgroups, a ragged last wave"""
    n1 = 12
    return Case("%s_uniform%d" % (op, nt), op, _uniform(100 + seed, n1**3), _nb_type(op, seed, n1**3), _uniform(200 + seed, nt),
                BOX / n1 * _spread(300 + seed, nt, 0.2, 4.5), seed, **kw)


def lattice(op, seed=2):
    """a perfect lattice; targets on sites, at cell centres and within 1e-3 of a box corner: whole shells at one distance, so the count
    jumps over the wanted one and the bracket collapses (wind); 63 targets"""
    n1 = 12
    s = BOX / n1
    g = cm.grid_positions(n1)
    rng = np.random.default_rng(400 + seed)
    sites = g[rng.permutation(len(g))[:21]]
    centres = np.mod(g[rng.permutation(len(g))[:21]] + 0.5 * s, BOX)
    corner = np.where(rng.random((21, 3)) < 0.5, 1e-3 * rng.random((21, 3)), BOX - 1e-3 * (0.01 + rng.random((21, 3))))
    return Case("%s_lattice" % op, op, g, _nb_type(op, seed, len(g)), np.concatenate([sites, centres, corner]),
                s * _spread(500 + seed, 63, 0.8, 2.6), seed)


def clump(op, seed=3):
    """a Gaussian clump of 1500 in a thin background of 228, plus an islet of exactly 40 that nothing else comes near; targets in the
    core, at the edge, in the void and at the islet's centre: maxcmpte == 1, repeated growth by 4, leaves of 8, no slope; 65 targets"""
    rng = np.random.default_rng(600 + seed)
    centre = np.array([2.5, 5.0, 3.0])
    bg = _clump(610 + seed, 228, 1500, centre, 0.15)
    isle_c = np.array([6.5, 1.25, 6.75])
    bg = bg[np.linalg.norm(db.min_image(bg - isle_c, BOX), axis=1) > 1.2]
    isle = isle_c + 0.01 * rng.normal(size=(40, 3))
    nbp = np.concatenate([bg, isle])
    core = centre + 0.05 * rng.normal(size=(24, 3))
    edge = centre + 0.45 * rng.normal(size=(20, 3))
    void = np.mod(centre + 4.0 + rng.uniform(-1.0, 1.0, size=(17, 3)), BOX)
    at_isle = isle_c + 1e-3 * rng.normal(size=(4, 3))
    h = np.concatenate([_spread(620 + seed, 24, 0.02, 1.0), _spread(630 + seed, 20, 0.05, 0.6), _spread(640 + seed, 17, 0.05, 0.3),
                        [0.13, 0.11, 0.2, 0.17]])
    return Case("%s_clump" % op, op, nbp, _nb_type(op, seed, len(nbp)), np.concatenate([core, edge, void, at_isle]), h, seed)


def sparse(op, n=60, nt=257, seed=4):
    """60 neighbours in the box, start radii of 0.05 - 0.45 Box: radii beyond Box / 2, `hs > R`; 257 targets: a ragged second block"""
    return Case("%s_sparse%d" % (op, n), op, _uniform(700 + seed + n, n), _nb_type(op, seed, n), _uniform(710 + seed, nt),
                BOX * _spread(720 + seed, nt, 0.05, 0.45), seed)


def few30():
    """30 dark-matter particles: fewer than the 40 wanted, so the bracket collapses at R = Box; the call must succeed"""
    return Case("wind_few30", "wind", _uniform(731, 30), DM, _uniform(732, 20), BOX * _spread(733, 20, 0.05, 0.3), 5)


def tiny(op, seed=6):
    """start radii of 1e-5 Box in a clump of sigma 2e-4 at 7.99 in every coordinate, and next to three periodic faces"""
    a = _clump(740 + seed, 112, 400, (7.99, 7.99, 7.99), 2e-4)
    b = _clump(741 + seed, 0, 400, (7.9999, 0.0001, 7.9999), 2e-4)
    nbp = np.concatenate([a, b])
    rng = np.random.default_rng(742 + seed)
    t = np.concatenate([np.array([7.99, 7.99, 7.99]) + 1e-4 * rng.normal(size=(33, 3)),
                        np.mod(np.array([7.9999, 0.0001, 7.9999]) + 1e-4 * rng.normal(size=(32, 3)), BOX)])
    t[t >= BOX] = 0.0
    return Case("%s_tiny" % op, op, nbp, _nb_type(op, seed, len(nbp)), t, 1e-5 * BOX * _spread(743 + seed, 65, 0.8, 1.5), seed)


def single(op, seed=7, **kw):
    return uniform(op, nt=1, seed=seed, **kw)


def wrap(op, seed=8, **kw):
    """targets within their radius of faces, edges and a corner, neighbours across; a bulk velocity a thousand times the dispersion"""
    n1 = 12
    s = BOX / n1
    return Case("%s_wrap" % op, op, _uniform(800 + seed, n1**3), _nb_type(op, seed, n1**3), _near_faces(810 + seed, 63, 0.3 * s),
                s * _spread(820 + seed, 63, 1.5, 3.0), seed, bulk=1e5, **kw)


def lanes(op, seed=9, **kw):
    """16^3 background, start radii of 4.5 spacings beside 0.8 spacings in the neighbouring lane: 380 - 500 accepted neighbours, so
    the lane list (256 entries) is flushed in the middle of the walk, with the running cut carried across; 130 targets"""
    n1 = 16
    s = BOX / n1
    # the wind loop searches with (5 / 6)^(1 / 3) of its start radius, the stellar loop with 1.07 of it
    h = np.full(130, (4.9 if op == "wind" else 4.5) * s) * _spread(900 + seed, 130, 0.97, 1.03)
    if op in ("stellar", "wind"):
        h[1::2] = 0.8 * s * _spread(901 + seed, 65, 0.9, 1.1)
    c = Case("%s_lanes" % op, op, _uniform(910 + seed, n1**3), _nb_type(op, seed, n1**3), _uniform(920 + seed, 130), h, seed, **kw)
    if op in ("stellar", "wind"):                     # queue order = lane order: big and small radii alternate within a wave
        c.queue = (c.nn + np.arange(c.nt)).astype(np.int32)
        c.active = c.queue
    return c


def flagged(op, seed=10, **kw):
    """5 % of the neighbour side garbage, 5 % of the rest no longer of the tree's type, both after the build"""
    src = {"stellar": GAS, "wind": DM, "bhvd": DM, "dynfric": STAR}[op]
    to = {"stellar": STAR, "wind": 2, "bhvd": 2, "dynfric": GAS}[op]
    c = uniform(op, nt=65, seed=seed, garbage_frac=0.05, retype_frac=0.05, retype_from=src, retype_to=to, **kw)
    c.name = "%s_flagged" % op + ("_m%d" % kw["method"] if "method" in kw else "")
    if op == "dynfric":
        # a random 5 % seldom holds the particle of lowest potential of a neighbourhood: mark that very particle for 30 holes
        inmask = ((1 << c.type0.astype(np.int64)) & tree_mask(c)) != 0
        lowest = []
        for i in c.queue[:30]:
            d = db.min_image(c.pos[i] - c.pos, BOX)
            inside = np.flatnonzero(inmask & ((d * d).sum(axis=1) < c.hsml[i] ** 2))
            lowest.append(inside[np.argmin(c.potential[inside])])
        c.garbage = np.union1d(c.garbage, [j for j in lowest if j < c.nn]).astype(np.int64)
        c.retype = np.setdiff1d(c.retype, c.garbage)
    return c


def stellar_narrow(seed=11):
    """a band of +- 0.002: ngb_narrow_down aims at int(DesNumNgb) = 33, outside it, so every star ends by R - L < 1e-4 L"""
    c = uniform("stellar", nt=63, seed=seed, dev=0.002)
    c.name = "stellar_narrow"
    return c


def stellar_template(kernel, weighting):
    c = uniform("stellar", nt=65, seed=20 + 2 * kernel + weighting, kernel=kernel, weighting=weighting)
    c.name = "stellar_k%d_w%d" % (kernel, weighting)
    return c


def wind_still():
    """zero velocities and accelerations, hubble = 0: the variance is exactly 0 and VDisp stays as it was"""
    c = uniform("wind", nt=65, seed=31, still=True, hubble=0.0)
    c.name = "wind_still"
    return c


# ---- single-pass cases (bhvd, dynfric) -----------------------------------------------------------------------------------------
def bhvd_uniform():
    """257 holes with Hsml of 1.5 - 3.5 spacings, ten of them with no dark matter inside Hsml; three swallowed holes and twenty
    dark-matter particles in the active list"""
    c = uniform("bhvd", nt=257, seed=41, swallowed=3, extra_active=20)
    c.hsml[c.nn:c.nn + c.nt] = BOX / 12 * _spread(341, 257, 1.5, 3.5)
    c.lonely = c.queue[5:15]
    c.hsml[c.lonely] = 1e-3
    return c


def bhvd_still():
    c = uniform("bhvd", nt=63, seed=42, still=True)
    c.hsml[c.nn:c.nn + c.nt] = BOX / 12 * _spread(342, 63, 1.5, 3.5)
    c.name = "bhvd_still"
    return c


def dynfric_template(kernel, method):
    """65 holes among gas, dark matter and stars; three of them with nothing but themselves inside their kernel (dens == 0)"""
    c = uniform("dynfric", nt=65, seed=50 + 3 * kernel + method, kernel=kernel, method=method)
    c.hsml[c.nn:c.nn + c.nt] = BOX / 12 * _spread(350 + kernel, 65, 1.5, 3.0)
    c.lonely = c.queue[7:10]
    c.hsml[c.lonely] = 1e-3
    c.name = "dynfric_k%d_m%d" % (kernel, method)
    return c


CASES = {}
for _op in ("stellar", "wind"):
    for _f in (uniform, single, lattice, clump, sparse, tiny, wrap, lanes, flagged):
        CASES["%s_%s" % (_op, _f.__name__)] = functools.partial(_f, _op)
CASES["wind_few30"] = few30
CASES["wind_still"] = wind_still
CASES["stellar_narrow"] = stellar_narrow
for _k in (1, 2, 4):
    for _w in (0, 1):
        CASES["stellar_k%d_w%d" % (_k, _w)] = functools.partial(stellar_template, _k, _w)
CASES["bhvd_uniform"] = bhvd_uniform
CASES["bhvd_still"] = bhvd_still
for _f in (single, wrap, lanes, flagged):
    CASES["bhvd_%s" % _f.__name__] = functools.partial(_f, "bhvd")
for _k in (1, 2, 4):
    for _m in (0, 1, 2):
        CASES["dynfric_k%d_m%d" % (_k, _m)] = functools.partial(dynfric_template, _k, _m)
CASES["dynfric_single"] = functools.partial(single, "dynfric", method=2)
CASES["dynfric_wrap"] = functools.partial(wrap, "dynfric", method=2)
CASES["dynfric_lanes"] = functools.partial(lanes, "dynfric", method=2, kernel=2)
for _m in (0, 1, 2):
    CASES["dynfric_flagged_m%d" % _m] = functools.partial(flagged, "dynfric", method=_m)
NAMES = {op: [k for k in CASES if k.startswith(op + "_")] for op in OPS}
SMALL = {"stellar": "stellar_k1_w0", "wind": "wind_wrap", "bhvd": "bhvd_wrap", "dynfric": "dynfric_k1_m1"}     # the reuse check reruns these


# ---- the bars, shared by the oracle check and the device check --------------------------------------------------------------------
HSML_BAR = 1e-9              # relative, per target: the radii go through pow()
SUM_BAR = 1e-11              # of the sum of the absolute values of the terms, per target


def _rel(err, scale):
    ok = scale > 0
    return float((err[ok] / scale[ok]).max()) if ok.any() else 0.0


def compare(c, ref, got):
    """`got` (the oracle's or the device's results, by queue position; MinPot arrays by slot) against the all-pairs result `ref`.
    Asserts the bars and returns the worst deviation of each quantity."""
    w = {}
    if c.op in ("stellar", "wind"):
        assert got["niterations"] == ref["niterations"], (c.name, got["niterations"], ref["niterations"])
    if c.op == "stellar":
        e = np.abs(got["Hsml"] / ref["Hsml"] - 1)
        w["Hsml"] = float(e.max())
        assert np.all(e < HSML_BAR), (c.name, "Hsml", w["Hsml"])
        e, s = np.abs(got["StarVolumeSPH"] - ref["StarVolumeSPH"]), ref["abs_StarVolumeSPH"]
        w["StarVolumeSPH"] = _rel(e, s)
        assert np.all(e <= SUM_BAR * s), (c.name, "StarVolumeSPH", w["StarVolumeSPH"])
        if "hsml_max_tried" in got:
            w["hsml_max_tried"] = abs(got["hsml_max_tried"] / ref["hsml_max_tried"] - 1)
            assert w["hsml_max_tried"] < HSML_BAR, (c.name, got["hsml_max_tried"], ref["hsml_max_tried"])
            assert got["hsml_max_tried"] >= got["Hsml"].max()
    if c.op in ("wind", "bhvd"):
        written = np.isfinite(ref["VDisp"])
        assert np.array_equal(np.isfinite(got["VDisp"]), written), (c.name, "which VDisp are written")
        key = "V2sum" if c.op == "wind" else "V2sumDM"
        with np.errstate(all="ignore"):
            s = ref[key] / ref["NumDM"]
        e = np.abs(3 * got["VDisp"] ** 2 - 3 * ref["VDisp"] ** 2)
        w["VDisp"] = _rel(e[written], s[written])
        assert np.all(e[written] <= SUM_BAR * s[written]), (c.name, "VDisp", w["VDisp"])
    if c.op == "wind" and "DMRadius" in got:
        e = np.abs(got["DMRadius"] / ref["DMRadius"] - 1)
        w["DMRadius"] = float(e.max())
        assert np.all(e < HSML_BAR), (c.name, "DMRadius", w["DMRadius"])
    if c.op == "bhvd":
        assert np.array_equal(got["NumDM"], ref["NumDM"]), (c.name, "NumDM")
        e, s = np.abs(got["V1sumDM"] - ref["V1sumDM"]), ref["abs_V1sumDM"]
        w["V1sumDM"] = _rel(e, s)
        assert np.all(e <= SUM_BAR * s), (c.name, "V1sumDM", w["V1sumDM"])
        e, s = np.abs(got["V2sumDM"] - ref["V2sumDM"]), ref["V2sumDM"]
        w["V2sumDM"] = _rel(e, s)
        assert np.all(e <= SUM_BAR * s), (c.name, "V2sumDM", w["V2sumDM"])
    if c.op == "dynfric":
        for k in ("MinPot", "MinPotPos", "MinPotVel", "updated"):
            assert np.array_equal(got[k], ref[k]), (c.name, k)
        if c.method > 0:
            d, pz = ref["dens"], ref["dens"] > 0
            e = np.abs(got["Density"] - d)
            w["Density"] = _rel(e, d)
            assert np.all(e <= SUM_BAR * d), (c.name, "Density", w["Density"])
            dd = np.where(pz, d, 1.0)
            e, s = np.abs(got["Vel"] - ref["Vel"]), ref["abs_mom"] / dd[:, None]
            w["Vel"] = _rel(e, s)
            assert np.all(e <= SUM_BAR * s), (c.name, "Vel", w["Vel"])
            e, s = np.abs(np.where(pz, got["RmsVel"] ** 2, got["RmsVel"]) - ref["v2"] / dd), ref["v2"] / dd
            w["RmsVel"] = _rel(e, s)
            assert np.all(e <= SUM_BAR * s), (c.name, "RmsVel", w["RmsVel"])
    return w


def line(c, ref, w, who):
    it = " passes %2d" % ref["niterations"] if "niterations" in ref else ""
    return "%-20s %-7s%s  %s" % (c.name, who, it, "  ".join("%s %.1e" % kv for kv in w.items()))
