"""The pair kernel (grav_pair_kernel_live beside the main walk, grav_pair_kernel behind it) after its instruction diet: lane conditions
carried as votes, prefix counts on the scalar masks, 32-bit offsets from scalar bases, leaf pushes below one count, tallies per wave.
The rewrite must keep the pairs, the lanes, the batches and the order: every launch form gives the same bits, the interaction counts are
the oracle's as integers, and the tallies are the oracle's sums.

Particle sets (those of test_gpu_walk_addr.py, built here): S-clusters in a periodic box, 24^3 at Nmesh 72 and 30^3 - 37 at Nmesh 90
(a ragged last task of 19 targets); oracle walk, random FullTreeGravAccel / GravPM, ErrTolForceAcc 0.005, relative criterion.
shq_set_walk_launch(2, 1) and shq_set_walk_overlap(2) make the production forms run at these sizes.

Bounds: forces within 1e-11 of the oracle's largest component (the bound of test_gpu_walk_addr.py for these shapes), and within 1e-13 of
the largest force against the launch without hand-over on the same context (the bound of
test_walk_launch_modes_agree_and_match_the_oracle); the potential as in test_gpu_walk_addr.py."""
import ctypes as C

import numpy as np
import pytest

import shenqi_amd as sq
from shenqi_amd import capi
import orc
import common as cm

# name: (particles, Nmesh)
SHAPES = {"c24": (24**3, 72), "ragged": (30**3 - 37, 90)}
SPARSE_LANES = 8   # a subtree that at most this many lanes of a task enter goes to the pair kernel at every threshold the library has had (8, 12)

_setups = {}
_walks = {}


def _setup(shape):
    """particles, tree, parameters and the oracle's walk of one shape: computed once, shared by the tests, never changed"""
    if shape not in _setups:
        n, nmesh = SHAPES[shape]
        pos = sq.synth_positions("cluster", n, L=cm.BOX)
        pman = cm.make_partmanager(pos)
        tree = sq.force_tree_full(pman)
        cm.reference_treepar(ErrTolForceAcc=0.005, MaxBHOpeningAngle=0.9, TreeUseBH=0)
        sq.gravshort_set_softenings(cm.BOX / 200)
        gp = sq.make_grav_params(cm.BOX, 1.5, nmesh, cm.G, cm.RHO0)
        rng = np.random.default_rng(17)
        told, pold = rng.normal(size=(n, 3)) * 500.0, rng.normal(size=(n, 3)) * 50.0
        mass = pman.Base["Mass"].copy()
        oacc, opot, onint = orc.grav_walk(tree.Nodes_base, tree.firstnode, pos, mass, np.linalg.norm(told + pold, axis=1) / cm.G, gp)
        orc.grav_postprocess(mass, gp, oacc, opot, True)
        for a in (pos, told, pold, oacc, opot, onint):
            a.setflags(write=False)
        _setups[shape] = dict(pos=pos, n=n, nmesh=nmesh, pman=pman, tree=tree, gp=gp, told=told, pold=pold, oacc=oacc, opot=opot, onint=onint)
    # the module-wide walk parameters of these cases (other tests set their own)
    cm.reference_treepar(ErrTolForceAcc=0.005, MaxBHOpeningAngle=0.9, TreeUseBH=0)
    sq.gravshort_set_softenings(cm.BOX / 200)
    return _setups[shape]


def _restore(c):
    capi.check(capi.hip.shq_set_walk_addr(c.h, 1))
    capi.check(capi.hip.shq_set_walk_overlap(c.h, 1))
    capi.check(capi.hip.shq_set_walk_launch(c.h, 1, 1))
    capi.check(capi.hip.shq_set_walk_sparse(c.h, 1))


def _walk(c, s, update_potential, sparse=1, overlap=2, addr=1):
    """upload, one walk in the launch form asked for, download; returns (acc, pot, nint, stats, the pair kernel's address form)"""
    pman, tree, gp = s["pman"], s["tree"], s["gp"]
    P = pman.Base
    P["FullTreeGravAccel"] = s["told"]
    P["GravPM"] = s["pold"]
    pv, tv = pman.view(), tree.view()
    capi.check(capi.hip.shq_particles_upload(c.h, C.byref(pv)))
    capi.check(capi.hip.shq_tree_upload(c.h, C.byref(tv)))
    capi.check(capi.hip.shq_grav_refresh_oldacc(c.h, gp.G))
    capi.check(capi.hip.shq_set_walk_launch(c.h, 2, 1))
    capi.check(capi.hip.shq_set_walk_sparse(c.h, sparse))
    capi.check(capi.hip.shq_set_walk_overlap(c.h, overlap))
    capi.check(capi.hip.shq_set_walk_addr(c.h, addr))
    capi.check(capi.hip.shq_grav_short_run(c.h, C.byref(gp), None, 0, int(update_potential), sq.WALK_EXACT))
    used = C.c_int(-1)
    capi.check(capi.hip.shq_walk_last_pair_addr(c.h, C.byref(used)))
    n = pman.NumPart
    acc = np.zeros((n, 3)); pot = np.zeros(n); nint = np.zeros(n, dtype=np.int64)
    st = sq.WalkStats()
    capi.check(capi.hip.shq_grav_short_download(c.h, capi.ptr(acc), capi.ptr(pot), capi.ptr(nint), C.byref(st)))
    return acc, pot, nint, (int(st.ninteractions), int(st.min_interactions), int(st.max_interactions)), used.value


# launch form: (walk_sparse, walk_overlap, walk_addr)
FORMS = {"beside": (1, 2, 1), "behind": (1, 0, 1), "whole records": (2, 2, 1), "64-bit": (1, 2, 0), "64-bit behind": (1, 0, 0),
         "no hand-over": (0, 2, 1)}


def _all_forms(ctx, shape, update_potential):
    """every launch form of one shape once, on the session's context; shared by the tests below"""
    key = (shape, update_potential)
    if key not in _walks:
        s = _setup(shape)
        res = {}
        try:
            for form, (sparse, overlap, addr) in FORMS.items():
                res[form] = _walk(ctx, s, update_potential, sparse, overlap, addr)
        finally:
            _restore(ctx)
        _walks[key] = res
    return _walks[key]


def _wrap(d):
    return d - cm.BOX * np.rint(d / cm.BOX)


def _self_pair_candidates(s):
    """Targets whose own leaf goes to the pair kernel with them among the lanes that open it (the CLAMP pair: the target meets itself as a
    leaf particle).  A task is 64 consecutive particles.  A lane enters a leaf only if it opened the leaf's father, and it opens the
    father only if it keeps it: not (r^2 > Rcut^2 and the largest |centre - target| component > Rcut + len / 2).  Where at most 8 targets
    of the task keep the father, at most 8 lanes enter the leaf, so the leaf (or a subtree around it) is handed over while the task has
    a free slot; the target itself is one of them (inside the cell, it opens every node on its path)."""
    pos, nodes, first = s["pos"], s["tree"].Nodes_base, s["tree"].firstnode
    rcut = s["gp"].Rcut
    isleaf = ((nodes["flags"] >> 3) & 3) == 0
    found = []
    for li in np.nonzero(isleaf & (nodes["noccupied"] > 0))[0]:
        fa = nodes["father"][li]
        if fa < 0:
            continue
        f = nodes[fa - first]
        for p in nodes["suns"][li][: nodes["noccupied"][li]]:
            t0 = (p // 64) * 64
            q = pos[t0:t0 + 64]
            cmax = np.abs(_wrap(f["center"] - q)).max(axis=1)
            r2 = (_wrap(f["cofm"] - q) ** 2).sum(axis=1)
            keep = ~((r2 > rcut * rcut) & (cmax > rcut + 0.5 * f["len"]))
            if keep[p - t0] and keep.sum() <= SPARSE_LANES:
                found.append(int(p))
    return found


def test_offset_rule_on_numbers():
    """node records of 128 bytes (numnodes + 1 of them: the rule of the main walk), leaf slots of 32 bytes and stack entries of 16 bytes
    must all end at or below 2^32; each limit on its own, at and around it"""
    fits = capi.hip.shq_pair_addr32_fits
    N, L, S = 2**25 - 1, 2**27, 2**28           # the largest that fit
    assert fits(N, L, S) == 1
    assert fits(N + 1, L, S) == 0 and fits(N, L + 1, S) == 0 and fits(N, L, S + 1) == 0
    assert fits(N - 1, L - 1, S - 1) == 1 and fits(0, 0, 0) == 1 and fits(1, 8, 4096) == 1
    assert fits(-1, L, S) == 0 and fits(N, -1, S) == 0 and fits(N, L, -1) == 0
    assert fits(2**40, 1, 1) == 0 and fits(1, 2**40, 1) == 0 and fits(1, 1, 2**40) == 0
    for nn in (N, N + 1):
        assert (fits(nn, L, S) == 1) == (capi.hip.shq_walk_addr32_fits(nn) == 1)
    for ls in (L, L + 1):
        assert (fits(N, ls, S) == 1) == (ls * 32 <= 2**32)
    for sc in (S, S + 1):
        assert (fits(N, L, sc) == 1) == (sc * 16 <= 2**32)
    # 512^3 particles: neither the pool (0.6 n nodes and more) nor the leaf copy (n + 8 slots) fits
    assert fits(int(0.6 * 512**3), 512**3 + 8, 4096) == 0 and fits(2**24, 512**3 + 8, 4096) == 0


@pytest.mark.parametrize("shape", list(SHAPES))
def test_particle_sets_reach_the_paths_on_the_host(shape):
    """leaves of every occupancy 1 ... 8 (every length of the leaf push); targets within a PM cell of a box face (the per-lane node wrap
    and the wrapped leaf particle); a handed-over leaf that contains one of the targets that open it (the self pair)"""
    s = _setup(shape)
    pos, nodes = s["pos"], s["tree"].Nodes_base
    leaves = nodes[((nodes["flags"] >> 3) & 3) == 0]
    occ = np.bincount(leaves["noccupied"], minlength=9)
    print("%s: leaves by occupancy %s" % (shape, occ.tolist()))
    assert (occ[1:9] > 0).all() and len(occ) == 9, occ
    cell = cm.BOX / s["nmesh"]
    near_face = ((pos < cell) | (pos > cm.BOX - cell)).any(axis=1)
    assert near_face.sum() >= 8, near_face.sum()
    selfp = _self_pair_candidates(s)
    print("%s: %d targets within a cell of a face, %d targets handed over with their own leaf" % (shape, near_face.sum(), len(selfp)))
    assert len(selfp) >= 1
    if shape == "ragged":
        assert s["n"] % 64 != 0


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_walk_reaches_the_batch_paths(shape):
    """a stack of at least 129 pairs at some round: rounds with two full batches, and on the way down a partial second batch and a single
    batch.  The high water is sticky per context, so this walk gets a context of its own."""
    s = _setup(shape)
    with sq.Context(0) as c:
        try:
            acc, pot, nint, st, used = _walk(c, s, 1)
            rec, high, mop = C.c_int64(0), C.c_int64(0), C.c_int64(0)
            capi.check(capi.hip.shq_walk_pair_status(c.h, C.byref(rec), C.byref(high), C.byref(mop)))
        finally:
            _restore(c)
    print("%s: pair stack high water %d, mopped %d, 32-bit form %d" % (shape, high.value, mop.value, used))
    assert high.value >= 129, high.value
    assert mop.value == 0
    assert used == 1
    assert np.array_equal(nint, s["onint"])


@pytest.mark.gpu
@pytest.mark.parametrize("update_potential", [1, 0])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_forms_agree_bit_for_bit(ctx, shape, update_potential):
    """beside against behind the walk, lean against whole records, 32-bit against 64-bit offsets: acc, pot, nint equal as arrays"""
    res = _all_forms(ctx, shape, update_potential)
    assert res["beside"][4] == 1 and res["behind"][4] == 1 and res["whole records"][4] == 1
    assert res["64-bit"][4] == 0 and res["64-bit behind"][4] == 0, "shq_set_walk_addr(0) must force the 64-bit form for the pair kernel too"
    for a, b in (("beside", "behind"), ("beside", "whole records"), ("beside", "64-bit"), ("behind", "64-bit behind")):
        for k, name in enumerate(("acc", "pot", "nint")):
            if name == "pot" and not update_potential:
                continue
            assert np.array_equal(res[a][k], res[b][k]), (a, b, name)


@pytest.mark.gpu
@pytest.mark.parametrize("update_potential", [1, 0])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_against_the_oracle_and_the_launch_without_hand_over(ctx, shape, update_potential):
    s = _setup(shape)
    res = _all_forms(ctx, shape, update_potential)
    scale = np.abs(s["oacc"]).max()
    ref = res["no hand-over"]
    fscale = np.abs(ref[0]).max()
    for form, (acc, pot, nint, st, used) in res.items():
        assert np.array_equal(nint, s["onint"]), form
        eo, en = np.abs(acc - s["oacc"]).max() / scale, np.abs(acc - ref[0]).max() / fscale
        print("%s %s pot %d: max |acc - oracle| / largest %.3e, |acc - no hand-over| / largest force %.3e" % (shape, form, update_potential, eo, en))
        assert eo < 1e-11, form
        assert en < 1e-13, form
        if update_potential:
            assert np.allclose(pot, s["opot"], rtol=1e-10, atol=1e-10 * np.abs(s["opot"]).max()), form


@pytest.mark.gpu
@pytest.mark.parametrize("update_potential", [1, 0])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_tallies_are_the_oracles(ctx, shape, update_potential):
    """the interaction sum, minimum and maximum that the pair kernel's waves tally (lane-local over a wave's tasks, reduced once)"""
    s = _setup(shape)
    res = _all_forms(ctx, shape, update_potential)
    onint = s["onint"]
    want = (int(onint.sum()), int(onint.min()), int(onint.max()))
    for form in ("beside", "behind", "64-bit", "64-bit behind", "whole records"):
        assert res[form][3] == want, (form, res[form][3], want)
