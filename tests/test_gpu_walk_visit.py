"""GPU tests of the exact walk's node visit at the smallest shapes that reach every path of it: the record fetch, the interior
test and the wrap vote, leaves with and without the periodic wrap, the hand-over of sparse subtrees, the link moves, the softened
branch of the monopole.  Reference: the CPU oracle; bounds: those of test_walk_launch_modes_agree_and_match_the_oracle."""
import ctypes as C

import numpy as np
import pytest

import shenqi_amd as sq
from shenqi_amd import capi
import orc
import common as cm

pytestmark = pytest.mark.gpu

# name: (particles, Nmesh).  12^3 + 5 with Nmesh 36: Rcut + 1.5 len exceeds the distance to a face for every cell, so no node is
# interior and the wrap vote runs on every visit.  20^3 + 37 clustered with Nmesh 60: interior and non-interior nodes, a ragged last
# wave, fewer tasks than resident waves.  close: pairs inside the softening length (the softened branch of the monopole and of the leaf
# particles is taken).  Two softening lengths, BOX / 20 and BOX / 200: cells on both sides of len^2 / theta^2 >= h^2, i.e. nodes whose
# accepting targets can and cannot lie inside the softening length.
SHAPES = {"small": (12**3 + 5, 36), "cluster": (20**3 + 37, 60), "close": (16**3, 48)}
SOFTENINGS = {"small": (20, 200), "cluster": (20, 200), "close": (16,)}
CASES = [(s, d) for s in SHAPES for d in SOFTENINGS[s]]


def _positions(shape):
    n = SHAPES[shape][0]
    if shape == "close":
        return cm.close_positions(16)
    if shape == "cluster":
        return sq.synth_positions("cluster", n, L=cm.BOX)
    return cm.random_positions(orc.boost_mt19937_uniform(3, 3 * n), n)


def _gpu_walk(ctx, pman, tree, gp, oldacc_from, active=None, update_potential=True):
    P = pman.Base
    P["FullTreeGravAccel"] = oldacc_from[0]
    P["GravPM"] = oldacc_from[1]
    pv, tv = pman.view(), tree.view()
    capi.check(capi.hip.shq_particles_upload(ctx.h, C.byref(pv)))
    capi.check(capi.hip.shq_tree_upload(ctx.h, C.byref(tv)))
    capi.check(capi.hip.shq_grav_refresh_oldacc(ctx.h, gp.G))
    a = None if active is None else np.ascontiguousarray(active, dtype=np.int32)
    capi.check(capi.hip.shq_grav_short_run(ctx.h, C.byref(gp), capi.ptr(a), 0 if a is None else len(a), int(update_potential), sq.WALK_EXACT))
    n = pman.NumPart
    acc = np.zeros((n, 3)); pot = np.zeros(n); nint = np.zeros(n, dtype=np.int64)
    st = sq.WalkStats()
    capi.check(capi.hip.shq_grav_short_download(ctx.h, capi.ptr(acc), capi.ptr(pot), capi.ptr(nint), C.byref(st)))
    return acc, pot, nint, st


_setups = {}


def _setup(shape, softdiv, usebh):
    """particles, tree, parameters and the oracle's walk of one case: computed once, shared by the tests, never changed"""
    key = (shape, softdiv, usebh)
    if key not in _setups:
        pos = _positions(shape)
        n = len(pos)
        pman = cm.make_partmanager(pos)
        tree = sq.force_tree_full(pman)
        cm.reference_treepar(ErrTolForceAcc=0.005, MaxBHOpeningAngle=0.9, TreeUseBH=usebh)
        sq.gravshort_set_softenings(cm.BOX / softdiv)
        gp = sq.make_grav_params(cm.BOX, 1.5, SHAPES[shape][1], cm.G, cm.RHO0)
        rng = np.random.default_rng(11)
        told, pold = rng.normal(size=(n, 3)) * 500.0, rng.normal(size=(n, 3)) * 50.0
        mass = pman.Base["Mass"].copy()
        oacc, opot, onint = orc.grav_walk(tree.Nodes_base, tree.firstnode, pos, mass, np.linalg.norm(told + pold, axis=1) / cm.G, gp)
        orc.grav_postprocess(mass, gp, oacc, opot, True)
        for a in (pos, told, pold, oacc, opot, onint):
            a.setflags(write=False)
        _setups[key] = dict(pos=pos, n=n, pman=pman, tree=tree, gp=gp, told=told, pold=pold, oacc=oacc, opot=opot, onint=onint)
    s = _setups[key]
    # the module-wide walk parameters of this case (other tests set their own)
    cm.reference_treepar(ErrTolForceAcc=0.005, MaxBHOpeningAngle=0.9, TreeUseBH=usebh)
    sq.gravshort_set_softenings(cm.BOX / softdiv)
    return s


@pytest.mark.parametrize("shape,softdiv", CASES)
@pytest.mark.parametrize("usebh", [1, 0])
def test_visit_paths_in_every_launch_form(ctx, shape, softdiv, usebh):
    """Plain, persistent, ring, ring + sparse beside and behind the main walk, one active list without the potential: interaction
    counts equal the oracle's as integers, forces within 1e-11 of the oracle's largest; plain and persistent bit-identical; beside
    and behind bit-identical; ring forms within 1e-13 of the plain launch (a target's leaf particles are summed behind its nodes)."""
    s = _setup(shape, softdiv, usebh)
    n, pman, tree, gp, told, pold = s["n"], s["pman"], s["tree"], s["gp"], s["told"].copy(), s["pold"].copy()
    oacc, opot, onint = s["oacc"], s["opot"], s["onint"]
    print("%s soft BOX/%d bh %d" % (shape, softdiv, usebh))
    res = {}
    try:
        for mode in ((0, 0), (2, 0), (2, 1)):
            capi.check(capi.hip.shq_set_walk_launch(ctx.h, *mode))
            res[mode] = _gpu_walk(ctx, pman, tree, gp, (told, pold))
        sub = np.arange(5, n, 7, dtype=np.int32)
        capi.check(capi.hip.shq_set_walk_launch(ctx.h, 2, 1))
        asub = _gpu_walk(ctx, pman, tree, gp, (told, pold), active=sub, update_potential=False)
        capi.check(capi.hip.shq_set_walk_sparse(ctx.h, 0))
        res[(2, 1, "no pair kernel")] = _gpu_walk(ctx, pman, tree, gp, (told, pold))
        capi.check(capi.hip.shq_set_walk_sparse(ctx.h, 1))
        capi.check(capi.hip.shq_set_walk_overlap(ctx.h, 2))
        res[(2, 1, "beside")] = _gpu_walk(ctx, pman, tree, gp, (told, pold))
        capi.check(capi.hip.shq_set_walk_overlap(ctx.h, 0))
        res[(2, 1, "behind")] = _gpu_walk(ctx, pman, tree, gp, (told, pold))
    finally:
        capi.check(capi.hip.shq_set_walk_overlap(ctx.h, 1))
        capi.check(capi.hip.shq_set_walk_launch(ctx.h, 1, 1))
        capi.check(capi.hip.shq_set_walk_sparse(ctx.h, 1))
    scale = np.abs(oacc).max()
    for mode, (acc, pot, nint, st) in res.items():
        print(mode, "max |acc - oracle| / largest %.3e, vs plain %.3e" % (np.abs(acc - oacc).max() / scale,
                                                                           np.abs(acc - res[(0, 0)][0]).max() / scale))
    for mode, (acc, pot, nint, st) in res.items():
        assert np.array_equal(nint, onint), mode
        assert st.ninteractions == onint.sum() and st.min_interactions == onint.min() and st.max_interactions == onint.max(), mode
        assert np.abs(acc - oacc).max() < 1e-11 * scale, mode
        assert np.allclose(pot, opot, rtol=1e-10, atol=1e-10 * np.abs(opot).max()), mode
    assert np.array_equal(res[(0, 0)][0], res[(2, 0)][0]) and np.array_equal(res[(0, 0)][1], res[(2, 0)][1])
    for k in range(3):
        assert np.array_equal(res[(2, 1, "beside")][k], res[(2, 1, "behind")][k]), k
    for mode in ((2, 1), (2, 1, "no pair kernel"), (2, 1, "beside"), (2, 1, "behind")):
        assert np.abs(res[mode][0] - res[(0, 0)][0]).max() < 1e-13 * scale, mode
    assert np.array_equal(asub[2][sub], onint[sub])
    assert np.abs(asub[0][sub] - oacc[sub]).max() < 1e-11 * scale


@pytest.mark.parametrize("shape,softdiv", [c for c in CASES if c[0] != "close"])   # close: one top leaf holds every particle, nothing is exported
def test_secondary_walk_visits(ctx, shape, softdiv):
    """The secondary (imported-query) walk runs the same visit with lanes waiting at their branches: the queries a three-rank top tree
    exports, walked on the undivided tree, against the oracle's secondary walk: counts as integers, forces within 1e-11 of the
    largest of the primary walk's."""
    s = _setup(shape, softdiv, 0)
    pman, pos, gp = s["pman"], s["pos"], s["gp"]
    told, pold = s["told"].copy(), s["pold"].copy()
    P = pman.Base
    P["FullTreeGravAccel"] = told
    P["GravPM"] = pold
    oldacc = np.linalg.norm(told + pold, axis=1) / cm.G
    full = sq.force_tree_full(pman)
    cm.make_domain(full, ntask=3, me=1, depth=2, pseudo=False)
    dom = sq.force_tree_full(pman)
    tl = cm.make_domain(dom, ntask=3, me=1, depth=2)
    pv, tv = pman.view(), dom.view()
    capi.check(capi.hip.shq_particles_upload(ctx.h, C.byref(pv)))
    capi.check(capi.hip.shq_tree_upload(ctx.h, C.byref(tv)))
    capi.check(capi.hip.shq_grav_refresh_oldacc(ctx.h, cm.G))
    sq.toptree_upload(ctx, dom, tl)
    counts, table = sq.grav_toptree_exports(ctx, gp, s["n"])
    assert len(table) > 0
    q = np.zeros(len(table), dtype=capi.GRAV_QUERY_DTYPE)
    q["Pos"] = pos[table["Index"]]
    q["OldAcc"] = oldacc[table["Index"]]
    q["NodeList"] = table["NodeList"]
    tv = full.view()
    capi.check(capi.hip.shq_tree_upload(ctx.h, C.byref(tv)))
    res = np.zeros(len(q), dtype=capi.GRAV_RESULT_DTYPE)
    nint2 = np.zeros(len(q), dtype=np.int64)
    capi.check(capi.hip.shq_grav_short_secondary(ctx.h, C.byref(gp), capi.ptr(q), len(q), capi.ptr(res), capi.ptr(nint2), 0))
    oacc2, _, onint2 = orc.grav_walk_secondary(full.Nodes_base, full.firstnode, pos, P["Mass"], q["Pos"], q["NodeList"], q["OldAcc"], gp)
    scale = np.abs(s["oacc"]).max()
    print("%s soft BOX/%d: %d queries, max |acc - oracle| / largest %.3e" % (shape, softdiv, len(q), np.abs(res["Acc"] * cm.G - oacc2 * cm.G).max() / scale))
    assert np.array_equal(nint2, onint2)
    assert np.abs(res["Acc"] * cm.G - oacc2 * cm.G).max() < 1e-11 * scale
