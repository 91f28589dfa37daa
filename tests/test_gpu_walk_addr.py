"""The production walk's record fetch at 32-bit byte offsets (shq_set_walk_addr), the opened leaf's bookkeeping under the lane mask and
the ring drain's pop: the 32-bit form against the 64-bit one bit for bit, in the launch forms that reach the ring, the drain and the
hand-over; the selection rule on numbers alone.

Particle sets: S-clusters in a periodic box, 24^3 and 30^3 - 37 (a ragged last task of 19 targets).  Both have targets within a PM cell of
the box faces (non-interior nodes, the wrap vote and the wrapped leaf) and leaves of eight particles in the cluster core (the ring of 32
slots fills and is drained in mid-walk): test_particle_sets_reach_the_paths checks that on the host.  Reference for the interaction
counts: the CPU oracle, as integers; forces within 1e-11 of the oracle's largest, the bound of test_visit_paths_in_every_launch_form
for the same launch forms."""
import ctypes as C

import numpy as np
import pytest

import shenqi_amd as sq
from shenqi_amd import capi
import orc
import common as cm

# name: (particles, Nmesh)
SHAPES = {"c24": (24**3, 72), "ragged": (30**3 - 37, 90)}
# launch form: (walk_sparse, walk_overlap, the getter's answer with shq_set_walk_addr(1)).  Without the hand-over the launch is not the
# production form and keeps the 64-bit address whatever is asked for.
FORMS = {"beside": (1, 2, 1), "behind": (1, 0, 1), "no pair kernel": (0, 2, 0)}

_setups = {}


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


def _walk(ctx, s, addr, update_potential):
    """upload, one walk with the address form asked for, download; returns (acc, pot, nint, the form the launch used)"""
    pman, tree, gp = s["pman"], s["tree"], s["gp"]
    P = pman.Base
    P["FullTreeGravAccel"] = s["told"]
    P["GravPM"] = s["pold"]
    pv, tv = pman.view(), tree.view()
    capi.check(capi.hip.shq_particles_upload(ctx.h, C.byref(pv)))
    capi.check(capi.hip.shq_tree_upload(ctx.h, C.byref(tv)))
    capi.check(capi.hip.shq_grav_refresh_oldacc(ctx.h, gp.G))
    capi.check(capi.hip.shq_set_walk_addr(ctx.h, addr))
    capi.check(capi.hip.shq_grav_short_run(ctx.h, C.byref(gp), None, 0, int(update_potential), sq.WALK_EXACT))
    used = C.c_int(-1)
    capi.check(capi.hip.shq_walk_last_addr(ctx.h, C.byref(used)))
    n = pman.NumPart
    acc = np.zeros((n, 3)); pot = np.zeros(n); nint = np.zeros(n, dtype=np.int64)
    capi.check(capi.hip.shq_grav_short_download(ctx.h, capi.ptr(acc), capi.ptr(pot), capi.ptr(nint), None))
    return acc, pot, nint, used.value


def test_selection_rule_on_numbers():
    """numnodes + 1 records of 128 bytes: the last one starts at numnodes << 7, and its last piece at + 0x70 must stay below 2^32"""
    fits = capi.hip.shq_walk_addr32_fits
    assert fits(2**25 - 1) == 1          # numnodes + 1 = 2^25: the last record starts at 2^32 - 128
    assert fits(2**25) == 0              # numnodes + 1 = 2^25 + 1
    assert fits(0) == 1 and fits(1) == 1 and fits(2**25 - 2) == 1
    assert fits(2**25 + 1) == 0 and fits(2**31) == 0 and fits(2**40) == 0 and fits(-1) == 0
    for nn in (2**25 - 1, 2**25):
        assert (fits(nn) == 1) == ((nn << 7) + 0x70 + 16 <= 2**32)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_particle_sets_reach_the_paths(shape):
    """targets within a PM cell of the box faces; leaves of eight particles, and more opened-leaf particles near the core than the ring
    of 32 slots holds; the ragged shape ends in a task that is not full"""
    s = _setup(shape)
    pos, nodes = s["pos"], s["tree"].Nodes_base
    cell = cm.BOX / s["nmesh"]
    near_face = ((pos < cell) | (pos > cm.BOX - cell)).any(axis=1)
    assert near_face.sum() >= 8, near_face.sum()
    leaves = nodes[((nodes["flags"] >> 3) & 3) == 0]
    full = leaves[leaves["noccupied"] == 8]
    print("%s: %d targets within a cell of a face, %d leaves, %d of eight particles" % (shape, near_face.sum(), len(leaves), len(full)))
    assert len(full) >= 8            # five of them opened by one wave overflow the ring
    if shape == "ragged":
        assert s["n"] % 64 != 0


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("update_potential", [1, 0])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_addr32_equals_addr64_bit_for_bit(ctx, shape, update_potential, form):
    s = _setup(shape)
    sparse, overlap, want32 = FORMS[form]
    res = {}
    try:
        capi.check(capi.hip.shq_set_walk_launch(ctx.h, 2, 1))
        capi.check(capi.hip.shq_set_walk_sparse(ctx.h, sparse))
        capi.check(capi.hip.shq_set_walk_overlap(ctx.h, overlap))
        for addr in (0, 1):
            res[addr] = _walk(ctx, s, addr, update_potential)
    finally:
        capi.check(capi.hip.shq_set_walk_addr(ctx.h, 1))
        capi.check(capi.hip.shq_set_walk_overlap(ctx.h, 1))
        capi.check(capi.hip.shq_set_walk_launch(ctx.h, 1, 1))
        capi.check(capi.hip.shq_set_walk_sparse(ctx.h, 1))
    assert res[0][3] == 0, "shq_set_walk_addr(0) must keep the 64-bit address"
    assert res[1][3] == want32, (form, res[1][3])
    names = ("acc", "pot", "nint")
    for k in range(3 if update_potential else 1):
        assert np.array_equal(res[0][k], res[1][k]), (form, names[k])
    assert np.array_equal(res[0][2], res[1][2]), (form, "nint")
    scale = np.abs(s["oacc"]).max()
    for addr in (0, 1):
        acc, pot, nint, _ = res[addr]
        assert np.array_equal(nint, s["onint"]), (form, addr)
        print("%s %s pot %d addr %d: max |acc - oracle| / largest %.3e" % (shape, form, update_potential, addr, np.abs(acc - s["oacc"]).max() / scale))
        assert np.abs(acc - s["oacc"]).max() < 1e-11 * scale, (form, addr)
        if update_potential:
            assert np.allclose(pot, s["opot"], rtol=1e-10, atol=1e-10 * np.abs(s["opot"]).max()), (form, addr)
