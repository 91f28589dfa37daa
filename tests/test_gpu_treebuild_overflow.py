"""GPU tests of the device tree build's node-pool retry (csrc/tree_build.hip): the first attempt reserves 0.6 n + 4096 nodes, a
tree that needs more ends the attempt on the device and the host doubles the pool and builds again (up to 5 attempts).  Every tree
that went through a retry must equal, field by field, the host builder's (pinned to the reference's insertion build by
test_oracle_cpu.py) and the build that did not retry: a retry that keeps anything of a failed attempt shows up here.
shq_set_tree_debug forces the retry at chosen pool sizes; the context is session-wide, so every test puts the default back."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import shenqi_amd as sq
from shenqi_amd import capi
import common as cm
import orc
import test_gpu_toptree_build as ttb
import toptree_build_checks as chk
from test_gpu_treebuild import canonical, preorder, _positions
from toptree_build_checks import tb

pytestmark = pytest.mark.gpu

SHQ_ERR_STATE = 4
N_CLUMP = 200000


@contextlib.contextmanager
def node_cap(ctx, cap):
    sq.set_tree_debug(ctx, cap)
    try:
        yield
    finally:
        sq.set_tree_debug(ctx, 0)


def expected_attempts(cap, nn):
    """the pool doubles until it holds the nn nodes of the tree"""
    k = 1
    while cap < nn:
        cap *= 2
        k += 1
    return k


def _upload(ctx, pman):
    pv = pman.view()
    capi.check(capi.hip.shq_particles_upload(ctx.h, C.byref(pv)))


def _clumps():
    pos, mass = cm.clump_positions(N_CLUMP, seed=0)
    pman = cm.make_partmanager(pos)
    pman.Base["Mass"] = mass
    return pos, pman


def _assert_same_tree(ref_nodes, ref_first, nodes, first, what=""):
    a, b = canonical(ref_nodes, ref_first), canonical(nodes, first)
    assert len(a["len"]) == len(b["len"]), what
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k)


def _father_ranks(nodes, firstnode, father):
    """the particles' leaves as pre-order ranks (the host numbers its nodes in creation order, the device in pre-order)"""
    order = preorder(nodes, firstnode)
    rank = np.full(len(nodes), -1, dtype=np.int64)
    rank[order] = np.arange(len(order))
    return np.where(father >= firstnode, rank[np.clip(father - firstnode, 0, len(nodes) - 1)], -1)


def test_clump_tree_overflows_first_pool_and_equals_host(ctx):
    """Tight clumps need ~1.3 nodes per particle: the device build retries on its own and still makes the host's tree, Father
    array included; the walks over it count the oracle's interactions and agree with its forces."""
    from test_forcetree_cpu import father_of
    pos, pman = _clumps()
    n = len(pos)
    host = sq.force_tree_full(pman)
    _upload(ctx, pman)
    st = sq.tree_build_device(ctx, cm.BOX)
    attempts = sq.tree_build_attempts(ctx)
    assert attempts >= 2, attempts
    nn = len(preorder(host.Nodes_base, host.firstnode))
    assert attempts == expected_attempts(int(0.6 * n) + 4096, nn)
    assert st.nparticles == n and st.numnodes == nn
    dnodes, father = sq.tree_download(ctx, host.firstnode, n)
    _assert_same_tree(host.Nodes_base, host.firstnode, dnodes, host.firstnode)
    assert np.array_equal(_father_ranks(host.Nodes_base, host.firstnode, father_of(host, n)),
                          _father_ranks(dnodes, host.firstnode, father))

    cm.reference_treepar(ErrTolForceAcc=0.005, MaxBHOpeningAngle=0.9, Rcut=6.0, TreeUseBH=1)
    sq.gravshort_set_softenings(cm.BOX / np.cbrt(n))
    gp = sq.make_grav_params(cm.BOX, 1.5, 64, cm.G, cm.RHO0)
    oacc, _, onint = orc.grav_walk(dnodes, host.firstnode, pos, pman.Base["Mass"], np.zeros(n), gp)
    oacc = oacc * cm.G
    for mode in (sq.WALK_EXACT, sq.WALK_EXACT | sq.WALK_TREE_ORDER):   # the second is the resident step's launch
        capi.check(capi.hip.shq_grav_short_run(ctx.h, C.byref(gp), None, 0, 1, mode))
        acc = np.zeros((n, 3)); nint = np.zeros(n, dtype=np.int64)
        capi.check(capi.hip.shq_grav_short_download(ctx.h, capi.ptr(acc), None, capi.ptr(nint), None))
        assert np.array_equal(nint, onint), mode
        assert np.abs(acc - oacc).max() <= 1e-11 * np.abs(oacc).max(), mode


@pytest.mark.parametrize("kind", ["cluster", "close"])
def test_forced_overflow_at_each_boundary(ctx, kind):
    """The first pool at 1 node (every attempt overflows on the top levels: the limit of 5 attempts ends the build), at
    ceil(nn / 16) (the fifth attempt fits), nn // 3 (overflow in a middle level), nn - 1 (overflow on the last node) and nn
    (fits exactly: pins the off-by-one of the capacity test).  Every tree equals the unforced build and the host's."""
    n = 16**3 if kind == "close" else 24**3
    pos = _positions(kind, n)
    n = len(pos)
    pman = cm.make_partmanager(pos)
    pman.Base["Mass"] = (1.0 + np.random.default_rng(3).random(n)).astype(np.float32)
    host = sq.force_tree_full(pman)
    _upload(ctx, pman)
    st = sq.tree_build_device(ctx, cm.BOX)
    assert sq.tree_build_attempts(ctx) == 1
    nn = int(st.numnodes)
    ref, _ = sq.tree_download(ctx, host.firstnode, 0)
    _assert_same_tree(host.Nodes_base, host.firstnode, ref, host.firstnode)
    assert nn > 16
    with node_cap(ctx, 1):
        with pytest.raises(sq.ShqError, match="node pool overflow"):
            sq.tree_build_device(ctx, cm.BOX)
        assert sq.tree_build_attempts(ctx) == 5
    for cap in (-(-nn // 16), nn // 3, nn - 1, nn):
        with node_cap(ctx, cap):
            st = sq.tree_build_device(ctx, cm.BOX)
            assert sq.tree_build_attempts(ctx) == expected_attempts(cap, nn), cap
        assert st.numnodes == nn and st.nparticles == n
        dnodes, _ = sq.tree_download(ctx, host.firstnode, 0)
        for k in ref.dtype.names:                                     # every field of every node, as the unforced build
            assert np.array_equal(dnodes[k], ref[k]), (cap, k)
        _assert_same_tree(host.Nodes_base, host.firstnode, dnodes, host.firstnode, cap)
    assert expected_attempts(nn - 1, nn) == 2 and expected_attempts(nn, nn) == 1


def test_mask_active_and_hmax_through_retry(ctx):
    """test_device_tree_mask_and_active's selections under a forced small pool equal force_tree_rebuild_mask; the close lattice's
    gas tree with resident Hsml passes the reference's check_tree / check_moments / check_hmax after a retry."""
    n = 20**3
    pos = sq.synth_positions("cluster", n, L=cm.BOX)
    pman = cm.make_partmanager(pos)
    rng = np.random.default_rng(11)
    P = pman.Base
    P["Type"] = rng.choice([0, 1, 4, 5], size=n).astype(np.uint8)
    flags = np.zeros(n, dtype=np.uint8)
    flags[rng.random(n) < 0.05] |= 1   # IsGarbage
    flags[rng.random(n) < 0.05] |= 2   # Swallowed
    P["Flags"] = flags
    P["Hsml"] = 0.02 * cm.BOX * (0.5 + rng.random(n))
    active = np.sort(rng.choice(n, size=n // 2, replace=False)).astype(np.int32)
    _upload(ctx, pman)
    sq.dynamics_upload(ctx, pman)
    for mask, act in ((sq.GASMASK, None), (sq.GASMASK + sq.BHMASK, active)):
        host = sq.force_tree_rebuild_mask(pman, mask, act)
        nn = len(preorder(host.Nodes_base, host.firstnode))
        cap = max(1, nn // 5)
        with node_cap(ctx, cap):
            st = sq.tree_build_device(ctx, cm.BOX, mask, act)
            assert sq.tree_build_attempts(ctx) == expected_attempts(cap, nn) >= 2, mask
        assert st.numnodes == nn
        dnodes, _ = sq.tree_download(ctx, host.firstnode, 0)
        assert canonical(host.Nodes_base, host.firstnode)["hmax"].max() > 0
        _assert_same_tree(host.Nodes_base, host.firstnode, dnodes, host.firstnode, mask)

    import forcetree_checks as ft
    from test_forcetree_cpu import positions, hsml_table
    pos = positions("close", 64)
    n = len(pos)
    pman = cm.make_partmanager(pos, ptype=0)
    pman.Base["Hsml"] = hsml_table(n)
    _upload(ctx, pman)
    sq.dynamics_upload(ctx, pman)
    with node_cap(ctx, n // 8):
        st = sq.tree_build_device(ctx, cm.BOX, mask=sq.GASMASK)
        assert sq.tree_build_attempts(ctx) >= 2
    assert st.nparticles == n
    nodes, father = sq.tree_download(ctx, n, n)
    nreal = ft.check_tree(nodes, n, father, pos)
    assert abs(nodes["mass"][0] - n) < 0.5
    ft.check_moments(nodes, n, father, pman.Base["Mass"], cm.BOX, nreal)
    ft.check_hmax(nodes, n, father, pos, pman.Base["Hsml"])


@pytest.fixture
def forced_domain_retry(ctx, monkeypatch):
    """every sq.tree_build_domain call of the test builds with a first pool of a fifth of (particles + TopNodes): it retries, and
    the fifth attempt holds more than any tree of those inputs.  Yields the attempt counts of the calls."""
    seen = []
    real = sq.tree_build_domain

    def build(c, BoxSize, geo, topleaves, ThisTask, firstnode, mask=None, active=None):
        with node_cap(c, max(1, (int(firstnode) + len(geo)) // 5)):
            out = real(c, BoxSize, geo, topleaves, ThisTask, firstnode, mask, active)
            seen.append(sq.tree_build_attempts(c))
        return out

    monkeypatch.setattr(sq, "tree_build_domain", build)
    yield seen


@pytest.mark.parametrize("seed,ntask,maxdepth", [(1, 3, 2), (2, 4, 3), (3, 2, 1)])
def test_domain_tree_through_retry(ctx, forced_domain_retry, seed, ntask, maxdepth):
    """test_domain_tree_equals_reference_build under a forced small pool: trees, top-leaf moments and pseudo-node links equal the
    reference build's before and after the exchange"""
    ttb.test_domain_tree_equals_reference_build(ctx, seed, ntask, maxdepth)
    assert forced_domain_retry and min(forced_domain_retry) >= 2, forced_domain_retry


def test_domain_deep_top_tree_through_retry(ctx, forced_domain_retry):
    ttb.test_domain_tree_deep_top_tree_many_tasks(ctx)
    assert forced_domain_retry and min(forced_domain_retry) >= 2, forced_domain_retry


def test_domain_complete_top_tree_few_local_gas_retries_on_its_own(ctx):
    """A gas tree on a gas-poor rank: a complete top tree of depth 4 (4681 TopNodes, every one a tree node) over a few hundred
    local gas particles needs more than 0.6 n + 4096 nodes.  No knob: the build retries, equals the reference build and does not
    report a foreign particle (Bad topleaf)."""
    rng = np.random.default_rng(21)
    geo, tl = cm.make_topnodes(rng, 2, maxdepth=4, psplit=1.0)
    assert len(geo) == 4681
    me = 1
    pos = rng.random((4000, 3)) * cm.BOX
    pos = pos[tl["Task"][cm.topleaf_of(pos, geo, cm.BOX)] == me][:800]
    n = len(pos)
    ptype = np.where(np.arange(n) % 8 < 3, 0, 1).astype(np.uint8)      # 300 gas among 800
    gas = np.flatnonzero(ptype == 0)
    assert len(gas) > 250 and 0.6 * len(gas) + 4096 < len(geo)          # the first pool cannot hold the TopNodes alone
    mass = rng.choice([1.0, 0.25, 3.0], size=n)
    hsml = 0.02 * cm.BOX * (1 + rng.random(n))
    pman = cm.make_partmanager(pos)
    P = pman.Base
    P["Type"], P["Mass"], P["Hsml"] = ptype, mass, hsml
    _upload(ctx, pman)
    sq.dynamics_upload(ctx, pman)
    firstnode = n + 5
    tl_dev = tl.copy()
    st, mom = sq.tree_build_domain(ctx, cm.BOX, geo, tl_dev, me, firstnode, mask=sq.GASMASK)
    assert sq.tree_build_attempts(ctx) >= 2
    assert st.nparticles == len(gas) and st.numnodes > 0.6 * len(gas) + 4096
    nodes, father = sq.tree_download(ctx, firstnode, numpart=n)
    hs = [float(h) if t in (0, 5) else None for h, t in zip(P["Hsml"], P["Type"])]
    lastnode_orc = firstnode + 20 * n + 10 * len(geo)
    t, ltn, omom = tb.build([[float(x) for x in p] for p in pos], [float(m) for m in P["Mass"]], hs, [int(i) for i in gas],
                            chk.geo_list(geo), [int(x) for x in tl["Task"]], me, cm.BOX, firstnode, lastnode_orc)
    number = chk.compare(nodes, firstnode, firstnode + len(nodes), t, lastnode_orc, moments=False)
    for k, (no, nd) in enumerate(tb.preorder(t)):
        if not nd.InternalTopLevel and nd.ChildType != tb.PSEUDO:
            g = nodes[k]
            assert g["mass"] == nd.mass and tuple(g["cofm"]) == tuple(nd.cofm) and g["hmax"] == nd.hmax, k
    for l in range(len(tl)):
        assert tl_dev["treenode"][l] == number[ltn[l]], l
        s, m, h = omom[l]
        assert tuple(mom["s"][l]) == tuple(s) and mom["mass"][l] == m and mom["hmax"][l] == h, l
    assert np.all(father[ptype != 0] == -1) and np.all(father[gas] >= firstnode)


def test_attempt_limit_fails_loudly_and_context_recovers(ctx):
    """A first pool of 1 node is still too small after 5 attempts: the build raises, leaves no tree to walk (SHQ_ERR_STATE, not
    half a tree), and the next build with the default pool equals the host tree."""
    pos, pman = _clumps()
    n = len(pos)
    _upload(ctx, pman)
    with node_cap(ctx, 1):
        with pytest.raises(sq.ShqError, match="node pool overflow"):
            sq.tree_build_device(ctx, cm.BOX)
        assert sq.tree_build_attempts(ctx) == 5
    cm.reference_treepar(ErrTolForceAcc=0.005, MaxBHOpeningAngle=0.9, Rcut=6.0, TreeUseBH=1)
    sq.gravshort_set_softenings(cm.BOX / np.cbrt(n))
    gp = sq.make_grav_params(cm.BOX, 1.5, 64, cm.G, cm.RHO0)
    assert capi.hip.shq_grav_short_run(ctx.h, C.byref(gp), None, 0, 1, sq.WALK_EXACT) == SHQ_ERR_STATE
    host = sq.force_tree_full(pman)
    sq.tree_build_device(ctx, cm.BOX)
    assert sq.tree_build_attempts(ctx) >= 2
    dnodes, _ = sq.tree_download(ctx, host.firstnode, 0)
    _assert_same_tree(host.Nodes_base, host.firstnode, dnodes, host.firstnode)


def test_dist_driver_keeps_retried_build_on_device(ctx):
    """DistTreePM on one rank over the clumps: the build retries on the device instead of falling back to a host build (no
    self.pman), makes the host's tree, and the step's tree forces have the bits of the same walk over the host-built tree."""
    from shenqi_amd import dist as sd
    pos, pman = _clumps()
    posm = np.concatenate([pos, pman.Base["Mass"].astype(np.float64)[:, None]], axis=1)
    dev = torch.device("cuda", 0)
    nmesh = 48
    cm.reference_treepar(ErrTolForceAcc=0.005, MaxBHOpeningAngle=0.9, Rcut=6.0, TreeUseBH=1)
    sq.gravshort_set_softenings(cm.BOX / np.cbrt(N_CLUMP))
    gp = sq.make_grav_params(cm.BOX, 1.5, nmesh, cm.G, cm.RHO0)
    dctx = sq.Context(0)
    try:
        comm = sd.Comm()
        drv = sd.DistTreePM(comm, dctx, nmesh, cm.BOX, 1.5, cm.G, dev, halo_factor=1.3)
        local = sd.exchange_to_owner(comm, drv.decomp, torch.from_numpy(posm).to(dev))
        drv.setup(local, gp.Rcut)
        assert not hasattr(drv, "pman")
        assert sq.tree_build_attempts(dctx) >= 2
        allp = drv.allp.cpu().numpy()
        m = len(allp)
        hp = cm.make_partmanager(np.ascontiguousarray(allp[:, :3]))
        hp.Base["Mass"] = allp[:, 3]
        host = sq.force_tree_full(hp)
        dnodes, _ = sq.tree_download(dctx, host.firstnode, 0)
        _assert_same_tree(host.Nodes_base, host.firstnode, dnodes, host.firstnode)
        drv.step(gp)
        acc, _, _, _ = drv.download()
    finally:
        dctx.close()
    _upload(ctx, hp)
    tv = host.view()
    capi.check(capi.hip.shq_tree_upload(ctx.h, C.byref(tv)))
    capi.check(capi.hip.shq_grav_short_run(ctx.h, C.byref(gp), None, 0, 1, sq.WALK_EXACT))
    mono = np.zeros((m, 3))
    capi.check(capi.hip.shq_grav_short_download(ctx.h, capi.ptr(mono), None, None, None))
    assert len(acc) == drv.nloc == N_CLUMP
    assert np.array_equal(acc, mono[:drv.nloc])
