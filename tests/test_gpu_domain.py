"""The domain decomposition on the device (shenqi_amd/csrc/domain.hip) against the plain-Python restatement of libgadget/domain.cpp
(tests/domain_restated.py) and, for the key, against the reference's own PEANO() (oracle/_ref where built, tests/golden/ref_domain.npz
otherwise).  Every comparison is integer equality."""
import ctypes as C
import os
import pickle
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import common as cm
import domain_restated as dr
import shenqi_amd as sq
from shenqi_amd import capi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = capi.PARTICLE_DTYPE.fields
ESZ, OFF_POS, OFF_FLAGS, OFF_TOPLEAF = capi.PARTICLE_DTYPE.itemsize, F["Pos"][1], F["Flags"][1], F["TopLeaf"][1]


@pytest.fixture(scope="module")
def tab():
    return dr.tables()


def records(pos, garbage=None, types=None):
    P = np.zeros(len(pos), dtype=capi.PARTICLE_DTYPE)
    P["Pos"] = pos
    P["ID"] = np.arange(len(pos))
    P["TopLeaf"] = -7
    P["Type"] = 1 if types is None else types
    if garbage is not None:
        P["Flags"] = np.asarray(garbage, dtype=np.uint8)
    return P


def settled(t):
    """torch fills and copies run on torch's stream, the library's kernels on its own non-blocking one: finish the former before
    the tensor is handed to the library"""
    torch.cuda.synchronize()
    return t


def dev(a):
    return settled(torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(DEV))


def parts_view(d_parts, n, box):
    return capi.DomainParts(d_parts.data_ptr(), ESZ, OFF_FLAGS, OFF_POS, n, box)


def device_keys(ctx, t, pos, box):
    d_pos = torch.from_numpy(np.ascontiguousarray(pos, dtype=np.float64)).to(DEV)
    d_keys = settled(torch.zeros(len(pos), dtype=torch.int64, device=DEV))
    capi.check(capi.hip.shq_peano_keys(ctx.h, C.byref(t), d_pos.data_ptr(), 24, len(pos), box, d_keys.data_ptr()))
    ctx.synchronize()
    return d_keys.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("box", dr.KEY_BOXES)
def test_keys_equal_the_reference(ctx, tab, box):
    """PEANO() bit for bit: random positions, 0, Box (1 - 2^-52), and positions on and next to exact cell boundaries of the 2^21 grid;
    from a packed array and from inside particle records"""
    t, nxt, sub = tab
    pos = dr.key_positions(box)
    want = dr.reference_PEANO(pos, box)
    assert np.array_equal(device_keys(ctx, t, pos, box), want)
    d_parts = dev(records(pos))
    d_keys = settled(torch.zeros(len(pos), dtype=torch.int64, device=DEV))
    capi.check(capi.hip.shq_peano_keys(ctx.h, C.byref(t), d_parts.data_ptr() + OFF_POS, ESZ, len(pos), box, d_keys.data_ptr()))
    ctx.synchronize()
    assert np.array_equal(d_keys.cpu().numpy().view(np.uint64), want)
    assert len(np.unique(want >> np.uint64(60))) == 8 and want.max() < (1 << 63)


def device_samples(ctx, t, d_parts, n, box, dist_, presort):
    out = settled(torch.full((n // dist_ + 1,), -1, dtype=torch.int64, device=DEV))
    ns = C.c_int64(-1)
    capi.check(capi.hip.shq_domain_samples(ctx.h, C.byref(t), C.byref(parts_view(d_parts, n, box)), dist_, presort, out.data_ptr(), C.byref(ns)))
    ctx.synchronize()
    return out.cpu().numpy().view(np.uint64)[:ns.value]


def test_samples_equal_the_restatement(ctx, tab):
    t, nxt, sub = tab
    box = 25000.0
    rng = np.random.default_rng(5)
    for n in (1, 255, 257, 5000):
        pos = rng.random((n, 3)) * box
        for gkind in ("none", "interleaved", "all"):
            garbage = {"none": np.zeros(n, bool), "interleaved": (np.arange(n) % 3 == 0) | (rng.random(n) < 0.2), "all": np.ones(n, bool)}[gkind]
            d_parts = dev(records(pos, garbage))
            keys = dr.PEANO(nxt, sub, pos, box)
            for dist_ in (1, 2, 256):
                for presort in (0, 1):
                    want = dr.samples(keys, garbage, dist_, presort)
                    got = device_samples(ctx, t, d_parts, n, box, dist_, presort)
                    assert np.array_equal(got, want), (n, gkind, dist_, presort)
                    if gkind == "all":
                        assert len(got) == 0
                    if gkind == "none" and n < dist_:
                        assert len(got) == 1


def device_local_toptree(ctx, lp, countlimit, costlimit, maxtop):
    d = settled(torch.from_numpy(np.ascontiguousarray(lp, dtype=np.uint64).view(np.int64).copy()).to(DEV))
    tree = np.zeros(maxtop, dtype=capi.LOCAL_TOPNODE_DTYPE)
    tree["Shift"] = -99                                                     # a mark: what the call does not write stays
    size = C.c_int(-1)
    rc = capi.hip.shq_domain_local_toptree(ctx.h, d.data_ptr(), len(lp), countlimit, costlimit, maxtop, tree.ctypes.data, C.byref(size))
    return rc, tree, size.value


def tree_cases():
    rng = np.random.default_rng(9)
    few = rng.integers(0, 1 << 63, 5, dtype=np.uint64)
    cell = np.uint64(0o1234567 << 42)                                       # seven leading digits: one depth-7 cell
    return {
        "one sample": np.array([12345678901234], dtype=np.uint64),
        "two identical keys": np.array([0o777 << 30] * 2, dtype=np.uint64),
        "three copies each": np.sort(np.repeat(few, 3)),
        "one depth-7 cell": np.sort(cell + rng.integers(0, 1 << 42, 300, dtype=np.uint64)),
        "uniform 5000": np.sort(rng.integers(0, 1 << 63, 5000, dtype=np.uint64)),
        "clustered": np.sort(np.concatenate([rng.integers(0, 1 << 63, 200, dtype=np.uint64), np.uint64(5 << 58) + rng.integers(0, 1 << 20, 800, dtype=np.uint64)])),
    }


@pytest.mark.parametrize("name", list(tree_cases()))
def test_local_toptree_equals_the_serial_loop(ctx, name):
    """node for node (StartKey, Shift, Daughter, Parent, Count, Cost) the tree of the reference's serial loop, for limits 0 (nothing
    truncated), in between, and above the total (root only); MaxTopNodes equal to the skeleton size succeeds, one less is the retry code
    and leaves the caller's array alone"""
    lp = tree_cases()[name]
    skel = dr.skeleton(lp, 10 ** 7)
    if name == "two identical keys":
        assert len(skel) == 169                                             # the chain down to Shift 0
    for limit in (0, max(len(lp) // 20, 2), len(lp) + 1):
        want = dr.to_array(dr.local_toptree(lp, limit, limit, 10 ** 7))
        for maxtop in (len(skel) + 50, len(skel)):
            rc, tree, size = device_local_toptree(ctx, lp, limit, limit, maxtop)
            assert rc == 0 and size == len(want)
            for f in ("StartKey", "Shift", "Daughter", "Parent", "Count", "Cost"):
                assert np.array_equal(tree[f][:size], want[f]), (name, limit, f)
            assert (tree["Shift"][size:] == -99).all()
        if limit > len(lp):
            assert len(want) == 1
        if limit == 0:
            assert len(want) == len(skel)
    # countlimit and costlimit are separate bounds: a node goes only when it is below both
    want = dr.to_array(dr.local_toptree(lp, 3, len(lp) + 1, 10 ** 7))
    rc, tree, size = device_local_toptree(ctx, lp, 3, len(lp) + 1, len(skel))
    assert rc == 0 and size == len(want) and np.array_equal(tree["Daughter"][:size], want["Daughter"])
    if len(skel) > 1:
        rc, tree, size = device_local_toptree(ctx, lp, 0, 0, len(skel) - 1)
        assert rc == capi.ERR_RETRY and size == -1 and (tree["Shift"] == -99).all()
        assert dr.skeleton(lp, len(skel) - 1) is None


def test_local_toptree_of_nothing_is_the_root(ctx):
    rc, tree, size = device_local_toptree(ctx, np.zeros(0, dtype=np.uint64), 0, 0, 4)
    assert rc == 0 and size == 1
    assert (tree["StartKey"][0], tree["Shift"][0], tree["Daughter"][0], tree["Parent"][0], tree["Count"][0], tree["Cost"][0]) == (0, 63, -1, -1, 0, 0)


def decomposition(nxt, sub, pos, garbage, box, ntask, ntopleaves=24):
    """TopNodes / TopLeaves / Tasks of the restatement for one set of particles (all samples on one rank)"""
    keys = dr.PEANO(nxt, sub, pos, box)
    lp = dr.samples(keys, garbage, 4, 1)
    limit = len(lp) // ntopleaves
    T = dr.local_toptree(lp, limit, limit, 10 ** 6)
    N, L = dr.finish(T, 10 ** 6, limit, limit)
    live = ~garbage
    count = np.bincount(dr.get_topleaf(N, keys[live]), minlength=len(L) - 1)
    return keys, N, L, count


def install(ctx, t, N, L, geo=None):
    capi.check(capi.hip.shq_domain_install(ctx.h, C.byref(t), N.ctypes.data, len(N), L.ctypes.data, len(L) - 1, None if geo is None else geo.ctypes.data))


@pytest.mark.parametrize("ntopleaves", [24, 20000])
def test_leaf_counts_topleaves_and_targets(ctx, tab, ntopleaves):
    """ntopleaves 20000: limit 0, the tree refined to more leaves than the LDS bins hold (the global-atomics kernel)"""
    t, nxt, sub = tab
    box = 25000.0
    rng = np.random.default_rng(21)
    n = 3000
    pos = np.concatenate([rng.random((n // 2, 3)) * box, (0.4 * box + rng.normal(0, 0.01 * box, (n - n // 2, 3))) % box])
    garbage = rng.random(n) < 0.1
    if ntopleaves > 1000:
        keys = dr.PEANO(nxt, sub, pos, box)
        T = dr.local_toptree(np.sort(keys[~garbage]), 2, 2, 10 ** 6)
        N, L = dr.finish(T, 10 ** 6, 10 ** 9, 10 ** 9)
        count = np.bincount(dr.get_topleaf(N, keys[~garbage]), minlength=len(L) - 1)
        assert len(L) - 1 > 8192
    else:
        keys, N, L, count = decomposition(nxt, sub, pos, garbage, box, 3, ntopleaves)
    d_parts = dev(records(pos, garbage))
    pv = parts_view(d_parts, n, box)
    install(ctx, t, N, L)
    got = np.full(len(L) - 1, -1, dtype=np.int64)
    capi.check(capi.hip.shq_domain_leaf_counts(ctx.h, C.byref(pv), got.ctypes.data))
    assert np.array_equal(got, count) and got.sum() == int((~garbage).sum())
    ntask = 3
    Tasks, status = dr.balance(N, L, count, ntask, n)
    install(ctx, t, N, L)                                                    # the final leaf numbers and tasks
    d_leaf = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    d_tgt = settled(torch.full((n,), -5, dtype=torch.int32, device=DEV))
    capi.check(capi.hip.shq_domain_particle_topleaves(ctx.h, C.byref(pv), d_leaf.data_ptr(), d_tgt.data_ptr()))
    ctx.synchronize()
    leaf, tgt = d_leaf.cpu().numpy(), d_tgt.cpu().numpy()
    want = dr.get_topleaf(N, keys)
    assert np.array_equal(leaf[~garbage], want[~garbage]) and (leaf[garbage] == -7).all()
    assert np.array_equal(tgt[~garbage], L["Task"][want[~garbage]]) and (tgt[garbage] == -1).all()
    assert set(tgt[~garbage]) == set(range(ntask))


def test_closure_with_tree_build_and_topleaf_maintenance(ctx, tab):
    """geo_out is the table the INTEGRATION.md loop fills with the reference's key function; shq_tree_build_domain accepts it; and after
    a drift of zero shq_domain_maintain_topleaf moves nothing: the key descent and the geometric descent name the same leaves"""
    import ref_outputs as ro
    import test_peano_ref_cpu as tp
    t, nxt, sub = tab
    rng = np.random.default_rng(33)
    n = 4000
    pos = np.concatenate([rng.random((n // 2, 3)) * cm.BOX, (0.7 * cm.BOX + rng.normal(0, 0.02 * cm.BOX, (n - n // 2, 3))) % cm.BOX])
    garbage = np.zeros(n, bool)
    keys, N, L, count = decomposition(nxt, sub, pos, garbage, cm.BOX, 1)
    dr.balance(N, L, count, 1, n)
    geo = np.zeros(len(N), dtype=capi.TOPNODE_GEO_DTYPE)
    install(ctx, t, N, L, geo)
    nodes = [dict(StartKey=int(r["StartKey"]), Shift=int(r["Shift"]), Daughter=int(r["Daughter"]), Leaf=int(r["Leaf"])) for r in N]
    depth = max((63 - nd["Shift"]) // 3 for nd in nodes)
    peano = ro.peano()
    if peano.lib is not None or depth <= max(ro.HK_BITS):
        want = tp.geo_from_topnodes(nodes, peano)
    else:                                    # the stored hilbert_key tables end at three levels: the automaton (pinned to them) goes on
        class Walk:
            @staticmethod
            def hilbert_key(x, y, z, bits):
                return int(dr.peano_key(nxt, sub, np.array([x]), np.array([y]), np.array([z]), bits)[0])
        want = tp.geo_from_topnodes(nodes, Walk)
    assert np.array_equal(geo["daughter"], want["daughter"]) and np.array_equal(geo["leaf"], want["leaf"])
    pman = cm.make_partmanager(pos)
    capi.check(capi.hip.shq_particles_upload(ctx.h, C.byref(pman.view())))
    tl = np.ascontiguousarray(L[:-1])
    sq.tree_build_domain(ctx, cm.BOX, geo, tl, 0, n + 5)
    d_parts = dev(pman.Base)
    d_leaf = settled(torch.full((n,), -1, dtype=torch.int32, device=DEV))
    capi.check(capi.hip.shq_domain_particle_topleaves(ctx.h, C.byref(parts_view(d_parts, n, cm.BOX)), d_leaf.data_ptr(), None))
    ctx.synchronize()
    before = d_leaf.cpu().numpy().copy()
    assert np.array_equal(before, dr.get_topleaf(N, keys)) and len(np.unique(before)) > 8
    nch = C.c_int64(-1)
    capi.check(capi.hip.shq_domain_maintain_topleaf(ctx.h, 1, 0, d_leaf.data_ptr(), None, C.byref(nch)))
    ctx.synchronize()
    assert nch.value == 0 and np.array_equal(d_leaf.cpu().numpy(), before)


# ---- end to end: DistDomain with the device operators -------------------------------------------------------------------------------
BOX = 25000.0
E2E_PARAMS = dict(DomainOverDecompositionFactor=4, TopNodeAllocFactor=0.01, SetAsideFactor=1.0)   # too few top nodes at first: the retry is taken
E2E_MAXPART = 6000


def e2e_share(rank, world):
    rng = np.random.default_rng(99)
    n = 4000
    pos = rng.random((n, 3)) * BOX
    pos[: n // 3] = (np.array([0.3, 0.6, 0.2]) * BOX + rng.normal(0, 0.01 * BOX, (n // 3, 3))) % BOX
    garbage = rng.random(n) < 0.05
    types = rng.choice([0, 1, 4, 5], n)
    ids = np.arange(n, dtype=np.int64)
    cls = ids % (world + 1)                                                   # an uneven split: the last rank holds two classes
    m = (cls == rank) | ((rank == world - 1) & (cls == world))
    return pos[m], garbage[m], types[m], ids[m]


def e2e_run(rank, world):
    """the same particles through DistDomain with the CPU operators and with the device operators; -> both outcomes"""
    from shenqi_amd import dist as sd
    t, nxt, sub = dr.tables()
    pos, garbage, types, ids = e2e_share(rank, world)
    comm = sd.Comm()
    cpu = dr.CpuDomainOps(nxt, sub, BOX, pos, garbage, ids, E2E_MAXPART)
    dc = sd.DistDomain(comm, cpu, E2E_PARAMS).decompose()
    P = np.zeros(E2E_MAXPART, dtype=capi.PARTICLE_DTYPE)
    P[:len(pos)] = records(pos, garbage, types)
    P["ID"][:len(pos)] = ids
    L = capi.ExchangeLayout()
    L.part_elsize, L.off_flags, L.off_type, L.off_pi = ESZ, OFF_FLAGS, F["Type"][1], F["PI"][1]
    L.off_reverselink = 0
    d_parts = dev(P)
    with sq.Context(0) as ctx:
        gpu = sd.GpuDomainOps(ctx, t, L, OFF_POS, OFF_TOPLEAF, BOX, d_parts, len(pos), [None] * 6, [0] * 6)
        dg = sd.DistDomain(comm, gpu, E2E_PARAMS).decompose()
        out = d_parts.cpu().numpy().view(capi.PARTICLE_DTYPE)[:gpu.numpart].copy()
    tables = lambda d: dict(N=d.TopNodes, L=d.TopLeaves, T=d.Tasks, policy=d.policy, factor=d.factor)   # noqa: E731
    return dict(cpu=tables(dc), gpu=tables(dg), cpu_ids=np.sort(cpu.ID), P=out, keys=dr.PEANO(nxt, sub, out["Pos"], BOX))


def e2e_check(res, rank, world):
    c, g = res["cpu"], res["gpu"]
    for f in ("StartKey", "Daughter", "Shift", "Leaf"):
        assert np.array_equal(c["N"][f], g["N"][f]), f
    assert np.array_equal(c["L"]["Task"], g["L"]["Task"]) and np.array_equal(c["L"]["topnode"], g["L"]["topnode"])
    assert np.array_equal(c["T"]["StartLeaf"][:world], g["T"]["StartLeaf"][:world]) and np.array_equal(c["T"]["EndLeaf"][:world], g["T"]["EndLeaf"][:world])
    assert c["policy"] == g["policy"] and c["factor"] == g["factor"] and g["factor"] > E2E_PARAMS["TopNodeAllocFactor"]
    P = res["P"]
    assert np.array_equal(np.sort(P["ID"].astype(np.int64)), res["cpu_ids"]) and not (P["Flags"] & 1).any()
    assert (g["L"]["Task"][P["TopLeaf"]] == rank).all()
    order = np.lexsort((res["keys"], P["Type"]))                              # sorted by (type, key)
    assert np.array_equal(res["keys"][order], res["keys"]) and np.array_equal(P["Type"][order], P["Type"])
    assert len(np.unique(P["Type"])) == 4


def test_dist_domain_one_rank(tab):
    e2e_check(e2e_run(0, 1), 0, 1)


def _worker(rank, world, initfile, outdir):
    os.environ["OMP_NUM_THREADS"] = "2"
    dist.init_process_group("gloo", init_method="file://" + initfile, rank=rank, world_size=world)
    try:
        with open(os.path.join(outdir, "e%d.pkl" % rank), "wb") as f:
            pickle.dump(e2e_run(rank, world), f)
    finally:
        dist.destroy_process_group()


def test_dist_domain_two_gloo_ranks_one_gpu():
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_worker, args=(2, os.path.join(tmp, "init"), tmp), nprocs=2, join=True)
        res = [pickle.load(open(os.path.join(tmp, "e%d.pkl" % r), "rb")) for r in range(2)]
    for r in range(2):
        e2e_check(res[r], r, 2)
    ids = np.concatenate([x["P"]["ID"].astype(np.int64) for x in res])
    assert len(np.unique(ids)) == len(ids)
    for f in ("StartKey", "Daughter", "Shift", "Leaf"):
        assert np.array_equal(res[0]["gpu"]["N"][f], res[1]["gpu"]["N"][f])
