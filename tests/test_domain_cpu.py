"""The host side of the domain decomposition (shenqi_amd/csrc/domain_host.hpp through the library's C-ABI) against the plain-Python
restatement of libgadget/domain.cpp in tests/domain_restated.py: the key automaton recovered from a key function, and the serial stages
domain_toptree_merge, domain_global_refine + domain_create_topleaves, domain_assign_topleaves_balanced + domain_set_task_leafs +
domain_check_memory_bound.  Every comparison is integer equality."""
import ctypes as C

import numpy as np
import pytest

import domain_restated as dr
import ref_outputs as ro
from shenqi_amd import capi
from shenqi_amd.dist import GpuDomainOps

NTASKS = (1, 2, 3, 5, 8)


@pytest.fixture(scope="module")
def tab():
    return dr.tables()


def host_key(t, x, y, z, bits):
    return int(capi.hip.shq_peano_key_host(C.byref(t), int(x), int(y), int(z), bits))


def test_tables_have_24_states_and_reproduce_the_small_key_tables(tab):
    t, nxt, sub = tab
    assert t.nstates == 24 and nxt.shape == (24, 8) and sub.shape == (24, 8)
    p = ro.peano()
    for bits in ro.HK_BITS:
        m = 1 << bits
        for x in range(m):
            for y in range(m):
                for z in range(m):
                    assert host_key(t, x, y, z, bits) == p.hilbert_key(x, y, z, bits)
    # the restatement's vectorised walk is the same automaton
    g = np.array([[x, y, z] for x in range(8) for y in range(8) for z in range(8)])
    assert np.array_equal(dr.peano_key(nxt, sub, g[:, 0], g[:, 1], g[:, 2], 3), [p.hilbert_key(x, y, z, 3) for x, y, z in g])


def test_stored_tables_are_the_derived_ones(tab):
    """tests/golden/ref_domain.npz against the derivation from the built reference function, wherever both exist; everywhere: deriving
    from a function that walks the tables gives the tables back (24 states, numbered in the same breadth-first order)"""
    t, nxt, sub = tab
    g = np.load(dr.DOMAIN_GOLD)
    assert np.array_equal(g["next"], nxt) and np.array_equal(g["sub"], sub)
    nl, sl = nxt.tolist(), sub.tolist()

    def walk(x, y, z, bits):
        key = s = 0
        for b in range(bits - 1, -1, -1):
            o = (((x >> b) & 1) << 2) | (((y >> b) & 1) << 1) | ((z >> b) & 1)
            key, s = (key << 3) | sl[s][o], nl[s][o]
        return key
    back = capi.peano_tables_from_key(walk)
    n2, s2 = capi.peano_tables_to_arrays(back)
    assert back.nstates == 24 and np.array_equal(n2, nxt) and np.array_equal(s2, sub)


def test_keys_at_21_bits_equal_the_reference(tab):
    t, nxt, sub = tab
    lib = ro.peano_lib()
    if lib is not None:
        xyz = np.random.default_rng(11).integers(0, 1 << 21, (4096, 3))
        want = np.array([lib.ref_peano_hilbert_key(int(a), int(b), int(c), 21) for a, b, c in xyz], dtype=np.uint64)
        assert np.array_equal(dr.peano_key(nxt, sub, xyz[:, 0], xyz[:, 1], xyz[:, 2]), want)
        assert all(host_key(t, *xyz[i], 21) == int(want[i]) for i in range(0, 4096, 16))
    for box in dr.KEY_BOXES:                      # the reference's PEANO(): built, or stored
        pos = dr.key_positions(box)
        want = dr.reference_PEANO(pos, box)
        assert np.array_equal(dr.PEANO(nxt, sub, pos, box), want)
        g = dr.grid_coords(pos, box)
        assert all(host_key(t, *g[i], 21) == int(want[i]) for i in range(0, len(pos), 8))


@pytest.mark.parametrize("fn", [lambda x, y, z, b: x ^ (y << 21), lambda x, y, z, b: (x * 2654435761 + y * 40503 + z) & ((1 << (3 * b)) - 1)])
def test_a_function_that_is_no_small_automaton_is_refused(fn):
    t = capi.PeanoTables()
    cb = capi.PEANO_KEYFN(fn)
    assert capi.hip.shq_peano_tables_from_key(C.cast(cb, C.c_void_p), C.byref(t)) == 1      # SHQ_ERR_INVALID
    assert t.nstates == 0


# ---- the serial stages ------------------------------------------------------------------------------------------------------------
def sample_sets(seed, nranks, kind):
    """sorted sample keys split across nranks the way the global sort leaves them"""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(40, 400))
    if kind == "uniform":
        k = rng.integers(0, 1 << 63, n, dtype=np.uint64)
    elif kind == "clustered":
        k = np.concatenate([rng.integers(0, 1 << 63, n // 4, dtype=np.uint64), np.uint64(0x1234567 << 36) + rng.integers(0, 1 << 30, n, dtype=np.uint64)])
    else:   # repeated keys: the chain down to Shift 0
        k = np.repeat(rng.integers(0, 1 << 63, n // 3, dtype=np.uint64), 3)
    k = np.sort(k)
    cuts = np.sort(rng.integers(0, len(k) + 1, nranks - 1))
    return np.split(k, cuts)


def local_trees(seed, nranks, kind, ntopleaves=12):
    sets = sample_sets(seed, nranks, kind)
    limit = sum(len(s) for s in sets) // ntopleaves
    return [dr.local_toptree(s, limit, limit, 10 ** 6) for s in sets], limit


def same(a, b, fields):
    return len(a) == len(b) and all(np.array_equal(a[f], b[f]) for f in fields)


LOCAL_FIELDS = ("StartKey", "Shift", "Daughter", "Parent", "Count", "Cost")


def merged_pair(seed, ntask, kind):
    """the combine order of NTask ranks through the library and through the restatement; -> (library tree, restated tree, limit)"""
    trees, limit = local_trees(seed, ntask, kind)
    lib = [dr.to_array(t) for t in trees]
    ref = [[dict(nd) for nd in t] for t in trees]
    big = 10 ** 5
    for recv, send in dr.combine_order(ntask):
        lib[recv] = GpuDomainOps.merge(lib[recv], lib[send], big)
        dr.merge(ref[recv], ref[send], big)
    return lib[0], ref[0], limit


@pytest.mark.parametrize("kind", ["uniform", "clustered", "repeated"])
@pytest.mark.parametrize("ntask", NTASKS)
def test_merge_and_finish_equal_the_restatement(ntask, kind):
    for seed in (1, 2, 3):
        got, ref, limit = merged_pair(100 * ntask + seed, ntask, kind)
        assert same(got, dr.to_array(ref), LOCAL_FIELDS)
        # finish: to find what it needs, then exactly that many nodes (succeeds) and one fewer (retry), library and restatement alike
        N, L = dr.finish([dict(nd) for nd in ref], 10 ** 5, limit, limit)
        need = len(N)
        for maxtop, ok in [(10 ** 5, True), (need, True)] + ([(need - 1, False)] if need > len(ref) else []):
            r = dr.finish([dict(nd) for nd in ref], maxtop, limit, limit)
            g = GpuDomainOps.finish(got, maxtop, limit, limit)
            assert (r is not None) == ok and (g is not None) == ok
            if ok:
                assert same(g[0], r[0], ("StartKey", "Daughter", "Shift", "Leaf"))
                assert np.array_equal(g[1]["topnode"][:-1], r[1]["topnode"][:-1]) and len(g[1]) == len(r[1])


def test_merge_without_room_is_refused_not_fatal():
    trees, _ = local_trees(7, 2, "clustered")
    A, B = dr.to_array(trees[0]), dr.to_array(trees[1])
    full = GpuDomainOps.merge(A, B, 10 ** 5)
    assert len(full) > len(A)                                       # the merge has to create daughters in A
    for maxtop in (len(full), len(full) - 1, len(A)):
        ref = [dict(nd) for nd in trees[0]]
        try:
            dr.merge(ref, trees[1], maxtop)
            ref = dr.to_array(ref)
        except dr.OutOfNodes:
            ref = None
        got = GpuDomainOps.merge(A, B, maxtop)
        assert (got is None) == (ref is None) == (maxtop < len(full))
        if got is not None:
            assert same(got, ref, LOCAL_FIELDS)


def lib_balance(N, L, count, ntask, maxpart, setaside=1.0):
    N, L = N.copy(), L.copy()
    Tasks = np.zeros(ntask + 1, dtype=capi.TASK_LEAFS_DTYPE)
    status = C.c_int(-1)
    count = np.ascontiguousarray(count, dtype=np.int64)
    rc = capi.hip.shq_domain_balance(N.ctypes.data, len(N), L.ctypes.data, len(L) - 1, count.ctypes.data, ntask, maxpart, setaside, Tasks.ctypes.data, C.byref(status))
    return rc, N, L, Tasks, status.value


def check_balance(N, L, count, ntask, maxpart):
    rN, rL = N.copy(), L.copy()
    rT, rstatus = dr.balance(rN, rL, count, ntask, maxpart)
    rc, gN, gL, gT, gstatus = lib_balance(N, L, count, ntask, maxpart)
    assert rc == 0 and gstatus == rstatus
    assert np.array_equal(gN["Leaf"], rN["Leaf"]) and np.array_equal(gL["Task"], rL["Task"]) and np.array_equal(gL["topnode"], rL["topnode"])
    assert np.array_equal(gT["StartLeaf"][:ntask], rT["StartLeaf"][:ntask]) and np.array_equal(gT["EndLeaf"][:ntask], rT["EndLeaf"][:ntask])
    assert gL["Task"][-1] == ntask and gL["topnode"][-1] == -1       # the sentinel entry
    assert set(gL["Task"][:-1]) == set(range(ntask))                  # every task holds a leaf
    return dr.balance.nrounds, rstatus


@pytest.mark.parametrize("ntask", NTASKS)
def test_balance_equals_the_restatement(ntask):
    rng = np.random.default_rng(50 + ntask)
    for seed, kind in enumerate(["uniform", "clustered", "repeated"]):
        _, ref, limit = merged_pair(900 + 10 * ntask + seed, ntask, kind)
        N, L = dr.finish(ref, 10 ** 5, limit, limit)
        ntl = len(L) - 1
        if ntl < ntask:
            continue
        for cost in (rng.integers(0, 1000, ntl), np.where(rng.random(ntl) < 0.6, 0, rng.integers(1, 50, ntl)), np.zeros(ntl, dtype=np.int64)):
            total = int(np.sum(cost))
            check_balance(N, L, cost, ntask, total + 1)
            if total > 0:                                              # a memory bound exceeded: no task can hold 1 / NTask of the particles
                assert check_balance(N, L, cost, ntask, total // ntask - 1 if total // ntask > 1 else 0)[1] == 1


def test_balance_just_enough_leaves_and_one_heavy_leaf():
    root = [dr.new_node(Count=800, Cost=800)]
    N, L = dr.finish(root, 100, 200, 200)                                  # the root split once: eight leaves
    assert len(L) - 1 == 8
    one = dr.to_array([dr.new_node(Count=800, Cost=800)])
    assert GpuDomainOps.finish(one, 9, 200, 200) is not None and GpuDomainOps.finish(one, 8, 200, 200) is None    # filled exactly / one short
    assert dr.finish([dr.new_node(Count=800, Cost=800)], 8, 200, 200) is None
    nrounds, _ = check_balance(N, L, np.arange(8) * 10 + 1, 8, 10 ** 6)   # NTopLeaves == NTask: one leaf per task from the start
    assert nrounds == 1
    N, L = dr.finish([dr.new_node(Count=6400, Cost=6400)], 1000, 200, 200)
    assert len(L) - 1 == 64
    for ntask in (2, 3, 5):
        cost = np.ones(64, dtype=np.int64)
        cost[3] = 100000                                               # one leaf holds most of the cost
        check_balance(N, L, cost, ntask, 10 ** 6)
        # With one segment per task every segment ends a task, and the last segment of the first round closes only when what is
        # left is at most half the next leaf's cost: never for a leaf with a cost.  So the first round takes every costly leaf, and
        # zero-cost leaves behind them (curload stays 0: all appended to one segment) fall to task 0 after it; a second full round
        # cannot be reached, whatever the costs.
        cost[8:] = 0
        nrounds, _ = check_balance(N, L, cost, ntask, 10 ** 6)
        assert nrounds == 1


def test_balance_refuses_fewer_leaves_than_tasks():
    N, L = dr.finish([dr.new_node(Count=800, Cost=800)], 100, 200, 200)
    rc, *_ = lib_balance(N, L, np.ones(8, dtype=np.int64), 9, 100)
    assert rc == 1
