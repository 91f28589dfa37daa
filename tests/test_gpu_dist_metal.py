"""GPU tests of the parts of the metal return a multi-rank driver needs (shq_metal_return_triples / _apply / _sums, csrc/sph_winds.hip)
and of the driver itself (shenqi_amd/dist.py:DistMetalReturn with GpuMetalOps).

In one context the parts must reproduce shq_metal_return bit for bit: same walk, same arithmetic, same order.  On two gloo ranks
sharing the GPU the reference is one context's shq_metal_return on the undivided set with the global queue (the ranks' queues one
after the other): the gas fields are bit-equal - same device arithmetic, same positions, same order - and MassReturn, summed per star
in (owner, particle) order instead of particle order, agrees to 1e-14 of its largest value.  The stellar-density stage must give the
undivided device result to 1e-9, the bar of the sharded density tests."""
import ctypes as C
import os
import pickle
import sys
import tempfile

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import shenqi_amd as sq  # noqa: E402
from shenqi_amd import capi  # noqa: E402
from shenqi_amd import dist as sd  # noqa: E402
import common as cm  # noqa: E402
import metal_dist_restated as mdr  # noqa: E402

pytestmark = pytest.mark.gpu

GAS_FIELDS = ("Density", "Metallicity", "Metals")


def one_shot(ctx, Pg, Sg, queue, rows, sphw, kt):
    """shq_metal_return on a copy of the set: (P, S, MassReturn, npairs)"""
    pman = sq.PartManager(len(Pg), cm.BOX)
    pman.Base[:] = Pg
    S = Sg.copy()
    tree = sq.force_tree_rebuild_mask(pman, sq.GASMASK)
    f = capi.SPH_DTYPE.fields
    gv = capi.GasMetalView(S.ctypes.data, S.dtype.itemsize, len(S), f["Density"][1], f["Metallicity"][1], f["Metals"][1], 9, 0)
    pv, tv = pman.view(), tree.view()
    queue = np.ascontiguousarray(queue, dtype=np.int32)
    cols = [np.ascontiguousarray(rows[:, 0]), np.ascontiguousarray(rows[:, 1]), np.ascontiguousarray(rows[:, 2]), np.ascontiguousarray(rows[:, 3:])]
    mret = np.full(len(queue), -1.0)
    npairs = C.c_int64()
    capi.check(capi.hip.shq_metal_return(ctx.h, C.byref(tv), C.byref(pv), C.byref(gv), capi.ptr(queue), len(queue), capi.ptr(cols[0]), capi.ptr(cols[1]),
                                         capi.ptr(cols[2]), capi.ptr(cols[3]), mdr.MAXGASMASS, sphw, kt, capi.ptr(mret), C.byref(npairs)))
    return pman.Base.copy(), S, mret, npairs.value


def same_gas(P, S, P2, S2):
    return np.array_equal(P["Mass"], P2["Mass"]) and all(np.array_equal(S[k], S2[k]) for k in GAS_FIELDS)


def in_parts(ctx, Pg, Sg, queue, rows, sphw, kt, shuffle=None):
    """triples, apply and sums on the undivided set: (P, S, MassReturn, triples, counts)"""
    ops = sd.GpuMetalOps(ctx, cm.BOX)
    P, S = Pg.copy(), Sg.copy()
    none = np.zeros(0, dtype=np.int32)
    trip, counts = ops.triples(P, len(P), queue, none, none, 1, 0, 0, sphw, kt)
    if shuffle is None:
        tm = ops.apply(P, S, trip, rows, mdr.MAXGASMASS)
    else:
        perm = np.random.default_rng(shuffle).permutation(len(trip))
        tm = np.empty(len(trip))
        tm[perm] = ops.apply(P, S, trip[perm], rows, mdr.MAXGASMASS)
    mret = ops.sums(trip["star"].astype(np.int32), trip["owner"], trip["part_index"], tm, len(queue))
    return P, S, mret, trip, counts


@pytest.mark.parametrize("sphw", [0, 1])
@pytest.mark.parametrize("kt", [1, 2, 4])
def test_parts_reproduce_the_one_shot_call(ctx, kt, sphw):
    Pg, Sg, queue, rows = mdr.global_set(sphw=sphw, kt=kt)
    oP, oS, omret, npairs = one_shot(ctx, Pg, Sg, queue, rows, sphw, kt)
    P, S, mret, trip, counts = in_parts(ctx, Pg, Sg, queue, rows, sphw, kt)
    assert npairs > 10000 and len(trip) == npairs == counts.sum()
    assert (oP["Mass"] != Pg["Mass"]).sum() > 100 and omret.sum() > 1
    assert same_gas(P, S, oP, oS)
    assert np.array_equal(mret, omret)
    # the list is sorted by (particle, star), owner = this rank throughout
    key = trip["part_index"].astype(np.int64) << 32 | trip["star"]
    assert (trip["owner"] == 0).all() and (np.diff(key) > 0).all()


def test_shuffled_triples_give_the_same_bits(ctx):
    Pg, Sg, queue, rows = mdr.global_set(sphw=1)
    P, S, mret, trip, _ = in_parts(ctx, Pg, Sg, queue, rows, 1, 1)
    P2, S2, mret2, _, _ = in_parts(ctx, Pg, Sg, queue, rows, 1, 1, shuffle=3)
    assert same_gas(P, S, P2, S2) and np.array_equal(mret, mret2)
    assert (P["Mass"] != Pg["Mass"]).sum() > 100


def test_many_stars_span_several_workgroups_and_route(ctx):
    """1000 stars: 4 workgroups of the emit kernel, ~16 000 triples.  The routed counts sum to npairs of the one-shot call; with the
    rows behind the last queued star declared imports of three made-up owners, the routed list is the restatement's."""
    Pg, Sg, queue, rows = mdr.global_set(21, hscale=1.0, ngrid=24, nstar=1500, nq=1000)
    oP, oS, omret, npairs = one_shot(ctx, Pg, Sg, queue, rows, 0, 1)
    P, S, mret, trip, counts = in_parts(ctx, Pg, Sg, queue, rows, 0, 1)
    assert npairs > 10000 and counts.sum() == npairs == len(trip)
    assert same_gas(P, S, oP, oS) and np.array_equal(mret, omret)
    n, nlocal = len(Pg), int(queue.max()) + 1
    assert n - nlocal > 10
    rng = np.random.default_rng(5)
    gown = rng.integers(0, 3, n - nlocal).astype(np.int32)
    gidx = rng.integers(0, 1 << 20, n - nlocal).astype(np.int32)
    ops = sd.GpuMetalOps(ctx, cm.BOX)
    got, gcounts = ops.triples(Pg.copy(), nlocal, queue, gown, gidx, 3, 1, 700, 0, 1)
    want, wcounts = mdr.triples(Pg, nlocal, queue, gown, gidx, 3, 1, 700, 0, 1, cm.BOX)
    assert np.array_equal(gcounts, wcounts) and gcounts.sum() == npairs and (gcounts > 0).all()
    assert all(np.array_equal(got[k], want[k]) for k in ("owner", "part_index", "star", "wk"))


def test_errors_leave_the_gas_untouched(ctx):
    Pg, Sg, queue, rows = mdr.global_set(9, hscale=1.0, ngrid=8, nstar=60, nq=10)
    ops = sd.GpuMetalOps(ctx, cm.BOX)
    none = np.zeros(0, dtype=np.int32)
    trip, _ = ops.triples(Pg.copy(), len(Pg), queue, none, none, 1, 0, 0, 1, 1)
    assert len(trip) > 50
    pman = sq.PartManager(len(Pg), cm.BOX)
    pman.Base[:] = Pg
    S = Sg.copy()
    f = capi.SPH_DTYPE.fields
    gv = capi.GasMetalView(S.ctypes.data, S.dtype.itemsize, len(S), f["Density"][1], f["Metallicity"][1], f["Metals"][1], 9, 0)
    pv = pman.view()
    tm = np.zeros(len(trip))

    def apply(t, table):
        t, table = np.ascontiguousarray(t), np.ascontiguousarray(table)
        return capi.hip.shq_metal_return_apply(ctx.h, C.byref(pv), C.byref(gv), capi.ptr(t), len(t), capi.ptr(table), len(table), mdr.MAXGASMASS, capi.ptr(tm))
    bad = trip.copy()
    bad["part_index"][3] = len(Pg)                           # a particle index out of range
    assert apply(bad, rows) == capi.ERR_INVALID
    bad = trip.copy()
    bad["part_index"][3] = int(queue[0])                     # a star is not a gas target
    assert apply(bad, rows) == capi.ERR_INVALID
    bad = trip.copy()
    bad["star"][5] = len(rows)                               # a star position out of range
    assert apply(bad, rows) == capi.ERR_INVALID
    zero = rows.copy()
    zero[int(trip["star"][7]), 0] = 0                        # StarVolumeSPH == 0 of a star a triple names
    assert apply(trip, zero) == capi.ERR_INVALID
    assert same_gas(pman.Base, S, Pg, Sg)
    # too small a capacity: the error code, the count still reported
    tree = sq.force_tree_rebuild_mask(pman, sq.GASMASK)
    tv = tree.view()
    small = np.zeros(len(trip) - 1, dtype=capi.METAL_TRIPLE_DTYPE)
    counts, nt = np.zeros(1, dtype=np.int64), C.c_int64()
    rc = capi.hip.shq_metal_return_triples(ctx.h, C.byref(tv), C.byref(pv), capi.ptr(queue), len(queue), 1, 1, len(Pg), None, None, 1, 0, 0, capi.ptr(small), len(small),
                                           capi.ptr(counts), C.byref(nt))
    assert rc == capi.ERR_INVALID and nt.value == len(trip) == counts[0]
    # a global queue that does not fit 31 bits
    rc = capi.hip.shq_metal_return_triples(ctx.h, C.byref(tv), C.byref(pv), capi.ptr(queue), len(queue), 1, 1, len(Pg), None, None, 1, 0, (1 << 31) - 5, None, 0,
                                           capi.ptr(counts), C.byref(nt))
    assert rc == capi.ERR_INVALID
    assert same_gas(pman.Base, S, Pg, Sg)
    assert apply(trip, rows) == 0 and not same_gas(pman.Base, S, Pg, Sg)      # and the good list goes through


def test_stellar_density_reports_the_largest_radius_tried(ctx):
    """shq_sph_stats.hsml_max_tried of shq_stellar_density: at least the largest Hsml a star ends with; from a third of the converged
    Hsml the loop has to search beyond where it started"""
    Pg, Sg, ng, nstar, prm = mdr.stars_set(True)
    ops = sd.GpuMetalOps(ctx, cm.BOX)
    P = Pg.copy()
    queue = np.arange(ng, ng + nstar, dtype=np.int32)
    vol, tried = ops.stellar_density(P, Sg, queue, prm)
    assert tried >= P["Hsml"][queue].max() > Pg["Hsml"][queue].max() and tried < cm.BOX
    assert (vol > 0).all()


def _worker(rank, world, initfile, outdir, what):
    os.environ["OMP_NUM_THREADS"] = "2"
    dist.init_process_group("gloo", init_method="file://" + initfile, rank=rank, world_size=world)
    try:
        res = {}
        with sq.Context(0) as ctx:
            ops = sd.GpuMetalOps(ctx, cm.BOX)
            for w in what:
                if w[0] == "run":
                    res[w] = mdr.run_rank(sd.Comm(), rank, ops, w[1], empty=w[2])
                else:
                    res[w] = mdr.run_rank_stars(sd.Comm(), rank, ops, w[1])
        with open(os.path.join(outdir, "r%d.pkl" % rank), "wb") as f:
            pickle.dump(res, f)
    finally:
        dist.destroy_process_group()


def spawn(what):
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_worker, args=(2, os.path.join(tmp, "init"), tmp, what), nprocs=2, join=True)
        results = []
        for r in range(2):
            with open(os.path.join(tmp, "r%d.pkl" % r), "rb") as f:
                results.append(pickle.load(f))
        return {w: [r[w] for r in results] for w in what}


def reference(ctx, sphw, empty=()):
    class FakeComm:
        size, rank = 2, 0
    Pg, Sg, queueg, rowsg = mdr.global_set(sphw=sphw)
    order = mdr.global_order(sd.SlabDecomp(FakeComm(), mdr.NMESH, cm.BOX), Pg, queueg, 2, empty)
    P, S, mret, _ = one_shot(ctx, Pg, Sg, queueg[order], rowsg[order], sphw, 1)
    return (P, S, mret), Pg, queueg, order


def test_two_gloo_ranks_one_gpu_equal_the_undivided_call(ctx):
    what = [("run", 0, ()), ("run", 1, ())]
    got = spawn(what)
    for w in what:
        ref, Pg, queueg, order = reference(ctx, w[1])
        worst = mdr.compare(got[w], ref, Pg, queueg, order)
        print("sharded metal return, SPHWeighting %d: largest differences %s" % (w[1], worst))
        assert all(r["nghost"] > 0 and r["ntriples_sent"] > 0 for r in got[w])
        assert (ref[0]["Mass"] != Pg["Mass"]).sum() > 100


def test_two_gloo_ranks_empty_queues(ctx):
    """a rank whose queue is empty while the other's is not; a global queue of 0"""
    what = [("run", 0, (1,)), ("run", 0, (0, 1))]
    got = spawn(what)
    ref, Pg, queueg, order = reference(ctx, 0, (1,))
    assert 0 < len(order) < len(queueg)
    mdr.compare(got[what[0]], ref, Pg, queueg, order)
    assert got[what[0]][1]["nq"] == 0 and len(got[what[0]][1]["mret"]) == 0 and got[what[0]][0]["nghost"] > 0
    Sg = mdr.global_set()[1]
    for r in got[what[1]]:                                   # nothing to return: nothing imported, nothing changed
        assert len(r["mret"]) == 0 and r["nghost"] == 0 and r["ntriples_sent"] == 0
        assert np.array_equal(r["mass"], Pg["Mass"][r["rows"]]) and np.array_equal(r["density"], Sg["Density"][Pg["PI"][r["gas_rows"]]])


def test_two_gloo_ranks_stellar_density(ctx):
    """the stellar-density stage from a third of the converged Hsml: a second import round, and the undivided device result to 1e-9"""
    what = [("stars", True, ())]
    got = spawn(what)[what[0]]
    Pg, Sg, ng, nstar, prm = mdr.stars_set(True)
    P = Pg.copy()
    queue = np.arange(ng, ng + nstar, dtype=np.int32)
    vol, _ = sd.GpuMetalOps(ctx, cm.BOX).stellar_density(P, Sg, queue, prm)
    worst = mdr.compare_stars(got, True, (P["Hsml"][queue], vol))
    print("sharded stellar density: largest relative differences of Hsml and StarVolumeSPH %s" % worst)
    assert all(r["nghost"] > 0 and r["rounds"] >= 2 for r in got)
