"""The mechanisms the sharded drivers of shenqi_amd/dist.py share, each on its own, on CPU: SlabDecomp.reach_mask against a restatement,
Comm's collectives on small host arrays over 1 (SHQ_COMM_FORCE), 2 and 3 gloo ranks and without a process group, append_records on a
padded dtype, and widen_until_covered with a scripted operator.  The drivers' own tests (test_dist_*_cpu.py) check what they compute;
these pin the pieces a new driver would pick up."""
import os
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# every length below is a multiple of 2^-10 (the cell is 1/4): sums and differences are exact, so the restatement and the formula
# under test must agree on the edge values too, not only away from them
NMESH, BOX = 48, 12.0
CELL = BOX / NMESH


class FakeComm:
    def __init__(self, size, rank=0):
        self.size, self.rank = size, rank


def restated_mask(a, b, x, halo):
    """within halo of [a, b) periodically: the distance of the nearest image to the interval, 0 inside; the left end closed
    (distance <= halo), the right end open (distance < halo); everything once the interval and both halos cover the box"""
    halo = np.broadcast_to(np.asarray(halo, dtype=np.float64), x.shape)
    out = np.zeros(len(x), dtype=bool)
    for k in (-1.0, 0.0, 1.0):
        xi = x + k * BOX
        left, right = xi < a, xi >= b
        out |= (~left & ~right) | (left & (a - xi <= halo)) | (right & (xi - b < halo))
    return out | ((b - a) + 2 * halo >= BOX)


def positions(a, b, halo):
    """about 200 positions: a grid, the exact edges of the reach and their neighbours, the ends of the box"""
    rng = np.random.default_rng(5)
    x = list(rng.integers(0, int(BOX * 1024), size=160) / 1024.0)
    for e in (a - halo, b + halo, a, b):
        e = e % BOX
        x += [e, (e + 1 / 1024.0) % BOX, (e - 1 / 1024.0) % BOX]
    x += [0.0, np.nextafter(BOX, 0.0), 1 / 1024.0, BOX - 1 / 1024.0]
    return np.array(x, dtype=np.float64)


@pytest.mark.parametrize("bounds,ycuts", [([0, 7, 30, 48], None), ([0, 9, 20, 48], [0.0, 2.5, 0.0, 0.0])])
def test_reach_mask_equals_restatement(bounds, ycuts):
    from shenqi_amd import dist as sd
    d3 = sd.SlabDecomp(FakeComm(3), NMESH, BOX, bounds, ycuts)
    rng = np.random.default_rng(11)
    nwrap = nedge = 0
    for d in range(3):
        a = bounds[d] * CELL
        b = (bounds[d + 1] + (1 if ycuts is not None and ycuts[d + 1] > 0.0 else 0)) * CELL
        assert (a, b) == d3.slab_range(d)
        for halo in (0.0, 0.375, 1.25, 6.0):            # 6.0: the span covers the box for every slab
            x = positions(a, b, halo)
            want = restated_mask(a, b, x, halo)
            got = d3.reach_mask(d, x, halo)
            assert got.dtype == bool and np.array_equal(got, want), (d, halo)
            tgot = d3.reach_mask(d, torch.from_numpy(x), halo)
            assert tgot.dtype == torch.bool and np.array_equal(tgot.numpy(), want), (d, halo)
            if (b - a) + 2 * halo >= BOX:
                assert want.all()
                continue
            assert want.any() and not want.all()
            # the edges themselves: a - halo belongs, b + halo does not
            lo, hi = (a - halo) % BOX, (b + halo) % BOX
            assert d3.reach_mask(d, np.array([lo]), halo)[0] and (halo == 0.0 or not d3.reach_mask(d, np.array([hi]), halo)[0])
            nedge += 1
            # positions that qualify only through the wrap: on the other side of the box's edge than the slab
            nwrap += int((want & ((x < a - halo) | (x >= b + halo))).sum())
        # one halo per position, some of them wide enough to cover the box on their own
        x = positions(a, b, 0.375)
        halos = rng.integers(0, 1536, size=len(x)) / 1024.0
        halos[::17] = 6.0
        want = restated_mask(a, b, x, halos)
        assert want[::17].all() and not want.all()
        assert np.array_equal(d3.reach_mask(d, x, halos), want)
        assert np.array_equal(d3.reach_mask(d, torch.from_numpy(x), torch.from_numpy(halos)).numpy(), want)
    assert nwrap > 0 and nedge > 0


def test_append_records_keeps_the_padded_itemsize():
    from shenqi_amd import capi
    from shenqi_amd import dist as sd
    assert capi.SPH_DTYPE.itemsize == 176 and sum(capi.SPH_DTYPE[n].itemsize for n in capi.SPH_DTYPE.names) < 176
    rng = np.random.default_rng(2)

    def records(n):
        r = np.zeros(n, dtype=capi.SPH_DTYPE)
        for name in r.dtype.names:
            r[name] = rng.integers(1, 1000, size=r[name].shape)
        return r
    local, ghosts = records(5), records(3)
    wide = np.concatenate([np.zeros((3, 160), dtype=np.uint8), ghosts.view(np.uint8).reshape(3, -1)], axis=1)
    for got, ng in ((ghosts.view(np.uint8).reshape(3, -1), 3), (wide[:, 160:], 3), (wide[:0, 160:], 0)):   # contiguous, a column slice, none
        out = sd.append_records(local, got)
        assert out.dtype == capi.SPH_DTYPE and out.itemsize == 176 and len(out) == 5 + ng
        for name in capi.SPH_DTYPE.names:
            assert np.array_equal(out[name][:5], local[name]) and np.array_equal(out[name][5:], ghosts[name][:ng]), name


def rank_inputs(r):
    """what rank r contributes to every collective of check_collectives (any rank can restate any other's)"""
    from shenqi_amd import capi
    rng = np.random.default_rng(100 + r)
    tree = np.zeros(4 + r, dtype=capi.LOCAL_TOPNODE_DTYPE)
    for name in ("StartKey", "Shift", "Daughter", "Parent", "Count", "Cost"):
        tree[name] = rng.integers(1, 1 << 30, size=len(tree))
    tree["StartKey"] += np.uint64(1) << np.uint64(63)
    return dict(f=0.1 * (r + 1) + 1e-3 * r, i=(1 << 60) + 3 * r + 1,                       # the count is odd and far above 2^53
                ints=rng.integers(-(1 << 40), 1 << 40, size=(3, 4, 5)), floats=rng.integers(-4096, 4096, size=(2, 7)) / 8.0,
                keys=(rng.integers(0, 1 << 62, size=[0, 3, 5][r % 3]).astype(np.uint64) << np.uint64(2)) + np.uint64(r), tree=tree)


def check_collectives(comm, world, rank):
    """every helper against the serial restatement over the ranks' inputs"""
    from shenqi_amd import capi
    every = [rank_inputs(r) for r in range(world)]
    mine = every[rank]
    g = comm.gather_scalar(mine["f"])
    assert g.dtype == np.float64 and np.array_equal(g, np.array([e["f"] for e in every]))
    g = comm.gather_scalar(mine["i"], np.int64)
    assert g.dtype == np.int64 and [int(v) for v in g] == [e["i"] for e in every]
    for key in ("ints", "floats"):
        keep = mine[key].copy()
        want = np.sum([e[key] for e in every], axis=0)            # in rank order or any other: the sums are exact
        got = comm.allreduce_sum_vec(mine[key])
        assert got.dtype == keep.dtype and got.shape == keep.shape and np.array_equal(got, want), key
        tgot = comm.allreduce_sum_vec(torch.from_numpy(mine[key]))
        assert torch.is_tensor(tgot) and np.array_equal(tgot.numpy(), want), key
        assert np.array_equal(mine[key], keep) and got is not mine[key], key      # the input stays, a new array comes back
    assert comm.allreduce_sum(float(rank + 1)) == float(sum(range(1, world + 1)))
    keys = comm.allgather_u64(mine["keys"])
    assert keys.dtype == np.uint64 and np.array_equal(keys, np.concatenate([e["keys"] for e in every]))
    assert len(every[0]["keys"]) == 0 and (world < 3 or len(keys) == 8)
    empty = np.zeros(0, dtype=capi.LOCAL_TOPNODE_DTYPE)
    for arr in (every[0]["tree"], empty):
        got = comm.bcast_array(arr if rank == 0 else empty, capi.LOCAL_TOPNODE_DTYPE)
        assert got.dtype == capi.LOCAL_TOPNODE_DTYPE and np.array_equal(got, arr)
    if world > 1:                         # point to point: the last rank's tree, then nothing, to rank 0
        for arr in (every[world - 1]["tree"], empty):
            if rank == world - 1:
                comm.send_array(arr, 0)
            elif rank == 0:
                got = comm.recv_array(world - 1, capi.LOCAL_TOPNODE_DTYPE)
                assert got.dtype == capi.LOCAL_TOPNODE_DTYPE and np.array_equal(got, arr)
    comm.barrier()


def scripted_widen(comm, rank, hfac):
    """rank 1 tries a radius beyond its halo in the first round; returns (rounds, the halos every call saw)"""
    from shenqi_amd import dist as sd
    start = [1.0, 2.0][rank]
    script = [[0.5, 0.5], [3.0 * hfac, 2.5]][rank]          # the radii tried by round
    seen = []

    def attempt(halos):
        seen.append(np.array(halos, dtype=np.float64))
        return script[len(seen) - 1]
    return sd.widen_until_covered(comm, hfac, start, attempt), seen


def _worker(rank, world, initfile, what):
    os.environ["OMP_NUM_THREADS"] = "2"
    torch.set_num_threads(2)
    from shenqi_amd import dist as sd
    single = sd.Comm()                      # before the group exists: the path of a run without one
    if world == 1:
        os.environ["SHQ_COMM_FORCE"] = "1"
    dist.init_process_group("gloo", init_method="file://" + initfile, rank=rank, world_size=world)
    try:
        comm = sd.Comm()
        assert comm.multi and not single.multi and comm.size == world and comm.rank == rank
        if what == "collectives":
            check_collectives(comm, world, rank)
            if world == 1:
                check_collectives(single, 1, 0)
        else:
            for hfac in (1.0, 1.3):
                rounds, seen = scripted_widen(comm, rank, hfac)
                assert rounds == 2 and len(seen) == 2
                assert np.array_equal(seen[0], [hfac * 1.0, hfac * 2.0])
                # rank 1 repeats on hfac x the radius it tried; rank 0, which stayed inside, on hfac x its halo - unchanged at hfac = 1
                assert np.array_equal(seen[1], [hfac * max(0.5, hfac * 1.0), hfac * max(3.0 * hfac, hfac * 2.0)])
                if hfac == 1.0:
                    assert seen[1][0] == seen[0][0] and seen[1][1] == 3.0
            calls = []
            assert sd.widen_until_covered(comm, 1.3, 0.0, lambda halos: calls.append(list(halos)) or 0.0) == 1     # no targets anywhere
            assert calls == [[0.0, 0.0]]
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [1, 2, 3])
def test_comm_collectives_gloo(world):
    """world 1: a one-rank group under SHQ_COMM_FORCE=1 goes through the collectives and gives what the path without a group gives"""
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_worker, args=(world, os.path.join(tmp, "init"), "collectives"), nprocs=world, join=True)


def test_helpers_without_process_group():
    from shenqi_amd import dist as sd
    comm = sd.Comm()
    assert not comm.multi and comm.size == 1 and comm.rank == 0
    check_collectives(comm, 1, 0)
    # one rank alone has nothing to import: one round, whatever its loop tried
    calls = []
    assert sd.widen_until_covered(comm, 1.3, 2.0, lambda halos: calls.append(list(halos)) or 100.0) == 1
    assert calls == [[1.3 * 2.0]]


def test_widen_until_covered_gloo():
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_worker, args=(2, os.path.join(tmp, "init"), "widen"), nprocs=2, join=True)
