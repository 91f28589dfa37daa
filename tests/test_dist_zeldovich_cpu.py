"""world_size-1 / -2 / -3 / -4 gloo tests of the sharded Zel'dovich displacements (shenqi_amd/dist.py:DistZeldovich) on CPU.  Every rank
starts with a share of the particles dealt without regard to the slabs, fills the Gaussian field of its own y-slab, and runs the
per-field loop on the torch.fft route with a numpy stand-in for the device phases (zeldovich_dist_cases.RestatedZeldovichOps).  The
reference is zeldovich_restated.displacement_fields on the undivided set at the bars of test_gpu_zeldovich._compare.  Bad input on one
rank must raise on every rank instead of hanging the others.  And the lattice sub-blocks of IDGenerator tile the lattice."""
import os
import pickle
import sys
import tempfile
import time

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import shenqi_amd as sq  # noqa: E402
import zeldovich_dist_cases as zc  # noqa: E402
from shenqi_amd import dist as sd  # noqa: E402

JOIN_TIMEOUT = 300       # seconds: a rank left inside a collective fails the test instead of hanging it


def _worker(rank, world, initfile, outdir, jobs):
    os.environ["OMP_NUM_THREADS"] = "2"
    dist.init_process_group("gloo", init_method="file://" + initfile, rank=rank, world_size=world)
    try:
        res = [zc.run_rank(sd.Comm(), zc.RestatedZeldovichOps(), case, **kw) for case, kw in jobs]
        with open(os.path.join(outdir, "r%d.pkl" % rank), "wb") as f:
            pickle.dump(res, f)
    finally:
        dist.destroy_process_group()


def spawn(world, jobs):
    """every job on `world` gloo ranks, one group for all of them: per job the ranks' results"""
    with tempfile.TemporaryDirectory() as tmp:
        pc = mp.spawn(_worker, args=(world, os.path.join(tmp, "init"), tmp, jobs), nprocs=world, join=False)
        deadline, done = time.monotonic() + JOIN_TIMEOUT, False
        try:
            while not done and time.monotonic() < deadline:       # join returns as soon as any one rank has ended
                done = pc.join(max(0.0, deadline - time.monotonic()))
            assert done, "the ranks did not finish: one of them is left inside a collective"
        finally:
            for p in pc.processes:
                if p.is_alive():
                    p.kill()
        results = []
        for r in range(world):
            with open(os.path.join(tmp, "r%d.pkl" % r), "rb") as f:
                results.append(pickle.load(f))
        return [[results[r][j] for r in range(world)] for j in range(len(jobs))]


def test_one_rank_without_process_group():
    N, size, scaledep = case = zc.CASES[0]
    res = zc.run_rank(sd.Comm(), zc.RestatedZeldovichOps(), case)
    assert res["rows_sent"] == 0 and res["filled"] and len(res["idx"]) == len(zc.particles(N))
    zc._compare(zc.assemble([res]), zc.reference(N, scaledep), "one rank %s" % (case,))


@pytest.mark.parametrize("case", zc.CASES, ids=lambda c: "-".join(map(str, c)))
def test_sharded_displacements_equal_the_restatement_gloo(case):
    N, size, scaledep = case
    ref = zc.reference(N, scaledep)
    results = spawn(size, [(case, dict(how=1)), (case, dict(how=2))])
    nf = 7 if scaledep else 4
    for how, ranks in zip((1, 2), results):
        # the routing, one all-to-all and one shift per field, the way back
        assert all(r["rows_sent"] > 0 and r["nalltoall"] == 2 + 2 * nf and r["filled"] for r in ranks)
        assert sum(len(r["idx"]) for r in ranks) == len(zc.particles(N))
        zc._compare(zc.assemble(ranks), ref, "%s deal %d" % (case, how))      # assemble: maxdisp, maxvel equal on all ranks


def test_rank_count_must_divide_the_mesh():
    results = spawn(3, [((16, 3, 0), {})])[0]
    assert all(r.get("constructor") and "divisible" in r["error"] for r in results)


def test_position_outside_the_box_on_one_rank_raises_on_every_rank():
    """only rank 1 holds the bad particle: every rank raises before any all-to-all, none hangs"""
    case = N, size, scaledep = zc.CASES[0]
    holder = zc.deal(len(zc.particles(N)), size, 1)
    assert holder[37] == 1
    jobs = []
    for bad in (zc.BOX, -1e-9, np.nan):
        pos = zc.particles(N).copy()
        pos[37, 1] = bad
        jobs.append((case, dict(pos=pos, holder=holder)))
    for results in spawn(size, jobs):          # one group for the three: a refused call leaves it usable
        assert all("error" in r and not r.get("constructor") and r["nalltoall"] == 0 for r in results), results
        assert "outside" in results[1]["error"] and "another rank" in results[0]["error"]


def test_non_finite_table_raises_on_every_rank():
    case = N, size, scaledep = zc.CASES[0]
    delta, growth = zc._tables(N)
    delta = delta.copy()
    delta[5] = np.inf
    results = spawn(size, [(case, dict(tables=(delta, growth)))])[0]
    assert all("non-finite" in r["error"] and r["nalltoall"] == 0 for r in results)


@pytest.mark.parametrize("grid", [(2, 1), (2, 3), (3, 2)], ids=lambda g: "x".join(map(str, g)))
def test_idgenerator_sub_blocks_tile_the_lattice(grid):
    Ngrid, L = 10, 25.0
    whole = sq.IDGenerator(Ngrid, L)
    assert (whole.offset, whole.size, whole.NumPart) == ((0, 0, 0), (10, 10, 10), 1000)
    ids = []
    for tx in range(grid[0]):
        for ty in range(grid[1]):
            g = sq.IDGenerator(Ngrid, L, (tx, ty), grid)
            assert g.offset == (tx * Ngrid // grid[0], ty * Ngrid // grid[1], 0) and g.size[2] == Ngrid
            assert g.NumPart == g.size[0] * g.size[1] * g.size[2]
            index = np.arange(g.NumPart)
            mine = sq.idgen_create_id_from_index(g, index)
            pos = sq.idgen_create_pos_from_index(g, index)
            # the one-rank generator numbers its points id - 1
            assert np.array_equal(pos, sq.idgen_create_pos_from_index(whole, mine.astype(np.int64) - 1))
            assert np.array_equal(sq.setup_grid(g, 0.25, 2.0)[0], pos + 0.25)
            ids.append(mine)
    assert np.array_equal(np.sort(np.concatenate(ids)), np.arange(1, Ngrid ** 3 + 1, dtype=np.uint64))
    with pytest.raises(ValueError):
        sq.IDGenerator(Ngrid, L, (2, 0), (2, 1))
