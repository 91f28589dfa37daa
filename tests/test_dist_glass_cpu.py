"""world_size-1 / -2 / -3 gloo tests of glass making across ranks (shenqi_amd/dist.py:DistGlass) on CPU.  Every rank starts with a share
of the particles dealt without regard to the slabs; the particle state lives on the slab owners for the whole loop and is re-homed
after every drift; the device phases are a numpy stand-in built on glass_restated (glass_dist_cases.RestatedGlassOps) on the
torch.fft route.  The reference is glass_restated on the undivided set, step by step from the driver's own state at the bars of
test_gpu_glass.py.  The stand-in deposits the integers the device deposits, so 14 steps in one call must give the same bits of Pos,
Vel and Disp for 1, 2 and 3 ranks and both deals (the statistics and spectrum sums are added in another order on every rank count:
they are held to their any-order bars, the mode counts to equality).  Bad input on one rank must raise on every rank.  And
setup_glass's sub-blocks: the whole lattice, and two x halves with the reference's seed + ThisTask."""
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
import glass_dist_cases as gc  # noqa: E402
import glass_restated as gr  # noqa: E402
from shenqi_amd import dist as sd  # noqa: E402

JOIN_TIMEOUT = 300       # seconds: a rank left inside a collective fails the test instead of hanging it
NGRID, N, SEED = 8, 12, 21      # 512 particles on a 12^3 mesh: slabs of 6 and of 4 planes
NSTEPS = 14


def _worker(rank, world, initfile, outdir, jobs):
    os.environ["OMP_NUM_THREADS"] = "2"
    dist.init_process_group("gloo", init_method="file://" + initfile, rank=rank, world_size=world)
    try:
        res = [gc.run_rank(sd.Comm(), gc.RestatedGlassOps(), kw.get("mesh", N), **{k: v for k, v in kw.items() if k != "mesh"}) for kw in jobs]
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


def _particles():
    pos = gc.particles(NGRID, SEED)
    return pos, np.ones(len(pos), dtype=np.float32)


@pytest.fixture(scope="module")
def runs():
    """per rank count the two deals: 14 one-step calls in sequence, and 14 steps in one call - one spawn per rank count"""
    pos, mass = _particles()
    out = {}
    for world in (2, 3):
        jobs = [dict(pos=pos, mass=mass, how=how, calls=calls) for how in (1, 2) for calls in ((1,) * NSTEPS, (NSTEPS,))]
        res = spawn(world, jobs)
        for j, kw in enumerate(jobs):
            out[(world, kw["how"], len(kw["calls"]))] = res[j]
    return out


def test_one_rank_without_process_group():
    pos, mass = _particles()
    assert (pos < 0).any() and (pos >= gc.L).any()
    res = gc.run_rank(sd.Comm(), gc.RestatedGlassOps(), N, pos, mass, calls=(1,))
    o = res["outs"][0]
    assert o["rows_sent"] == 0 and o["rehomed"] == [0] and len(res["idx"]) == len(pos)
    # the torch.fft route exchanges on any rank count: 2 + nsteps + (nsteps + 1) * 4
    assert o["nalltoall"] == 2 + 1 + 2 * 4
    print(gc.compare_step(pos, np.zeros((len(pos), 3), dtype=np.float32), mass, gc.assemble([res]), N, "one rank"))


@pytest.mark.parametrize("world,how", [(2, 1), (2, 2), (3, 1), (3, 2)])
def test_every_step_from_the_drivers_own_state(runs, world, how):
    pos, mass = _particles()
    ranks = runs[(world, how, NSTEPS)]
    vel = np.zeros((len(pos), 3), dtype=np.float32)
    worst = dict(disp=0.0, vel=0.0, pos=0.0)
    for s in range(NSTEPS):
        out = gc.assemble(ranks, s)
        for r in ranks:       # the routing and the way back, one re-homing, two forces of 4 exchanges and 4 shifts
            assert r["outs"][s]["nalltoall"] == 2 + 1 + 2 * 8
        assert sum(r["outs"][s]["rows_sent"] for r in ranks) > 0
        e = gc.compare_step(pos, vel, mass, out, N, "%d ranks deal %d step %d" % (world, how, s))
        worst = {k: max(worst[k], e[k]) for k in worst}
        pos, vel = out["Pos"], out["Vel"]
    print("worst error / bar over %d steps:" % NSTEPS, {k: round(v, 4) for k, v in worst.items()})


def test_fourteen_steps_have_the_same_bits_on_every_rank_count_and_deal(runs):
    pos, mass = _particles()
    one = gc.assemble([gc.run_rank(sd.Comm(), gc.RestatedGlassOps(), N, pos, mass, calls=(NSTEPS,))])
    assert np.abs(one["Disp"]).max() > 0 and one["steps"][-1]["force_std"] < one["steps"][0]["force_std"]
    anyorder = 3 * (N**3) * 2.0**-53
    for world in (2, 3):
        for how in (1, 2):
            got = gc.assemble(runs[(world, how, 1)])
            for k in gc.FIELDS:
                assert np.array_equal(one[k], got[k]), (world, how, k, int(np.sum(one[k] != got[k])))
            assert np.array_equal(one["nmodes"], got["nmodes"]) and (got["nmodes"].sum(axis=1) == 2 * (N**3 - 1)).all()
            for k in ("kk", "power", "norm"):
                nz = one[k] != 0
                assert np.array_equal(nz, got[k] != 0) and np.abs(got[k][nz] / one[k][nz] - 1).max() <= anyorder, (world, how, k)
            tol = 3 * (3 * len(pos)) * 2.0**-53
            for a, b in zip(one["steps"], got["steps"]):
                assert (a["t_f"], a["t_v"], a["t_x"]) == (b["t_f"], b["t_v"], b["t_x"])
                assert abs(b["force_std"] / a["force_std"] - 1) <= tol and abs(b["vel_std"] / a["vel_std"] - 1) <= tol
    # and the sequence of one-step calls composes to the same bits
    seq = gc.assemble(runs[(2, 1, NSTEPS)], NSTEPS - 1)
    for k in gc.FIELDS:
        assert np.array_equal(one[k], seq[k]), k


@pytest.mark.parametrize("world", [2, 3])
def test_rehomed_counts_the_owner_changes_of_the_restated_positions(runs, world):
    pos, mass = _particles()
    moved, _ = gc.restated_owner_changes(pos, np.zeros((len(pos), 3), dtype=np.float32), mass, N, world, NSTEPS)
    assert sum(moved) > 0
    for how in (1, 2):
        ranks = runs[(world, how, 1)]
        assert list(gc.assemble(ranks)["rehomed"]) == moved, (world, how)
        for r in ranks:
            assert r["outs"][0]["nalltoall"] == 2 + NSTEPS + (NSTEPS + 1) * 8


def test_rank_count_must_divide_the_mesh():
    pos, mass = _particles()
    results = spawn(3, [dict(mesh=16, pos=pos, mass=mass)])[0]
    assert all(r.get("constructor") and "divisible" in r["error"] for r in results)


def test_bad_input_on_one_rank_raises_on_every_rank():
    """only rank 1 holds the bad particle: every rank raises in the first collective, before any all-to-all, none hangs"""
    pos, mass = _particles()
    holder = gc.deal(len(pos), 2, 1)
    assert holder[37] == 1
    jobs = []
    for what in ("pos", "vel", "mass", "far"):
        p, v, m = pos.copy(), np.zeros((len(pos), 3), dtype=np.float32), mass.copy()
        if what == "pos":
            p[37, 1] = np.nan
        elif what == "vel":
            v[37, 2] = np.inf
        elif what == "mass":
            m[37] = np.nan
        else:
            p[37, 0] = 2.0**31 * gc.L
        jobs.append(dict(pos=p, vel=v, mass=m, holder=holder, calls=(2,)))
    jobs.append(dict(pos=pos, mass=0.0, holder=holder, calls=(2,)))         # every rank sees the total mass
    jobs.append(dict(pos=pos, mass=mass, holder=holder, calls=(1,)))        # a refused call leaves the group usable
    res = spawn(2, jobs)
    for results in res[:4]:
        assert all("error" in r and not r.get("constructor") and r["nalltoall"] == 0 for r in results), results
        assert "another rank" in results[0]["error"] and "glass:" in results[1]["error"]
    assert all("total mass" in r["error"] for r in res[4])
    assert all("error" not in r for r in res[5])


def test_setup_block_of_the_whole_lattice_and_of_two_halves():
    Ngrid, box, shift, seed = 6, 25.0, 0.125, 77
    whole = sq.glass_setup_positions_block(Ngrid, box, shift, seed, (0, 0), (Ngrid, Ngrid))
    assert np.array_equal(whole, gr.setup_positions(Ngrid, box, shift, seed))
    assert np.array_equal(whole, sq.glass_setup_positions(Ngrid, box, shift, seed))
    # two tasks along x, the reference's seed + ThisTask: the restatement's draws on each task's own lattice points
    import zeldovich_restated as zr
    for task in range(2):
        g = sq.IDGenerator(Ngrid, box, (task, 0), (2, 1))
        got = sq.glass_setup_positions_block(Ngrid, box, shift, seed + task, g.offset, g.size)
        u = zr.raw_outputs(zr.init_genrand([(seed + task) & 0xFFFFFFFF]), 3 * g.NumPart)[0].astype(np.float64) / 4294967296.0
        lattice = sq.idgen_create_pos_from_index(g, np.arange(g.NumPart))
        assert np.array_equal(got, lattice + (shift + box / Ngrid * 3 * (u.reshape(g.NumPart, 3) - 0.5)))
    # a y split too: the sub-block's index order is x slowest, z fastest within the block
    g = sq.IDGenerator(Ngrid, box, (1, 2), (2, 3))
    got = sq.glass_setup_positions_block(Ngrid, box, 0.0, seed, g.offset, g.size)
    assert got.shape == (g.NumPart, 3)
    assert np.abs(got - sq.idgen_create_pos_from_index(g, np.arange(g.NumPart))).max() <= 1.5 * box / Ngrid
    with pytest.raises(Exception):
        sq.glass_setup_positions_block(Ngrid, box, 0.0, seed, (4, 0), (3, Ngrid))
