"""GPU tests of the sharded TreePM step on MOVING particles: DistTreePM.move + step(moved=True) - ghosts re-imported for the drifted
positions, the tree rebuilt, the local rows' previous-step accelerations carried across the new ghost count - with one rank and with
two gloo ranks sharing the GPU, against the oracle run per rank over that rank's own sources."""
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

from test_gpu_dist import NPART, NMESH, BOX, G, _global_particles  # noqa: E402

pytestmark = pytest.mark.gpu

CELL = BOX / NMESH
DRIFT_CELLS = 0.25      # the largest displacement of a drift, in mesh cells (over all ranks)
NSTEPS = 3


def _params():
    """(gp_bh, gp): Barnes-Hut for step 1, the relative criterion after it - the parameters of test_gpu_dist"""
    import shenqi_amd as sq
    import common as cm
    cm.reference_treepar(ErrTolForceAcc=0.005, MaxBHOpeningAngle=0.9, Rcut=6.0, TreeUseBH=1)
    sq.gravshort_set_softenings(BOX / np.cbrt(NPART))
    gp_bh = sq.make_grav_params(BOX, 1.5, NMESH, G, cm.RHO0)
    cm.reference_treepar(ErrTolForceAcc=0.005, MaxBHOpeningAngle=0.9, Rcut=6.0, TreeUseBH=0)
    gp = sq.make_grav_params(BOX, 1.5, NMESH, G, cm.RHO0)
    return gp_bh, gp


def drift(decomp, rank, local, acc, gpm, dmax):
    """local (tensor [n, 4]) moved by dx = s (acc + gpm) with s = DRIFT_CELLS CELL / dmax (dmax: the largest |acc + gpm| of all
    ranks), wrapped into the box; a particle whose new x would leave the slab of its rank gets -dx_x instead (migration between ranks
    is not this test's subject)"""
    dx = torch.from_numpy((acc + gpm) * (DRIFT_CELLS * CELL / dmax))
    new = local.clone()
    new[:, :3] = torch.remainder(local[:, :3] + dx, BOX)
    left = decomp.owner_of(new[:, 0], new[:, 1]) != rank
    new[left, 0] = torch.remainder(local[left, 0] - dx[left, 0], BOX)
    new[:, :3][new[:, :3] >= BOX] = 0.0      # remainder of a tiny negative number rounds to BOX itself
    return new


def _run_rank(rank, world, outdir, overlap, cut=None):
    import shenqi_amd as sq
    from shenqi_amd import dist as sd
    dev = torch.device("cuda", 0)
    comm = sd.Comm()
    mine = torch.from_numpy(_global_particles()[rank::world].copy()).to(dev)
    ctx = sq.Context(0)
    gp_bh, gp = _params()
    bounds = None if world == 1 else sd.balanced_bounds(comm, NMESH, BOX, mine[:, 0]) if cut is None else [0, cut, NMESH]
    drv = sd.DistTreePM(comm, ctx, NMESH, BOX, 1.5, G, dev, halo_factor=1.3, bounds=bounds)
    drv.setup(sd.exchange_to_owner(comm, drv.decomp, mine), gp.Rcut)
    for k in range(1, NSTEPS + 1):
        drv.step(gp_bh if k == 1 else gp, overlap=overlap, moved=k > 1)
        acc, _, gpm, ppot, nint = drv.download(ninteractions=True)
        np.savez(os.path.join(outdir, "s%d_r%d.npz" % (k, rank)), local=drv.local.cpu().numpy(), allp=drv.allp.cpu().numpy(),
                 acc=acc, gpm=gpm, ppot=ppot, nint=nint)
        if k < NSTEPS:
            t = torch.tensor([float(np.linalg.norm(acc + gpm, axis=1).max())], dtype=torch.float64)
            if world > 1:
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
            drv.move(drift(drv.decomp, rank, drv.local.cpu(), acc, gpm, float(t.item())).to(dev))
    ctx.close()


def _worker(rank, world, initfile, outdir, overlap, cut):
    os.environ["OMP_NUM_THREADS"] = "2"
    dist.init_process_group("gloo", init_method="file://" + initfile, rank=rank, world_size=world)
    try:
        _run_rank(rank, world, outdir, overlap, cut)
    finally:
        dist.destroy_process_group()


def oracle_rank(allp, nloc, oldacc, gp):
    """the oracle over one rank's own source set (local + ghost rows), for its first nloc rows as targets: (acc, nint)"""
    import orc
    pos, mass = np.ascontiguousarray(allp[:, :3]), allp[:, 3].astype(np.float32)
    nodes, first, _ = orc.tree_build(pos, mass, BOX)
    old = np.zeros(len(pos))
    old[:nloc] = oldacc
    targets = np.arange(nloc, dtype=np.int32)
    oacc, opot, onint = orc.grav_walk(nodes, first, pos, mass, old, gp, targets=targets)
    orc.grav_postprocess(mass, gp, oacc, opot, True, targets=targets)
    return oacc, onint


def check_steps(S, world, overlap, gp, ghosts_change):
    """S[k][r]: what rank r saved after step k (1-based).  Asserts steps 2 and 3 against the per-rank oracle and the conditions that
    keep the comparison from passing vacuously; returns the observed figures."""
    import orc
    e = 61 - int(np.frexp(float(NPART))[1])
    seen = dict(nghost=[[len(S[k][r]["allp"]) - len(S[k][r]["local"]) for k in range(1, NSTEPS + 1)] for r in range(world)],
                other_order_differs={}, zero_oldacc_differs={})
    for k in range(2, NSTEPS + 1):
        glob = np.concatenate([S[k][r]["local"] for r in range(world)])       # the global set of step k, rank after rank
        assert len(glob) == NPART
        og, opot, _, _ = orc.pm_force(glob[:, :3].copy(), glob[:, 3].astype(np.float32), NMESH, BOX, 1.5, G, fixed_point_log2scale=e, use_stencil=1)
        first = 0
        other = zero = 0
        for r in range(world):
            now, prev = S[k][r], S[k - 1][r]
            nloc = len(now["local"])
            assert nloc == len(prev["local"]) and np.array_equal(now["allp"][:nloc], now["local"])
            sl = slice(first, first + nloc)
            first += nloc
            err_pm = np.abs(now["gpm"] - og[sl]).max() / np.abs(og).max()
            err_pot = np.abs(now["ppot"] - opot[sl]).max() / np.abs(opot).max()
            # OldAcc from the device's own numbers: FullTreeGravAccel of step k - 1 and GravPM of step k (the reference's order) or,
            # with overlap, of step k - 1 (the walk runs before its own step's PM exists)
            new_pm = np.linalg.norm(prev["acc"] + now["gpm"], axis=1) / G
            old_pm = np.linalg.norm(prev["acc"] + prev["gpm"], axis=1) / G
            oacc, onint = oracle_rank(now["allp"], nloc, old_pm if overlap else new_pm, gp)
            _, onint_other = oracle_rank(now["allp"], nloc, new_pm if overlap else old_pm, gp)
            _, onint_zero = oracle_rank(now["allp"], nloc, np.zeros(nloc), gp)
            other += int((onint_other != onint).sum())
            zero += int((onint_zero != onint).sum())
            ndiff = int((now["nint"] != onint).sum())
            err = np.abs(now["acc"] - oacc).max() / np.abs(oacc).max()
            print("world %d overlap %d step %d rank %d: nloc %d nghost %d, %d targets differ from the oracle, force %.2e, PM %.2e, PM pot %.2e"
                  % (world, overlap, k, r, nloc, len(now["allp"]) - nloc, ndiff, err, err_pm, err_pot))
            assert err_pm < 1e-10 and err_pot < 1e-10
            assert np.array_equal(now["nint"], onint), "step %d rank %d: %d of %d interaction counts differ" % (k, r, ndiff, nloc)
            assert err < 1e-11
        assert first == NPART
        seen["other_order_differs"][k] = other
        seen["zero_oldacc_differs"][k] = zero
        assert zero > 0                                  # (c) a zeroed OldAcc would have been noticed
    assert seen["other_order_differs"][NSTEPS] > 0       # (b) GravPM(k) and GravPM(k - 1) give different counts: the order is pinned
    if ghosts_change:                                    # (a) the ghost count of a rank changed from step to step: a new row count
        assert all(any(g[k] != g[k - 1] for g in seen["nghost"]) for k in range(1, NSTEPS)), seen["nghost"]
    print("world %d overlap %d:" % (world, overlap), seen)
    return seen


# (world, cut): one rank; two ranks cut by balanced_bounds (plane 30); two ranks cut at plane 19, whose halo ends inside the large clump
CASES = [(1, None), (2, None), (2, 19)]


@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("world,cut", CASES, ids=["one-rank", "two-ranks-balanced", "two-ranks-cut19"])
def test_dist_step_on_moving_particles(world, cut, overlap):
    """setup, a Barnes-Hut step, then twice: drift by s (FullTreeGravAccel + GravPM) of the step just taken, move(), step(moved=True)
    with the relative criterion.  For steps 2 and 3 every rank's interaction counts equal, as integers, those of the oracle over that
    rank's own local + ghost rows, fed OldAcc = |FullTreeGravAccel(k-1) + GravPM| / G formed from the device's own downloads: the
    GravPM of step k without overlap (the reference's order, run.cpp:518-523), of step k - 1 with overlap (that walk runs before its
    own PM).  Forces to 1e-11 of the largest, GravPM and the PM potential to 1e-10 against the oracle PM of the gathered set.
    s makes the largest displacement of all ranks DRIFT_CELLS = 1/4 of a mesh cell.  The conditions that keep this from passing
    vacuously, asserted on what the device returned; with the oracle alone in the device's place (same particles, cuts and drift) they
    read:
    (b) at step 3 (step 2) the GravPM of the other step changes the count of 35 (84) of the 4096 targets, whatever the cut;
    (c) OldAcc = 0 changes the count of 4095 of the 4096 targets at either step;
    (a) the ghost count of a rank changes from step to step: 1826, 1841, 1845 on rank 0 of the cut at plane 19.  With balanced_bounds
    it cannot: that cut is plane 30, rank 0 imports all of rank 1 and rank 1 imports what lies outside 1.95 < x < 3.05, both edges in
    the uniform background, where a drift scaled by the clumps' accelerations moves nothing (at ONE cell the closest particle is
    5.8e-4 from an edge and moves 3e-5; the counts stay 2431 and 1515).  The cases cut at plane 19 are there for (a): rank 0's import
    ends at x = 5.117, inside the large clump."""
    import shenqi_amd as sq  # noqa: F401
    with tempfile.TemporaryDirectory() as tmp:
        if world == 1:
            _run_rank(0, 1, tmp, overlap)
        else:
            mp.spawn(_worker, args=(world, os.path.join(tmp, "init"), tmp, overlap, cut), nprocs=world, join=True)
        S = {k: [dict(np.load(os.path.join(tmp, "s%d_r%d.npz" % (k, r)))) for r in range(world)] for k in range(1, NSTEPS + 1)}
    check_steps(S, world, overlap, _params()[1], ghosts_change=cut is not None)
