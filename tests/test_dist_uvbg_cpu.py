"""world_size-1 / -2 / -3 / -4 gloo tests of the sharded excursion-set reionisation (shenqi_amd/dist.py:DistUVBG) on CPU.  Every rank
starts with a random share of the particles, routes them to the owners of their UVBG planes, deposits in fixed point with scales from
the global sums, and runs the radius loop on the torch.fft route with a numpy stand-in for the device phases
(uvbg_dist_cases.RestatedUvbgOps).  The reference is uvbg_restated.calculate_uvbg on the undivided set under the rules of
test_parity_with_the_restatement, with at most 0.1 % of the cells left out as near the threshold.  Every case must ionise cells
either side of the first cut and at the box wrap and set zreion of gas there (asserted on the reference first)."""
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

import uvbg_dist_cases as uc  # noqa: E402
from shenqi_amd import dist as sd  # noqa: E402


def _worker(rank, world, initfile, outdir, jobs):
    os.environ["OMP_NUM_THREADS"] = "2"
    dist.init_process_group("gloo", init_method="file://" + initfile, rank=rank, world_size=world)
    try:
        res = []
        for case, kw in jobs:
            try:
                res.append(uc.run_rank(sd.Comm(), uc.RestatedUvbgOps(), case, **kw))
            except ValueError as e:          # the constructor's refusal
                res.append(dict(error=str(e), constructor=True))
        with open(os.path.join(outdir, "r%d.pkl" % rank), "wb") as f:
            pickle.dump(res, f)
    finally:
        dist.destroy_process_group()


def spawn(world, jobs):
    """every job on `world` gloo ranks, one group for all of them: per job the ranks' results"""
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_worker, args=(world, os.path.join(tmp, "init"), tmp, jobs), nprocs=world, join=True)
        results = []
        for r in range(world):
            with open(os.path.join(tmp, "r%d.pkl" % r), "rb") as f:
                results.append(pickle.load(f))
        return [[results[r][j] for r in range(world)] for j in range(len(jobs))]


def test_one_rank_without_process_group():
    N, size, ftype, rtom, use_sfr = case = uc.CASES[0]
    ref = uc.reference(*case)
    uc.assert_coverage(ref, N, size)
    res = uc.run_rank(sd.Comm(), uc.RestatedUvbgOps(), case)
    assert res["rows_sent"] == 0 and len(res["idx"]) == len(ref["fesc"])
    uc.compare(uc.assemble([res], N), ref, N, size)


@pytest.mark.parametrize("case", uc.CASES, ids=lambda c: "-".join(map(str, c)))
def test_sharded_reionisation_equals_the_restatement_gloo(case):
    N, size = case[0], case[1]
    ref = uc.reference(*case)
    uc.assert_coverage(ref, N, size)
    results = spawn(size, [(case, {})])[0]
    assert all(r["rows_sent"] > 0 and r["nalltoall"] > 2 * ref["nradii"] for r in results)
    assert sum(len(r["idx"]) for r in results) == len(ref["fesc"])
    uc.compare(uc.assemble(results, N), ref, N, size)


def test_unequal_slab_widths():
    case = uc.CASES[0]
    N, size = case[0], case[1]
    ref = uc.reference(*case)
    results = spawn(2, [(case, dict(bounds=[0, 12, 32]))])[0]
    assert [r["J21"].shape[0] for r in results] == [12, 20]
    uc.compare(uc.assemble(results, N), ref, N, size)


def test_negative_escape_fraction_raises_on_every_rank():
    """only rank 1 holds stars, so only rank 1 sees the negative escape fraction: every rank raises, none hangs, no array changed"""
    case = uc.CASES[0]
    N, size = case[0], case[1]
    _, types, *_ = uc.particles(N, size)
    holder = np.where(types == 4, 1, np.arange(len(types)) % 2)
    # a star right of the cut belongs to rank 1 after the routing as well; those left of it would take the flag to rank 0
    pos = uc.particles(N, size)[0]
    holder = np.where((types == 4) & (pos[:, 0] < uc.BOX / 2), -1, holder)            # held by nobody: left out of the run
    results = spawn(2, [(case, dict(holder=holder, EscapeFractionNorm=-0.2))])[0]
    assert all("negative escape fraction" in r["error"] and r["untouched"] for r in results)
    assert not (types[results[0]["idx"]] == 4).any() and (types[results[1]["idx"]] == 4).any()


def test_rank_count_must_divide_the_mesh():
    results = spawn(3, [((32, 3, 0, 0, 0), {})])[0]
    assert all(r.get("constructor") and "divisible" in r["error"] for r in results)


def test_no_stars():
    case = uc.CASES[0]
    N, size = case[0], case[1]
    _, types, _, _, _, _, zr = uc.particles(N, size, stars=False)
    got = uc.assemble(spawn(2, [(case, dict(stars=False))])[0], N)
    assert np.all(got["xHI"] == 1) and np.all(got["J21"] == 0)
    assert np.all(got["local_J21"][types == 0] == 0)
    assert np.array_equal(got["zreion"], zr)
    assert got["vol"] == 1.0 and abs(got["mass"] - 1.0) <= 1e-15
