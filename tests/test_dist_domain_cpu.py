"""DistDomain (shenqi_amd/dist.py), the driver of the full domain decomposition, over real gloo process groups of 2, 3 and 4 ranks with
the CPU operators of tests/domain_restated.py: every rank ends with the same TopNodes / TopLeaves / Tasks, they are the tables the
restatement gives when it runs all ranks in one process on the same particles split the same way (its own policy loop, global sample
sort, combine order and balance), no particle is lost or doubled, and every particle sits on the task of its leaf."""
import os
import pickle
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

BOX = 25000.0
NPART = 6000
# TopNodeAllocFactor starts too small for the skeleton: the first attempts end in "retry with more top nodes"
PARAMS = dict(DomainOverDecompositionFactor=4, TopNodeAllocFactor=0.05, SetAsideFactor=1.0)


def global_particles(seed=17):
    """uniform background + two clumps, some garbage; IDs are the global indices"""
    rng = np.random.default_rng(seed)
    n = NPART
    pos = rng.random((n, 3)) * BOX
    pos[: n // 3] = (np.array([0.3, 0.6, 0.2]) * BOX + rng.normal(0, 0.01 * BOX, (n // 3, 3))) % BOX
    pos[n // 3: n // 2] = (np.array([0.8, 0.1, 0.7]) * BOX + rng.normal(0, 0.002 * BOX, (n // 2 - n // 3, 3))) % BOX
    garbage = rng.random(n) < 0.05
    return pos, garbage, np.arange(n, dtype=np.int64)


def rank_share(rank, world, maxpart):
    """an uneven initial split: rank r holds every particle whose ID mod (world + 1) is r (the last rank two classes)"""
    pos, garbage, ids = global_particles()
    cls = ids % (world + 1)
    m = (cls == rank) | ((rank == world - 1) & (cls == world))
    return dict(Pos=pos[m], garbage=garbage[m], ID=ids[m], MaxPart=maxpart)


def _worker(rank, world, initfile, outdir, maxpart, dodf):
    os.environ["OMP_NUM_THREADS"] = "2"
    torch.set_num_threads(2)
    dist.init_process_group("gloo", init_method="file://" + initfile, rank=rank, world_size=world)
    try:
        from shenqi_amd import dist as sd
        import domain_restated as dr
        _, nxt, sub = dr.tables()
        sh = rank_share(rank, world, maxpart)
        ops = dr.CpuDomainOps(nxt, sub, BOX, sh["Pos"], sh["garbage"], sh["ID"], maxpart)
        dd = sd.DistDomain(sd.Comm(), ops, dict(PARAMS, DomainOverDecompositionFactor=dodf)).decompose()
        with open(os.path.join(outdir, "d%d.pkl" % rank), "wb") as f:
            pickle.dump(dict(N=dd.TopNodes, L=dd.TopLeaves, T=dd.Tasks, policy=dd.policy, factor=dd.factor, ID=ops.ID, TopLeaf=ops.TopLeaf, keys=ops.keys), f)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,maxpart,dodf", [(2, 8000, 4), (3, 8000, 4), (4, 8000, 4), (3, 2300, 1)])
def test_dist_domain_equals_the_restatement_in_one_process(world, maxpart, dodf):
    """MaxPart 2300 on three ranks with three top leaves asked for: the first policy ends outside the memory bound (one task would hold
    more than MaxPart), so the loop moves on to the policy with twice the leaves"""
    import domain_restated as dr
    _, nxt, sub = dr.tables()
    ref = dr.decompose_serial(nxt, sub, [rank_share(r, world, maxpart) for r in range(world)], BOX,
                              dict(PARAMS, DomainOverDecompositionFactor=dodf))
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_worker, args=(world, os.path.join(tmp, "init"), tmp, maxpart, dodf), nprocs=world, join=True)
        out = [pickle.load(open(os.path.join(tmp, "d%d.pkl" % r), "rb")) for r in range(world)]
    _, garbage, ids = global_particles()
    for r, d in enumerate(out):
        for f in ("StartKey", "Daughter", "Shift", "Leaf"):
            assert np.array_equal(d["N"][f], ref["TopNodes"][f]), (r, f)
        assert np.array_equal(d["L"]["Task"], ref["TopLeaves"]["Task"]) and np.array_equal(d["L"]["topnode"], ref["TopLeaves"]["topnode"])
        assert np.array_equal(d["T"]["StartLeaf"][:world], ref["Tasks"]["StartLeaf"][:world])
        assert np.array_equal(d["T"]["EndLeaf"][:world], ref["Tasks"]["EndLeaf"][:world])
        assert d["policy"] == ref["policy"] and d["factor"] == ref["factor"]
        assert sorted(d["ID"].tolist()) == ref["ids"][r]
        assert np.all(d["L"]["Task"][d["TopLeaf"]] == r)                       # every particle sits on the task of its leaf
        assert sorted(zip(d["ID"].tolist(), d["TopLeaf"].tolist())) == ref["leaf_of"][r]
        assert np.all(np.diff(d["keys"].astype(np.float64)) >= 0)              # and the rank is left in key order
    assert sorted(np.concatenate([d["ID"] for d in out]).tolist()) == ids[~garbage].tolist()   # the live particles, each once
    assert ref["factor"] > PARAMS["TopNodeAllocFactor"]                        # the retry with more top nodes was taken
    assert (ref["policy"] > 0) == (maxpart < 8000)
