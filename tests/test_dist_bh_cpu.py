"""world_size-1 / -2 / -3 gloo tests of the sharded black-hole step (shenqi_amd/dist.py:DistBlackHole) on CPU: every rank owns an x-slab,
imports the neighbours' gas and holes within reach, walks its own queued holes (the restatements of tests/bh_dist_restated.py stand in
for shq_bh_accretion_marks / _marks_resolve / _feedback_effects / _effects_apply), sends marks and effects to the particles' owners,
who apply them in the order of the global queue, and refreshes its ghosts between the two walks.

The yardstick is oracle/blackhole.py's accretion + feedback on the undivided set with the ranks' queues concatenated in rank order.
Integers are equal; floats are compared to 1e-12 of the field's largest value: a hole's sums run over its neighbours in the row order
of local + ghost particles, which is not the undivided set's, so they are not bit-equal across decompositions.

blackhole_fixtures.setup scatters its holes, and a merging pair then lies across a slab face about once in sixty pairs; the set here
places pairs and the chain across the faces on purpose (bh_dist_restated.place_holes) and the two-rank cases assert what it must hold."""
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
sys.path.insert(0, os.path.join(ROOT, "oracle"))

CASES = ("thermal", "bound", "kinetic")


def _worker(rank, world, initfile, outdir, case, empty):
    os.environ["OMP_NUM_THREADS"] = "2"
    dist.init_process_group("gloo", init_method="file://" + initfile, rank=rank, world_size=world)
    try:
        import bh_dist_restated as bdr
        from shenqi_amd import dist as sd
        res = bdr.run_rank(sd.Comm(), rank, bdr.RestatedBhOps(), case, empty=empty)
        with open(os.path.join(outdir, "r%d.pkl" % rank), "wb") as f:
            pickle.dump(res, f)
    finally:
        dist.destroy_process_group()


def spawn(world, case, empty=()):
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_worker, args=(world, os.path.join(tmp, "init"), tmp, case, empty), nprocs=world, join=True)
        results = []
        for r in range(world):
            with open(os.path.join(tmp, "r%d.pkl" % r), "rb") as f:
                results.append(pickle.load(f))
        return results


def check(results, case, world, empty=()):
    import bh_dist_restated as bdr
    ref = bdr.reference(case, world, empty)
    worst = bdr.compare(bdr.assemble(results, ref), ref, 1e-12, 1e-12, 1e-12)
    print("sharded black-hole step, %s on %d ranks: largest differences %s" % (case, world, worst))
    assert ref["counts"][0] > 0 and ref["counts"][1] > 0
    return ref


def test_dist_bh_one_rank_without_process_group():
    import bh_dist_restated as bdr
    from shenqi_amd import dist as sd
    res = bdr.run_rank(sd.Comm(), 0, bdr.RestatedBhOps(), "thermal")
    assert res["nghost"] == 0 and sum(res["marks_sent"]) == 0 and sum(res["effects_sent"]) == 0
    check([res], "thermal", 1)


@pytest.mark.parametrize("case", CASES)
def test_two_ranks_equal_the_undivided_restatement_gloo(case):
    import bh_dist_restated as bdr
    results = spawn(2, case)
    ref = check(results, case, 2)
    c = bdr.straddle_conditions(ref, results)
    print("what the set holds, %s: %s" % (case, c))
    assert c["consecutive"] == 0                                       # no two hole IDs consecutive: the mark rule cannot fall either way
    assert all(r["nghost"] > 0 for r in results)
    sent_m, sent_e = np.sum([r["marks_sent"] for r in results], axis=0), np.sum([r["effects_sent"] for r in results], axis=0)
    assert (sent_m > 0).all() and sent_e[0] > 0 and sent_e[1] > 0      # merger and gas marks, hole and gas swallows crossed the face
    # swallowers on either side of the face, one of the swallowed an active hole whose Mass grew in its owner's postprocess
    assert c["swallower_left"] > 0 and c["swallower_right"] > 0 and c["grown_ghost"] > 0
    assert c["drawn_by_both_remote"] > 0
    if case != "bound":                                                # (in "bound" the chain's third hole is not in the queue)
        assert c["chain"] > 0
    if case == "kinetic":                                              # (nearly every hole there is in the kinetic mode)
        assert sent_e[3] > 0 and c["kicked_by_both"] > 0
    else:
        assert sent_e[2] > 0 and c["heated_by_both"] > 0


@pytest.mark.parametrize("case", CASES)
def test_three_ranks_equal_the_undivided_restatement_gloo(case):
    results = spawn(3, case)
    check(results, case, 3)
    assert all(r["nghost"] > 0 for r in results)
    assert sum(sum(r["marks_sent"]) for r in results) > 0 and sum(sum(r["effects_sent"]) for r in results) > 0


def test_one_rank_with_an_empty_queue_gloo():
    results = spawn(2, "thermal", empty=(1,))
    ref = check(results, "thermal", 2, empty=(1,))
    assert results[1]["nq"] == 0 and results[0]["nq"] == len(ref["queue"]) > 0
    assert results[1]["nghost"] > 0 and sum(results[0]["effects_sent"]) > 0 and sum(results[1]["effects_sent"]) == 0


def test_global_queue_of_zero_gloo():
    """nothing imported, nothing changed"""
    import bh_dist_restated as bdr
    results = spawn(2, "thermal", empty=(0, 1))
    ref = bdr.reference("thermal", 2, (0, 1))
    got = bdr.assemble(results, ref)
    for r in results:
        assert r["nghost"] == 0 and r["counts"] == (0, 0) and sum(r["marks_sent"]) == 0 and sum(r["effects_sent"]) == 0
    for rec, src in (("P", "Pg"), ("S", "Sg"), ("B", "Bg")):
        for name in ref[src].dtype.names:
            assert np.array_equal(got[rec][name], ref[src][name], equal_nan=True), (rec, name)
