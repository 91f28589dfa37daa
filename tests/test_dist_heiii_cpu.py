"""Helium reionisation across ranks on the CPU: shenqi_amd/dist.py:DistHeIII with tests/heiii_dist_restated.py:RestatedHeiiiOps (numpy
stand-ins of shq_heiii_open / _sweep / _commit / _close) on one rank without a process group and on 2 and 3 gloo ranks, against
turn_on_quasars_ranks on the undivided set: the reference's loop for the candidate split that is given, one iteration and one bubble at a
time.  Flags, Entropy, log and result are exactly equal: the same libm, and every particle is heated once.

The set (heiii_dist_restated.global_set): 2 x 14^3 particles split by x, 60 candidates dealt to the ranks, the target reached in the
second batch.  Its seeds were chosen by the restatement alone so that it holds what the multi-rank loop is about; the tests assert it."""
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

# name -> (case of heiii_dist_restated.global_set, culling)
CASES = {
    "main": ({}, True),
    "main_uncut": ({}, False),
    "no_groups": (dict(no_groups=(1,), desired_ion_frac=0.9), True),      # to the end of the shorter list
    "no_gas": (dict(no_gas=(1,)), True),
    "no_candidates": (dict(min_mass=1e9, desired_ion_frac=0.5), True),
    "at_target": (dict(desired_ion_frac=0.01), True),
    "flash": (dict(flash=True), True),
    "var_positive": (dict(var_bubble=1.0e4), True),
    "negative_radius": (dict(var_bubble=4.0e6, desired_ion_frac=0.5), True),
    "u1_zero": (dict(var_bubble=1.0e4, u1_zero=2, desired_ion_frac=0.9), True),
}
PER_WORLD = {2: tuple(CASES), 3: ("main", "no_groups", "u1_zero")}


def _worker(rank, world, initfile, outdir, names):
    os.environ["OMP_NUM_THREADS"] = "2"
    dist.init_process_group("gloo", init_method="file://" + initfile, rank=rank, world_size=world)
    try:
        import heiii_dist_restated as hd
        from shenqi_amd import dist as sd
        res = {}
        for name in names:
            case, cull = CASES[name]
            res[name] = hd.run_rank(sd.Comm(), rank, hd.RestatedHeiiiOps(cull=cull), dict(case, world=world))
        with open(os.path.join(outdir, "r%d.pkl" % rank), "wb") as f:
            pickle.dump(res, f)
    finally:
        dist.destroy_process_group()


_spawned = {}


def spawned(world, name):
    """every case of a rank count in one pair (triple) of child processes, started once"""
    if world not in _spawned:
        with tempfile.TemporaryDirectory() as tmp:
            mp.spawn(_worker, args=(world, os.path.join(tmp, "init"), tmp, PER_WORLD[world]), nprocs=world, join=True)
            per_rank = []
            for r in range(world):
                with open(os.path.join(tmp, "r%d.pkl" % r), "rb") as f:
                    per_rank.append(pickle.load(f))
        _spawned[world] = {n: [pr[n] for pr in per_rank] for n in PER_WORLD[world]}
    return _spawned[world][name]


def check(results, name, world):
    """flags, Entropy, log and result exactly the restatement's, on every rank"""
    import heiii_dist_restated as hd
    case = dict(CASES[name][0], world=world)
    wflags, wentropy, wlog, wres, ev = hd.reference(**case)
    flags, entropy = hd.assemble(results, case)
    assert np.array_equal(flags, wflags), np.flatnonzero(flags != wflags)[:10]
    assert np.array_equal(entropy, wentropy)
    for r in results:
        assert r["error"] is None and r["log"] == wlog and r["res"] == wres
    assert sum(r["nrows"] for r in results) == wres["n_flash"] + wres["n_ionized"]
    return wlog, wres, ev


def test_one_task_restatement_is_the_one_rank_restatement():
    import heiii_dist_restated as hd
    import heiii_restated as hr
    s = hd.global_set(world=1)
    Pg, Sg, G = s["Pg"], s["Sg"], s["rank_groups"][0]
    args = (Pg["Pos"], Pg["Type"], Pg["Flags"], Pg["PI"], Sg["Density"], Sg["Entropy"])
    flags, entropy, log, res, ev = hd.turn_on_quasars_ranks(*args, [G], len(G), s["rnd"], s["params"])
    wflags, wentropy, wlog, wres = hr.turn_on_quasars(*args, G, s["rnd"], s["params"])
    assert np.array_equal(flags, wflags) and np.array_equal(entropy, wentropy) and res == wres and res["n_ionized"] > 100
    assert [tuple(line[1:]) for line in log] == [tuple(line) for line in wlog] and all(line[0] in (0, -1) for line in log)
    assert ev["two_host"] == 0 and ev["unhosted"] == 0 and ev["split_bubbles"] == 0


def test_one_rank_without_process_group():
    import heiii_dist_restated as hd
    from shenqi_amd import dist as sd
    res = hd.run_rank(sd.Comm(), 0, hd.RestatedHeiiiOps(), dict(world=1))
    wlog, wres, _ = check([res], "main", 1)
    assert wres["n_iterations"] > 32 and res["nsweeps"] == 2 and wres["n_ionized"] > 100


@pytest.mark.parametrize("world", [2, 3])
def test_ranks_equal_the_undivided_restatement_gloo(world):
    results = spawned(world, "main")
    wlog, wres, ev = check(results, "main", world)
    print("what the set holds on %d ranks: %s, %d iterations" % (world, ev, wres["n_iterations"]))
    assert ev["two_host"] >= 1                     # the spurious erase
    assert ev["after_two_host_unhosted"] >= 1      # ... and a position nobody hosts after it
    assert ev["index0"] >= 1
    assert ev["face_split"] >= 1                   # a bubble across the periodic x face ionising gas of two ranks
    assert ev["idle"] >= 1 and any(min(r["kept"]) == 0 and r["nrows"] > 0 for r in results)   # a batch in which a rank with gas keeps no bubble
    assert wres["n_iterations"] > 32 and 2 <= results[0]["nsweeps"] <= 3
    # the driver's replay of the counters sees the same events (it runs on to the end of its last batch, the loop stops inside it)
    assert all(r["events"] == results[0]["events"] for r in results) and all(results[0]["events"][k] >= ev[k] for k in ("two_host", "unhosted", "index0"))
    assert any(line[0] == -1 for line in wlog) and {line[0] for line in wlog} >= set(range(world))


def test_culling_changes_nothing_but_the_tests_made_gloo():
    cut, uncut = spawned(2, "main"), spawned(2, "main_uncut")
    check(uncut, "main_uncut", 2)
    for a, b in zip(cut, uncut):
        assert np.array_equal(a["flags"], b["flags"]) and np.array_equal(a["entropy"], b["entropy"]) and a["log"] == b["log"] and a["res"] == b["res"]
        assert a["ntests"] <= b["ntests"]
    assert sum(a["ntests"] for a in cut) < sum(b["ntests"] for b in uncut)
    assert all(k == n for k, n in zip(uncut[0]["kept"], uncut[1]["kept"]))      # without culling every rank sweeps every lit bubble


@pytest.mark.parametrize("world,name", [(2, "no_groups"), (3, "no_groups"), (2, "no_gas"), (2, "var_positive")])
def test_uneven_ranks_gloo(world, name):
    results = spawned(world, name)
    wlog, wres, ev = check(results, name, world)
    assert wres["n_ionized"] > 50 and (wres["n_iterations"] > 32 or name == "no_groups")
    if name == "no_gas":
        assert results[1]["nrows"] == 0 and results[1]["ntests"] == 0 and len(results[1]["entropy"]) == 0
    if name == "no_groups":
        assert all(line[0] != 1 for line in wlog)


def test_nothing_to_do_gloo():
    """a global candidate count of 0; a box already at the target; the flash"""
    _, wres, _ = check(spawned(2, "no_candidates"), "no_candidates", 2)
    assert wres["n_candidates"] == 0 and wres["n_iterations"] == 0 and wres["init_ionfrac"] < 0.5
    _, wres, _ = check(spawned(2, "at_target"), "at_target", 2)
    assert wres["n_candidates"] == 0 and wres["n_ionized"] == 0 and wres["init_ionfrac"] >= 0.01
    results = spawned(2, "flash")
    _, wres, _ = check(results, "flash", 2)
    assert wres["n_flash"] > 1000 and wres["init_ionfrac"] == 1.0 and all(0 < r["nrows"] < wres["n_flash"] for r in results)


def test_a_negative_radius_raises_on_every_rank_gloo():
    import heiii_dist_restated as hd
    results = spawned(2, "negative_radius")
    case = dict(CASES["negative_radius"][0], world=2)
    s = hd.global_set(**case)
    flags, entropy = hd.assemble(results, case)
    assert all(r["error"] is not None and "negative radius" in r["error"] and r["nrows"] == 0 for r in results)
    assert np.array_equal(flags, s["Pg"]["Flags"]) and np.array_equal(entropy, s["Sg"]["Entropy"])
    with pytest.raises(ValueError):
        hd.reference(**case)


@pytest.mark.parametrize("world", [2, 3])
def test_an_infinite_radius_takes_everything_everywhere_gloo(world):
    """u1 = 0 in gaussian_rng with var_bubble > 0: R = +inf, never culled, every eligible particle of every rank"""
    results = spawned(world, "u1_zero")
    wlog, wres, _ = check(results, "u1_zero", world)
    big = max(line[4] for line in wlog)
    assert big > 1000 and wres["final_ionfrac"] > 0.9 and all(r["nrows"] > 100 for r in results)


def test_culling_rule_against_the_particle_test():
    """heiii_bubble_reaches may say False only where no particle of the box [lo, hi] passes the sweep's test.  Brute force over random
    extents and bubbles, the extents' corners among the particles; centres and particles inside the periodic box (where a real run
    keeps them), and outside it by up to a box length, where NEAREST wraps only once and the rule must keep what it cannot prove."""
    import heiii_restated as hr
    from shenqi_amd import dist as sd
    L = 1000.0
    rng = np.random.default_rng(0)
    culled = {False: 0, True: 0}
    for it in range(4000):
        outside = it % 2 == 1
        lo = rng.uniform(-L, 2 * L, 3) if outside else rng.uniform(0, L, 3)
        hi = lo + rng.uniform(0, 0.6 * L, 3)
        if not outside:
            hi = np.minimum(hi, np.nextafter(L, 0))
        x = rng.uniform(lo, hi, (200, 3))
        x[0], x[1] = lo, hi
        c = rng.uniform(-L, 2 * L, 3) if outside else rng.uniform(0, L, 3)
        R = rng.uniform(0, 0.3 * L) if it % 7 else rng.uniform(0, 0.01 * L)
        if it % 5 == 0:       # a particle right under the centre on two axes: only the third axis can prove anything
            x[2, :2] = np.clip(c[:2], lo[:2], hi[:2])
        dx, dy, dz = (hr.nearest(c[d] - x[:, d], L) for d in range(3))
        r2 = dx * dx
        r2 = r2 + dy * dy
        r2 = r2 + dz * dz
        if not sd.heiii_bubble_reaches(c, R, lo, hi, L):
            culled[outside] += 1
            assert not np.any(~(r2 > R * R)), (c, R, lo, hi)
    assert culled[False] > 500 and culled[True] > 100
    # the two boxes a rule without the |t| <= L guard culls although a particle sits under the centre, and what is never culled
    assert sd.heiii_bubble_reaches([1.2, 0.5, 0.5], 0.05, [0.1, 0.4, 0.4], [0.3, 0.6, 0.6], 1.0)
    assert sd.heiii_bubble_reaches([0.995, 0.5, 0.5], 0.003, [-0.01, 0.4, 0.4], [0.2, 0.6, 0.6], 1.0)
    assert not sd.heiii_bubble_reaches([0.5, 0.5, 0.5], 0.05, [0.1, 0.4, 0.4], [0.3, 0.6, 0.6], 1.0)
    for R in (np.inf, np.nan):
        assert sd.heiii_bubble_reaches([0.5, 0.5, 0.5], R, [0.1, 0.4, 0.4], [0.3, 0.6, 0.6], 1.0)
    assert sd.heiii_bubble_reaches([np.nan, 0.5, 0.5], 0.05, [0.1, 0.4, 0.4], [0.3, 0.6, 0.6], 1.0)
    assert sd.heiii_bubble_reaches([0.5, 0.5, 0.5], 0.05, [np.nan, 0.4, 0.4], [0.3, 0.6, 0.6], 1.0)
    assert sd.heiii_bubble_reaches([0.9, 0.5, 0.5], 0.05, [0.0, 0.4, 0.4], [0.5, 0.6, 0.6], 1.0)      # half a box wide
