"""GPU tests of helium reionisation in phases (shq_heiii_open / _sweep / _commit / _close / _host_numbers, csrc/heiii.hip) and of the
multi-rank driver on them (shenqi_amd/dist.py:DistHeIII with GpuHeiiiOps).

  * the parts against the one call: DistHeIII on one rank, fed the downloaded FOF catalogue, and shq_heiii_reionization on the same set
    give the same flags and Entropy bit for bit, the same log, result and number of sweeps;
  * against the restatement (tests/heiii_dist_restated.py): flags exact, Entropy to 1e-14 (the device's pow is not glibc's; the bar of
    tests/test_gpu_heiii.py), log and result exact;
  * the phases called directly: extents, a sweep of 300 bubbles with sparse seq against a numpy first-hit, the empty list, seq_stop = 0,
    every out-of-order call (open while a density walk is open among them), every refused argument;
  * two runs give the same bits; two gloo ranks sharing the GPU, in fresh child processes, against the restatement for that split."""
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
import heiii_dist_restated as hd  # noqa: E402
import test_gpu_heiii as one  # noqa: E402  (its particle set, FOF call and parameters)

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE = 1, 4
RESULT_FIELDS = ("init_ionfrac", "final_ionfrac", "n_candidates", "n_iterations", "n_flash", "n_ionized")


@pytest.mark.parametrize("case", ["stop_in_first_batch", "three_batches"])
def test_parts_equal_the_one_call(ctx, case):
    pman, S, ngas = one._particles(16, 160)
    groups = one._fof(ctx, pman, S, 16)
    rnd = np.random.default_rng(5).random(4096)
    if case == "stop_in_first_batch":
        init = np.count_nonzero((pman.Base["Type"] == 0) & (pman.Base["Flags"] & 4 != 0)) / ngas
        p = one._params(ngas, desired_ion_frac=init + 0.01)
    else:
        p = one._params(ngas, mean_bubble=700.0, qso_candidate_min_mass=2.0)
    P, S2 = pman.Base.copy(), S.copy()
    res, log = sq.heiii_reionization(ctx, pman, S, one._struct(p), rnd)          # first: it reads the resident catalogue
    nsweeps = one._stats(ctx).nsweeps
    drv = sd.DistHeIII(sd.Comm(), sd.GpuHeiiiOps(ctx, one.BOX))
    dlog, dres = drv.run(P, S2, groups, len(groups), one._struct(p), rnd)
    assert np.array_equal(P["Flags"], pman.Base["Flags"]) and np.array_equal(S2["Entropy"], S["Entropy"])
    assert dres == {k: getattr(res, k) for k in RESULT_FIELDS} and drv.nsweeps == nsweeps
    assert len(dlog) == len(log)
    for got, want in zip(dlog, log):
        grp = int(want["group"])
        assert got == (0 if grp >= 0 else -1, grp, tuple(float(x) for x in want["pos"]), float(want["ionfrac"]), int(want["n_ionized"]))
    assert res.n_ionized > 0 and drv.nrows == res.n_ionized
    assert (nsweeps == 1 and res.n_iterations < 32) if case == "stop_in_first_batch" else nsweeps >= 3


def _against_restatement(results, case):
    wflags, wentropy, wlog, wres, ev = hd.reference(**case)
    flags, entropy = hd.assemble(results, case)
    assert np.array_equal(flags, wflags), np.flatnonzero(flags != wflags)[:10]
    assert np.all(np.abs(entropy - wentropy) <= 1e-14 * np.abs(wentropy))
    for r in results:
        assert r["error"] is None and r["log"] == wlog and r["res"] == wres
    return wlog, wres, ev


@pytest.mark.parametrize("case", [dict(world=1), dict(world=1, var_bubble=1.0e4, u1_zero=2, desired_ion_frac=0.9), dict(world=1, flash=True)])
def test_one_rank_equals_the_restatement(ctx, case):
    res = hd.run_rank(sd.Comm(), 0, sd.GpuHeiiiOps(ctx, hd.BOX), case)
    wlog, wres, _ = _against_restatement([res], case)
    assert wres["n_flash"] > 1000 if case.get("flash") else wres["n_ionized"] > 100


def test_two_runs_give_the_same_bits(ctx):
    a, b = (hd.run_rank(sd.Comm(), 0, sd.GpuHeiiiOps(ctx, hd.BOX), dict(world=1)) for _ in range(2))
    assert np.array_equal(a["flags"], b["flags"]) and np.array_equal(a["entropy"], b["entropy"]) and a["log"] == b["log"] and a["res"] == b["res"]


def _records(n, nelig, seed=2):
    """n particles of which exactly nelig are eligible gas, inside the middle 0.8^3 of the box; the rest dark matter, garbage gas and
    ionised gas, spread over the whole box"""
    rng = np.random.default_rng(seed)
    P = np.zeros(n, dtype=capi.PARTICLE_DTYPE)
    P["Pos"] = rng.uniform(0, hd.BOX, (n, 3))
    P["Mass"], P["Hsml"], P["ID"] = 1.0, hd.BOX / 20, np.arange(n) + 1
    kind = np.full(n, 3)                                   # 0 eligible, 1 garbage gas, 2 ionised gas, 3 dark matter
    kind[:n // 2] = rng.integers(1, 3, n // 2)
    kind[rng.choice(n // 2, nelig, replace=False)] = 0
    kind = kind[rng.permutation(n)]
    P["Pos"][kind == 0] = 0.1 * hd.BOX + 0.8 * P["Pos"][kind == 0]
    P["Type"] = np.where(kind == 3, 1, 0)
    P["Flags"] = np.where(kind == 1, 1, 0) | np.where(kind == 2, 4, 0) | (rng.integers(0, 16, n) << 4)
    gas = np.flatnonzero(kind != 3)
    P["PI"][gas] = np.arange(len(gas))
    S = np.zeros(len(gas), dtype=capi.SPH_DTYPE)
    S["Density"], S["Entropy"] = rng.uniform(0.5, 50.0, len(S)), rng.uniform(1.0, 10.0, len(S))
    return P, S, kind == 0


def _bubbles(nb, seed=4):
    rng = np.random.default_rng(seed)
    b = np.zeros(nb, dtype=capi.HEIII_BUBBLE_DTYPE)
    b["c"], b["R"] = rng.uniform(0, hd.BOX, (nb, 3)), rng.uniform(0.04, 0.1, nb) * hd.BOX
    b["seq"] = np.sort(rng.choice(1023, nb, replace=False))
    b["seq"][-1], b["R"][-1] = 1023, 0.3 * hd.BOX       # the last counter of the histogram gets hits of its own
    return b


@pytest.mark.parametrize("nelig", [0, 1, 255, 257, 5000])
def test_extents_are_numpys(ctx, nelig):
    P, S, elig = _records(12000, nelig)
    ops = sd.GpuHeiiiOps(ctx, hd.BOX)
    n_flash, nion, m, lo, hi = ops.open(P, S, hd.params_struct(hd.params_dict(len(S))))
    try:
        assert n_flash == 0 and m == nelig and nion == np.count_nonzero((P["Type"] == 0) & (P["Flags"] & 4 != 0))
        if nelig:
            assert np.array_equal(lo, P["Pos"][elig].min(axis=0)) and np.array_equal(hi, P["Pos"][elig].max(axis=0))
            assert np.all(lo > P["Pos"].min(axis=0)) and np.all(hi < P["Pos"].max(axis=0))      # the others lie beyond them
        else:
            assert np.all(lo > hi) and np.all(np.isinf(lo)) and np.all(np.isinf(hi))
    finally:
        assert ops.close(P, S) == 0


def test_sweep_commit_close_against_numpy(ctx):
    """300 bubbles with sparse seq up to 1023 over 5000 eligible records in 20 workgroups: the LDS histogram's loops beyond one pass of
    256 threads and its flush to counts[seq]; then the empty list, seq_stop = 0, a second sweep of what is left, close"""
    P, S, elig = _records(12000, 5000)
    P0, S0 = P.copy(), S.copy()
    p = hd.params_struct(hd.params_dict(len(S)))
    gpu, ref = sd.GpuHeiiiOps(ctx, hd.BOX), hd.RestatedHeiiiOps()
    Pr, Sr = P.copy(), S.copy()
    assert gpu.open(P, S, p)[:3] == ref.open(Pr, Sr, p)[:3]
    bub = _bubbles(300)
    got, want = gpu.sweep(bub, 1024), ref.sweep(bub, 1024)
    assert np.array_equal(got, want) and np.count_nonzero(want) > 150 and want[1023] > 0 and want.sum() > 1000
    assert np.all(want[np.setdiff1d(np.arange(1024), bub["seq"])] == 0)
    assert np.array_equal(gpu.sweep(bub, 1024), want)                                # a sweep may be repeated
    assert gpu.commit(0) == 0                                                         # seq_stop = 0 commits nothing
    assert np.array_equal(gpu.sweep(bub, 1024), want)
    stop = int(bub["seq"][150]) + 1
    assert gpu.commit(stop) == ref.commit(stop) == int(want[:stop].sum()) > 0
    assert np.array_equal(gpu.sweep(bub[:0], 1), np.zeros(1, dtype=np.uint64))        # the empty list
    ref.sweep(bub[:0], 1)
    assert gpu.commit(1) == ref.commit(1) == 0
    rest = bub[140:].copy()                                                           # what is left, numbered anew from 0
    rest["seq"] = np.arange(len(rest))
    got, want2 = gpu.sweep(rest, len(rest)), ref.sweep(rest, len(rest))
    assert np.array_equal(got, want2) and want2[:10].sum() == 0 and want2.sum() == want[stop:].sum()
    assert gpu.commit(len(rest)) == ref.commit(len(rest))
    assert np.array_equal(P["Flags"], P0["Flags"]) and np.array_equal(S["Entropy"], S0["Entropy"])      # nothing written before close
    assert gpu.close(P, S) == ref.close(Pr, Sr) == int(want.sum())
    assert np.array_equal(P["Flags"], Pr["Flags"]) and np.all(np.abs(S["Entropy"] - Sr["Entropy"]) <= 1e-14 * np.abs(Sr["Entropy"]))
    assert np.array_equal(P["Flags"] & ~np.uint8(4), P0["Flags"] & ~np.uint8(4)) and (S["Entropy"] != S0["Entropy"]).sum() == want.sum()
    st = one._stats(ctx)
    assert st.nsweeps == 5 and st.ntests == 3 * 5000 * 300 + (5000 - int(want[:stop].sum())) * len(rest) and st.neligible == 5000


def test_host_numbers_are_the_restatements(ctx):
    import heiii_restated as hr
    rnd = np.random.default_rng(3).random(512)
    rnd[7] = 0.0
    minids = np.array([7, 8, 511, 512, 12345678901234567], dtype=np.uint64)
    p = hd.params_dict(123456, mean_bubble=1500.0, var_bubble=2.5e5)
    radii, nn = sq.heiii_host_numbers(hd.params_struct(p), minids, rnd)
    want = [hr.gaussian_rng(1500.0, hr._libm.sqrt(2.5e5), int(m), rnd) for m in minids]
    assert np.array_equal(radii, want, equal_nan=True) and np.isinf(radii[0])
    a3inv = 1 / hr._libm.pow(p["atime"], 3)
    rhobar = p["OmegaBaryon"] * (3 * hr.HUBBLE * p["HubbleParam"] * hr.HUBBLE * p["HubbleParam"]) / (8 * np.pi * hr.GRAVITY) * a3inv
    assert nn == int(p["n_gas_tot"] * (4 * np.pi / 3. * hr._libm.pow(p["mean_bubble"], 3) * rhobar) / p["OmegaBaryon"])


def test_calls_out_of_order_and_refused_arguments(ctx):
    P, S, elig = _records(3000, 700)
    P0, S0 = P.copy(), S.copy()
    pman = sd.records_pman(sq, hd.BOX, P)
    pv, sv = pman.view(), capi.sph_view(S)
    p = hd.params_struct(hd.params_dict(len(S)))
    h = capi.hip
    counts = np.zeros(1024, dtype=np.uint64)
    bub = _bubbles(40)
    n64 = [C.c_int64() for _ in range(4)]
    lo, hi = np.zeros(3), np.zeros(3)

    def open_():
        return h.shq_heiii_open(ctx.h, C.byref(p), C.byref(pv), C.byref(sv), C.byref(n64[0]), C.byref(n64[1]), C.byref(n64[2]), capi.ptr(lo), capi.ptr(hi))

    def sweep(b, nseq=1024):
        b = np.ascontiguousarray(b)
        return h.shq_heiii_sweep(ctx.h, capi.ptr(b), len(b), nseq, capi.ptr(counts))

    def untouched():
        return all(np.array_equal(a[k], b[k], equal_nan=True) for a, b in ((pman.Base, P0), (S, S0)) for k in b.dtype.names)
    # no run: sweep, commit and close refuse
    assert sweep(bub) == ERR_STATE and h.shq_heiii_commit(ctx.h, 5, None) == ERR_STATE
    assert h.shq_heiii_close(ctx.h, C.byref(pv), C.byref(sv), None) == ERR_STATE
    assert open_() == 0 and n64[2].value == 700
    assert open_() == ERR_STATE                                         # another run while one is open
    assert h.shq_heiii_commit(ctx.h, 5, None) == ERR_STATE              # commit without a sweep
    for bad in ("negative", "minus_inf", "seq_equal", "seq_down", "seq_beyond"):
        b = bub.copy()
        if bad == "negative":
            b["R"][3] = -1.0
        elif bad == "minus_inf":
            b["R"][3] = -np.inf
        elif bad == "seq_equal":
            b["seq"][5] = b["seq"][4]
        elif bad == "seq_down":
            b["seq"][[5, 6]] = b["seq"][[6, 5]]
        else:
            b["seq"][-1] = 1024
        assert sweep(b) == ERR_INVALID and untouched(), bad
        assert h.shq_heiii_commit(ctx.h, 5, None) == ERR_STATE, bad     # the refused sweep did not count as one
    assert sweep(bub, 1025) == ERR_INVALID and sweep(bub, 0) == ERR_INVALID and sweep(bub[:30], 20) == ERR_INVALID
    assert sweep(bub) == 0 and counts.sum() > 0
    assert h.shq_heiii_commit(ctx.h, -1, None) == ERR_INVALID and h.shq_heiii_commit(ctx.h, 1025, None) == ERR_INVALID
    assert h.shq_heiii_commit(ctx.h, 1024, C.byref(n64[3])) == 0 and n64[3].value == counts.sum()
    assert h.shq_heiii_commit(ctx.h, 1024, None) == ERR_STATE           # a second commit needs a sweep of its own
    fewer = sd.records_pman(sq, hd.BOX, P[:-5])
    assert h.shq_heiii_close(ctx.h, C.byref(fewer.view()), C.byref(sv), None) == ERR_INVALID and untouched()   # not the records of the open
    assert h.shq_heiii_close(ctx.h, C.byref(pv), C.byref(sv), C.byref(n64[3])) == 0 and n64[3].value == counts.sum()   # still closable
    assert not untouched() and np.count_nonzero(pman.Base["Flags"] != P0["Flags"]) == counts.sum()
    assert h.shq_heiii_close(ctx.h, C.byref(pv), C.byref(sv), None) == ERR_STATE
    assert open_() == 0 and h.shq_heiii_close(ctx.h, C.byref(pv), C.byref(sv), None) == 0                         # and a new run opens


def test_open_and_an_sph_walk_exclude_each_other(ctx):
    """shq_heiii_open while a density walk is open (shq_density_open ... shq_density_close): SHQ_ERR_STATE, the records untouched, no run
    left behind; after the walk is closed a run opens.  And the other way round: no SPH walk opens while a run is open."""
    import common as cm
    import test_gpu_sph_dist as sphd
    pman, S, BhP, _ = sphd._gas(n1=8)
    dp = cm.density_params(update_hsml=0)
    tree = sq.force_tree_rebuild_mask(pman, sq.GASMASK)
    pv, tv, sv, bv = pman.view(), tree.view(), capi.sph_view(S), capi.bh_view(BhP)
    p = hd.params_struct(hd.params_dict(len(S), BoxSize=cm.BOX))
    h = capi.hip
    n64 = [C.c_int64() for _ in range(3)]
    lo, hi = np.zeros(3), np.zeros(3)
    counts = np.zeros(4, dtype=np.uint64)
    nredo = C.c_int64()

    def open_():
        return h.shq_heiii_open(ctx.h, C.byref(p), C.byref(pv), C.byref(sv), C.byref(n64[0]), C.byref(n64[1]), C.byref(n64[2]), capi.ptr(lo), capi.ptr(hi))

    def density_open():
        return h.shq_density_open(ctx.h, C.byref(tv), C.byref(pv), C.byref(sv), C.byref(bv), None, 0, C.byref(dp), 0, None)
    capi.check(density_open())
    P0, S0 = pman.Base.copy(), S.copy()
    assert open_() == ERR_STATE
    assert all(np.array_equal(a[k], b[k], equal_nan=True) for a, b in ((pman.Base, P0), (S, S0)) for k in b.dtype.names)
    assert h.shq_heiii_sweep(ctx.h, None, 0, 4, capi.ptr(counts)) == ERR_STATE           # no run stayed behind
    assert h.shq_heiii_commit(ctx.h, 0, None) == ERR_STATE and h.shq_heiii_close(ctx.h, C.byref(pv), C.byref(sv), None) == ERR_STATE
    capi.check(h.shq_density_ev_primary(ctx.h))                                            # the walk itself is unharmed
    capi.check(h.shq_density_ev_postprocess(ctx.h, C.byref(nredo)))
    capi.check(h.shq_density_close(ctx.h, None, C.byref(pv), C.byref(sv), C.byref(bv), None, None, None))
    assert nredo.value == 0 and np.all(S["Density"] > 0)
    assert open_() == 0 and n64[2].value == len(S)                                         # the walk is closed: a run opens
    assert density_open() == ERR_STATE                                                     # ... and keeps SPH walks out
    assert h.shq_heiii_sweep(ctx.h, None, 0, 4, capi.ptr(counts)) == 0 and h.shq_heiii_commit(ctx.h, 4, None) == 0
    assert h.shq_heiii_close(ctx.h, C.byref(pv), C.byref(sv), C.byref(n64[0])) == 0 and n64[0].value == 0
    capi.check(density_open())                                                             # the run is closed: a walk opens
    capi.check(h.shq_density_ev_primary(ctx.h))
    capi.check(h.shq_density_ev_postprocess(ctx.h, C.byref(nredo)))
    capi.check(h.shq_density_close(ctx.h, None, C.byref(pv), C.byref(sv), C.byref(bv), None, None, None))


def _worker(rank, world, initfile, outdir, cases):
    os.environ["OMP_NUM_THREADS"] = "2"
    dist.init_process_group("gloo", init_method="file://" + initfile, rank=rank, world_size=world)
    try:
        res = []
        with sq.Context(0) as ctx:
            for case, cull in cases:
                res.append(hd.run_rank(sd.Comm(), rank, sd.GpuHeiiiOps(ctx, hd.BOX, cull=cull), case))
        with open(os.path.join(outdir, "r%d.pkl" % rank), "wb") as f:
            pickle.dump(res, f)
    finally:
        dist.destroy_process_group()


def test_two_gloo_ranks_one_gpu_equal_the_restatement_for_that_split(ctx):
    """fresh child processes sharing the GPU, the CPU test's set and the events it asserts; with and without culling"""
    case = dict(world=2)
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_worker, args=(2, os.path.join(tmp, "init"), tmp, [(case, True), (case, False)]), nprocs=2, join=True)
        per_rank = []
        for r in range(2):
            with open(os.path.join(tmp, "r%d.pkl" % r), "rb") as f:
                per_rank.append(pickle.load(f))
    cut, uncut = [pr[0] for pr in per_rank], [pr[1] for pr in per_rank]
    wlog, wres, ev = _against_restatement(cut, case)
    _against_restatement(uncut, case)
    print("sharded helium reionisation on 2 ranks: %s, %d iterations, tests made %s (culled) %s (all)"
          % (ev, wres["n_iterations"], [r["ntests"] for r in cut], [r["ntests"] for r in uncut]))
    assert ev["two_host"] >= 1 and ev["after_two_host_unhosted"] >= 1 and ev["index0"] >= 1 and ev["face_split"] >= 1 and ev["idle"] >= 1
    assert wres["n_iterations"] > 32 and any(min(r["kept"]) == 0 and r["nrows"] > 0 for r in cut)
    for a, b in zip(cut, uncut):
        assert np.array_equal(a["flags"], b["flags"]) and np.array_equal(a["entropy"], b["entropy"])
    assert sum(r["ntests"] for r in cut) < sum(r["ntests"] for r in uncut)
