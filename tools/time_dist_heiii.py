"""Device time of helium reionisation in phases (shq_heiii_open / _sweep / _commit / _close driven by dist.py:DistHeIII) beside the one
call (shq_heiii_reionization) on tools/time_heiii.py's clustered 2 x 128^3 set: about 1000 candidates, a target that lights LIT bubbles.

  one rank, one context   the one call with and without shq_set_inputs_current (with: no upload), then DistHeIII on one rank without a
                          process group (its open uploads: it works on its own copy of the records).  Device ms from
                          shq_heiii_last_stats: the one call's lists / sweeps / commits / whole call; the run's open / sweeps / commits /
                          close.  wall = host clock around the call.
  two ranks, one GPU      two gloo ranks in fresh child processes with a context each on device 0, the particles split at x = BoxSize / 2,
                          every group hosted by the rank that holds its centre: with and without culling, per rank the tests made, the
                          bubbles swept per batch and the device ms of the sweeps.  The two processes share the device, so these sweep
                          times are not a scaling number; the tests made are the point.

Writes profiles/dist_heiii_timing.json (or --out) and prints it as one JSON line.  Nothing here runs on more than one GPU."""
import argparse
import ctypes as C
import json
import os
import pickle
import sys
import tempfile
import time

import numpy as np
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import shenqi_amd as sq  # noqa: E402
from shenqi_amd import capi  # noqa: E402
from shenqi_amd import dist as sd  # noqa: E402
import time_heiii as th  # noqa: E402


def stats(ctx):
    st = capi.HeiiiStats()
    capi.check(capi.hip.shq_heiii_last_stats(ctx.h, C.byref(st)))
    return st


def med(rows):
    return [float(x) for x in np.median(np.array(rows, dtype=np.float64), axis=0)]


def _worker(rank, world, initfile, tmp, N, ncand):
    os.environ["OMP_NUM_THREADS"] = "2"
    dist.init_process_group("gloo", init_method="file://" + initfile, rank=rank, world_size=world)
    try:
        with open(os.path.join(tmp, "set.pkl"), "rb") as f:
            groups, minmass, desired, mean, rnd, rounds = pickle.load(f)
        pman, S, n = th.particles(N, 4 * ncand)
        half = 0.5 * th.BOX
        mine = np.flatnonzero((pman.Base["Pos"][:, 0] >= half) == (rank == 1))
        P0 = pman.Base[mine].copy()
        gas = P0["Type"] == 0
        S0 = S[P0["PI"][gas]].copy()
        P0["PI"][gas] = np.arange(len(S0))
        hosted = groups[(groups["CM"][:, 0] >= half) == (rank == 1)]
        out = {}
        with sq.Context(0) as ctx:
            for cull in (True, False):
                rows = []
                for r in range(1 + rounds):
                    P, Sr = P0.copy(), S0.copy()
                    drv = sd.DistHeIII(sd.Comm(), sd.GpuHeiiiOps(ctx, th.BOX, cull=cull))
                    log, res = drv.run(P, Sr, hosted, len(groups), th.hparams(n, minmass, desired, mean), rnd)
                    st = stats(ctx)
                    if r > 0:
                        rows.append(list(st.ms))
                out["culled" if cull else "all"] = dict(gas=int(len(S0)), hosted_groups=int(len(hosted)), eligible=int(st.neligible), ntests=int(drv.ntests),
                                                       kept_per_batch=[int(k) for k in drv.kept], rows_written=int(drv.nrows),
                                                       open_sweeps_commits_total_ms=med(rows), iterations=int(res["n_iterations"]),
                                                       n_ionized=int(res["n_ionized"]), final_ionfrac=float(res["final_ionfrac"]),
                                                       events=dict(drv.events))
        with open(os.path.join(tmp, "r%d.pkl" % rank), "wb") as f:
            pickle.dump(out, f)
    finally:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--lit", type=int, default=250)
    ap.add_argument("--candidates", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dist_heiii_timing.json"))
    a = ap.parse_args()
    N = a.size
    pman, S, n = th.particles(N, 4 * a.candidates)
    flags0, ent0 = pman.Base["Flags"].copy(), S["Entropy"].copy()
    rnd = np.random.default_rng(5).random(1 << 14)
    mean = 0.02 * th.BOX
    out = dict(N=N, particles=2 * n, mean_bubble=mean)
    with sq.Context(0) as ctx:
        groups = th.fof(ctx, pman, S, N)
        masses = np.sort(groups["Mass"])[::-1]
        minmass = float(masses[min(a.candidates, len(masses)) - 1])
        capi.check(capi.hip.shq_set_inputs_current(ctx.h, 3))
        _, log = sq.heiii_reionization(ctx, pman, S, th.hparams(n, minmass, 0.99, mean), rnd)
        nz = np.flatnonzero(log["group"] >= 0)
        desired = float(log["ionfrac"][nz[min(a.lit, len(nz)) - 1]])
        out.update(groups=len(groups), desired=desired)
        for name, mask in (("one_call_resident", 3), ("one_call_upload", 0)):
            rows = []
            for r in range(1 + a.rounds):
                pman.Base["Flags"], S["Entropy"] = flags0, ent0
                th.fof(ctx, pman, S, N)
                capi.check(capi.hip.shq_set_inputs_current(ctx.h, mask))
                t0 = time.perf_counter()
                res, log = sq.heiii_reionization(ctx, pman, S, th.hparams(n, minmass, desired, mean), rnd)
                wall = (time.perf_counter() - t0) * 1e3
                capi.check(capi.hip.shq_set_inputs_current(ctx.h, 0))
                st = stats(ctx)
                if r > 0:
                    rows.append(list(st.ms) + [wall])
            out[name] = dict(lists_sweeps_commits_call_ms_wall_ms=med(rows), nsweeps=int(st.nsweeps), ntests=int(st.ntests), iterations=int(res.n_iterations),
                             n_ionized=int(res.n_ionized), candidates=int(res.n_candidates))
        one_flags, one_entropy = pman.Base["Flags"].copy(), S["Entropy"].copy()
        rows = []
        for r in range(1 + a.rounds):
            pman.Base["Flags"], S["Entropy"] = flags0, ent0
            P, Sr = pman.Base.copy(), S.copy()
            drv = sd.DistHeIII(sd.Comm(), sd.GpuHeiiiOps(ctx, th.BOX))
            t0 = time.perf_counter()
            dlog, dres = drv.run(P, Sr, groups, len(groups), th.hparams(n, minmass, desired, mean), rnd)
            wall = (time.perf_counter() - t0) * 1e3
            st = stats(ctx)
            ms = list(st.ms)
            if r > 0:
                rows.append(ms[:3] + [ms[3] - ms[0] - ms[1] - ms[2], ms[3], wall])
        out["phases_one_rank"] = dict(open_sweeps_commits_close_total_ms_wall_ms=med(rows), nsweeps=int(drv.nsweeps), ntests=int(drv.ntests),
                                      iterations=int(dres["n_iterations"]), n_ionized=int(dres["n_ionized"]),
                                      same_bits_as_the_one_call=bool(np.array_equal(P["Flags"], one_flags) and np.array_equal(Sr["Entropy"], one_entropy)))
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "set.pkl"), "wb") as f:
            pickle.dump((groups, minmass, desired, mean, rnd, a.rounds), f)
        mp.spawn(_worker, args=(2, os.path.join(tmp, "init"), tmp, N, a.candidates), nprocs=2, join=True)
        ranks = []
        for r in range(2):
            with open(os.path.join(tmp, "r%d.pkl" % r), "rb") as f:
                ranks.append(pickle.load(f))
    out["two_ranks_one_gpu"] = ranks
    out["note"] = ("device ms are HIP-event times from shq_heiii_last_stats, medians over the rounds after one warm-up; the phased run uploads its own "
                   "copy of the records in open, so it compares with one_call_upload; the two ranks are two processes sharing one device")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
