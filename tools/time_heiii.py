"""Device time of shq_heiii_reionization (helium reionisation by quasar bubbles, one rank) on clustered 2 x 128^3 and 2 x 256^3 sets,
with about 1000 candidate groups (the most massive ones of the catalogue shq_fof leaves) and a target that lights LIT bubbles.

  call      wall = host clock around the call (uploads skipped: shq_set_inputs_current), device = shq_heiii_last_stats ms[3]
  phases    ms[0] candidates + eligible list, ms[1] sweeps, ms[2] stop replays + partitions + applies
  sweeps    per sweep: draws, lit bubbles, eligible particles
Model per sweep (from shapes): bytes = eligible x (32 B record read + 4 B hit write); distance tests = eligible x lit, about 12 f64
operations each (3 differences, NEAREST's 2 compares and select per axis, 3 products, 2 sums, the compare); the sweep's share of the
HBM peak (8 TB/s) and of the f64 vector peak (78.6 TFLOP/s) is printed, whichever is larger bounds it.  The restatement's CPU time
(heiii_restated.py, the first RESTATE iterations, scaled) is for context only.  One JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import shenqi_amd as sq  # noqa: E402
from shenqi_amd import capi  # noqa: E402

BOX = 100000.0
HBM_PEAK = 8.0e12
F64_PEAK = 78.6e12
FLOP_PER_TEST = 12


def particles(N, nhalo, seed=3):
    """N^3 dark matter, 60 % of it in nhalo halos of power-law sizes, and N^3 gas next to it"""
    rng = np.random.default_rng(seed)
    n = N ** 3
    sep = BOX / N
    centres = rng.uniform(0, BOX, (nhalo, 3))
    w = rng.pareto(1.5, nhalo) + 1
    nin = int(0.6 * n)
    h = rng.choice(nhalo, nin, p=w / w.sum())
    r = 0.15 * sep * np.cbrt(w[h] / w.min())
    dm = np.concatenate([centres[h] + rng.normal(size=(nin, 3)) * r[:, None], rng.uniform(0, BOX, (n - nin, 3))])
    gas = dm + rng.normal(0, 0.05 * sep, dm.shape)
    pman = sq.PartManager(2 * n, BOX)
    P = pman.Base
    P["Pos"] = np.mod(np.concatenate([dm, gas]), BOX)
    P["Type"][:n] = 1
    P["Type"][n:] = 0
    P["Mass"] = np.where(P["Type"] == 0, 0.2, 1.0).astype(np.float32)
    P["ID"] = np.arange(1, 2 * n + 1, dtype=np.uint64)
    P["Hsml"] = sep
    P["PI"][n:] = np.arange(n)
    S = np.zeros(n, dtype=capi.SPH_DTYPE)
    S["Density"] = rng.uniform(0.5, 50.0, n)
    S["Entropy"] = rng.uniform(1.0, 10.0, n)
    return pman, S, n


def fof(ctx, pman, S, N):
    pv, sv = pman.view(), capi.sph_view(S)
    capi.check(capi.hip.shq_set_inputs_current(ctx.h, 0))
    capi.check(capi.hip.shq_particles_upload(ctx.h, C.byref(pv)))
    sq.dynamics_upload(ctx, pman)
    capi.check(capi.hip.shq_sph_state_upload(ctx.h, C.byref(pv), C.byref(sv)))
    ng = C.c_int64()
    fp = capi.FofParams(BOX, 0.2 * BOX / N, 2, 1 + 16 + 32, 32, 0)
    capi.check(capi.hip.shq_fof(ctx.h, C.byref(fp), capi.ptr(np.ascontiguousarray(pman.Base["ID"])), None, None, C.byref(ng)))
    groups = np.zeros(ng.value, dtype=capi.FOF_GROUP_DTYPE)
    capi.check(capi.hip.shq_fof_groups_download(ctx.h, capi.ptr(groups), len(groups)))
    return groups


def hparams(n, minmass, desired, mean):
    p = capi.HeiiiParams()
    for k, v in dict(BoxSize=BOX, atime=0.25, qso_candidate_min_mass=minmass, qso_candidate_max_mass=1e30, mean_bubble=mean, var_bubble=0.0,
                     heIIIreion_finish_frac=0.999, desired_ion_frac=desired, qso_inst_heating=2e-12, uu_in_cgs=1e10, OmegaBaryon=0.045,
                     HubbleParam=0.7, n_gas_tot=n).items():
        setattr(p, k, v)
    return p


def one_size(ctx, N, rounds, warmup, lit, ncand, restate):
    pman, S, n = particles(N, 4 * ncand)
    flags0, ent0 = pman.Base["Flags"].copy(), S["Entropy"].copy()
    rnd = np.random.default_rng(5).random(1 << 14)
    mean = 0.02 * BOX
    groups = fof(ctx, pman, S, N)
    masses = np.sort(groups["Mass"])[::-1]
    minmass = float(masses[min(ncand, len(masses)) - 1])
    # the target: the fraction after the lit-th lit bubble of a run to the end of the list
    capi.check(capi.hip.shq_set_inputs_current(ctx.h, 3))
    _, log = sq.heiii_reionization(ctx, pman, S, hparams(n, minmass, 0.99, mean), rnd)
    nz = np.flatnonzero(log["group"] >= 0)
    desired = float(log["ionfrac"][nz[min(lit, len(nz)) - 1]])
    out = dict(N=N, particles=2 * n, groups=len(groups), mean_bubble=mean, desired=desired)
    walls, st = [], None
    for r in range(warmup + rounds):
        pman.Base["Flags"], S["Entropy"] = flags0, ent0
        fof(ctx, pman, S, N)
        capi.check(capi.hip.shq_set_inputs_current(ctx.h, 3))
        t0 = time.perf_counter()
        res, log = sq.heiii_reionization(ctx, pman, S, hparams(n, minmass, desired, mean), rnd)
        wall = (time.perf_counter() - t0) * 1e3
        capi.check(capi.hip.shq_set_inputs_current(ctx.h, 0))
        st = capi.HeiiiStats()
        capi.check(capi.hip.shq_heiii_last_stats(ctx.h, C.byref(st)))
        if r >= warmup:
            walls.append((wall, list(st.ms)))
    ns = min(st.nsweeps, capi.HEIII_NSTAT)
    sweeps = []
    for k in range(ns):
        m, L = st.sweep_eligible[k], st.sweep_lit[k]
        sweeps.append(dict(draws=st.sweep_draws[k], lit=L, eligible=m, bytes=36 * m, tests=m * L, flop=FLOP_PER_TEST * m * L))
    sweep_ms = float(np.median([w[1][1] for w in walls]))
    tb = sum(s["bytes"] for s in sweeps)
    tf = sum(s["flop"] for s in sweeps)
    out.update(candidates=res.n_candidates, iterations=res.n_iterations, lit=int(np.count_nonzero(log["group"] >= 0)), n_ionized=res.n_ionized,
               final_ionfrac=res.final_ionfrac, wall_ms=float(np.median([w[0] for w in walls])),
               device_ms=float(np.median([w[1][3] for w in walls])), phase_ms=[float(np.median([w[1][i] for w in walls])) for i in range(4)],
               nsweeps=st.nsweeps, neligible=st.neligible, ntests=st.ntests, sweeps=sweeps,
               sweep_bytes=tb, sweep_flop=tf, sweep_hbm_share=tb / (sweep_ms * 1e-3) / HBM_PEAK if sweep_ms > 0 else None,
               sweep_f64_share=tf / (sweep_ms * 1e-3) / F64_PEAK if sweep_ms > 0 else None,
               sweep_tests_per_s=st.ntests / (sweep_ms * 1e-3) if sweep_ms > 0 else None)
    if restate:
        import heiii_restated as hr
        P = pman.Base
        pd = dict(BoxSize=BOX, atime=0.25, qso_candidate_min_mass=minmass, qso_candidate_max_mass=1e30, mean_bubble=mean, var_bubble=0.0,
                  heIIIreion_finish_frac=0.999, desired_ion_frac=desired, qso_inst_heating=2e-12, uu_in_cgs=1e10, OmegaBaryon=0.045,
                  HubbleParam=0.7, CurrentParticleOffset=(0.0, 0.0, 0.0), n_gas_tot=n)
        t0 = time.perf_counter()
        hr.turn_on_quasars(P["Pos"], P["Type"], flags0, P["PI"], S["Density"], ent0, groups, rnd, pd, stop_after=restate)
        t = time.perf_counter() - t0
        out.update(restated_s_first=t, restated_iterations=restate, restated_s_scaled=t * res.n_iterations / restate)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,256")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--lit", type=int, default=250)
    ap.add_argument("--candidates", type=int, default=1000)
    ap.add_argument("--restate", type=int, default=20, help="iterations of the restatement to time (0: none)")
    a = ap.parse_args()
    res = []
    with sq.Context(0) as ctx:
        for N in [int(x) for x in a.sizes.split(",")]:
            r = one_size(ctx, N, a.rounds, a.warmup, a.lit, a.candidates, a.restate)
            print(json.dumps(r), file=sys.stderr)
            res.append(r)
    print(json.dumps(dict(heiii=res)))


if __name__ == "__main__":
    main()
