"""Device time of the star-formation kernel for 128^3 gas particles of which a few per cent lie on the effective equation of state (the
dense part drawn as tests/sfr_cases.py draws its set: Sherwood / Verner96, self-shielding on, the global UVB at z = 3, the reference's
default star-formation parameters), through shq_cooling -> shq_starformation; and the route the call replaces: shq_cooling's list, the
same engine on 16 host threads over the caller's records, and the upload of the particle and SPH records that the next device call then
needs because the host has changed them.

    python tools/time_sfr.py [out.json]        (default profiles/sfr_timing.json)

Kernel times are HIP-event times (shq_sfr_result.kernel_ms): the median of 5 calls after 1 warm-up call, per setting; every call starts
from the same records.  The host figure is the same engine on the CPU of the same box, not the reference's loop."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import shenqi_amd as sq                 # noqa: E402
from shenqi_amd import capi             # noqa: E402
import cooling_restated as cr           # noqa: E402
import sfr_cases as sc                  # noqa: E402

BOXSIZE = 20000.0
DENSE_SHARE = 0.04


def particles(n, par):
    un = sc.case().units
    rng = np.random.default_rng(128)
    P = np.zeros(n, dtype=capi.PARTICLE_DTYPE)
    P["Pos"] = rng.random((n, 3)) * BOXSIZE
    P["Mass"] = rng.uniform(0.4, 2.5, n)
    P["Hsml"] = rng.uniform(0.5, 5.0, n)
    P["TimeBinHydro"] = rng.integers(16, 20, n)
    P["PI"] = np.arange(n)
    P["Flags"] = ((rng.integers(0, 4, n) << 4) | (8 * (rng.random(n) < 0.3))).astype(np.uint8)
    S = np.zeros(n, dtype=capi.SPH_DTYPE)
    dens = 10.0 ** rng.uniform(-7, -2.5, n) * cr.PROTONMASS / un.density_in_phys_cgs / sc.A3INV
    mu = 4.0 / (1 + 3 * cr.HYDROGEN_MASSFRAC)
    u = 10.0 ** rng.uniform(2.5, 7.5, n) * cr.BOLTZMANN / (cr.GAMMA_MINUS1 * cr.PROTONMASS * mu) / un.uu_in_cgs
    dense = rng.random(n) < DENSE_SHARE
    dens[dense] = par["PhysDensThresh"] / sc.A3INV * 10.0 ** rng.uniform(0, 4, dense.sum())
    u[dense] = 10.0 ** rng.uniform(np.log10(par["EgySpecCold"]), 7, dense.sum())
    S["Density"] = dens
    S["Entropy"] = u / (np.exp(cr.GAMMA_MINUS1 * np.log(dens * sc.A3INV)) / cr.GAMMA_MINUS1)
    S["Ne"] = rng.uniform(0, 1.2, n)
    S["Metallicity"] = rng.uniform(0, 0.05, n)
    S["DivVel"], S["CurlVel"] = rng.normal(0, 300, n), np.abs(rng.normal(0, 300, n))
    return P, S, rng.integers(1, 2 ** 56, n, dtype=np.uint64), dense


def step(par):
    case = sc.case()
    st = capi.CoolingStep()
    st.redshift, st.a3inv, st.hubble = sc.REDSHIFT, sc.A3INV, sc.HUBBLE
    for b in range(capi.TIMEBINS + 1):
        st.kf.dloga_for_bin[b] = 0.0 if b <= 15 else 2.5e-4 * 2.0 ** (b - 16)
        st.lastred_for_bin[b] = sc.REDSHIFT
    for k, v in case.uv.items():
        setattr(st.GlobalUVBG, k, v)
    st.uvbg_mode, st.StarformationOn = capi.COOL_UVBG_GLOBAL, 1
    st.temp_to_u, st.HIReionTemp, st.MinGasTemp, st.lmfp_heat = par["temp_to_u"], 0.0, 100.0, case.lmfp_heat
    st.PhysDensThresh, st.OverDensThresh = par["PhysDensThresh"], par["OverDensThresh"]
    return st


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sfr_timing.json")
    N = 128 ** 3
    par = sc.params(avg_baryon_mass=1.0, winds_subgrid=1)
    lp, st, rnd = sc.lib_params(par), step(par), sc.rnd_table()
    P0, S0, ids, dense = particles(N, par)
    pman = sq.PartManager(N, BOXSIZE)
    pman.Base[:] = P0
    eeqos = np.flatnonzero(dense).astype(np.int32)
    res = dict(workload="shq_starformation on the eeqos list of 128^3 gas particles, the dense part drawn as tests/sfr_cases.particles", nparticles=N,
               n_eeqos=int(len(eeqos)), ncalls=5, warmup_calls=1)
    pi = P0["PI"][eeqos]
    arrays = dict(Density=S0["Density"][pi], Entropy=S0["Entropy"][pi], Ne=S0["Ne"][pi], Metallicity=S0["Metallicity"][pi], Mass=P0["Mass"][eeqos].astype(np.float64),
                  Hsml=P0["Hsml"][eeqos], DivVel=S0["DivVel"][pi], CurlVel=S0["CurlVel"][pi], dloga=np.array([st.kf.dloga_for_bin[int(b)] for b in P0["TimeBinHydro"][eeqos]]),
                  DelayTime=S0["DelayTime"][pi], timebin=P0["TimeBinHydro"][eeqos], flags=P0["Flags"][eeqos], ID=ids[eeqos])
    case = sc.case()
    t0 = time.perf_counter()
    host = sq.sfr_eval_host(case.tables(), lp, "STARFORM", arrays, case.uvbg(), sc.REDSHIFT, sc.A3INV, sc.HUBBLE, rnd, nthreads=16)
    res["host_engine_ms_16_threads"] = (time.perf_counter() - t0) * 1e3
    one = np.array([int(np.flatnonzero(~dense)[0])], dtype=np.int32)      # shq_cooling over one particle: the upload, and next to no cooling
    with sq.Context(0) as ctx:
        sq.cooling_set_tables(ctx, case.tables())
        outs = {}
        for refill in (1, 0):
            sq.sfr_set_refill(ctx, refill)
            ms, wall, wall_cur = [], [], []
            for it in range(6):
                pman.Base[:] = P0
                S = S0.copy()
                capi.check(capi.hip.shq_set_inputs_current(ctx.h, 0))
                sq.cooling(ctx, pman, S, st, active=one)        # uploads the records: the state shq_cooling leaves behind
                capi.check(capi.hip.shq_set_inputs_current(ctx.h, capi.CURRENT_PARTICLES | capi.CURRENT_SPH))
                t0 = time.perf_counter()
                outs[refill] = (sq.starformation(ctx, pman, S, lp, st, eeqos, ids, rnd), S["Entropy"].copy())
                wall_cur.append((time.perf_counter() - t0) * 1e3)
                ms.append(outs[refill][0][0].kernel_ms)
                capi.check(capi.hip.shq_set_inputs_current(ctx.h, 0))
                t0 = time.perf_counter()
                sq.cooling(ctx, pman, S, st, active=one)        # what the next device call pays after the host has changed the records
                wall.append((time.perf_counter() - t0) * 1e3)
            tag = "refill" if refill else "plain"
            res[f"kernel_ms_{tag}_median"] = float(np.median(ms[1:]))
            res[f"kernel_ms_{tag}_min"], res[f"kernel_ms_{tag}_max"] = float(min(ms[1:])), float(max(ms[1:]))
            res[f"starformation_wall_ms_{tag}_median"] = float(np.median(wall_cur[1:]))
            res["records_upload_wall_ms_median"] = float(np.median(wall[1:]))
    r = outs[1][0][0]
    res.update(steps_per_particle_mean=r.steps / max(len(eeqos), 1), n_newstars=int(r.n_newstars), n_split=int(r.n_split), n_deferred=int(r.n_deferred),
               refill_equals_plain=bool(np.array_equal(outs[1][1], outs[0][1]) and np.array_equal(outs[1][0][1][0], outs[0][0][1][0])),
               newstars_equal_host=bool(int((host.decision != 0)[host.status == 0].sum()) == r.n_newstars),
               parent_route_ms=res["host_engine_ms_16_threads"] + res["records_upload_wall_ms_median"],
               parent_route_note="the host engine over the eeqos list of the caller's records (which shq_cooling has written) plus the upload of the particle and "
                                 "SPH records that the next device call needs afterwards; shq_starformation under shq_set_inputs_current needs neither",
               host_note="shq_sfr_eval_host, the same engine on the CPU of the same box; not the reference's loop")
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
