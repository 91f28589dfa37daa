"""Device time of the run-log loops (shenqi_amd/csrc/stats.hip) on one rank: --ndm^3 dark matter + --ngas^3 gas (256^3 + 128^3 by
default), the gas with 176-byte SPH slots, uniformly random positions, gas of cgs-like magnitudes so that the rate network is solved.

  energy      shq_energy_statistics without and with the temperature solves: the call's own HIP-event time (kernel_ms: the record
              pass and the fixed-order sums; with temperatures also the gas selection and the solve kernel) and the whole synchronous
              call on the stream (tools/domain_timing.py's `timed`, medians of --rounds after one warm-up)
  bh          shq_bh_totals over --nbh slots and shq_bh_details of all of them

Two yardsticks, as for shq_startup_particles (tools/time_startup.py):

  copy_ms       the time of copying the same records once on the same box (read and write, at the rate of a plain contiguous device
                copy, domain_timing.copy_rate); over_copy = kernel time / copy_ms.  over_read divides by half of it, the time of
                reading the records once: tools/time_startup.py's over_copy for a loop that only reads
  route_before  what a caller had before this call: a device-to-host copy of the records and the gas slots (wall clock, pageable
                memory) plus the same sums in numpy, and for the temperatures shq_cooling_eval_host over 16 threads

Writes one JSON object to --out (profiles/stats_timing.json)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import shenqi_amd as sq  # noqa: E402
from shenqi_amd import capi  # noqa: E402
from domain_timing import timed, copy_rate  # noqa: E402
import cooling_restated as cr  # noqa: E402
import stats_restated as sr  # noqa: E402

DEV = "cuda:0"
BOX = 20000.0
GM1 = 5.0 / 3 - 1


def dev(a):
    return torch.from_numpy(a.view(np.uint8).reshape(-1)).to(DEV)


def wall(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def numpy_sums(P, S, Time):
    """the loop of stats.cpp:235-272 without get_temp, vectorised"""
    a1, a2, a3 = Time, Time * Time, Time * Time * Time
    m = P["Mass"].astype(np.float64)
    pos, vel = P["Pos"], P["Vel"]
    out = {}
    for t in (0, 1):
        k = P["Type"] == t
        mk = m[k]
        out[t] = [mk.sum(), (0.5 * mk * P["Potential"][k] / a1).sum(), (0.5 * mk * (vel[k] * vel[k]).sum(axis=1) / a2).sum(), (mk[:, None] * vel[k]).sum(axis=0),
                  (mk[:, None] * pos[k]).sum(axis=0), (mk[:, None] * np.cross(pos[k], vel[k])).sum(axis=0)]
    gas = np.flatnonzero(P["Type"] == 0)
    slot = S[P["PI"][gas]]
    egyspec = slot["Entropy"] / GM1 * np.power(slot["Density"] / a3, GM1)
    out["eint"] = (m[gas] * egyspec).sum()
    return out, slot["Density"], egyspec, slot["Ne"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ngas", type=int, default=128)
    ap.add_argument("--ndm", type=int, default=256)
    ap.add_argument("--nbh", type=int, default=100000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stats_timing.json"))
    args = ap.parse_args()
    rng = np.random.default_rng(20261020)
    ng, nd = args.ngas ** 3, args.ndm ** 3
    n = ng + nd
    res = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, ngas=ng, ndm=nd)
    rate = copy_rate(1 << 29)
    res["copy_TBps"] = rate / 1e12
    P = np.zeros(n, dtype=capi.PARTICLE_DTYPE)
    gas = np.sort(rng.permutation(n)[:ng])
    P["Type"] = 1
    P["Type"][gas] = 0
    P["PI"][gas] = rng.permutation(ng).astype(np.int32)
    P["Pos"] = rng.random((n, 3)) * BOX
    P["Vel"] = rng.normal(size=(n, 3)) * 100.0
    P["Potential"] = -1e5 * rng.random(n)
    P["Mass"] = 1.0
    P["Mass"][gas] = 0.2
    S = np.zeros(ng, dtype=capi.SPH_DTYPE)
    S["Density"] = 10.0 ** rng.uniform(-6, 2, ng)
    mu = 4.0 / (1 + 3 * 0.76)
    u = 10.0 ** rng.uniform(2, 8, ng) * cr.BOLTZMANN / (GM1 * cr.PROTONMASS * mu)
    S["Entropy"] = u * GM1 / np.power(S["Density"] / sr.TIME ** 3, GM1)
    S["Ne"] = rng.uniform(0, 1.2, ng)
    L = sq.stats_layout()
    record_bytes = n * 160
    with sq.Context(0) as ctx:
        sq.cooling_set_tables(ctx, sr.device_tables())
        d_parts, d_sph = dev(P), dev(S)
        e = res["energy"] = dict(record_bytes=record_bytes, slot_bytes=ng * 176, copy_ms=2 * record_bytes / rate * 1e3)
        for name, want in (("without_temperatures", False), ("with_temperatures", True)):
            par = sr.stats_params(capi.COOL_UVBG_GLOBAL, want)
            kernel = []

            def call():
                sums, _ = sq.energy_statistics(ctx, L, d_parts, n, d_sph, ng, par, ng)
                kernel.append(sums.kernel_ms)
                return sums

            t = timed(ctx, call, args.rounds)
            sums = call()
            km = float(np.median(kernel[1:]))
            e[name] = dict(call_ms=t, kernel_ms=km, over_copy=km / e["copy_ms"], over_read=2 * km / e["copy_ms"],
                           n_status=list(sums.n_status), TemperatureComp0=sums.TemperatureComp[0], EnergyIntComp0=sums.EnergyIntComp[0])
            again = call()
            e[name]["same_bytes_twice"] = bytes(again)[:capi.StatsSums.kernel_ms.offset] == bytes(sums)[:capi.StatsSums.kernel_ms.offset]
        # the same particles ordered by type, so that a wave holds one type (one butterfly per wave) and the gas slots are read by
        # neighbouring lanes; the slots stay in their shuffled order
        d_sorted = dev(P[np.argsort(P["Type"], kind="stable")])
        bt = e["ordered_by_type"] = {}
        for name, want in (("without_temperatures", False), ("with_temperatures", True)):
            par = sr.stats_params(capi.COOL_UVBG_GLOBAL, want)
            kernel = [sq.energy_statistics(ctx, L, d_sorted, n, d_sph, ng, par, ng)[0].kernel_ms for _ in range(args.rounds + 1)]
            km = float(np.median(kernel[1:]))
            bt[name] = dict(kernel_ms=km, over_copy=km / e["copy_ms"])
        del d_sorted
        # ---- the route before: records and slots to the host, the loop in numpy, get_temp on the host engine ----
        rb = res["route_before"] = {}
        rb["records_d2h_ms"] = wall(lambda: (d_parts.cpu(), d_sph.cpu()))[0]
        t, (hs, dens, egy, ne) = wall(lambda: numpy_sums(P, S, sr.TIME))
        rb["numpy_sums_ms"] = t
        rb["eint_rel_diff"] = abs(hs["eint"] / e["with_temperatures"]["EnergyIntComp0"] - 1)
        c = sr.cooling()
        rb["host_get_temp_16_threads_ms"] = wall(lambda: sq.cooling_eval_host(sr.unit_tables(), "TEMP", dens, egy, ne, c.uvbg(), 1.0 / sr.TIME - 1, nthreads=16))[0]
        rb["without_temperatures_ms"] = rb["records_d2h_ms"] + rb["numpy_sums_ms"]
        rb["with_temperatures_ms"] = rb["without_temperatures_ms"] + rb["host_get_temp_16_threads_ms"]
        rb["over_call_without_temperatures"] = rb["without_temperatures_ms"] / e["without_temperatures"]["call_ms"]
        rb["over_call_with_temperatures"] = rb["with_temperatures_ms"] / e["with_temperatures"]["call_ms"]
        del d_parts, d_sph
        # ---- black holes ----
        nbh = args.nbh
        B = np.zeros(nbh, dtype=capi.BH_DTYPE)
        B["Mass"], B["Mdot"] = 10.0 ** rng.uniform(-5, -1, nbh), 10.0 ** rng.uniform(-9, -3, nbh)
        B["SwallowID"] = np.where(np.arange(nbh) % 3 == 1, np.uint64(7), sr.NOT_SWALLOWED)
        PB = np.zeros(nbh, dtype=capi.PARTICLE_DTYPE)
        PB["Type"], PB["PI"] = 5, rng.permutation(nbh).astype(np.int32)
        d_bh, d_pb = dev(B), dev(PB)
        b = res["bh"] = dict(nbh=nbh)
        b["totals_call_ms"] = timed(ctx, lambda: sq.bh_totals(ctx, d_bh, nbh), args.rounds)
        out = torch.zeros(nbh * capi.BHINFO_SIZE, dtype=torch.uint8, device=DEV)
        Lb, X = sq.bh_detail_layout(), sq.bh_detail_arrays()

        def details():
            capi.check(capi.hip.shq_bh_details(ctx.h, C.byref(Lb), d_pb.data_ptr(), nbh, d_bh.data_ptr(), nbh, C.byref(X), None, nbh, 0.5, out.data_ptr()))

        b["details_call_ms"] = timed(ctx, details, args.rounds)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
