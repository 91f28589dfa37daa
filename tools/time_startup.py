"""Device time of the run start-up (shenqi_amd/csrc/startup.hip) on one rank: --ndm^3 dark matter + --ngas^3 gas (256^3 + 128^3 by
default), the gas with 176-byte SPH slots, uniformly random positions.

  records     shq_startup_particles: the fused pass (all four loops) and each loop alone, in restart mode and, for the INIT loop, in
              initial-conditions mode (which also writes the block of init.cpp:163-177 into every gas slot)
  hsml        shq_set_init_hsml on the device-built GASMASK + BHMASK tree
  entropy     shq_init_entropy from EgyWtDensity
  setup       the whole shq_setup_smoothinglengths (wall clock: it includes the one upload and the write-back), its rounds

Event times on the context's stream, medians of --rounds after one warm-up (tools/domain_timing.py's `timed`).  Two yardsticks:

  *_over_copy   pass time / (the bytes the pass must touch / the rate of a plain contiguous device copy, domain_timing.copy_rate - the
                same stream tools/copy_probe.hip measures): the records once for a loop that only reads, twice when it writes them back
  route_before  what a caller had before these calls: a device-to-host copy of the records (wall clock, pageable memory), the host
                mirror's tree build + set_init_hsml, one one-shot density call with update_hsml, and one entropy round as numpy +
                a one-shot density call.

Writes one JSON object to --out (profiles/startup_timing.json)."""
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

DEV = "cuda:0"
BOX = 20000.0
U_INIT, ATIME = 37.5, 0.25


def dev(a):
    return torch.from_numpy(a.view(np.uint8).reshape(-1)).to(DEV)


def wall(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ngas", type=int, default=128)
    ap.add_argument("--ndm", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "startup_timing.json"))
    args = ap.parse_args()
    rng = np.random.default_rng(20261019)
    ng, nd = args.ngas ** 3, args.ndm ** 3
    n = ng + nd
    res = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, ngas=ng, ndm=nd)
    rate = copy_rate(1 << 29)
    res["copy_TBps"] = rate / 1e12
    pman = sq.PartManager(n, BOX)
    P = pman.Base
    gas = np.sort(rng.permutation(n)[:ng])
    P["Type"] = 1
    P["Type"][gas] = 0
    P["PI"][gas] = np.arange(ng)
    P["Pos"] = rng.random((n, 3)) * BOX
    P["Mass"] = 1.0
    P["Mass"][gas] = 0.2
    P["Mass"][::5] = 0          # recovered from the mass table
    P["Hsml"] = BOX / args.ngas
    P["ID"] = np.arange(n, dtype=np.uint64)
    SphP = np.zeros(ng, dtype=capi.SPH_DTYPE)
    BhP = np.zeros(1, dtype=capi.BH_DTYPE)
    mt = [0.2, 1.0, 0, 0, 0, 0]
    ms = sq.mean_separation(BOX, [ng, nd, 0, 0, 0, 0])
    L = sq.startup_layout()
    with sq.Context(0) as ctx:
        d_parts, d_sph, d_bh = dev(P), dev(SphP), dev(BhP)
        r = res["records"] = dict(record_bytes=n * 160, slot_bytes=ng * 176)
        for name, which, mode, nbytes in (("fused_restart", 15, 3, 2 * n * 160), ("omega", 1, 3, n * 160), ("positions", 2, 3, n * 160), ("hsml", 4, 3, n * 160),
                                          ("init_restart", 8, 3, 2 * n * 160 + ng * 176), ("init_ic", 8, -1, 2 * n * 160 + ng * 176),
                                          ("fused_ic", 15, -1, 2 * n * 160 + ng * 176)):
            par = sq.startup_params(BOX, mt, ms, 7, 4, mode)
            rep = C.pointer(capi.StartupReport())

            def call():
                capi.check(capi.hip.shq_startup_particles(ctx.h, C.byref(L), d_parts.data_ptr(), n, d_sph.data_ptr(), ng, d_bh.data_ptr(), 1, C.byref(par), which, rep))

            t = timed(ctx, call, args.rounds)
            r[name] = dict(ms=t, bytes=nbytes, over_copy=t * 1e-3 / (nbytes / rate))
        r["badmass_first_call_only"] = True     # the first OMEGA call recovers the zero masses; later rounds find none and leave the tile clean
        # ---- the route before: records to the host ----
        rb = res["route_before"] = {}
        rb["records_d2h_ms"] = wall(lambda: (d_parts.cpu(), d_sph.cpu()))[0]
        del d_parts, d_sph
        # ---- the first smoothing length ----
        P["Mass"][P["Mass"] == 0] = 1.0
        sq.set_densitypar(DensityResolutionEta=1.0, MaxNumNgbDeviation=0.5, DensityKernelType=1, BlackHoleNgbFactor=2.0, MinGasHsml=0.006)
        des = sq.GetNumNgb()
        pv = pman.view()
        capi.check(capi.hip.shq_particles_upload(ctx.h, C.byref(pv)))
        sq.dynamics_upload(ctx, pman)
        tb = sq.tree_build_device(ctx, BOX, sq.GASMASK + sq.BHMASK)
        h = res["hsml"] = dict(tree_build_ms=tb.build_ms, numnodes=tb.numnodes)
        nodes = torch.empty(n, dtype=torch.int32, device=DEV)
        h["set_init_hsml_ms"] = timed(ctx, lambda: capi.check(capi.hip.shq_set_init_hsml(ctx.h, float(ms[0]), des, nodes.data_ptr())), args.rounds)
        h["set_init_hsml_without_nodes_ms"] = timed(ctx, lambda: capi.check(capi.hip.shq_set_init_hsml(ctx.h, float(ms[0]), des, None)), args.rounds)
        h["bytes"] = n * (1 + 4) + ng * (32 + 4 + 8)     # flags and father of every particle; posm, Hsml and a node of the gas
        h["over_copy"] = h["set_init_hsml_without_nodes_ms"] * 1e-3 / (h["bytes"] / rate)
        t, tree = wall(lambda: sq.force_tree_rebuild_mask(pman, sq.GASMASK + sq.BHMASK))
        rb["host_tree_build_ms"] = t
        rb["host_set_init_hsml_ms"] = wall(lambda: sq.set_init_hsml(tree, float(ms[0]), pman))[0]
        # ---- entropy and the whole call ----
        dp = sq.make_density_params(BOX, BlackHoleOn=0, MinGasHsml=0.006)
        SphP["Density"] = SphP["EgyWtDensity"] = SphP["Entropy"] = -1
        hs0 = P["Hsml"].copy()
        t, stats = wall(lambda: sq.setup_smoothinglengths(ctx, -1, pman, SphP, None, dp, float(ms[0]), U_INIT, ATIME, 1))
        s = res["setup"] = dict(wall_ms=t, rounds=stats.nrounds, maxdiff=[float(x) for x in stats.maxdiff], first_pass_kernel_ms=stats.first.kernel_ms,
                                first_pass_iterations=stats.first.niterations)
        t, _ = wall(lambda: sq.setup_smoothinglengths(ctx, -1, pman, SphP, None, dp, float(ms[0]), U_INIT, ATIME, 0))
        s["wall_without_disph_ms"] = t
        s["per_round_ms"] = (s["wall_ms"] - t) / max(stats.nrounds, 1)
        sv = capi.sph_view(SphP)
        capi.check(capi.hip.shq_particles_upload(ctx.h, C.byref(pv)))
        capi.check(capi.hip.shq_sph_state_upload(ctx.h, C.byref(pv), C.byref(sv)))
        e = res["entropy"] = dict(bytes=n * 1 + ng * 24)
        e["init_entropy_ms"] = timed(ctx, lambda: sq.init_entropy(ctx, U_INIT, ATIME ** 3, True), args.rounds)
        e["over_copy"] = e["init_entropy_ms"] * 1e-3 / (e["bytes"] / rate)
        # ---- the route before: one-shot density calls with numpy between ----
        P["Hsml"] = hs0
        rb["one_shot_density_update_hsml_ms"] = wall(lambda: sq.density(ctx, None, 1, 0, 0, None, tree, pman, SphP, None))[0]

        def one_round():
            SphP["Entropy"] = (5.0 / 3 - 1) * U_INIT / np.power(SphP["EgyWtDensity"] / ATIME ** 3, 5.0 / 3 - 1)
            old = SphP["EgyWtDensity"].copy()
            sq.density(ctx, None, 0, 1, 0, None, tree, pman, SphP, None)
            return np.max(np.abs(SphP["EgyWtDensity"] - old) / SphP["EgyWtDensity"])

        rb["one_entropy_round_ms"] = wall(one_round)[0]
        rb["setup_estimate_ms"] = rb["records_d2h_ms"] + rb["host_tree_build_ms"] + rb["host_set_init_hsml_ms"] + rb["one_shot_density_update_hsml_ms"] + \
            stats.nrounds * rb["one_entropy_round_ms"]
        s["route_before_over_setup"] = rb["setup_estimate_ms"] / s["wall_ms"]
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
