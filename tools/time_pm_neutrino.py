"""Device time of the PM with the massive-neutrino hook at the bench configuration (256^3 S-cluster, Nmesh 768), three routes alternated in
one process:
  plain    shq_pm_run (five fused FFT passes)
  measure  shq_pm_measure_power(1) + shq_pm_run (the existing P(k) route: forward, P(k) sweep + Green sweep, inverse)
  neutrino shq_pm_forward + shq_pm_download_power + shq_pm_set_mode_factor(T = 1) + shq_pm_run (the split X pass)
Device times come from the library's PM events (deposit start -> readout end; for the neutrino route the forward's and the finish's spans,
without the host's download and table in between); wall times are host clocks around each route with a device synchronise at the end.
The host time of the k2 tabulation is that of a vectorised numpy stand-in for the reference-side OpenMP loop (a log, a sqrt and an
interpolation per k2), not of the reference's spline.  One JSON line.  SHQ_PM_PK_SWEEP=1 selects the P(k) sweep variant of the neutrino
route (the "pk" field says which ran)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import shenqi_amd as sq  # noqa: E402
from shenqi_amd import capi  # noqa: E402

G = 43.0071


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n1", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--check", default="", help="comma-separated meshes: only compare plain and T = 1 GravPM on a 64^3 cluster, per mesh")
    args = ap.parse_args()
    if args.check:
        return check([int(x) for x in args.check.split(",")])
    n1 = args.n1
    n, L, nmesh = n1**3, 1.0, 3 * n1
    pos = sq.synth_positions("cluster", n, seed=20240601, L=L)
    pos = pos[sq.hilbert_order(pos, L)]
    pman = sq.PartManager(n, L)
    pman.Base["Pos"] = pos
    pman.Base["Type"] = 1
    pman.Base["Mass"] = 1.0
    ctx = sq.Context(0)
    h = ctx.h
    pv = pman.view()
    capi.check(capi.hip.shq_particles_upload(h, C.byref(pv)))
    pmp = sq.PMParams(nmesh, 0, L, 1.5, G)
    nk2 = 3 * (nmesh // 2) ** 2 + 1
    ones = np.ones(nk2)
    kk = np.zeros(nmesh); power = np.zeros(nmesh); nmodes = np.zeros(nmesh, dtype=np.int64); norm = C.c_double()

    def between(a, b):
        ms = C.c_double()
        capi.check(capi.hip.shq_timer_between_ms(h, a, 0, b, 0, C.byref(ms)))
        return ms.value

    def plain():
        capi.check(capi.hip.shq_pm_run(h, C.byref(pmp)))
        capi.check(capi.hip.shq_synchronize(h))
        return between(8, 13)

    def measure():
        capi.check(capi.hip.shq_pm_measure_power(h, 1))
        capi.check(capi.hip.shq_pm_run(h, C.byref(pmp)))
        capi.check(capi.hip.shq_synchronize(h))
        capi.check(capi.hip.shq_pm_measure_power(h, 0))
        return between(8, 13)

    def neutrino():
        capi.check(capi.hip.shq_pm_forward(h, C.byref(pmp)))
        capi.check(capi.hip.shq_pm_download_power(h, nmesh, capi.ptr(kk), capi.ptr(power), capi.ptr(nmodes), C.byref(norm)))
        fwd = between(8, 10)
        capi.check(capi.hip.shq_pm_set_mode_factor(h, nmesh, capi.ptr(ones)))
        capi.check(capi.hip.shq_pm_run(h, C.byref(pmp)))
        capi.check(capi.hip.shq_synchronize(h))
        return fwd + between(11, 13)

    routes = {"plain": plain, "measure": measure, "neutrino": neutrino}
    dev = {k: [] for k in routes}
    wall = {k: [] for k in routes}
    for r in range(args.warmup + args.rounds):
        for name, fn in routes.items():
            capi.check(capi.hip.shq_synchronize(h))
            t0 = time.perf_counter()
            d = fn()
            t = (time.perf_counter() - t0) * 1e3
            if r >= args.warmup:
                dev[name].append(d)
                wall[name].append(t)
    # the neutrino route with T = 1 gives the plain PM's bits
    g0 = np.zeros((n, 3)); g1 = np.zeros((n, 3))
    plain()
    capi.check(capi.hip.shq_pm_download(h, capi.ptr(g0), None))
    neutrino()
    capi.check(capi.hip.shq_pm_download(h, capi.ptr(g1), None))
    same_bits = bool(np.array_equal(g0, g1))
    gravpm_max_rel_diff = float(np.abs(g1 - g0).max() / np.abs(g0).max())
    # host: the k2 table (numpy stand-in for the OpenMP loop of INTEGRATION.md)
    xs = np.linspace(-3, 3, 64)
    ys = np.exp(-xs * xs)
    tab = []
    for _ in range(5):
        t0 = time.perf_counter()
        k2 = np.arange(1, nk2, dtype=np.float64)
        T = np.empty(nk2)
        T[0] = 1.0
        T[1:] = 1.0 + 0.01 * np.interp(np.log(np.sqrt(k2) * 2 * np.pi / 100.0), xs, ys)
        tab.append((time.perf_counter() - t0) * 1e3)
    med = {k: float(np.median(v)) for k, v in dev.items()}
    out = {
        "tool": "time_pm_neutrino", "n": n, "nmesh": nmesh, "rounds": args.rounds,
        "pk": "sweep" if os.environ.get("SHQ_PM_PK_SWEEP", "0") not in ("", "0") else "fused",
        "device_ms_median": med,
        "device_ms_min": {k: float(np.min(v)) for k, v in dev.items()},
        "wall_ms_median": {k: float(np.median(v)) for k, v in wall.items()},
        "neutrino_minus_plain_ms": med["neutrino"] - med["plain"],
        "measure_minus_neutrino_ms": med["measure"] - med["neutrino"],
        "unit_table_same_bits_as_plain": same_bits,
        "unit_table_gravpm_max_rel_diff": gravpm_max_rel_diff,
        "k2_table_host_ms_numpy": float(np.median(tab)),
    }
    print(json.dumps(out), flush=True)
    ctx.close()


def check(meshes):
    n, L = 64**3, 1.0
    pos = sq.synth_positions("cluster", n, seed=20240601, L=L)
    pos = pos[sq.hilbert_order(pos, L)]
    pman = sq.PartManager(n, L)
    pman.Base["Pos"] = pos
    pman.Base["Type"] = 1
    pman.Base["Mass"] = 1.0
    ctx = sq.Context(0)
    h = ctx.h
    pv = pman.view()
    capi.check(capi.hip.shq_particles_upload(h, C.byref(pv)))
    out = {}
    for nmesh in meshes:
        pmp = sq.PMParams(nmesh, 0, L, 1.5, G)
        g0 = np.zeros((n, 3)); g1 = np.zeros((n, 3)); g2 = np.zeros((n, 3))
        capi.check(capi.hip.shq_pm_run(h, C.byref(pmp)))
        capi.check(capi.hip.shq_pm_download(h, capi.ptr(g0), None))
        capi.check(capi.hip.shq_pm_forward(h, C.byref(pmp)))
        capi.check(capi.hip.shq_pm_run(h, C.byref(pmp)))
        capi.check(capi.hip.shq_pm_download(h, capi.ptr(g1), None))
        capi.check(capi.hip.shq_pm_run(h, C.byref(pmp)))
        capi.check(capi.hip.shq_pm_download(h, capi.ptr(g2), None))
        out[nmesh] = {"same_bits": bool(np.array_equal(g0, g1)), "max_rel_diff": float(np.abs(g1 - g0).max() / np.abs(g0).max()),
                      "plain_repeat_same_bits": bool(np.array_equal(g0, g2))}
    print(json.dumps({"tool": "time_pm_neutrino", "check": out}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
