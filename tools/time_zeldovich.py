"""Time of one displacement_fields (four fields: Density, DispX/Y/Z) for an Ngrid^3 lattice at Nmesh = 2 Ngrid, in one process:

  (a) shq_zeldovich_displacements, cold (the Gaussian field is filled) and with the field resident, with shq_zeldovich_phase_ms:
      fill | uploads, transfers, transforms and readouts | particle loop | all of it on the device; wall = host clock around the call
  (b) the composition available without it: the restatement's Gaussian fill on the host (tests/zeldovich_restated.py, numpy), four
      shq_pm_apply calls (spectrum up, mesh down, each), a numpy CIC readout and particle loop.  --skip-b leaves it out.

(a) runs warmup + rounds times per state (the cold rounds drop the field first); the medians are reported, and the fill's time per
column (Nmesh^2 columns).  (b) runs once: it takes seconds to minutes.  Writes one JSON line per mesh size to --out."""
import argparse
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

BOX = 205000.0
SEED = 181170


def delta_spec(k):
    return 40.0 * k**-1.1 / (1.0 + (k * 2000.0) ** 2)


def new_call(ctx, pos, N, delta, rounds, warmup, cold):
    rows = []
    for it in range(warmup + rounds):
        if cold:
            capi.check(capi.hip.shq_zeldovich_drop_field(ctx.h))
        t0 = time.perf_counter()
        out = sq.displacement_fields(ctx, pos, N, BOX, SEED, delta, vel_prefac=1.0)
        wall = (time.perf_counter() - t0) * 1e3
        if it >= warmup:
            rows.append(out["phase_ms"] + [wall])
    r = np.median(np.array(rows), axis=0)
    return dict(fill_ms=r[0], fields_ms=r[1], finalize_ms=r[2], device_ms=r[3], wall_ms=r[4]), out


def composition(ctx, pos, N, delta):
    import ctypes as C
    import zeldovich_restated as zr
    t = {}
    t0 = time.perf_counter()
    table = zr.seed_table(N, SEED)
    dense = np.zeros((N, N, N // 2 + 1), dtype=np.complex128)
    for cols in np.array_split(np.arange(N * N), max(1, N * N // 32768)):   # bounded memory: 2 x 32768 states at a time
        i, j = cols // N, cols % N
        dense[i, j] = zr.fill_gaussian(N, SEED, columns=cols, table=table)[i, j]
    spec = zr.reference_layout(dense)
    t["host_fill_ms"] = (time.perf_counter() - t0) * 1e3
    n = len(delta)
    dens, disp = np.zeros(n), np.zeros(n)
    capi.check(capi.hip.shq_zeldovich_factor_tables(N, BOX, capi.ptr(delta), None, capi.ptr(dens), capi.ptr(disp), None))
    t0 = time.perf_counter()
    meshes = []
    for kind, axis, tab in ((0, 0, dens), (1, 0, disp), (1, 1, disp), (1, 2, disp)):
        tf = capi.PMTransfer(kind, axis, 0, 0, tab.ctypes.data)
        mesh = np.zeros((N, N, N))
        capi.check(capi.hip.shq_pm_apply(ctx.h, N, capi.ptr(spec), C.byref(tf), capi.ptr(mesh)))
        meshes.append(mesh)
    t["pm_apply_x4_ms"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    density = zr.cic_readout(meshes[0], pos, N, BOX)
    d = np.stack([zr.cic_readout(meshes[1 + k], pos, N, BOX) for k in range(3)], axis=1)
    newpos = zr.periodic_wrap(pos + d, BOX)
    maxdisp, maxvel = max(0.0, d.max()), (d * d).sum(axis=1).max()
    t["host_readout_finalize_ms"] = (time.perf_counter() - t0) * 1e3
    t["total_ms"] = t["host_fill_ms"] + t["pm_apply_x4_ms"] + t["host_readout_finalize_ms"]
    return t, dict(Pos=newpos, Disp=d, Density=density, maxdisp=maxdisp, maxvel=maxvel)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ngrid", type=int, nargs="+", default=[256])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-b", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = []
    with sq.Context(0) as ctx:
        for ngrid in args.ngrid:
            N = 2 * ngrid
            pos, _ = sq.setup_grid(sq.IDGenerator(ngrid, BOX), 0.0, 1.0)
            delta = sq.tabulate_by_k2(delta_spec, N, BOX)
            cold, _ = new_call(ctx, pos, N, delta, args.rounds, args.warmup, True)
            warm, got = new_call(ctx, pos, N, delta, args.rounds, args.warmup, False)
            res = dict(ngrid=ngrid, nmesh=N, nparticles=len(pos), fields=4, cold=cold, resident=warm,
                       fill_ns_per_column=cold["fill_ms"] * 1e6 / (N * N), c2r_and_readout_ms_per_field=warm["fields_ms"] / 4)
            if not args.skip_b:
                comp, ref = composition(ctx, pos, N, delta)
                res["composition"] = comp
                res["speedup_cold_wall"] = comp["total_ms"] / cold["wall_ms"]
                res["speedup_resident_wall"] = comp["total_ms"] / warm["wall_ms"]
                res["max_rel_diff_disp"] = float(np.abs(got["Disp"] - ref["Disp"]).max() / np.abs(ref["Disp"]).max())
            line = json.dumps(res)
            print(line, flush=True)
            lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
