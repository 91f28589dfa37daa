"""Time of glass_evolve (nsteps steps, nsteps + 1 PM forces) for setup_glass's Ngrid^3 input at Nmesh = 2 Ngrid, in one process:

  (a) shq_glass_evolve with shq_glass_phase_ms: upload | all forces | all particle loops | all of it on the device; wall = the host
      clock around the call (it includes the host's validation scan and the staging of the Python wrapper).  warmup + rounds calls,
      the median and the min / max of the rounds are reported, and the per-force and per-particle-kernel quotients.
  (b) the yardstick: the same force composed from the calls that existed before - numpy deposit, shq_fft_r2c, a host spectrum pass,
      three shq_pm_apply with SHQ_TF_DIFF, numpy gather and kicks (the restatement with its transforms swapped for the library's).
      --b-forces forces are timed (default 2: a force takes seconds) and the 14-step figure is that mean times nsteps + 1 plus the
      particle loops; the JSON says how many were timed.  --skip-b leaves it out.
  (c) the sanity bound from inside the project: shq_pm_phase_ms of one gravity PM run (one forward, one inverse, one four-field
      readout) at the same Nmesh and particle count.

Writes one JSON line per size to --out."""
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

BOX = 1.0


def new_call(ctx, pos, N, nsteps, rounds, warmup, spectra):
    rows = []
    for it in range(warmup + rounds):
        t0 = time.perf_counter()
        out = sq.glass_evolve(ctx, N, BOX, pos, None, 1.0, nsteps=nsteps, spectra=spectra)
        wall = (time.perf_counter() - t0) * 1e3
        if it >= warmup:
            rows.append(out["phase_ms"] + [wall])
    a = np.array(rows)
    names = ("upload_ms", "forces_ms", "particle_loops_ms", "device_ms", "wall_ms")
    med, lo, hi = np.median(a, axis=0), a.min(axis=0), a.max(axis=0)
    res = {k: dict(median=float(m), min=float(l), max=float(h)) for k, m, l, h in zip(names, med, lo, hi)}
    res["ms_per_force"] = float(med[1]) / (nsteps + 1)
    res["ms_per_particle_kernel"] = float(med[2]) / max(nsteps + 1, 1) if nsteps > 0 else 0.0
    return res, out


def composed_force(ctx, pos, mass, N):
    """one glass force from shq_fft_r2c + host spectrum pass + 3 shq_pm_apply; returns (Disp float32, seconds by part)"""
    import glass_restated as gr
    t = {}
    t0 = time.perf_counter()
    cell, res = gr.cic_cells(pos, N, BOX)
    mesh = np.zeros(N**3)
    for idx, w in gr.connections(cell, res, N):
        mesh += np.bincount((idx[0] * N + idx[1]) * N + idx[2], weights=w * mass, minlength=N**3)
    mesh = mesh.reshape(N, N, N)
    t["deposit_ms"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    spec = np.zeros((N, N // 2 + 1, N), dtype=np.complex128)           # the reference's Fourier layout [y][z'][x]
    capi.check(capi.hip.shq_fft_r2c(ctx.h, N, capi.ptr(mesh), capi.ptr(spec)))
    t["r2c_ms"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    k1 = np.where(np.arange(N) <= N // 2, np.arange(N), np.arange(N) - N).astype(np.int64)
    k2 = (k1[:, None, None] ** 2 + k1[None, : N // 2 + 1, None] ** 2 + k1[None, None, :] ** 2)
    s = gr.sinc_table(N)
    f = s[:, None, None] * s[None, : N // 2 + 1, None] * s[None, None, :]
    m = spec.real**2 + spec.imag**2
    nzm = k2 > 0
    binsperunit = (N - 1) / np.log(np.sqrt(3) * N / 2.0)
    kint = np.floor(binsperunit * np.log(np.where(nzm, k2, 1)) / 2.0).astype(np.int64)
    w = np.where((k1[None, : N // 2 + 1, None] == 0) | (k1[None, : N // 2 + 1, None] == N // 2), 1.0, 2.0) * np.ones_like(m)
    use = nzm & (kint < N)
    np.bincount(kint[use], weights=(w * m * (f * f + 1))[use], minlength=N)
    table = np.zeros(3 * (N // 2) ** 2 + 1)
    table[1:] = gr.pot_factor(BOX, float(mass.sum())) * (1.0 / np.arange(1, len(table))) * (-1.0 * (N / BOX))
    t["host_spectrum_pass_ms"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    meshes = []
    for axis in range(3):
        tf = capi.PMTransfer(2, axis, 1, 0, table.ctypes.data)          # SHQ_TF_DIFF, zero mode set to 0
        out = np.zeros((N, N, N))
        capi.check(capi.hip.shq_pm_apply(ctx.h, N, capi.ptr(spec), C.byref(tf), capi.ptr(out)))
        meshes.append(out)
    t["pm_apply_x3_ms"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    disp = np.stack([gr.gather_f32(meshes[k], pos, N, BOX) for k in range(3)], axis=1)
    t["gather_ms"] = (time.perf_counter() - t0) * 1e3
    return disp, t


def composition(ctx, pos, N, nsteps, nforces):
    import glass_restated as gr
    mass = np.ones(len(pos))
    vel = np.zeros((len(pos), 3), dtype=np.float32)
    parts, disp0 = [], None
    for i in range(nforces):
        disp, t = composed_force(ctx, pos, mass, N)
        disp0 = disp if disp0 is None else disp0
        parts.append(t)
        t0 = time.perf_counter()
        vel = gr.kick(vel, disp)
        pos = gr.drift(pos, vel)
        vel = gr.kick(vel, disp)
        gr.glass_stats(disp, vel)
        loop_ms = (time.perf_counter() - t0) * 1e3
    mean = {k: float(np.mean([p[k] for p in parts])) for k in parts[0]}
    force_ms = sum(mean.values())
    return dict(forces_timed=nforces, per_force=mean, ms_per_force=force_ms, particle_loops_ms_per_step=loop_ms,
                total_ms_extrapolated=force_ms * (nsteps + 1) + loop_ms * nsteps), disp0


def gravity_pm(ctx, pos, N):
    import common as cm
    wrapped = np.mod(pos, BOX)
    pman = cm.make_partmanager(np.ascontiguousarray(wrapped), box=BOX)
    pv = pman.view()
    capi.check(capi.hip.shq_particles_upload(ctx.h, C.byref(pv)))
    pmp = sq.PMParams(N, 0, BOX, 1.5, cm.G)
    ms = (C.c_double * 6)()
    rows = []
    for _ in range(4):
        capi.check(capi.hip.shq_pm_run(ctx.h, C.byref(pmp)))
        capi.check(capi.hip.shq_pm_phase_ms(ctx.h, C.byref(ms)))
        rows.append(list(ms))
    r = np.median(np.array(rows[1:]), axis=0)
    return dict(deposit_ms=r[0], r2c_ms=r[1], transfer_ms=r[2], c2r_ms=r[3], readout_ms=r[4], total_ms=r[5])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ngrid", type=int, nargs="+", default=[128])
    ap.add_argument("--nsteps", type=int, default=14)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--b-forces", type=int, default=2)
    ap.add_argument("--skip-b", action="store_true")
    ap.add_argument("--skip-c", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = []
    with sq.Context(0) as ctx:
        for ngrid in args.ngrid:
            N = 2 * ngrid
            pos = sq.glass_setup_positions(ngrid, BOX, 0.0, 1234)
            zp = 2 * ((N // 2 + 1 + 3) // 4 * 4)
            res = dict(ngrid=ngrid, nmesh=N, nparticles=len(pos), nsteps=args.nsteps,
                       mesh_bytes_x2=2 * N * N * zp * 8, particle_bytes=len(pos) * 52)
            res["call"], got = new_call(ctx, pos, N, args.nsteps, args.rounds, args.warmup, False)
            res["call_with_spectra"], _ = new_call(ctx, pos, N, args.nsteps, max(2, args.rounds // 2), 0, True)
            res["force_std"] = [s["force_std"] for s in got["steps"]]
            if not args.skip_c:
                res["gravity_pm"] = gravity_pm(ctx, pos, N)
                res["force_over_gravity_pm"] = res["call"]["ms_per_force"] / res["gravity_pm"]["total_ms"]
            if not args.skip_b:
                res["composition"], disp0 = composition(ctx, pos, N, args.nsteps, args.b_forces)
                one = sq.glass_evolve(ctx, N, BOX, pos, None, 1.0, nsteps=0)
                res["composition"]["max_rel_diff_disp"] = float(np.abs(one["Disp"].astype(np.float64) - disp0).max() / np.abs(disp0).max())
                res["speedup_wall"] = res["composition"]["total_ms_extrapolated"] / res["call"]["wall_ms"]["median"]
            line = json.dumps(res)
            print(line, flush=True)
            lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
