"""Time of shq_thermal_speeds for the whole Ngrid^3 lattice of one species, in one process: shq_thermal_phase_ms (upload | kernel | all of
it on the device) and the host clock around the call, without and with the optional dvel and speed outputs.
warmup + rounds calls; the median and the min / max of the rounds are reported.  --host-draws PROGRAM runs the host yardstick
(tools/thermal_host_draws.cpp, built by the caller) for the same lattice and puts its line beside the call's.

Writes one JSON line per size to --out."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import shenqi_amd as sq  # noqa: E402


def timed(ctx, vel, ngrid, v_amp, table, cumprob, fdvel, rounds, warmup, **want):
    rows = []
    for it in range(warmup + rounds):
        t0 = time.perf_counter()
        out = sq.thermal_speeds(ctx, vel, ngrid, v_amp, table, cumprob, fdvel, **want)
        wall = (time.perf_counter() - t0) * 1e3
        if it >= warmup:
            rows.append(out["phase_ms"] + [wall])
    a = np.array(rows)
    names = ("upload_ms", "kernel_ms", "device_ms", "wall_ms")
    res = {k: dict(median=float(m), min=float(l), max=float(h)) for k, m, l, h in zip(names, np.median(a, axis=0), a.min(axis=0), a.max(axis=0))}
    return res, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ngrid", type=int, nargs="+", default=[256])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-draws", default="", help="the built tools/thermal_host_draws.cpp")
    ap.add_argument("--host-columns", type=int, default=0, help="columns the host yardstick runs (0: all of them)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    fdvel, cumprob, _ = sq.thermal_tables(50.0)
    lines = []
    with sq.Context(0) as ctx:
        for ngrid in args.ngrid:
            n = ngrid**3
            vel = np.random.default_rng(ngrid).standard_normal((n, 3)).astype(np.float32) * np.float32(100.0)
            table = sq.thermal_seed_table(2, ngrid)
            res = dict(ngrid=ngrid, nparticles=n, columns=ngrid * ngrid, vel_bytes=12 * n)
            res["call"], out = timed(ctx, vel, ngrid, 100.0, table, cumprob, fdvel, args.rounds, args.warmup)
            res["call"]["kernel_ns_per_particle"] = res["call"]["kernel_ms"]["median"] * 1e6 / n
            res["with_dvel_and_speed"], _ = timed(ctx, vel, ngrid, 100.0, table, cumprob, fdvel, max(2, args.rounds // 2), 0,
                                                  want_dvel=True, want_speed=True)
            speed = np.sqrt(((out["Vel"].astype(np.float64) - vel) ** 2).sum(axis=1))
            res["mean_speed_over_v_amp"] = float(speed.mean() / 100.0)
            if args.host_draws:
                cmd = [args.host_draws, str(ngrid)] + ([str(args.host_columns)] if args.host_columns else [])
                res["host"] = json.loads(subprocess.check_output(cmd).decode())
                res["host_draws_over_kernel"] = res["host"]["host_serial_draws_ms_scaled"] / res["call"]["kernel_ms"]["median"]
                res["host_draws_over_wall"] = res["host"]["host_serial_draws_ms_scaled"] / res["call"]["wall_ms"]["median"]
            line = json.dumps(res)
            print(line, flush=True)
            lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
