"""Device time of the cooling kernel for 128^3 gas particles drawn as the random set of tests/cooling_cases.py (Sherwood / Verner96,
self-shielding on, the global UVB at z = 3, log-uniform density and energy, mixed HeIII flags and time steps), through shq_cooling_eval
UNEW (DoCooling per particle), with the refill on and off; the call's wall time; and shq_cooling_eval_host at 16 threads on the same box.

    python tools/time_cooling.py [out.json]        (default profiles/cooling_timing.json)

Kernel times are HIP-event times (shq_cooling_last_kernel): the median of 5 calls after 1 warm-up call, per setting.  The host figure is
the same engine on the CPU, information about the port and no claim about the reference's loop, which cannot run here."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import shenqi_amd as sq                 # noqa: E402
import cooling_cases as cc              # noqa: E402


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "cooling_timing.json")
    N = 128 ** 3
    case, (rho, u, ne, Z, heiii, dt), mes = cc.random_case(n=N)
    tables, uv = case.tables(), case.uvbg()
    kw = dict(Z=Z, heiii=heiii, dt=dt, min_egy_spec=mes, lmfp_heat=case.lmfp_heat)
    t0 = time.perf_counter()
    host = sq.cooling_eval_host(tables, "UNEW", rho, u, ne, uv, case.redshift, nthreads=16, **kw)
    host_ms = (time.perf_counter() - t0) * 1e3
    res = dict(workload="shq_cooling_eval UNEW, 128^3 particles drawn as tests/cooling_cases.random_case", nparticles=N, ncalls=5, warmup_calls=1)
    with sq.Context(0) as ctx:
        sq.cooling_set_tables(ctx, tables)
        outs = {}
        for refill in (1, 0):
            sq.cooling_set_refill(ctx, refill)
            ms, wall = [], []
            for it in range(6):
                t0 = time.perf_counter()
                outs[refill] = sq.cooling_eval(ctx, "UNEW", rho, u, ne, uv, case.redshift, **kw)
                wall.append((time.perf_counter() - t0) * 1e3)
                ms.append(sq.cooling_last_kernel(ctx)[0])
            tag = "refill" if refill else "plain"
            res[f"kernel_ms_{tag}_median"] = float(np.median(ms[1:]))
            res[f"kernel_ms_{tag}_min"], res[f"kernel_ms_{tag}_max"] = float(min(ms[1:])), float(max(ms[1:]))
            res[f"call_wall_ms_{tag}_median"] = float(np.median(wall[1:]))
    steps = outs[1][3]
    res.update(steps_per_particle_mean=float(steps.mean()), steps_per_particle_max=int(steps.max()),
               steps_per_wave_of_64_max_mean=float(steps[:N // 64 * 64].reshape(-1, 64).max(axis=1).mean()),
               refill_equals_plain=bool(all(np.array_equal(a, b) for a, b in zip(outs[1], outs[0]))),
               u_equals_host_share=float(np.mean(outs[1][0] == host[0])), status_ok_share=float(np.mean(outs[1][2] == 0)),
               host_engine_ms_16_threads=host_ms,
               host_note="shq_cooling_eval_host, the same engine on the CPU of the same box; not the reference's loop and no speed-up claim")
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
