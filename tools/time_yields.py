"""Device time of shq_metal_yields for 2^20 active stars over the case mix of tests/yields_fixtures.py (the test population, tiled), and
the restatement's host time per star beside it (scipy quad / brentq in Python: not the reference's loop, and no speed-up claim).

    python tools/time_yields.py [out.json]        (default profiles/yields_timing.json)

Kernel times are HIP-event times of the two passes (shq_metal_yields_last_ms): the median of 9 calls after 2 warm-up calls.  Bytes per
star: what the two kernels read and write of the per-star arrays (44 B in and 41 B out in the first pass; 60 B in and 88 B out per
queue star in the second); the tables are read once per workgroup.  pow() calls per star are counted on the host, from the restatement's
mass limits, by the rule of csrc/yields_math.hpp: four per family whose clamped bin is not empty, per pass, and two for SN Ia above 40 Myr, per pass."""
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
import ctypes as C                      # noqa: E402
import yields_restated as yr            # noqa: E402
import yields_fixtures as yf            # noqa: E402


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "yields_timing.json")
    T = yr.Tables()
    imf_norm = yr.compute_imf_norm(T)
    tt = yf.time_table()
    mmf = yr.maxmassfrac(T, yf.HUBBLEPARAM, yf.SN1AN0, imf_norm)
    P1, S1, _, _, ages = yf.population(T, tt, mmf, 2, ngas=0, ndm=0)
    t0 = time.perf_counter()
    ref = yr.metal_return_init(T, P1, S1.copy(), None, yf.COSMO, yf.ATIME, yf.HUBBLEPARAM, yf.SN1AN0, imf_norm, ages=ages)
    host_s = time.perf_counter() - t0
    n1, N = len(S1), 1 << 20
    reps = (N + n1 - 1) // n1
    S = np.tile(S1, reps)[:N].copy()
    pman = sq.PartManager(N, 1.0)
    Pt = np.tile(P1, reps)[:N]
    Pt["PI"] = (Pt["PI"] + n1 * (np.arange(N) // n1)).astype(np.int32)
    keep = Pt["PI"] < N
    Pt["PI"][~keep] = np.flatnonzero(~np.isin(np.arange(N), Pt["PI"][keep]))[: (~keep).sum()]
    pman.Base[:] = Pt
    # pow() count per star from the oracle's limits (the device takes the same branches: tests/test_gpu_yields.py)
    lo, hi, age = ref["LowDyingMass"], ref["HighDyingMass"], ref["StellarAges"]
    agb = np.minimum(hi, T.SNAGBSWITCH) > np.maximum(lo, T.agb_masses[0])
    snii = np.minimum(hi, T.snii_masses[-1]) > np.maximum(lo, T.SNAGBSWITCH)
    inq = np.zeros(n1, bool)
    inq[P1["PI"][ref["queue"]]] = True
    pows = (4 * agb + 4 * snii + 2 * (age >= 40)) * (1 + inq)
    with sq.Context(0) as ctx:
        sq.yields_init(ctx, T.raw, tt, yf.SN1AN0, yf.HUBBLEPARAM, imf_norm)
        ms, wall, nq = [], [], 0
        for it in range(11):
            Sc = S.copy()
            t0 = time.perf_counter()
            r = sq.metal_yields(ctx, pman, Sc, yf.ATIME)
            wall.append((time.perf_counter() - t0) * 1e3)
            m = (C.c_double * 2)()
            capi.check(capi.hip.shq_metal_yields_last_ms(ctx.h, C.byref(m)))
            ms.append((m[0], m[1]))
            nq = len(r["queue"])
        ms, wall = np.array(ms[2:]), np.array(wall[2:])
    res = dict(workload="shq_metal_yields, 2^20 active stars, the case mix of tests/yields_fixtures.py (seed 2) tiled", nstars=N, nqueue=nq,
               kernel_ms_pass1_median=float(np.median(ms[:, 0])), kernel_ms_pass2_median=float(np.median(ms[:, 1])),
               kernel_ms_total_median=float(np.median(ms.sum(axis=1))), kernel_ms_total_min=float(ms.sum(axis=1).min()),
               kernel_ms_total_max=float(ms.sum(axis=1).max()), call_wall_ms_median=float(np.median(wall)), ncalls=len(ms), warmup_calls=2,
               bytes_per_star_pass1=44 + 41, bytes_per_queue_star_pass2=4 + 7 * 8 + 11 * 8,
               bytes_total=int(N * 85 + nq * 148), pow_per_star_mean=float(pows.mean()), pow_per_star_max=int(pows.max()),
               host_restatement_us_per_star=host_s / n1 * 1e6,
               host_note="scipy quad / brentq restatement in Python (tests/yields_restated.py), not the reference's loop; not a speed-up claim")
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
