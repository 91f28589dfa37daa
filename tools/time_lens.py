"""Device time of shq_lens_planes (the lensing potential planes, one rank) on the resident route: 256^3 dark matter (--kind cluster,
the default, or uniform), plane resolution 1024, three normals and four cuts (the default list of Thickness = BoxSize / 4), once without
and once with the PM neutrino correction at Nmesh 768, with the binning pass' two bound estimates.

  binning      shq_lens_phase_ms [0]: the particle pass (resident: nothing staged) with the count planes' zeroing
  solves       [1]: counts -> density, the batched 2-D r2c / filter / c2r of all 12 planes
  correction   [2]: the mesh upload (host -> device), the projections (one mesh read per normal), the Nmesh solves, the bilinear add
  device       [3]: all of it, downloads of the planes and counts included; wall = host clock around the call
Estimates for the binning pass: its particle bytes (33 per particle: (x, y, z, m) and the flag byte) at the copy-probe rate, and its
u32 atomics (4 bytes per accepted (particle, plane)) at the ~1.3 TB/s chip-wide float-atomic rate (MI355X_MICROARCH.md).  One JSON line."""
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

BOX = 1000000.0
COPY_TBPS = 5.6        # profiles/r04_copy_probe.txt, copy at 768^3 x pitch 388 complex
ATOMIC_TBPS = 1.3


def time_call(ctx, pman, R, nu, rounds, warmup):
    rows = []
    out = None
    for it in range(warmup + rounds):
        t0 = time.perf_counter()
        out = sq.lens_planes(ctx, pman, R, [0, 1, 2], CutPoints=None, Thickness=BOX / 4, atime=0.5, comoving_distance=1.3e6,
                             HubbleParam=0.7, omega_source=0.3, num_particles_tot=pman.NumPart, nu=nu)
        wall = (time.perf_counter() - t0) * 1e3
        ms = (C.c_double * 4)()
        capi.check(capi.hip.shq_lens_phase_ms(ctx.h, C.byref(ms)))
        if it >= warmup:
            rows.append([ms[0], ms[1], ms[2], ms[3], wall])
    r = np.median(np.array(rows), axis=0)
    return dict(binning_ms=r[0], solves_ms=r[1], correction_ms=r[2], device_ms=r[3], wall_ms=r[4]), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ngrid", type=int, default=256)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--nmesh", type=int, default=768)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kind", default="cluster", choices=["cluster", "uniform"])
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    n = args.ngrid ** 3
    pos = sq.synth_positions(args.kind, n, L=BOX)
    pman = sq.PartManager(n, BOX)
    pman.Base["Pos"] = pos
    pman.Base["Type"] = 1
    pman.Base["Mass"] = 1.0
    del pos
    N = args.nmesh
    g = np.sin(2 * np.pi * np.arange(N) / N)
    real = np.empty((N, N, N))
    real[...] = g[:, None, None] + 0.5 * g[None, :, None] + 0.25 * g[None, None, :] ** 2
    res = dict(kind=args.kind, nparticles=n, resolution=args.res, normals=3, cuts=4, nmesh=N)
    with sq.Context(0) as ctx:
        pv = pman.view()
        capi.check(capi.hip.shq_particles_upload(ctx.h, C.byref(pv)))
        capi.check(capi.hip.shq_set_inputs_current(ctx.h, 1))
        plain, (planes, npl, _) = time_call(ctx, pman, args.res, None, args.rounds, args.warmup)
        accepted = int(npl.sum())
        nu = dict(Nmesh=N, x0=0, real=real, inv_fft_norm=1.0 / N ** 3, mean_mass_cell=1.0)
        corr, _ = time_call(ctx, pman, args.res, nu, args.rounds, args.warmup)
        capi.check(capi.hip.shq_set_inputs_current(ctx.h, 0))
    pbytes = 33 * n
    abytes = 4 * accepted
    est = pbytes / (COPY_TBPS * 1e12) * 1e3 + abytes / (ATOMIC_TBPS * 1e12) * 1e3
    res.update(plain=plain, with_correction=corr, accepted_adds=accepted, particle_bytes=pbytes, atomic_bytes=abytes,
               estimate_ms=est, binning_over_estimate=plain["binning_ms"] / est, mesh_bytes=8 * N ** 3)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
