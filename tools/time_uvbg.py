"""Device time of shq_uvbg_calculate (the excursion-set reionisation, one rank) at Nmesh 64, 256 and 512 with ReionUseParticleSFR 0 and 1,
and of the shq_pm_apply route at 256 in the same process, with the algorithmic bytes of the radius loop.

  whole call    HIP events of the library around everything on the device (shq_uvbg_phase_ms [3]: uploads, f_esc, deposit, forward
                transforms, radius loop, readout, downloads); wall = host clock around the call
  radius loop   shq_uvbg_phase_ms [1]: per radius and field the filtered X / Y / Z inverse, then the cell kernel
  pm_apply      the route without this call: per radius and field one shq_pm_apply (host spectrum in, host real mesh out), the forward
                transforms by shq_fft_r2c; host clock, the deposit / cell loop / readout on the host not included
Radius-loop bytes per radius = nfields x 6 x mesh (X, Y, Z inverse: each a read and a write of an Nmesh^2 x pitch mesh of doubles)
+ nfields x 8 Nmesh^3 (the cell kernel's reads of the real meshes) + 8 Nmesh^3 (xHI read and write).  Particles: a perturbed grid of
min(Nmesh/2, 128)^3 DM and as many gas particles, star clusters, in a 100 Mpc/h box with the reference's default parameters.  One JSON line."""
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

BOX = 100000.0
COSMO = dict(Time=0.1, Omega0=0.3, OmegaBaryon=0.045, HubbleParam=0.7, RhoCrit=3 * 0.1 ** 2 / (8 * np.pi * 43007.1),
             hubble=0.1 * np.sqrt(0.3 / 0.1 ** 3 + 0.7), UnitLength_in_cm=3.085678e21, UnitMass_in_g=1.989e43, UnitTime_in_s=3.085678e16)


def params(N, use_sfr):
    up, uc = capi.UvbgParams(), capi.UvbgCosmo()
    for k, v in dict(ReionRBubbleMax=20340.0, ReionRBubbleMin=406.8, ReionDeltaRFactor=1.1, ReionFilterType=0, RtoMFilterType=0,
                     ReionGammaHaloBias=2.0, ReionNionPhotPerBary=4000.0, AlphaUV=3.0, EscapeFractionNorm=0.2,
                     EscapeFractionScaling=0.5, ReionUseParticleSFR=use_sfr, ReionSFRTimescale=0.1, UVBGdim=N, BoxSize=BOX).items():
        setattr(up, k, v)
    for k, v in COSMO.items():
        setattr(uc, k, v)
    return up, uc


def particles(N, seed=7):
    rng = np.random.default_rng(seed)
    ng = min(max(N // 2, 16), 128)
    g = (np.stack(np.meshgrid(*[np.arange(ng, dtype=np.float64)] * 3, indexing="ij"), -1).reshape(-1, 3) + 0.5) * (BOX / ng)
    pos = np.concatenate([g, g + 0.3 * BOX / ng])
    pos += rng.normal(0, 0.2 * BOX / ng, pos.shape)
    stars = rng.uniform(0, BOX, (64, 3)).repeat(32, axis=0) + rng.normal(0, BOX / N, (64 * 32, 3))
    pos = np.mod(np.concatenate([pos, stars]), BOX)
    n = len(pos)
    types = np.concatenate([np.full(len(g), 1), np.full(len(g), 0), np.full(len(stars), 4)]).astype(np.uint8)
    mtot = COSMO["Omega0"] * COSMO["RhoCrit"] * BOX ** 3
    mass = np.where(types == 4, 1e-3, mtot / (2 * len(g))).astype(np.float32)
    pm = sq.PartManager(n, BOX)
    pm.Base["Pos"] = pos
    pm.Base["Type"] = types
    pm.Base["Mass"] = mass
    fesc = 10 ** rng.uniform(-2, 2, n)
    sfr = np.where(types == 0, 10 ** rng.uniform(-4, 0, n), 0.0)
    return pm, fesc, sfr


def loop_bytes(N, nradii, nf):
    zp = capi.hip.shq_pm_slab_pitch(N) or N + 2
    mesh = N * N * zp * 8
    return nradii * (nf * 6 * mesh + nf * 8 * N ** 3 + 8 * N ** 3), zp


def time_call(ctx, N, use_sfr, rounds, warmup):
    pm, fesc0, sfr = particles(N)
    up, uc = params(N, use_sfr)
    n = pm.NumPart
    rows = []
    nr = 0
    for it in range(warmup + rounds):
        fesc, lj, zr = fesc0.copy(), np.zeros(n), np.full(n, -1.0)
        t0 = time.perf_counter()
        _, _, nr = sq.calculate_uvbg(ctx, pm, up, uc, fesc, sfr, lj, zr)
        wall = (time.perf_counter() - t0) * 1e3
        ms = (C.c_double * 4)()
        capi.check(capi.hip.shq_uvbg_phase_ms(ctx.h, C.byref(ms)))
        if it >= warmup:
            rows.append([ms[0], ms[1], ms[2], ms[3], wall])
    r = np.median(np.array(rows), axis=0)
    nf = 3 if use_sfr else 2
    nbytes, zp = loop_bytes(N, nr, nf)
    return dict(Nmesh=N, use_sfr=use_sfr, nparticles=n, nradii=nr, nfields=nf, pitch=zp, front_ms=r[0], radius_loop_ms=r[1],
                readout_ms=r[2], device_ms=r[3], wall_ms=r[4], loop_bytes=nbytes, loop_TBps=nbytes / (r[1] * 1e-3) / 1e12)


def time_pm_apply(ctx, N, nradii, nf, rounds):
    """the host round trip per radius and field: shq_pm_apply of a kept host spectrum into a host real mesh (filter as a RADIAL table)"""
    rng = np.random.default_rng(3)
    real = rng.random((N, N, N))
    spec = np.zeros(N * N * (N // 2 + 1) * 2)
    capi.check(capi.hip.shq_fft_r2c(ctx.h, N, capi.ptr(real), capi.ptr(spec)))
    table = np.exp(-np.arange(3 * (N // 2) ** 2 + 1) / 100.0) / N ** 3
    tf = capi.PMTransfer(0, 0, 2, 0, table.ctypes.data_as(C.c_void_p))
    out = np.zeros((N, N, N))
    capi.check(capi.hip.shq_pm_apply(ctx.h, N, capi.ptr(spec), C.byref(tf), capi.ptr(out)))
    ts = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        for _ in range(nradii * nf):
            capi.check(capi.hip.shq_pm_apply(ctx.h, N, capi.ptr(spec), C.byref(tf), capi.ptr(out)))
        ctx.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(Nmesh=N, nradii=nradii, nfields=nf, calls=nradii * nf, wall_ms=float(np.median(ts)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", default="64,256,512")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--apply-rounds", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    res = dict(calls=[])
    with sq.Context(0) as ctx:
        for N in [int(x) for x in args.meshes.split(",")]:
            for use_sfr in (0, 1):
                r = time_call(ctx, N, use_sfr, args.rounds, args.warmup)
                res["calls"].append(r)
                print(json.dumps(r), file=sys.stderr)
        if args.apply_rounds > 0:
            ref = [r for r in res["calls"] if r["Nmesh"] == 256 and r["use_sfr"] == 0]
            if ref:
                res["pm_apply_256"] = time_pm_apply(ctx, 256, ref[0]["nradii"], ref[0]["nfields"], args.apply_rounds)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
