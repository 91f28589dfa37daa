"""Device time of shq_uvbg_calculate (the excursion-set reionisation, one rank) at Nmesh 64, 256 and 512 with ReionUseParticleSFR 0 and 1,
and of the shq_pm_apply route at 256 in the same process, with the algorithmic bytes of the radius loop.

  whole call    HIP events of the library around everything on the device (shq_uvbg_phase_ms [3]: uploads, f_esc, deposit, forward
                transforms, radius loop, readout, downloads); wall = host clock around the call
  radius loop   shq_uvbg_phase_ms [1]: per radius and field the filtered X / Y / Z inverse, then the cell kernel
  pm_apply      the route without this call: per radius and field one shq_pm_apply (host spectrum in, host real mesh out), the forward
                transforms by shq_fft_r2c; host clock, the deposit / cell loop / readout on the host not included
Radius-loop bytes per radius = nfields x 6 x mesh (X, Y, Z inverse: each a read and a write of an Nmesh^2 x pitch mesh of doubles)
+ nfields x 8 Nmesh^3 (the cell kernel's reads of the real meshes) + 8 Nmesh^3 (xHI read and write).  Particles: a perturbed grid of
min(Nmesh/2, 128)^3 DM and as many gas particles, star clusters, in a 100 Mpc/h box with the reference's default parameters.  One JSON line.

--sharded: the several-rank route rehearsed on one card in one process - dist.DistUVBG with GpuUvbgOps under SHQ_COMM_FORCE=1 (one
rank that still runs every collective) at the meshes of --sharded-meshes with the full radius schedule, next to shq_uvbg_calculate on
the same inputs.  Per phase the sum of torch events around the library calls (median over the calls); `other_ms` is what the whole
call takes beyond them - routing, pack, the self all-to-alls and their copies: the price of the route, not of the kernels.  And one
filter pass (shq_uvbg_slab_xfilter, out of place) against one shq_pm_slab2_xfinish (in place, the yardstick) at the same N and nyl = N.
The result is merged into --out under "sharded"; nothing here has run on more than one GPU."""
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


class TimedOps:
    """GpuUvbgOps with torch events around every library call, summed per phase"""

    def __init__(self, ops, torch):
        self.ops, self.torch, self.spans = ops, torch, []
        self.device = ops.device

    def __getattr__(self, name):
        fn = getattr(self.ops, name)
        if name in ("pitch", "full", "to_real"):
            return fn

        def timed(*a, **k):
            if name == "fft_yz":
                key = "fft_yz_forward" if a[2] == 0 else "fft_yz_inverse"
            else:
                key = name
            e0, e1 = self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **k)
            e1.record()
            self.spans.append((key, e0, e1))
            return out
        return timed

    def take(self):
        self.torch.cuda.synchronize()
        ms = {}
        for key, e0, e1 in self.spans:
            ms[key] = ms.get(key, 0.0) + e0.elapsed_time(e1)
        self.spans = []
        return ms


def time_sharded(meshes, rounds, warmup, backend):
    """DistUVBG on one forced rank next to shq_uvbg_calculate, and the filter pass next to shq_pm_slab2_xfinish"""
    import tempfile
    import torch
    import torch.distributed as dist
    from shenqi_amd import dist as sd
    os.environ["SHQ_COMM_FORCE"] = "1"
    out = dict(backend=backend, runs=[])
    with tempfile.TemporaryDirectory() as tmp:
        dist.init_process_group(backend, init_method="file://" + os.path.join(tmp, "init"), rank=0, world_size=1)
        try:
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream), sq.Context(0, stream.cuda_stream) as ctx:     # the library on torch's stream: events see its kernels
                for N in meshes:
                    pm, fesc0, sfr = particles(N)
                    up, uc = params(N, 1)
                    n = pm.NumPart
                    pos, mass, types = np.array(pm.Base["Pos"]), np.array(pm.Base["Mass"]), np.array(pm.Base["Type"]).astype(np.uint8)
                    ops = TimedOps(sd.GpuUvbgOps(ctx), torch)
                    drv = sd.DistUVBG(sd.Comm(), N, BOX, ops)
                    rows, one = [], []
                    for it in range(warmup + rounds):
                        fesc, lj, zr = fesc0.copy(), np.zeros(n), np.full(n, -1.0)
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        _, _, nr = drv.calculate(up, uc, pos, mass, types, fesc, sfr, lj, zr)
                        torch.cuda.synchronize()
                        wall = (time.perf_counter() - t0) * 1e3
                        ms = ops.take()
                        ms["wall_ms"] = wall
                        ms["other_ms"] = wall - sum(v for k, v in ms.items() if k != "wall_ms")
                        fesc, lj, zr = fesc0.copy(), np.zeros(n), np.full(n, -1.0)
                        t0 = time.perf_counter()
                        sq.calculate_uvbg(ctx, pm, up, uc, fesc, sfr, lj, zr)
                        w1 = (time.perf_counter() - t0) * 1e3
                        pms = (C.c_double * 4)()
                        capi.check(capi.hip.shq_uvbg_phase_ms(ctx.h, C.byref(pms)))
                        if it >= warmup:
                            rows.append(ms)
                            one.append([pms[0], pms[1], pms[2], pms[3], w1])
                    med = {k: float(np.median([r[k] for r in rows])) for k in rows[0]}
                    o = np.median(np.array(one), axis=0)
                    # one filter pass against one xfinish, nyl = N
                    zpc = ops.pitch() // 2
                    g = torch.Generator(device="cuda").manual_seed(1)
                    spec = torch.view_as_complex(torch.randn((N, N, zpc, 2), dtype=torch.float64, device="cuda", generator=g))
                    dst, work = torch.empty_like(spec), spec.clone()
                    pmp = sq.PMParams(N, 0, BOX, 1.5, 43007.1)

                    def span(fn, reps=12):
                        ts = []
                        for _ in range(reps):
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record()
                            fn()
                            e1.record()
                            torch.cuda.synchronize()
                            ts.append(e0.elapsed_time(e1))
                        return float(np.median(ts[2:]))
                    base = ops.ops
                    t_filter = span(lambda: base.xfilter(spec, dst, 0, N, 0))
                    t_plain = span(lambda: base.xfilter(spec, dst, 0, N, nr - 1))
                    t_finish = span(lambda: capi.check(capi.hip.shq_pm_slab2_xfinish(ctx.h, C.byref(pmp), C.c_void_p(work.data_ptr()), 0, N, None)))
                    res = dict(Nmesh=N, nparticles=n, nradii=nr, nfields=3, sharded_phase_ms=med, nalltoall=drv.nalltoall,
                               one_call=dict(front_ms=o[0], radius_loop_ms=o[1], readout_ms=o[2], device_ms=o[3], wall_ms=o[4]),
                               filter_pass_ms=t_filter, filter_pass_unfiltered_ms=t_plain, xfinish_ms=t_finish, nyl=N,
                               filter_over_xfinish=t_filter / t_finish)
                    out["runs"].append(res)
                    print(json.dumps(res), file=sys.stderr)
        finally:
            dist.destroy_process_group()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", default="64,256,512")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--apply-rounds", type=int, default=2)
    ap.add_argument("--out", default="")
    ap.add_argument("--sharded", action="store_true", help="time DistUVBG under SHQ_COMM_FORCE=1 instead; merged into --out")
    ap.add_argument("--sharded-meshes", default="128,256")
    ap.add_argument("--backend", default="gloo", help="process-group backend of the one-rank rehearsal (gloo stages through the host)")
    args = ap.parse_args()
    if args.sharded:
        res = {}
        if args.out and os.path.exists(args.out):
            with open(args.out) as f:
                res = json.loads(f.read())
        res["sharded"] = time_sharded([int(x) for x in args.sharded_meshes.split(",")], args.rounds, args.warmup, args.backend)
        line = json.dumps(res)
        print(line)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return
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
