"""Device time of glass making across ranks in phases (shq_glass_slab_* driven by dist.py:DistGlass) beside the one-rank call
(shq_glass_evolve) on the same box, at Nmesh 256 and 512 (--sizes), Ngrid = Nmesh / 2, --nsteps steps.

  one rank                     shq_glass_evolve: shq_glass_phase_ms (HIP events) and a host clock.
  one rank, SHQ_COMM_FORCE=1   one gloo rank in a fresh child process that still runs every collective: per phase (planes, deposit,
                               fft_yz, xforward, xtransfer, gather, particles) the time of the phase's calls summed over the call, each
                               taken with a host clock around the call and a synchronise of the context's stream, and per force; the
                               re-homing (planes, selection, the all-to-all) and the rows it moved; the call's wall time, which also
                               holds the host-staged gloo exchanges.  Then the pass comparison, reported, not gated: K launches back
                               to back between two synchronises, the passes alternating, the median over the rounds -
                                 MODE 7 (shq_glass_slab_xforward) with and without the sums against MODE 3 (shq_uvbg_slab_xforward),
                                 MODE 8 (shq_glass_slab_xtransfer, the three axes) against MODE 6 (shq_zeldovich_slab_xtransfer).
  two ranks, one GPU           two gloo ranks in fresh child processes with a context each on device 0, the particles dealt round-robin.
                               The two processes share the device, so these are not scaling numbers.

Medians over --rounds after one warm-up.  Writes profiles/dist_glass_timing.json (or --out) and prints it as one JSON line.
Nothing here runs on more than one GPU."""
import argparse
import ctypes as C
import json
import os
import pickle
import sys
import tempfile
import time

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import shenqi_amd as sq  # noqa: E402
from shenqi_amd import capi  # noqa: E402
from shenqi_amd import dist as sd  # noqa: E402

BOX = 1.0
SEED = 21
PHASES = ("planes", "deposit", "fft_yz", "xforward", "xtransfer", "gather", "particles")


class TimedOps(sd.GpuGlassOps):
    """GpuGlassOps with a host clock around every phase call, each ended by a synchronise of the context's stream"""

    def __init__(self, ctx):
        super().__init__(ctx)
        self.ms = dict.fromkeys(PHASES, 0.0)

    def _timed(self, name, fn, *args):
        torch.cuda.synchronize()
        self.ctx.synchronize()
        t0 = time.perf_counter()
        r = fn(*args)
        self.ctx.synchronize()
        self.ms[name] += (time.perf_counter() - t0) * 1e3
        return r


for _name in PHASES:
    def _wrap(name):
        def method(self, *args):
            return self._timed(name, getattr(sd.GpuGlassOps, name).__get__(self), *args)
        return method
    setattr(TimedOps, _name, _wrap(_name))


class TimedGlass(sd.DistGlass):
    rehome_ms = 0.0

    def _rehome(self, S):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        super()._rehome(S)
        torch.cuda.synchronize()
        self.rehome_ms += (time.perf_counter() - t0) * 1e3


def med(rows):
    return [float(x) for x in np.median(np.array(rows, dtype=np.float64), axis=0)]


def phased(ctx, comm, N, pos, nsteps, rounds):
    rows = []
    for r in range(1 + rounds):
        ops = TimedOps(ctx)
        drv = TimedGlass(comm, N, BOX, ops)
        comm.barrier()
        t0 = time.perf_counter()
        got = drv.evolve(pos, None, 1.0, nsteps, spectra=True)
        wall = (time.perf_counter() - t0) * 1e3
        if r > 0:
            rows.append([ops.ms[k] for k in PHASES] + [drv.rehome_ms, wall])
    m = dict(zip(PHASES + ("rehome", "wall"), med(rows)))
    nf = nsteps + 1
    per_force = dict(deposit=m["deposit"] / nf, fft_yz=m["fft_yz"] / nf, xforward=m["xforward"] / nf, xtransfer_3_axes=m["xtransfer"] / nf,
                     gather_3_axes=m["gather"] / nf)
    return dict(ms=m, per_force_ms=per_force, particles=int(len(pos)), nsteps=nsteps, rows_sent=int(drv.rows_sent), rehomed=[int(x) for x in drv.rehomed],
                rehome_ms_per_step=m["rehome"] / max(nsteps, 1), nalltoall=int(drv.nalltoall)), got


def one_call(ctx, N, pos, nsteps, rounds):
    rows = []
    for r in range(1 + rounds):
        t0 = time.perf_counter()
        got = sq.glass_evolve(ctx, N, BOX, pos, None, 1.0, nsteps=nsteps, spectra=True)
        wall = (time.perf_counter() - t0) * 1e3
        if r > 0:
            rows.append(list(got["phase_ms"]) + [wall])
    m = dict(zip(("upload", "forces", "particle_loops", "device_total", "wall"), med(rows)))
    m["per_force"] = m["forces"] / (nsteps + 1)
    return m, got


def pass_comparison(ctx, N, nyl, rounds, K=20):
    """K launches of each pass between two synchronises, the passes alternating"""
    gops = sd.GpuGlassOps(ctx)
    gops.tables(N, BOX, float((N // 2) ** 3))
    k2 = np.arange(3 * (N // 2) ** 2 + 1, dtype=np.float64)
    delta = 1.0 / (1.0 + k2)
    capi.check(capi.hip.shq_zeldovich_slab_tables(ctx.h, N, BOX, capi.ptr(delta), None))
    zpc = gops.pitch(N) // 2
    g = torch.Generator(device="cuda").manual_seed(N)
    spec = torch.view_as_complex(torch.randn((N, nyl, zpc, 2), dtype=torch.float64, device="cuda", generator=g))
    work = spec.clone()       # the forward passes run in place: their input may be anything finite, and stays finite over K unscaled passes
    out = torch.empty_like(spec)
    sums = torch.zeros(3 * N + 1, dtype=torch.float64, device="cuda")
    p, w, q, s = (C.c_void_p(t.data_ptr()) for t in (spec, work, out, sums))
    torch.cuda.synchronize()

    def run(which):
        work.copy_(spec)
        work.mul_(1e-100)
        torch.cuda.synchronize()
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(K):
            if which == "mode3":
                capi.check(capi.hip.shq_uvbg_slab_xforward(ctx.h, N, w, 0, nyl))
            elif which == "mode7":
                capi.check(capi.hip.shq_glass_slab_xforward(ctx.h, N, w, 0, nyl, None))
            elif which == "mode7_sums":
                capi.check(capi.hip.shq_glass_slab_xforward(ctx.h, N, w, 0, nyl, s))
            elif which == "mode6":
                capi.check(capi.hip.shq_zeldovich_slab_xtransfer(ctx.h, N, BOX, p, q, 0, nyl, 2))
            else:
                capi.check(capi.hip.shq_glass_slab_xtransfer(ctx.h, N, p, q, 0, nyl, which))
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3 / K

    names = ("mode3", "mode7", "mode7_sums", "mode6", 0, 1, 2)
    rows = []
    for r in range(1 + rounds):
        row = [run(n) for n in names]
        if r > 0:
            rows.append(row)
    m = med(rows)
    res = dict(nyl=nyl, launches_per_sample=K, bytes_moved=int(2 * spec.numel() * 16), mode3_xforward_ms=m[0], mode7_xforward_ms=m[1],
               mode7_xforward_sums_ms=m[2], mode6_disp_y_ms=m[3], mode8_x_ms=m[4], mode8_y_ms=m[5], mode8_z_ms=m[6],
               spread_ms=[float(x) for x in (np.max(rows, axis=0) - np.min(rows, axis=0))])
    res["mode7_over_mode3"] = m[1] / m[0]
    res["mode7_sums_over_mode3"] = m[2] / m[0]
    res["mode8_y_over_mode6"] = m[5] / m[3]
    return res


def _worker(rank, world, initfile, tmp, sizes, nsteps, rounds):
    os.environ["OMP_NUM_THREADS"] = "8"
    if world == 1:
        os.environ["SHQ_COMM_FORCE"] = "1"
    dist.init_process_group("gloo", init_method="file://" + initfile, rank=rank, world_size=world)
    try:
        out = {}
        with sq.Context(0) as ctx:
            comm = sd.Comm()
            assert comm.multi
            for N in sizes:
                Ngrid = N // 2
                pos = sq.glass_setup_positions(Ngrid, BOX, 0.0, SEED)
                mine = np.ascontiguousarray(pos[rank::world])
                res, got = phased(ctx, comm, N, mine, nsteps, rounds)
                res["Ngrid"] = Ngrid
                if world == 1:
                    res["one_call_ms"], ref = one_call(ctx, N, pos, nsteps, rounds)
                    res["max_abs_diff_to_one_call"] = {k: float(np.abs(got[k].astype(np.float64) - ref[k]).max()) for k in ("Pos", "Vel", "Disp")}
                    res["pass_comparison"] = [pass_comparison(ctx, N, N, rounds), pass_comparison(ctx, N, N // 2, rounds)]
                out[str(N)] = res
        with open(os.path.join(tmp, "r%d.pkl" % rank), "wb") as f:
            pickle.dump(out, f)
    finally:
        dist.destroy_process_group()


def spawn(world, sizes, nsteps, rounds):
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_worker, args=(world, os.path.join(tmp, "init"), tmp, sizes, nsteps, rounds), nprocs=world, join=True)
        ranks = []
        for r in range(world):
            with open(os.path.join(tmp, "r%d.pkl" % r), "rb") as f:
                ranks.append(pickle.load(f))
        return ranks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--nsteps", type=int, default=14)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--box-name", default="", help="what to call this machine in the result")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dist_glass_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_dist_glass: no GPU")
    out = dict(BoxSize=BOX, seed=SEED, nsteps=a.nsteps, rounds=a.rounds, gpus=1, box=a.box_name or torch.cuda.get_device_name(0))
    out["one_rank_forced_collectives"] = spawn(1, a.sizes, a.nsteps, a.rounds)[0]
    out["two_ranks_one_gpu"] = spawn(2, a.sizes, a.nsteps, a.rounds)
    out["note"] = ("phase ms: a host clock around each phase call ended by a synchronise of the context's stream, summed over the call; per_force_ms "
                   "divides by the nsteps + 1 forces; wall also holds the gloo exchanges, which are staged through the host; one_call_ms is "
                   "shq_glass_phase_ms (HIP events) and a host clock; medians over the rounds after one warm-up; the two ranks are two processes "
                   "sharing one device; a phase that is the first device work after a host-staged exchange holds whatever an idle device takes to "
                   "wake up; the pass comparison is K launches back to back and is the figure to judge the passes by")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
