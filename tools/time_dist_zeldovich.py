"""Device time of the sharded Zel'dovich displacements in phases (shq_zeldovich_slab_* driven by dist.py:DistZeldovich) beside the one
call (shq_zeldovich_displacements) on the same context and lattice, at Nmesh 256 and 512 (--sizes), Ngrid = Nmesh / --ngrid-div.

  one rank, SHQ_COMM_FORCE=1   one gloo rank in a fresh child process that still runs every collective: per phase (fill, tables,
                               xtransfer, yz inverse, gather, finalize) the time of the phase's calls summed over the 7 fields, each
                               taken with a host clock around the call and a synchronise of the context's stream; the call's wall
                               time, which also holds the host-staged gloo exchanges; then the one call's phase_ms and wall time.
                               Two comparisons on that context, reported, not gated:
                                 the MODE 6 transfer pass (shq_zeldovich_slab_xtransfer) against the MODE 5 filter pass
                                 (shq_uvbg_slab_xfilter) at the same N, nyl and box: K launches back to back, one synchronise, the two
                                 alternating, the median over the rounds;
                                 the slab fill of the whole mesh (y0 = 0, nyl = N) against the one-shot fill (shq_zeldovich_fill
                                 after shq_zeldovich_drop_field).
  two ranks, one GPU           two gloo ranks in fresh child processes with a context each on device 0, the lattice dealt round-robin.
                               The two processes share the device, so these are not scaling numbers.

Medians over --rounds after one warm-up.  Writes profiles/dist_zeldovich_timing.json (or --out) and prints it as one JSON line.
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

BOX = 25.0
SEED = 181170
PHASES = ("fill", "tables", "xtransfer", "fft_yz", "gather", "finalize")


def delta_of(k):
    return 3.0 * k / (1.0 + (k / 2.0) ** 3)


def growth_of(k):
    return 1.0 + 0.2 * np.tanh(k)


def tables(N):
    k = np.sqrt(np.arange(3 * (N // 2) ** 2 + 1, dtype=np.float64)) * 2 * np.pi / BOX
    d, g = delta_of(k), growth_of(k)
    d[0] = g[0] = 0.0
    return d, g


class TimedOps(sd.GpuZeldovichOps):
    """GpuZeldovichOps with a host clock around every phase call, each ended by a synchronise of the context's stream"""

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
            return self._timed(name, getattr(sd.GpuZeldovichOps, name).__get__(self), *args)
        return method
    setattr(TimedOps, _name, _wrap(_name))


def med(rows):
    return [float(x) for x in np.median(np.array(rows, dtype=np.float64), axis=0)]


def phased(ctx, comm, N, pos, rounds):
    delta, growth = tables(N)
    zp = capi.ZeldovichParams(N, SEED, 0, 0, 1, 0, BOX, 37.5)
    rows, refill = [], None
    for r in range(1 + rounds):
        ops = TimedOps(ctx)
        drv = sd.DistZeldovich(comm, N, BOX, ops)       # a fresh driver: every round fills
        comm.barrier()
        t0 = time.perf_counter()
        got = drv.displacements(zp, delta, growth, pos)
        wall = (time.perf_counter() - t0) * 1e3
        if r > 0:
            rows.append([ops.ms[k] for k in PHASES] + [wall])
        if r == rounds:      # the second species on the same driver: no fill
            ops.ms = dict.fromkeys(PHASES, 0.0)
            t0 = time.perf_counter()
            drv.displacements(zp, delta, growth, pos)
            refill = dict(filled=bool(drv.filled), wall_ms=(time.perf_counter() - t0) * 1e3)
    out = dict(zip(PHASES + ("wall",), med(rows)))
    return dict(ms=out, particles=int(len(pos)), rows_sent=int(drv.rows_sent), nalltoall=int(drv.nalltoall), second_species=refill,
                maxdisp=got["maxdisp"]), got


def one_call(ctx, N, pos, rounds):
    delta, growth = tables(N)
    rows = []
    for r in range(1 + rounds):
        capi.check(capi.hip.shq_zeldovich_drop_field(ctx.h))
        t0 = time.perf_counter()
        got = sq.displacement_fields(ctx, pos, N, BOX, SEED, delta, growth, vel_prefac=37.5, ScaleDepVelocity=True)
        wall = (time.perf_counter() - t0) * 1e3
        if r > 0:
            rows.append(list(got["phase_ms"]) + [wall])
    capi.check(capi.hip.shq_zeldovich_drop_field(ctx.h))
    return dict(zip(("fill", "fields", "particle_loop", "device_total", "wall"), med(rows))), got


def pass_comparison(ctx, N, nyl, rounds, K=20):
    """K launches of each pass between two synchronises, the two passes alternating"""
    delta, growth = tables(N)
    zops = sd.GpuZeldovichOps(ctx)
    zops.tables(N, BOX, delta, growth)
    radii = np.array([BOX / 8, BOX / 16, BOX / N])
    capi.check(capi.hip.shq_uvbg_slab_tables(ctx.h, 0, N, BOX, capi.ptr(radii), len(radii)))
    zpc = zops.pitch(N) // 2
    g = torch.Generator(device="cuda").manual_seed(N)
    spec = torch.view_as_complex(torch.randn((N, nyl, zpc, 2), dtype=torch.float64, device="cuda", generator=g))
    out = torch.empty_like(spec)
    p, q = C.c_void_p(spec.data_ptr()), C.c_void_p(out.data_ptr())
    torch.cuda.synchronize()

    def run(which):
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(K):
            if which == "mode5":
                capi.check(capi.hip.shq_uvbg_slab_xfilter(ctx.h, N, p, q, 0, nyl, 0))
            else:
                capi.check(capi.hip.shq_zeldovich_slab_xtransfer(ctx.h, N, BOX, p, q, 0, nyl, which))
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3 / K

    names = ("mode5", 0, 2, 6)
    rows = []
    for r in range(1 + rounds):
        row = [run(w) for w in names]
        if r > 0:
            rows.append(row)
    m = med(rows)
    res = dict(nyl=nyl, launches_per_sample=K, mode5_xfilter_ms=m[0], mode6_density_ms=m[1], mode6_disp_y_ms=m[2], mode6_vel_z_ms=m[3],
               bytes_moved=int(2 * spec.numel() * 16))
    res["mode6_disp_over_mode5"] = m[2] / m[0]
    return res


def fill_comparison(ctx, N, rounds):
    zops = sd.GpuZeldovichOps(ctx)
    rows = []
    for r in range(1 + rounds):
        capi.check(capi.hip.shq_zeldovich_drop_field(ctx.h))
        ctx.synchronize()
        t0 = time.perf_counter()
        capi.check(capi.hip.shq_zeldovich_fill(ctx.h, N, SEED, 0, 0))
        ctx.synchronize()
        t1 = time.perf_counter()
        spec = zops.fill(N, SEED, 0, 0, 0, N)
        ctx.synchronize()
        t2 = time.perf_counter()
        del spec
        if r > 0:
            rows.append([(t1 - t0) * 1e3, (t2 - t1) * 1e3])
    capi.check(capi.hip.shq_zeldovich_drop_field(ctx.h))
    m = med(rows)
    return dict(one_shot_fill_ms=m[0], slab_fill_whole_mesh_ms=m[1], slab_over_one_shot=m[1] / m[0])


def _worker(rank, world, initfile, tmp, sizes, div, rounds):
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
                Ngrid = N // div
                pos, _ = sq.setup_grid(sq.IDGenerator(Ngrid, BOX), 0.5 * BOX / Ngrid, 1.0)
                mine = np.ascontiguousarray(pos[rank::world])
                res, got = phased(ctx, comm, N, mine, rounds)
                res["Ngrid"] = Ngrid
                if world == 1:
                    res["one_call_ms"], ref = one_call(ctx, N, pos, rounds)
                    scale = np.abs(ref["Disp"]).max()
                    res["max_rel_diff_to_one_call"] = {k: float(np.abs(got[k] - ref[k]).max() / np.abs(ref[k]).max()) for k in ("Density", "Disp", "Vel")}
                    res["max_disp"] = float(scale)
                    res["pass_comparison"] = [pass_comparison(ctx, N, N, rounds), pass_comparison(ctx, N, N // 2, rounds)]
                    res["fill_comparison"] = fill_comparison(ctx, N, rounds)
                out[str(N)] = res
        with open(os.path.join(tmp, "r%d.pkl" % rank), "wb") as f:
            pickle.dump(out, f)
    finally:
        dist.destroy_process_group()


def spawn(world, sizes, div, rounds):
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_worker, args=(world, os.path.join(tmp, "init"), tmp, sizes, div, rounds), nprocs=world, join=True)
        ranks = []
        for r in range(world):
            with open(os.path.join(tmp, "r%d.pkl" % r), "rb") as f:
                ranks.append(pickle.load(f))
        return ranks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--ngrid-div", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dist_zeldovich_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_dist_zeldovich: no GPU")
    out = dict(BoxSize=BOX, Seed=SEED, ScaleDepVelocity=1, rounds=a.rounds, gpus=1)
    out["one_rank_forced_collectives"] = spawn(1, a.sizes, a.ngrid_div, a.rounds)[0]
    out["two_ranks_one_gpu"] = spawn(2, a.sizes, a.ngrid_div, a.rounds)
    out["note"] = ("phase ms: a host clock around each phase call ended by a synchronise of the context's stream, summed over the call's 7 fields; "
                   "wall also holds the gloo exchanges, which are staged through the host; one_call_ms is shq_zeldovich_phase_ms (HIP events) and a "
                   "host clock; medians over the rounds after one warm-up; the two ranks are two processes sharing one device; fft_yz is the first "
                   "device work after each host-staged exchange, so its figure holds whatever an idle device takes to wake up and is not the "
                   "passes' own time")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
