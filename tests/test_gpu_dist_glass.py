"""GPU tests of glass making across ranks (shenqi_amd/dist.py:DistGlass with GpuGlassOps on shq_glass_slab_*).

The passes alone, in this process without a group: the transfer pass (fft_pass_strided MODE 8) and the X forward with the glass's sums
(MODE 7) against numpy on two half slabs, the window deposit against the one-window deposit and glass_restated.deposit, and planes,
deposit and gather at the box edge and outside the box.  End to end two gloo ranks share the one GPU, one spawn for the module (one
more for the one-rank forced group): every step from the driver's own state against glass_restated at the bars of test_gpu_glass.py;
on the bespoke sizes the SAME BITS of Pos, Vel and Disp from 14 steps in one call whatever the rank count and whoever held which
particle, 5 + 9 steps equal to 14, a second run equal to the first (the statistics and spectrum sums are atomic sums in any order:
they are held to their any-order bars, the mode counts to equality); rows are re-homed in every step; two species; bad input on one
rank; and the sharded phases leave the PM's state and the one-rank resident Zel'dovich field alone."""
import ctypes as C
import os
import pickle
import sys
import tempfile
import traceback

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import shenqi_amd as sq  # noqa: E402
from shenqi_amd import capi  # noqa: E402
from shenqi_amd import dist as sd  # noqa: E402
import common as cm  # noqa: E402
import glass_dist_cases as gc  # noqa: E402
import glass_restated as gr  # noqa: E402
from test_gpu_zeldovich import _tables, zctx  # noqa: E402,F401
import zeldovich_dist_cases as zc  # noqa: E402

pytestmark = pytest.mark.gpu

ERR_INVALID = 1
L = gc.L
BESPOKE = [(16, 32, 21), (16, 48, 22)]           # (Ngrid, Nmesh, seed)
TORCH = [(12, 18, 23)]                           # no bespoke transform: the torch.fft route
NSTEPS = 14


def _vp(t):
    return C.c_void_p(t.data_ptr())


def _mass(n):
    return np.ones(n, dtype=np.float32)


def _species():
    Ngrid = 16
    cdm, gas = gc.particles(Ngrid, 31), gc.particles(Ngrid, 32, False) + 0.5 * L / Ngrid
    return np.concatenate([cdm, gas]), np.concatenate([np.full(len(cdm), 0.84, dtype=np.float32), np.full(len(gas), 0.16, dtype=np.float32)])


def _job(comm, ops, job):
    kind = job[0]
    if kind == "calls":
        (Ngrid, N, seed), how, calls = job[1], job[2], job[3]
        pos = gc.particles(Ngrid, seed)
        return gc.run_rank(comm, ops, N, pos, _mass(len(pos)), how=how, calls=calls)
    if kind == "species":
        pos, mass = _species()
        return gc.run_rank(comm, ops, 32, pos, mass, calls=(1,))
    if kind == "bad":           # only the last rank holds the bad particle
        Ngrid, N, seed = BESPOKE[0]
        pos = gc.particles(Ngrid, seed).copy()
        holder = gc.deal(len(pos), comm.size, 1)
        assert holder[37] == comm.size - 1 or comm.size != 2
        pos[37, 1] = np.nan
        return gc.run_rank(comm, ops, N, pos, _mass(len(pos)), holder=holder, calls=(2,))
    raise ValueError(kind)


def _worker(rank, world, initfile, outdir, jobs):
    os.environ["OMP_NUM_THREADS"] = "2"
    if world == 1:
        os.environ["SHQ_COMM_FORCE"] = "1"          # one rank that still runs every collective
    dist.init_process_group("gloo", init_method="file://" + initfile, rank=rank, world_size=world)
    try:
        with sq.Context(0) as ctx:
            ops = sd.GpuGlassOps(ctx)
            comm = sd.Comm()
            assert comm.multi
            res = [_job(comm, ops, job) for job in jobs]
        with open(os.path.join(outdir, "r%d.pkl" % rank), "wb") as f:
            pickle.dump(res, f)
    except BaseException:       # the parent reports only the rank that ended first, which may be the one its peer left alone
        traceback.print_exc()
        sys.stderr.flush()
        raise
    finally:
        dist.destroy_process_group()


def spawn(world, jobs):
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_worker, args=(world, os.path.join(tmp, "init"), tmp, jobs), nprocs=world, join=True)
        results = []
        for r in range(world):
            with open(os.path.join(tmp, "r%d.pkl" % r), "rb") as f:
                results.append(pickle.load(f))
        return {job: [results[r][j] for r in range(world)] for j, job in enumerate(jobs)}


@pytest.fixture(scope="module")
def two_ranks():
    """every shape as 14 one-step calls; the bespoke ones as one call of 14 steps with both deals; 0 steps, 5 + 9 steps and a second run
    of the first shape; two species; bad input: one spawn"""
    first = BESPOKE[0]
    return spawn(2, [("calls", s, 1, (1,) * NSTEPS) for s in BESPOKE + TORCH]
                 + [("calls", s, how, (NSTEPS,)) for s in BESPOKE for how in (1, 2)]
                 + [("calls", first, 1, (0,)), ("calls", first, 1, (5, 9)), ("calls", first, 1, (NSTEPS,), "again"), ("species",), ("bad",)])


@pytest.fixture(scope="module")
def one_rank():
    return spawn(1, [("calls", s, 1, (NSTEPS,)) for s in BESPOKE])


# ---- the passes alone

def _random_slab(N, zpc):
    rng = np.random.default_rng(N)
    return rng.normal(0, 1, (N, N, zpc)) + 1j * rng.normal(0, 1, (N, N, zpc))


@pytest.mark.parametrize("N", [32, 48])
def test_transfer_pass_against_numpy(ctx, N):
    """fft_pass_strided MODE 8 on one rank, no process group: nyl = N / 2 at y0 = 0 and N / 2 (the ky offset), the three axes, to 1e-12
    of the result's maximum - the bar test_strided_transfer_pass_against_numpy holds MODE 6 to.  The output starts as NaN; the kept
    spectrum must come through untouched (the pass stores out of place)."""
    ops = sd.GpuGlassOps(ctx)
    totmass = 4096.0
    ops.tables(N, L, totmass)
    zpc, Nc, h = ops.pitch(N) // 2, N // 2 + 1, N // 2
    assert zpc >= Nc
    pad = _random_slab(N, zpc)
    for y0 in (0, h):
        part = np.ascontiguousarray(pad[:, y0:y0 + h])
        kept = torch.from_numpy(part).cuda()
        for axis in range(3):
            want = np.fft.ifft(gc.slab_transfer(part[:, :, :Nc], N, L, totmass, y0, h, axis), axis=0, norm="forward")
            out = torch.full_like(kept, float("nan"))
            ops.xtransfer(N, kept, out, y0, h, axis)
            ctx.synchronize()
            got = out.cpu().numpy()
            err, tol = np.abs(got[:, :, :Nc] - want).max(), 1e-12 * np.abs(want).max()
            print(f"N {N} y0 {y0} axis {axis}: max |diff| {err:.3e}, bar {tol:.3e}")
            assert err <= tol, (N, y0, axis, err, tol)
            assert not got[:, :, Nc:].any()                           # pad columns are stored as 0
            assert np.array_equal(kept.cpu().numpy(), part)           # only read


@pytest.mark.parametrize("N", [32, 48])
def test_forward_pass_with_the_glass_sums(ctx, N):
    """fft_pass_strided MODE 7 on the same halves: the mode counts of the two halves add up, as integers, to the restatement's and to
    2 (N^3 - 1); kk, power and norm within 1e-11 + 3 N^3 2^-53; norm only from the half with y = 0; the spectrum has the bits of the
    same pass without sums."""
    ops = sd.GpuGlassOps(ctx)
    ops.tables(N, L, 1.0)
    zpc, Nc, h = ops.pitch(N) // 2, N // 2 + 1, N // 2
    pad = _random_slab(N, zpc)
    full = np.fft.fft(pad[:, :, :Nc], axis=0)
    kk, power, nmodes, norm = gr.glass_power(full, N)
    tot = np.zeros(3 * N + 1)
    cnt = np.zeros(N, dtype=np.int64)
    for y0 in (0, h):
        part = np.ascontiguousarray(pad[:, y0:y0 + h])
        a, b = torch.from_numpy(part).cuda(), torch.from_numpy(part).cuda()
        sums = torch.zeros(3 * N + 1, dtype=torch.float64, device="cuda")
        ops.xforward(N, a, y0, h, sums)
        ops.xforward(N, b, y0, h, None)
        ctx.synchronize()
        got = a.cpu().numpy()
        assert np.array_equal(got, b.cpu().numpy())
        want = full[:, y0:y0 + h]
        assert np.abs(got[:, :, :Nc] - want).max() <= 1e-12 * np.abs(want).max()
        s = sums.cpu().numpy()
        assert (s[3 * N] != 0) == (y0 == 0)
        tot += s
        cnt += s[2 * N:3 * N].copy().view(np.int64)
    bar = 1e-11 + 3 * N**3 * 2.0**-53
    nz = nmodes > 0
    assert np.array_equal(cnt, nmodes) and cnt.sum() == 2 * (N**3 - 1)
    assert np.abs(tot[N:2 * N][nz] / kk[nz] - 1).max() <= bar
    assert np.abs(tot[:N][nz] / power[nz] - 1).max() <= bar
    assert not tot[:N][~nz].any() and abs(tot[3 * N] / norm - 1) <= bar


def _deposit(ops, N, pos, mass, exp, plane0, nxl, nalloc):
    """shq_glass_slab_deposit into a window with a NaN guard plane on either side: (return code, window as int64, guards untouched)"""
    zp = ops.pitch(N) or N + 2
    big = torch.full((nalloc + 2, N, zp), float("nan"), dtype=torch.float64, device="cuda")
    win = big[1:1 + nalloc]
    p, m = torch.from_numpy(np.array(pos)).cuda(), torch.from_numpy(np.array(mass, dtype=np.float32)).cuda()      # copies: torch takes no read-only array
    torch.cuda.synchronize()
    rc = capi.hip.shq_glass_slab_deposit(ops.ctx.h, N, L, _vp(p), _vp(m), len(pos), exp, plane0, nxl, nalloc, _vp(win))
    ops.ctx.synchronize()
    guards = bool(torch.isnan(big[0]).all() and torch.isnan(big[-1]).all())
    return rc, win.view(torch.int64).cpu().numpy(), guards


def _planes(ops, N, pos):
    return ops.planes(N, L, torch.from_numpy(np.array(pos)).cuda()).cpu().numpy()


@pytest.mark.parametrize("N", [32, 18])
def test_half_windows_and_the_ghost_add_equal_the_one_window_deposit(ctx, N):
    ops = sd.GpuGlassOps(ctx)
    pos = gc.particles(16, 100 + N)
    assert (pos < 0).any() and (pos >= L).any()
    n, h = len(pos), N // 2
    mass = _mass(n)
    exp = 13                                                   # frexp(4096.0): 2^12 is 0.5 * 2^13
    rc, one, guards = _deposit(ops, N, pos, mass, exp, 0, N, N)
    assert rc == 0 and guards
    owner = _planes(ops, N, pos) // h
    assert np.array_equal(owner, gc.owners(pos, N, 2))
    whole = np.zeros_like(one)
    for r in range(2):
        sel = owner == r
        assert sel.any()
        rc, half, guards = _deposit(ops, N, pos[sel], mass[sel], exp, r * h, h, h + 1)
        assert rc == 0 and guards
        whole[r * h:(r + 1) * h] += half[:h]
        whole[((r + 1) * h) % N] += half[h]                    # the ghost plane, added into the right-hand neighbour's plane 0
    assert np.array_equal(whole, one)
    mesh = one[:, :, :N].astype(np.float64) * 2.0**(exp - 61)
    ref = gr.deposit(pos, mass, N, L)
    assert np.abs(mesh - ref).max() <= 1e-11 * np.abs(ref).max()
    assert not one[:, :, N:].any()


@pytest.mark.parametrize("N", [24, 18])
def test_planes_deposit_and_gather_at_the_edges(ctx, N):
    """positions at nextafter(L, 0), at negative x and at x >= L: the device's base plane is cic_setup's, the window that holds it
    takes the particle, the other window refuses it - SHQ_ERR_INVALID, nothing deposited, the output keeps its sentinel, the planes
    outside the window keep their NaN fill"""
    ops = sd.GpuGlassOps(ctx)
    h, cell = N // 2, L / N
    edge = np.nextafter(L, 0.0)
    x = np.array([edge, -0.25 * cell, -1e-300, L, L + 0.25 * cell, 2 * L + (h + 0.5) * cell, -(h - 0.5) * cell, (h - 1) * cell + 0.75 * cell])
    pos = np.stack([x, np.full(len(x), 0.3 * L), np.full(len(x), edge)], axis=1)
    planes = _planes(ops, N, pos)
    assert np.array_equal(planes, np.floor(x / cell).astype(np.int64) % N)
    # x / cell rounds up to N at the edge: cell N is cell 0, rank 0's plane 0, although the position is below L
    assert planes[0] == 0 and planes[1] == N - 1 and planes[2] == N - 1 and planes[4] == 0 and planes[5] == h and planes[6] == h and planes[7] == h - 1
    zp = ops.pitch(N) or N + 2
    for p in range(len(x)):
        r = planes[p] // h
        one, m = pos[p:p + 1], _mass(1)
        rc, win, guards = _deposit(ops, N, one, m, 1, r * h, h, h + 1)
        # the whole of 1.0 at the scale 2^(61 - 1): eight weights, each a product of three factors rounded at 2^-53, then to an integer
        assert rc == 0 and guards and abs(int(win.sum()) - 2**60) <= 8 * (3 * 2**7 + 1)
        rc, win, guards = _deposit(ops, N, one, m, 1, (1 - r) * h, h, h + 1)
        assert rc == ERR_INVALID and guards and not win.any()
        big = torch.full((h + 3, N, zp), float("nan"), dtype=torch.float64, device="cuda")
        big[1:h + 2] = 1.0
        window = big[1:h + 2]
        d = torch.full((1, 3), 7.0, dtype=torch.float32, device="cuda")
        pt = torch.from_numpy(one.copy()).cuda()
        torch.cuda.synchronize()
        rc = capi.hip.shq_glass_slab_gather(ctx.h, N, L, _vp(pt), 1, _vp(window), (1 - r) * h, h, h + 1, _vp(d), 1)
        ctx.synchronize()
        assert rc == ERR_INVALID and (d.cpu().numpy() == 7.0).all()
        rc = capi.hip.shq_glass_slab_gather(ctx.h, N, L, _vp(pt), 1, _vp(window), r * h, h, h + 1, _vp(d), 1)
        ctx.synchronize()
        got = d.cpu().numpy()[0]
        assert rc == 0 and got[0] == 7.0 and got[2] == 7.0 and abs(got[1] - 1.0) <= 8 * 2.0**-23     # the weights add up to 1


# ---- end to end

@pytest.mark.parametrize("shape", BESPOKE + TORCH, ids=lambda s: "-".join(map(str, s)))
def test_every_step_from_the_drivers_own_state(two_ranks, shape):
    Ngrid, N, seed = shape
    pos = gc.particles(Ngrid, seed)
    mass, vel = _mass(len(pos)), np.zeros((len(pos), 3), dtype=np.float32)
    ranks = two_ranks[("calls", shape, 1, (1,) * NSTEPS)]
    worst = dict(disp=0.0, vel=0.0, pos=0.0)
    for s in range(NSTEPS):
        out = gc.assemble(ranks, s)
        assert all(r["outs"][s]["nalltoall"] == 2 + 1 + 2 * 8 for r in ranks)
        e = gc.compare_step(pos, vel, mass, out, N, "%s step %d" % (shape, s))
        worst = {k: max(worst[k], e[k]) for k in worst}
        # the rows re-homed in this step: the owner changes between the driver's own positions
        assert out["rehomed"][0] == int((gc.owners(out["Pos"], N, 2) != gc.owners(pos, N, 2)).sum())
        pos, vel = out["Pos"], out["Vel"]
    print("worst error / bar over %d steps:" % NSTEPS, shape, {k: round(v, 4) for k, v in worst.items()})


def test_bits_do_not_depend_on_the_rank_count_the_deal_or_the_split(two_ranks, one_rank):
    for shape in BESPOKE:
        Ngrid, N, seed = shape
        a, b, c = (gc.assemble(r[("calls", shape, how, (NSTEPS,))]) for r, how in ((two_ranks, 1), (one_rank, 1), (two_ranks, 2)))
        others = [b, c]
        if shape == BESPOKE[0]:
            others += [gc.assemble(two_ranks[("calls", shape, 1, (5, 9))], 1), gc.assemble(two_ranks[("calls", shape, 1, (NSTEPS,), "again")]),
                       gc.assemble(two_ranks[("calls", shape, 1, (1,) * NSTEPS)], NSTEPS - 1)]
        for other in others:
            for k in gc.FIELDS:
                assert np.array_equal(a[k], other[k]), (shape, k, int(np.sum(a[k] != other[k])))
        assert np.abs(a["Disp"]).max() > 0 and a["steps"][-1]["force_std"] < a["steps"][0]["force_std"]
        anyorder, tol = 3 * (N**3) * 2.0**-53, 3 * (3 * len(a["Pos"])) * 2.0**-53
        for other in (b, c):
            assert np.array_equal(a["nmodes"], other["nmodes"]) and (a["nmodes"].sum(axis=1) == 2 * (N**3 - 1)).all()
            for k in ("kk", "power", "norm"):
                nz = a[k] != 0
                assert np.array_equal(nz, other[k] != 0) and np.abs(other[k][nz] / a[k][nz] - 1).max() <= anyorder, (shape, k)
            for x, y in zip(a["steps"], other["steps"]):
                assert (x["t_f"], x["t_v"], x["t_x"]) == (y["t_f"], y["t_v"], y["t_x"])
                assert abs(y["force_std"] / x["force_std"] - 1) <= tol and abs(y["vel_std"] / x["vel_std"] - 1) <= tol
        for ranks in (two_ranks[("calls", shape, 1, (NSTEPS,))], one_rank[("calls", shape, 1, (NSTEPS,))]):
            F = 8 if len(ranks) > 1 else 4
            assert all(r["outs"][0]["nalltoall"] == 2 + NSTEPS + (NSTEPS + 1) * F for r in ranks)


def test_rows_are_rehomed_in_every_step(two_ranks, one_rank):
    """(Ngrid 16, Nmesh 32, seed 21): glass_restated alone moves 76, 41, 15, 15, 12, 14, 7, 6, 3, 3, 4, 4, 5, 9 particles across the
    two-rank boundary there, so every step of the resident loop has rows to re-home"""
    shape = BESPOKE[0]
    for how in (1, 2):
        moved = gc.assemble(two_ranks[("calls", shape, how, (NSTEPS,))])["rehomed"]
        assert len(moved) == NSTEPS and (moved > 0).all(), moved
        # the same bits as the sequence of one-step calls, whose counts are checked against the driver's own positions
        seq = [gc.assemble(two_ranks[("calls", shape, 1, (1,) * NSTEPS)], s)["rehomed"][0] for s in range(NSTEPS)]
        assert list(moved) == seq
    assert all(r["outs"][0]["rows_sent"] > 0 for r in two_ranks[("calls", shape, 1, (NSTEPS,))])
    assert not gc.assemble(one_rank[("calls", shape, 1, (NSTEPS,))])["rehomed"].any()


def test_one_force_and_one_step_against_the_one_rank_call(two_ranks, ctx):
    """shq_glass_evolve on the undivided set runs its passes in another order, so not bits: the opening force and the first drift at
    the bars"""
    shape = Ngrid, N, seed = BESPOKE[0]
    pos = gc.particles(Ngrid, seed)
    mass = _mass(len(pos))
    force = gc.assemble(two_ranks[("calls", shape, 1, (0,))])
    assert np.array_equal(force["Pos"], pos) and not force["Vel"].any() and force["steps"] == [] and force["nmodes"].shape == (0, N)
    one = sq.glass_evolve(ctx, N, L, pos, None, mass, nsteps=0)
    d0, m0, _ = gr.glass_force(pos, mass, N, L)
    bar0 = gc._disp_bar(m0)
    assert np.abs(force["Disp"].astype(np.float64) - one["Disp"]).max() <= bar0
    step = gc.assemble(two_ranks[("calls", shape, 1, (1,) * NSTEPS)], 0)
    one = sq.glass_evolve(ctx, N, L, pos, None, mass, nsteps=1)
    v1 = gr.kick(np.zeros_like(d0), d0)
    bar_p = (bar0 * gr.HDT + gc._ulp32(v1)) * gr.DT + 2 * float(np.spacing(np.abs(one["Pos"]).max()))
    assert np.abs(step["Pos"] - one["Pos"]).max() <= bar_p


def test_two_species(two_ranks):
    pos, mass = _species()
    out = gc.assemble(two_ranks[("species",)])
    print(gc.compare_step(pos, np.zeros((len(pos), 3), dtype=np.float32), mass, out, 32, "two species"))
    eq, m0, _ = gr.glass_force(out["Pos"], _mass(len(pos)), 32, L)             # the masses matter
    assert np.abs(eq.astype(np.float64) - out["Disp"]).max() > 100 * gc._disp_bar(m0)


def test_bad_input_on_one_rank_raises_on_both(two_ranks):
    results = two_ranks[("bad",)]
    assert all("error" in r and not r.get("constructor") and r["nalltoall"] == 0 for r in results), results
    assert "another rank" in results[0]["error"] and "position" in results[1]["error"]


# ---- no interference

class _forced_group:
    """a one-rank gloo group under SHQ_COMM_FORCE=1, so that DistGlass runs every collective inside this process"""

    def __enter__(self):
        self.before = os.environ.get("SHQ_COMM_FORCE")
        os.environ["SHQ_COMM_FORCE"] = "1"
        self.tmp = tempfile.TemporaryDirectory()
        dist.init_process_group("gloo", init_method="file://" + os.path.join(self.tmp.name, "init"), rank=0, world_size=1)

    def __exit__(self, *exc):
        dist.destroy_process_group()
        self.tmp.cleanup()
        if self.before is None:
            del os.environ["SHQ_COMM_FORCE"]
        else:
            os.environ["SHQ_COMM_FORCE"] = self.before


def _slab_phases(ctx, N):
    """a full set of slab phases on the context: tables, planes, and two forces with the spectrum's sums around a particle kernel"""
    drv = sd.DistGlass(sd.Comm(), N, L, sd.GpuGlassOps(ctx))
    assert drv.comm.multi and drv.comm.size == 1
    got = drv.evolve(gc.particles(8, 4), None, 1.0, 1, spectra=True)
    assert drv.nalltoall == 2 + 1 + 2 * 4 and np.abs(got["Disp"]).max() > 0 and got["nmodes"].sum() == 2 * (N**3 - 1)
    return got


def test_no_interference_with_a_pending_spectrum(zctx):
    """test_gpu_dist_zeldovich's check: DistGlass under SHQ_COMM_FORCE=1 between shq_pm_forward and shq_pm_run, at the PM's own mesh
    size (its twiddles) and at another"""
    ctx = zctx
    n, box, nmesh = 40000, cm.BOX, 48
    pos = cm.random_positions(np.random.default_rng(3).random(3 * n), n)
    pman = cm.make_partmanager(pos)
    pmp = sq.PMParams(nmesh, 0, box, 1.5, cm.G)
    T = 1.0 + 0.3 * np.exp(-np.arange(3 * (nmesh // 2) ** 2 + 1) / 36.0)
    capi.check(capi.hip.shq_pm_set_deposit_log2scale(ctx.h, 40))
    calls = []

    def run(with_glass):
        pv = pman.view()
        capi.check(capi.hip.shq_particles_upload(ctx.h, C.byref(pv)))
        capi.check(capi.hip.shq_pm_forward(ctx.h, C.byref(pmp)))
        z0 = C.c_int(-1)
        capi.check(capi.hip.shq_pm_mesh_prezeroed(ctx.h, C.byref(z0)))
        if with_glass:
            calls.append(_slab_phases(ctx, 32))
            calls.append(_slab_phases(ctx, nmesh))
            z1 = C.c_int(-1)
            capi.check(capi.hip.shq_pm_mesh_prezeroed(ctx.h, C.byref(z1)))
            assert z1.value == z0.value
            assert capi.hip.shq_pm_get_deposit_log2scale(ctx.h) == 40
        capi.check(capi.hip.shq_pm_set_mode_factor(ctx.h, nmesh, capi.ptr(T)))
        capi.check(capi.hip.shq_pm_run(ctx.h, C.byref(pmp)))
        g = np.zeros((n, 3)); pp = np.zeros(n)
        capi.check(capi.hip.shq_pm_download(ctx.h, capi.ptr(g), capi.ptr(pp)))
        return g, pp

    try:
        ref = run(False)
        with _forced_group():
            got = run(True)
    finally:
        capi.check(capi.hip.shq_pm_set_deposit_log2scale(ctx.h, -1))     # the session context goes back to its own scale rule
    assert len(calls) == 2
    assert np.array_equal(ref[0], got[0]) and np.array_equal(ref[1], got[1])


def test_the_one_rank_resident_field_survives(zctx):
    N = 24
    delta, growth = _tables(N)
    pos = zc.particles(N)
    a = sq.displacement_fields(zctx, pos, N, zc.BOX, 11, delta)
    assert a["phase_ms"][0] > 0
    with _forced_group():
        _slab_phases(zctx, N)           # the same mesh size
        _slab_phases(zctx, 16)
    b = sq.displacement_fields(zctx, pos, N, zc.BOX, 11, delta)
    assert b["phase_ms"][0] == 0
    for k in ("Pos", "Vel", "Density", "Disp"):
        assert np.array_equal(a[k], b[k]), k
