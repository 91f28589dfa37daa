"""GPU tests of the sharded Zel'dovich displacements (shenqi_amd/dist.py:DistZeldovich with GpuZeldovichOps on shq_zeldovich_slab_*).

Two gloo ranks share the one GPU, one spawn for the module.  The slab fill must give the bits of the one-rank field's rows; the
transfer pass (fft_pass_strided MODE 6) is held to numpy on its own; end to end the reference is zeldovich_restated.displacement_fields
on the undivided set at the bars of test_gpu_zeldovich._compare, and on the bespoke route also the one-rank call.  There the results
must be the SAME BITS whatever the rank count and whoever held which particle: a rank fills exactly its own columns and a mesh line sees
the same kernel arithmetic on any rank.  The sharded phases must leave the PM's state and the one-rank resident field alone."""
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
import zeldovich_dist_cases as zc  # noqa: E402
import zeldovich_restated as zr  # noqa: E402
from test_gpu_zeldovich import BAR, BOX, _compare, _delta, _growth, _tables, zctx  # noqa: E402,F401

pytestmark = pytest.mark.gpu

ERR_INVALID = 1
BESPOKE = [(16, 2, 1), (48, 2, 1), (64, 2, 0)]
TORCH = [(18, 2, 1)]
EDGE = [24, 18]                                    # one mesh size per transform route
ALL = ("Pos", "Vel", "Density", "Disp", "maxdisp", "maxvel")


def edge_particles():
    """the eight particles of test_last_position_below_the_box_edge: BoxSize 1, every choice of the axes at nextafter(1, 0)"""
    edge = np.nextafter(1.0, 0.0)
    inner = np.array([[0.3, 0.55, 0.71], [0.12, 0.91, 0.47], [0.66, 0.05, 0.38], [0.83, 0.29, 0.14],
                      [0.41, 0.77, 0.95], [0.58, 0.18, 0.62], [0.07, 0.49, 0.86], [0.24, 0.64, 0.02]])
    at_edge = np.array([(0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1), (1, 1, 0)], dtype=bool)
    return np.ascontiguousarray(np.where(at_edge, edge, inner))


def edge_tables(N):
    return zr.tabulate_k2(_delta, N, 1.0), zr.tabulate_k2(_growth, N, 1.0)


def _job(comm, ops, job):
    kind = job[0]
    if kind == "case":
        return zc.run_rank(comm, ops, job[1], how=job[2])
    if kind == "edge":          # all eight start on rank 1 (on the only rank of a one-rank group)
        N = job[1]
        pos = edge_particles()
        return zc.run_rank(comm, ops, (N, comm.size, 1), pos=pos, holder=np.full(len(pos), comm.size - 1), box=1.0, tables=edge_tables(N))
    if kind == "reuse":         # one driver: a species, another species, another seed; and a fresh driver for the second species
        case = job[1]
        drv = sd.DistZeldovich(comm, case[0], BOX, ops)
        a = zc.run_rank(comm, ops, case, drv=drv)
        b = zc.run_rank(comm, ops, case, drv=drv, other=True)
        fresh = zc.run_rank(comm, ops, case, other=True)
        c = zc.run_rank(comm, ops, case, drv=drv, other=True, seed=zc.SEED + 1)
        return dict(idx=a["idx"], a=a, b=b, fresh=fresh, c=c)
    raise ValueError(kind)


def _worker(rank, world, initfile, outdir, jobs):
    os.environ["OMP_NUM_THREADS"] = "2"
    if world == 1:
        os.environ["SHQ_COMM_FORCE"] = "1"          # one rank that still runs every collective
    dist.init_process_group("gloo", init_method="file://" + initfile, rank=rank, world_size=world)
    try:
        with sq.Context(0) as ctx:
            ops = sd.GpuZeldovichOps(ctx)
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
    """every case on two ranks, the bespoke ones also with the other deal; the box edge; the reuse sequence: one spawn"""
    return spawn(2, [("case", c, 1) for c in BESPOKE + TORCH] + [("case", c, 2) for c in BESPOKE] + [("edge", N) for N in EDGE]
                 + [("reuse", BESPOKE[0])])


@pytest.fixture(scope="module")
def one_rank():
    return spawn(1, [("case", c, 1) for c in BESPOKE])


# ---- the slab fill

def _slab_fill(ctx, N, seed, unitary, invert, y0, nyl):
    """shq_zeldovich_slab_fill into a buffer of NaNs: every element, pad columns included, must be written"""
    zpc = capi.hip.shq_zeldovich_slab_pitch(N) // 2 or N // 2 + 1
    spec = torch.full((N, nyl, zpc), float("nan"), dtype=torch.complex128, device="cuda")
    torch.cuda.synchronize()
    capi.check(capi.hip.shq_zeldovich_slab_fill(ctx.h, N, seed, unitary, invert, y0, nyl, C.c_void_p(spec.data_ptr())))
    ctx.synchronize()
    return spec.cpu().numpy()


def _check_slabs(ctx, N, seed, unitary, invert, tag):
    dense = sq.zeldovich_field(ctx, N, seed, unitary, invert).transpose(2, 0, 1)          # [y][z'][x] -> [x][y][z']
    Nc = N // 2 + 1
    for P in (2, 3):
        bounds = [N * r // P for r in range(P + 1)]
        for y0, y1 in zip(bounds[:-1], bounds[1:]):
            got = _slab_fill(ctx, N, seed, unitary, invert, y0, y1 - y0)
            assert np.array_equal(got[:, :, :Nc], dense[:, y0:y1]), (tag, N, P, y0)
            assert np.all(got[:, :, Nc:] == 0), (tag, N, P, y0)
    return dense


@pytest.mark.parametrize("N", [16, 24, 18])
def test_slab_fill_has_the_bits_of_the_one_rank_field(zctx, N):
    flags = ((0, 0), (1, 0), (0, 1), (1, 1)) if N == 16 else ((0, 0),)
    for unitary, invert in flags:
        dense = _check_slabs(zctx, N, 4242, unitary, invert, "flags %d %d" % (unitary, invert))
        assert dense[0, 0, 0] == 0 and np.abs(dense).max() > 0
    if N == 24:
        # 64 columns per launch: a half slab of 24 x 12 = 288 columns takes five launches, the last wave half filled
        capi.check(capi.hip.shq_zeldovich_set_fill_chunk(zctx.h, 64))
        _check_slabs(zctx, N, 4242, 0, 0, "chunk 64")


# ---- the transfer pass alone

def _numpy_transfer(spec, N, L, y0, nyl, field, delta, growth):
    """the transfer in the restatement's operation order on rows [y0, y0 + nyl) of [x][y][z'], then the unscaled inverse along x"""
    return torch.fft.ifft(zc.RestatedZeldovichOps.transfer(_Tabs(delta, growth), N, L, torch.from_numpy(spec), y0, nyl, field), dim=0,
                          norm="forward").numpy()


class _Tabs:
    def __init__(self, delta, growth):
        self.tabs = (delta, growth)


@pytest.mark.parametrize("N", [32, 48])
def test_strided_transfer_pass_against_numpy(ctx, N):
    """fft_pass_strided MODE 6 on one rank, no process group: nyl = N / 2 at y0 = 0 and N / 2 (the ky offset), fields 0, 2 and 6 (the
    density factor, a gradient along y from delta, one along z from growth), to 1e-12 of the result's maximum.  The kept spectrum
    must come through untouched (the pass stores out of place)."""
    ops = sd.GpuZeldovichOps(ctx)
    delta, growth = _tables(N)
    ops.tables(N, BOX, delta, growth)
    zpc, Nc, h = ops.pitch(N) // 2, N // 2 + 1, N // 2
    assert zpc >= Nc
    rng = np.random.default_rng(N)
    pad = rng.normal(0, 1, (N, N, zpc)) + 1j * rng.normal(0, 1, (N, N, zpc))
    for y0 in (0, h):
        part = np.ascontiguousarray(pad[:, y0:y0 + h])
        kept = torch.from_numpy(part).cuda()
        for field in (0, 2, 6):
            want = _numpy_transfer(part[:, :, :Nc], N, BOX, y0, h, field, delta, growth)
            out = torch.full_like(kept, float("nan"))
            ops.xtransfer(N, BOX, kept, out, y0, h, field)
            ctx.synchronize()
            got = out.cpu().numpy()[:, :, :Nc]
            err, tol = np.abs(got - want).max(), 1e-12 * np.abs(want).max()
            print(f"N {N} y0 {y0} field {field}: max |diff| {err:.3e}, bar {tol:.3e}")
            assert err <= tol, (N, y0, field, err, tol)
            assert np.array_equal(kept.cpu().numpy(), part)           # only read


# ---- end to end

@pytest.mark.parametrize("case", BESPOKE + TORCH, ids=lambda c: "-".join(map(str, c)))
def test_two_ranks_equal_the_restatement(two_ranks, zctx, case):
    N, size, scaledep = case
    ranks = two_ranks[("case", case, 1)]
    nf = 7 if scaledep else 4
    assert all(r["rows_sent"] > 0 and r["nalltoall"] == 2 + 2 * nf and r["filled"] for r in ranks)
    got = zc.assemble(ranks)
    _compare(got, zc.reference(N, scaledep), "two ranks %s" % (case,))
    if case in BESPOKE:         # the one-rank call on the undivided set: another pass order, so not bits
        delta, growth = _tables(N)
        one = sq.displacement_fields(zctx, zc.particles(N), N, BOX, zc.SEED, delta, growth if scaledep else None, vel_prefac=zc.VEL_PREFAC,
                                     ScaleDepVelocity=scaledep)
        _compare(got, one, "two ranks against the one-rank call %s" % (case,))


def test_bits_do_not_depend_on_the_rank_count_or_the_deal(two_ranks, one_rank):
    for case in BESPOKE:
        a, b, c = (zc.assemble(r[("case", case, how)]) for r, how in ((two_ranks, 1), (one_rank, 1), (two_ranks, 2)))
        for other in (b, c):
            for k in ALL:
                assert np.array_equal(a[k], other[k]), (case, k, int(np.sum(a[k] != other[k])))
        assert np.abs(a["Disp"]).max() > 0


@pytest.mark.parametrize("N", EDGE)
def test_box_edge_on_two_ranks(two_ranks, ctx, N):
    pos = edge_particles()
    ranks = two_ranks[("edge", N)]
    assert len(ranks[0]["idx"]) == 0 and len(ranks[1]["idx"]) == 8
    # x at the edge is cell N, which is cell 0: rank 0's plane 0; of the three inner x only 0.66 lies in rank 1's half
    assert ranks[0]["rows_sent"] == 0 and ranks[1]["rows_sent"] == 7
    delta, growth = edge_tables(N)
    ref = zr.displacement_fields(N, 1.0, zc.SEED, 0, 0, zc.VEL_PREFAC, 1, delta, growth, pos)
    _compare(zc.assemble(ranks), ref, f"N {N} box edge on two ranks", box=1.0)
    # the same particle offered to rank 1's window: refused through the flag, nothing written, nothing read outside the window
    zp = capi.hip.shq_zeldovich_slab_pitch(N) or N + 2
    window = torch.zeros((N // 2 + 1, N, zp), dtype=torch.float64, device="cuda")
    one = torch.from_numpy(pos[3:4].copy()).cuda()
    assert float(one[0, 0]) == np.nextafter(1.0, 0.0)
    out = torch.full((1,), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    rc = capi.hip.shq_zeldovich_slab_gather(ctx.h, N, 1.0, C.c_void_p(one.data_ptr()), 1, C.c_void_p(window.data_ptr()), N // 2, N // 2, N // 2 + 1,
                                            C.c_void_p(out.data_ptr()))
    ctx.synchronize()
    assert rc == ERR_INVALID and float(out[0]) == 7.0
    rc = capi.hip.shq_zeldovich_slab_gather(ctx.h, N, 1.0, C.c_void_p(one.data_ptr()), 1, C.c_void_p(window.data_ptr()), 0, N // 2, N // 2 + 1,
                                            C.c_void_p(out.data_ptr()))
    ctx.synchronize()
    assert rc == 0 and float(out[0]) == 0.0


def test_kept_field_is_reused(two_ranks):
    ranks = two_ranks[("reuse", BESPOKE[0])]
    for r in ranks:
        assert r["a"]["filled"] and not r["b"]["filled"] and r["fresh"]["filled"] and r["c"]["filled"]
    a, b, fresh, c = (zc.assemble([r[k] for r in ranks]) for k in ("a", "b", "fresh", "c"))
    for k in ALL:
        assert np.array_equal(b[k], fresh[k]), k
    assert not np.array_equal(a["Disp"], b["Disp"]) and not np.array_equal(b["Disp"], c["Disp"])
    N, _, scaledep = BESPOKE[0]
    _compare(b, zc.reference(N, scaledep, other=True), "second species")
    _compare(c, zc.reference(N, scaledep, other=True, seed=zc.SEED + 1), "another seed")


# ---- no interference

class _forced_group:
    """a one-rank gloo group under SHQ_COMM_FORCE=1, so that DistZeldovich runs every collective inside this process"""

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


def _slab_phases(ctx, N, scaledep=1):
    """a full set of slab phases on the context: fill, tables, and per field the transfer pass, the Y/Z inverse and the gather"""
    drv = sd.DistZeldovich(sd.Comm(), N, BOX, sd.GpuZeldovichOps(ctx))
    assert drv.comm.multi and drv.comm.size == 1
    delta, growth = _tables(N)
    got = drv.displacements(zc.params(N, scaledep), delta, growth, zc.particles(N))
    assert drv.filled and drv.nalltoall == 2 + 7 and np.abs(got["Disp"]).max() > 0
    return got


def test_no_interference_with_a_pending_spectrum(zctx):
    """test_gpu_dist_uvbg's check: DistZeldovich under SHQ_COMM_FORCE=1 between shq_pm_forward and shq_pm_run, at the PM's own mesh
    size (its twiddles) and at another"""
    ctx = zctx
    n, L, nmesh = 40000, cm.BOX, 48
    pos = cm.random_positions(np.random.default_rng(3).random(3 * n), n)
    pman = cm.make_partmanager(pos)
    pmp = sq.PMParams(nmesh, 0, L, 1.5, cm.G)
    T = 1.0 + 0.3 * np.exp(-np.arange(3 * (nmesh // 2) ** 2 + 1) / 36.0)
    capi.check(capi.hip.shq_pm_set_deposit_log2scale(ctx.h, 40))
    calls = []

    def run(with_zel):
        pv = pman.view()
        capi.check(capi.hip.shq_particles_upload(ctx.h, C.byref(pv)))
        capi.check(capi.hip.shq_pm_forward(ctx.h, C.byref(pmp)))
        z0 = C.c_int(-1)
        capi.check(capi.hip.shq_pm_mesh_prezeroed(ctx.h, C.byref(z0)))
        if with_zel:
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
    a = sq.displacement_fields(zctx, pos, N, BOX, 11, delta)
    assert a["phase_ms"][0] > 0
    with _forced_group():
        _slab_phases(zctx, N)           # the same mesh size, another seed
        _slab_phases(zctx, 16)
    b = sq.displacement_fields(zctx, pos, N, BOX, 11, delta)
    assert b["phase_ms"][0] == 0
    for k in ("Pos", "Vel", "Density", "Disp"):
        assert np.array_equal(a[k], b[k]), k
