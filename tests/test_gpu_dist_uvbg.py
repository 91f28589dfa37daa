"""GPU tests of the sharded excursion-set reionisation (shenqi_amd/dist.py:DistUVBG with GpuUvbgOps on shq_uvbg_slab_*).

Two gloo ranks share the one GPU.  The reference is uvbg_restated.calculate_uvbg on the undivided set under the rules of
test_parity_with_the_restatement (uvbg_dist_cases.compare).  On the bespoke route the grids and every particle's results must also be
the SAME BITS whatever the rank count and whoever held which particle at the start: the deposit is fixed point with scales from the
global sums, a mesh line sees the same kernel arithmetic on any rank, and every host makes the same filter tables.  The sharded phases
must leave the PM's state alone, and the strided filter pass (fft_pass_strided MODE 5) is held to numpy on its own."""
import ctypes as C
import os
import pickle
import sys
import tempfile

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
import uvbg_dist_cases as uc  # noqa: E402
import uvbg_restated as ur  # noqa: E402
from test_gpu_uvbg import COSMO, _params, _structs, uctx  # noqa: E402,F401

pytestmark = pytest.mark.gpu

# two ranks: the cut of the 64 case moves to plane 32
BESPOKE = [(32, 2, 0, 0, 0), (48, 2, 2, 0, 1), (64, 2, 1, 0, 0)]
TORCH = [(36, 2, 2, 0, 1)]


def _worker(rank, world, initfile, outdir, jobs):
    os.environ["OMP_NUM_THREADS"] = "2"
    if world == 1:
        os.environ["SHQ_COMM_FORCE"] = "1"          # one rank that still runs every collective
    dist.init_process_group("gloo", init_method="file://" + initfile, rank=rank, world_size=world)
    try:
        with sq.Context(0) as ctx:
            ops = sd.GpuUvbgOps(ctx)
            comm = sd.Comm()
            assert comm.multi
            res = [uc.run_rank(comm, ops, case, how=how) for case, how in jobs]
        with open(os.path.join(outdir, "r%d.pkl" % rank), "wb") as f:
            pickle.dump(res, f)
    finally:
        dist.destroy_process_group()


def spawn(world, jobs):
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_worker, args=(world, os.path.join(tmp, "init"), tmp, jobs), nprocs=world, join=True)
        results = []
        for r in range(world):
            with open(os.path.join(tmp, "r%d.pkl" % r), "rb") as f:
                results.append(pickle.load(f))
        return {job: uc.assemble([results[r][j] for r in range(world)], job[0][0]) for j, job in enumerate(jobs)}


@pytest.fixture(scope="module")
def two_ranks():
    """every case on two ranks, the bespoke ones also with the particles dealt to the ranks in another order: one spawn"""
    return spawn(2, [(c, 1) for c in BESPOKE + TORCH] + [(c, 2) for c in BESPOKE])


@pytest.mark.parametrize("case", BESPOKE + TORCH, ids=lambda c: "-".join(map(str, c)))
def test_two_ranks_equal_the_restatement(two_ranks, case):
    N, size = case[0], case[1]
    ref = uc.reference(*case)
    uc.assert_coverage(ref, N, size)
    uc.compare(two_ranks[(case, 1)], ref, N, size)


def test_bits_do_not_depend_on_the_rank_count_or_the_deal(two_ranks):
    one = spawn(1, [(c, 1) for c in BESPOKE])
    for case in BESPOKE:
        a, b, c = two_ranks[(case, 1)], one[(case, 1)], two_ranks[(case, 2)]
        for other in (b, c):
            for k in ("J21", "xHI", "fesc", "local_J21", "zreion"):
                assert np.array_equal(a[k], other[k]), (case, k, int(np.sum(a[k] != other[k])))
            assert a["nradii"] == other["nradii"]
            assert abs(a["vol"] - other["vol"]) <= 1e-12 and abs(a["mass"] - other["mass"]) <= 1e-12      # summed in another order
        assert (a["J21"] > 0).any() and (a["zreion"] != uc.particles(case[0], case[1])[6]).any()


def test_no_interference_with_a_pending_spectrum(uctx):
    """test_gpu_uvbg's check at its sizes, with DistUVBG under SHQ_COMM_FORCE=1 between shq_pm_forward and shq_pm_run"""
    ctx = uctx
    n, L, nmesh = 40000, cm.BOX, 48
    pos = cm.random_positions(np.random.default_rng(3).random(3 * n), n)
    pman = cm.make_partmanager(pos)
    types = np.where(np.arange(n) % 7 == 0, 4, np.where(np.arange(n) % 2 == 0, 0, 1)).astype(np.uint8)
    pman.Base["Type"] = types
    pmp = sq.PMParams(nmesh, 0, L, 1.5, cm.G)
    T = 1.0 + 0.3 * np.exp(-np.arange(3 * (nmesh // 2) ** 2 + 1) / 36.0)
    capi.check(capi.hip.shq_pm_set_deposit_log2scale(ctx.h, 40))
    rng = np.random.default_rng(2)
    up, uc_ = _structs(_params(32, 0, 0, 1, BoxSize=L, ReionRBubbleMax=L, ReionRBubbleMin=L / 100), COSMO)
    calls = []

    def uvbg():
        drv = sd.DistUVBG(sd.Comm(), 32, L, sd.GpuUvbgOps(ctx))
        assert drv.comm.multi and drv.comm.size == 1
        lj, zr = np.zeros(n), np.full(n, -1.0)
        calls.append(drv.calculate(up, uc_, pos, np.asarray(pman.Base["Mass"]), types, rng.uniform(0, 5, n), rng.uniform(0, 1, n), lj, zr))
        assert drv.nalltoall > 2 * drv.nradii and (lj > 0).any()

    def run(with_uvbg):
        pv = pman.view()
        capi.check(capi.hip.shq_particles_upload(ctx.h, C.byref(pv)))
        capi.check(capi.hip.shq_pm_forward(ctx.h, C.byref(pmp)))
        z0 = C.c_int(-1)
        capi.check(capi.hip.shq_pm_mesh_prezeroed(ctx.h, C.byref(z0)))
        if with_uvbg:
            uvbg()
            z1 = C.c_int(-1)
            capi.check(capi.hip.shq_pm_mesh_prezeroed(ctx.h, C.byref(z1)))
            assert z1.value == z0.value
            assert capi.hip.shq_pm_get_deposit_log2scale(ctx.h) == 40
        capi.check(capi.hip.shq_pm_set_mode_factor(ctx.h, nmesh, capi.ptr(T)))
        capi.check(capi.hip.shq_pm_run(ctx.h, C.byref(pmp)))
        g = np.zeros((n, 3)); pp = np.zeros(n)
        capi.check(capi.hip.shq_pm_download(ctx.h, capi.ptr(g), capi.ptr(pp)))
        return g, pp

    ref = run(False)
    before = os.environ.get("SHQ_COMM_FORCE")
    os.environ["SHQ_COMM_FORCE"] = "1"
    with tempfile.TemporaryDirectory() as tmp:
        dist.init_process_group("gloo", init_method="file://" + os.path.join(tmp, "init"), rank=0, world_size=1)
        try:
            got = run(True)
        finally:
            dist.destroy_process_group()
            if before is None:
                del os.environ["SHQ_COMM_FORCE"]
            else:
                os.environ["SHQ_COMM_FORCE"] = before
    assert len(calls) == 1
    assert np.array_equal(ref[0], got[0]) and np.array_equal(ref[1], got[1])


@pytest.mark.parametrize("N", [32, 48])
def test_strided_filter_pass_against_numpy(ctx, N):
    """fft_pass_strided MODE 5 on one rank, no process group: the kept spectrum of a field, the pass with nyl = N and with nyl = N / 2
    at y0 = 0 and N / 2 (the ky offset), then the Y/Z inverse, against numpy's irfftn of the spectrum times the same table over ncell
    to 1e-12 of the field's maximum.  The kept spectrum must come through untouched (the pass stores out of place)."""
    L = 20000.0
    ops = sd.GpuUvbgOps(ctx)
    p, _ = _structs(_params(N, 0), COSMO)
    radii = sd.uvbg_radii(p)
    ops.tables(p, radii)
    zp = ops.pitch()
    zpc, Nc = zp // 2, N // 2 + 1
    assert zp > 0
    field = np.random.default_rng(N).normal(1.0, 0.5, (N, N, N))
    spec = np.fft.rfftn(field)                                     # [x][y][z']
    pad = np.zeros((N, N, zpc), dtype=np.complex128)
    pad[:, :, :Nc] = spec
    pad[:, :, Nc:] = 7.0 - 3.0j                                    # a pad column must not reach the result
    k1 = np.fft.fftfreq(N, 1.0 / N).astype(np.int64)
    k2 = k1[:, None, None] ** 2 + k1[None, :, None] ** 2 + np.arange(Nc)[None, None, :] ** 2

    def yz_inverse(planes):
        ops.fft_yz(planes, N, 1, 0, None, 1)
        ctx.synchronize()
        return planes.view(torch.float64).cpu().numpy()[:, :, :N]

    for r in (3, len(radii) - 1):
        Tk = np.ones(k2.shape) if r == len(radii) - 1 else ur.filter_table(0, N, L, radii[r])[k2]
        want = np.fft.irfftn(spec * Tk / (N * N * N), s=(N, N, N), axes=(0, 1, 2), norm="forward")
        tol = 1e-12 * np.abs(want).max()
        kept = torch.from_numpy(pad).cuda()
        whole = torch.empty_like(kept)
        ops.xfilter(kept, whole, 0, N, r)
        halves = torch.empty_like(kept)
        h = N // 2
        for y0 in (0, h):
            part = kept[:, y0:y0 + h].contiguous()
            out = torch.full_like(part, float("nan"))
            ops.xfilter(part, out, y0, h, r)
            ctx.synchronize()
            assert torch.equal(part, kept[:, y0:y0 + h])           # only read
            halves[:, y0:y0 + h] = out
        ctx.synchronize()
        assert torch.equal(kept.cpu(), torch.from_numpy(pad))
        assert torch.equal(whole[:, :, :Nc], halves[:, :, :Nc])     # a line's arithmetic does not depend on the slab it is in
        for got in (yz_inverse(whole), yz_inverse(halves)):
            assert np.abs(got - want).max() <= tol, (N, r, np.abs(got - want).max(), tol)
