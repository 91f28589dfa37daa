"""GPU tests of the sharded slab PM with a global_analysis hook (MassiveNuLinRespOn: the P(k) sums all-reduced over the ranks, the
hook's factor T[k2] in front of the Green's function) and the hybrid-neutrino deposit type mask, on the one-GPU box: one rank in
process, two and three gloo ranks sharing the GPU, and a one-rank RCCL group with the collectives forced.  The reference result is the
single-GPU route shq_pm_forward -> shq_pm_set_mode_factor -> shq_pm_run on the whole particle set."""
import ctypes as C
import math
import os
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

from test_dist_neutrino_cpu import nu_table  # noqa: E402

pytestmark = pytest.mark.gpu

NPART, BOX, G, ASMTH = 16**3, 8.0, 43.0071, 1.5
ERR_INVALID, ERR_STATE = 1, 4
ALL_TYPES = -1
NO_TYPE2 = ALL_TYPES & ~(1 << 2)


def _global_particles():
    import orc
    import common as cm
    pos = cm.random_positions(orc.boost_mt19937_uniform(0, 3 * NPART), NPART)
    return np.concatenate([pos, np.ones((NPART, 1))], axis=1)


def _global_types():
    t = np.ones(NPART, dtype=np.int64)
    t[3::8] = 2                                           # about 1/8 hybrid-neutrino tracers
    return t


def _ones(N):
    return np.ones(3 * (N // 2) ** 2 + 1)


def _pm_rank(rank, world, outdir, nmesh, split=False):
    """one rank of the sharded PM: plain, T = 1, measure-power only, a real T with the finish's sums, and the masked deposit"""
    import shenqi_amd as sq
    from shenqi_amd import dist as sd
    dev = torch.device("cuda", 0)
    comm = sd.Comm()
    posm_g, types_g = _global_particles(), _global_types()
    mine = torch.from_numpy(posm_g[rank::world].copy()).to(dev)
    mine_t = torch.from_numpy(types_g[rank::world].copy()).to(dev)
    ctx = sq.Context(0)
    try:
        bounds = sd.balanced_bounds(comm, nmesh, BOX, mine[:, 0]) if world == 2 else None
        ycuts = [0.0, 5.06, 0.0] if split else None
        ops = sd.GpuOps(ctx, nmesh, BOX, ASMTH, G, dev)
        pm = sd.SlabPM(comm, nmesh, BOX, ASMTH, G, ops, bounds, ycuts)
        local, ltypes = sd.exchange_to_owner(comm, pm.d, mine, types=mine_t)
        nloc = int(local.shape[0])
        ops.set_deposit_scale(comm.allreduce_sum(float(local[:, 3].sum().item())))
        ops.set_particles(local, nloc, types=ltypes)
        T = nu_table(nmesh)
        res = {"local": local.cpu().numpy(), "types": ltypes.cpu().numpy()}

        def run(name, **kw):
            pm.force(**kw)
            g, p = ops.results(nloc)
            res[name] = np.concatenate([g, p[:, None]], axis=1)
            res[name + "_power"], res[name + "_finish"] = pm.power, pm.power_finish

        run("plain")
        run("one", analysis=lambda kk, power, nmodes, norm: _ones(nmesh))
        run("measure", measure_power=True)
        run("nu", analysis=lambda kk, power, nmodes, norm: T, measure_power=True)
        ops.set_deposit_types(NO_TYPE2)
        run("masked", analysis=lambda kk, power, nmodes, norm: T)
        run("masked_plain")
        ops.set_deposit_types(ALL_TYPES)
        np.save(os.path.join(outdir, "pm%d.npy" % rank), np.array([res], dtype=object), allow_pickle=True)
    finally:
        ctx.close()


def _pm_worker(rank, world, initfile, outdir, nmesh, backend="gloo", split=False):
    os.environ["OMP_NUM_THREADS"] = "2"
    if backend == "nccl":
        os.environ["SHQ_COMM_FORCE"] = "1"
        os.environ["SHQ_COMM_MAX_MSG"] = "300000"   # the spectrum goes as several row-chunked rounds
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", init_method="file://" + initfile, rank=rank, world_size=world,
                                device_id=torch.device("cuda", 0))
    else:
        dist.init_process_group(backend, init_method="file://" + initfile, rank=rank, world_size=world)
    try:
        _pm_rank(rank, world, outdir, nmesh, split)
    finally:
        dist.destroy_process_group()


def _single_gpu(ctx, nmesh, T, mask=ALL_TYPES):
    """the single-GPU neutrino route on the whole set: forward, its sums, the table, the measuring finish"""
    import shenqi_amd as sq
    from shenqi_amd import capi
    import common as cm
    posm, types = _global_particles(), _global_types()
    h = ctx.h
    e = 61 - math.frexp(float(posm[:, 3].sum()))[1]
    capi.check(capi.hip.shq_pm_set_deposit_log2scale(h, e))
    try:
        pman = cm.make_partmanager(posm[:, :3].copy())
        pman.Base["Mass"] = posm[:, 3]
        pman.Base["Type"] = types
        pv = pman.view()
        capi.check(capi.hip.shq_particles_upload(h, C.byref(pv)))
        capi.check(capi.hip.shq_pm_set_deposit_types(h, mask))
        pmp = sq.PMParams(nmesh, 0, BOX, ASMTH, G)

        def power():
            kk, pw, nm, norm = np.zeros(nmesh), np.zeros(nmesh), np.zeros(nmesh, dtype=np.int64), C.c_double()
            capi.check(capi.hip.shq_pm_download_power(h, nmesh, capi.ptr(kk), capi.ptr(pw), capi.ptr(nm), C.byref(norm)))
            return kk, pw, nm, norm.value

        capi.check(capi.hip.shq_pm_forward(h, C.byref(pmp)))
        dens = power()
        capi.check(capi.hip.shq_pm_measure_power(h, 1))
        capi.check(capi.hip.shq_pm_set_mode_factor(h, nmesh, capi.ptr(np.ascontiguousarray(T))))
        capi.check(capi.hip.shq_pm_run(h, C.byref(pmp)))
        fin = power()
        g, p = np.zeros((NPART, 3)), np.zeros(NPART)
        capi.check(capi.hip.shq_pm_download(h, capi.ptr(g), capi.ptr(p)))
        return np.concatenate([g, p[:, None]], axis=1), dens, fin
    finally:
        capi.check(capi.hip.shq_pm_measure_power(h, 0))
        capi.check(capi.hip.shq_pm_set_mode_factor(h, 0, None))
        capi.check(capi.hip.shq_pm_set_deposit_types(h, ALL_TYPES))
        capi.check(capi.hip.shq_pm_set_deposit_log2scale(h, -1))


def _close(a, b, tol):
    return np.abs(a - b).max() <= tol * np.abs(b).max()


def _sums_close(got, want, tol=1e-12):
    kk, pw, nm, norm = got
    wkk, wpw, wnm, wnorm = want
    assert np.array_equal(np.asarray(nm, np.int64), np.asarray(wnm, np.int64))
    assert _close(kk, wkk, tol) and _close(pw, wpw, tol)
    assert abs(norm - wnorm) <= tol * abs(wnorm)


def _check_pm(ctx, outdir, world, nmesh, bespoke):
    outs = [np.load(os.path.join(outdir, "pm%d.npy" % r), allow_pickle=True)[0] for r in range(world)]
    posm_g, types_g = _global_particles(), _global_types()
    key = {tuple(p): i for i, p in enumerate(map(tuple, posm_g[:, :3]))}
    idx = np.concatenate([[key[tuple(p)] for p in o["local"][:, :3]] for o in outs]).astype(np.int64)
    assert len(idx) == NPART and len(set(idx.tolist())) == NPART
    assert np.array_equal(np.concatenate([o["types"] for o in outs]), types_g[idx])     # types travelled with their rows
    res = {k: np.concatenate([o[k] for o in outs]) for k in ("plain", "one", "measure", "nu", "masked", "masked_plain")}
    # the reduced sums are the same on every rank
    for name in ("one", "measure", "nu", "masked"):
        for which in ("_power", "_finish"):
            for o in outs[1:]:
                if outs[0][name + which] is None:
                    assert o[name + which] is None
                else:
                    assert all(np.array_equal(a, b) for a, b in zip(o[name + which], outs[0][name + which]))
    # T = 1: the plain sharded run's bits on the bespoke route up to Nmesh 128; above, the split and the fused pass compile to arithmetic
    # that may round differently (2e-15 relative at 768)
    for name in ("one", "measure"):
        if bespoke and nmesh <= 128:
            assert np.array_equal(res[name], res["plain"])
        else:
            assert _close(res[name], res["plain"], 1e-14 if bespoke else 1e-12)
    T = nu_table(nmesh)
    ref, dens, fin = _single_gpu(ctx, nmesh, T)
    assert _close(res["nu"], ref[idx], 1e-12)
    _sums_close(outs[0]["nu_power"], dens)
    _sums_close(outs[0]["nu_finish"], fin)
    _sums_close(outs[0]["one_power"], dens)
    _sums_close(outs[0]["measure_finish"], dens)             # T = 1: the finish's sums are the density's
    assert not _close(res["nu"], res["plain"], 1e-3)
    # deposit mask: the single-GPU masked route; tracers still receive GravPM; the mask changes the result
    mref, mdens, _ = _single_gpu(ctx, nmesh, T, NO_TYPE2)
    assert _close(res["masked"], mref[idx], 1e-12)
    _sums_close(outs[0]["masked_power"], mdens)
    tr = types_g[idx] == 2
    assert np.abs(res["masked"][tr, :3]).max() > 0
    assert not _close(res["masked"], res["nu"], 1e-3)
    mplain, _, _ = _single_gpu(ctx, nmesh, _ones(nmesh), NO_TYPE2)
    assert _close(res["masked_plain"], mplain[idx], 1e-12)


@pytest.mark.parametrize("nmesh,bespoke", [(48, True), (128, True), (384, True), (36, False)])
def test_sharded_neutrino_pm_single_rank(ctx, nmesh, bespoke):
    """one rank in process, as test_dist_driver_single_rank: the split X pass (fft_pass_strided MODES 3, 4) on the bespoke route, the
    P(k) sweep and the Green's kernel with a table on the torch route (Nmesh 36 has no bespoke transform).  At 384 the pass's persistent
    workgroups take several tiles each, as on every production mesh: the X pass has 384 x 49 = 18816 tiles, the grid at most 8 x the
    resident workgroups (<= 8 per CU x 256 CUs), 16384."""
    with tempfile.TemporaryDirectory() as tmp:
        _pm_rank(0, 1, tmp, nmesh)
        _check_pm(ctx, tmp, 1, nmesh, bespoke)


def test_sharded_neutrino_pm_tile_loop(ctx, monkeypatch):
    """SHQ_FFT_GRID_MUL=1: the grid is the resident workgroups only (<= 8 per CU x 256 CUs = 2048; 4 per CU at these passes' register
    counts) for the 128 x 17 = 2176 X-pass tiles of a 128 mesh, so the workgroups of MODES 3 and 4 go round their tile loop: the next
    tile's T gather, the LDS reused across tiles, a histogram of several tiles before its flush.  Forces, both sets of sums and nmodes against the single-GPU route with a real T, and
    the T = 1 bits of the plain run."""
    monkeypatch.setenv("SHQ_FFT_GRID_MUL", "1")
    with tempfile.TemporaryDirectory() as tmp:
        _pm_rank(0, 1, tmp, 128)
        _check_pm(ctx, tmp, 1, 128, True)


def test_sharded_neutrino_pm_torch_fft_knob(ctx, monkeypatch):
    """SHQ_SLAB_TORCH_FFT=1 sends a bespoke mesh size through the torch route: the same results within 1e-12"""
    monkeypatch.setenv("SHQ_SLAB_TORCH_FFT", "1")
    with tempfile.TemporaryDirectory() as tmp:
        _pm_rank(0, 1, tmp, 48)
        _check_pm(ctx, tmp, 1, 48, False)


@pytest.mark.parametrize("world,nmesh,split", [(2, 48, False), (2, 48, True), (3, 48, False)])
def test_sharded_neutrino_pm_gloo_ranks(ctx, world, nmesh, split):
    """two ranks plane-aligned and cut below the plane (ycuts), three ranks: the reduced sums are the same on every rank and those of
    the single-GPU route on the whole set; the forces too; T = 1 keeps the plain sharded run's bits"""
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_pm_worker, args=(world, os.path.join(tmp, "init"), tmp, nmesh, "gloo", split), nprocs=world, join=True)
        _check_pm(ctx, tmp, world, nmesh, True)


def test_sharded_neutrino_pm_one_rccl_rank_collectives_forced(ctx):
    """the real collectives (RCCL transposes in row-chunked rounds, the vector all-reduce on the device) and the fused pack / unpack"""
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_pm_worker, args=(1, os.path.join(tmp, "init"), tmp, 48, "nccl"), nprocs=1, join=True)
        _check_pm(ctx, tmp, 1, 48, True)


def test_slab_deposit_mask_and_types_errors(ctx):
    """a mask other than all types on a device set without types is SHQ_ERR_STATE on every slab deposit; a types array of the wrong
    length is SHQ_ERR_INVALID; shq_particles_set_device resets the types"""
    from shenqi_amd import capi
    h = ctx.h
    posm = torch.from_numpy(_global_particles()[:2000].copy()).to("cuda:0")
    types = torch.full((2000,), 2, dtype=torch.uint8, device="cuda:0")
    N = 48
    pm = capi.PMParams(N, 0, BOX, ASMTH, G)
    zp = int(capi.hip.shq_pm_slab_pitch(N))
    mesh2 = torch.zeros((N, N, zp), dtype=torch.int64, device="cuda:0")
    mesh = torch.zeros((N, N, N + 2), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    capi.check(capi.hip.shq_pm_set_deposit_log2scale(h, 40))
    try:
        capi.check(capi.hip.shq_particles_set_device(h, C.c_void_p(posm.data_ptr()), 2000, 2000, 0))
        capi.check(capi.hip.shq_pm_set_deposit_types(h, NO_TYPE2))
        assert capi.hip.shq_pm_slab2_deposit(h, C.byref(pm), 0, N, 0, N, C.c_void_p(mesh2.data_ptr())) == ERR_STATE
        assert capi.hip.shq_pm_slab2_deposit_ghosts(h, C.byref(pm), 0, N, 0, N, 1, C.c_void_p(mesh2.data_ptr())) == ERR_STATE
        assert capi.hip.shq_pm_slab_deposit(h, C.byref(pm), 0, N, C.c_void_p(mesh.data_ptr())) == ERR_STATE
        assert capi.hip.shq_particles_set_device_types(h, C.c_void_p(types.data_ptr()), 1999) == ERR_INVALID
        # every row Type 2 and Type 2 left out: nothing is deposited
        capi.check(capi.hip.shq_particles_set_device_types(h, C.c_void_p(types.data_ptr()), 2000))
        capi.check(capi.hip.shq_pm_slab2_deposit(h, C.byref(pm), 0, N, 0, N, C.c_void_p(mesh2.data_ptr())))
        ctx.synchronize()
        assert int(mesh2.abs().sum().item()) == 0
        # a new set is Type 1 again (and without types): refused under the mask, deposited under all types
        capi.check(capi.hip.shq_particles_set_device(h, C.c_void_p(posm.data_ptr()), 2000, 2000, 0))
        assert capi.hip.shq_pm_slab2_deposit(h, C.byref(pm), 0, N, 0, N, C.c_void_p(mesh2.data_ptr())) == ERR_STATE
        capi.check(capi.hip.shq_pm_set_deposit_types(h, ALL_TYPES))
        capi.check(capi.hip.shq_pm_slab2_deposit(h, C.byref(pm), 0, N, 0, N, C.c_void_p(mesh2.data_ptr())))
        ctx.synchronize()
        assert int(mesh2.sum().item()) > 0
        # slab X calls on a mesh size without a bespoke transform are refused
        spec = torch.zeros((36, 1, 20), dtype=torch.complex128, device="cuda:0")
        pm36 = capi.PMParams(36, 0, BOX, ASMTH, G)
        assert capi.hip.shq_pm_slab2_xforward(h, C.byref(pm36), C.c_void_p(spec.data_ptr()), 0, 1) == ERR_INVALID
    finally:
        capi.check(capi.hip.shq_pm_set_deposit_types(h, ALL_TYPES))
        capi.check(capi.hip.shq_pm_set_deposit_log2scale(h, -1))


# ---- end to end: DistTreePM with types, a deposit mask and the analysis hook -------------------------------------------------
def _tree_rank(rank, world, outdir):
    import shenqi_amd as sq
    from shenqi_amd import dist as sd
    import common as cm
    dev = torch.device("cuda", 0)
    comm = sd.Comm()
    N = 48
    posm_g, types_g = _global_particles(), _global_types()
    mine = torch.from_numpy(posm_g[rank::world].copy()).to(dev)
    mine_t = torch.from_numpy(types_g[rank::world].copy()).to(dev)
    T = nu_table(N)
    cm.reference_treepar(ErrTolForceAcc=0.005, MaxBHOpeningAngle=0.9, Rcut=6.0, TreeUseBH=1)
    sq.gravshort_set_softenings(BOX / np.cbrt(NPART))
    gp_bh = sq.make_grav_params(BOX, ASMTH, N, G, cm.RHO0)
    cm.reference_treepar(ErrTolForceAcc=0.005, MaxBHOpeningAngle=0.9, Rcut=6.0, TreeUseBH=0)
    gp = sq.make_grav_params(BOX, ASMTH, N, G, cm.RHO0)
    bounds = sd.balanced_bounds(comm, N, BOX, mine[:, 0])
    res = {}
    for overlap in (True, False):
        ctx = sq.Context(0)
        try:
            drv = sd.DistTreePM(comm, ctx, N, BOX, ASMTH, G, dev, halo_factor=1.3, bounds=bounds)
            local, ltypes = sd.exchange_to_owner(comm, drv.decomp, mine, types=mine_t)
            drv.setup(local, gp.Rcut, types=ltypes)
            drv.ops.set_deposit_types(NO_TYPE2)
            drv.step(gp_bh, overlap=overlap, analysis=lambda *s: T)
            bh = drv.download()
            drv.step(gp, overlap=overlap, analysis=lambda *s: T, measure_power=True)
            acc, pot, gpm, ppot = drv.download()
            assert int(drv.types.shape[0]) == int(drv.allp.shape[0])
            res[overlap] = np.concatenate([drv.local.cpu().numpy(), drv.local_types.cpu().numpy()[:, None].astype(np.float64),
                                           bh[0], acc, gpm, ppot[:, None]], axis=1)
            res["power%d" % overlap] = drv.pm.power_finish
            # ghosts carry their owner's type
            gh = drv.allp[drv.nloc:].cpu().numpy()
            key = {tuple(p): i for i, p in enumerate(map(tuple, posm_g[:, :3]))}
            gidx = np.array([key[tuple(p)] for p in gh[:, :3]], dtype=np.int64)
            assert np.array_equal(drv.types[drv.nloc:].cpu().numpy().astype(np.int64), types_g[gidx])
        finally:
            ctx.close()
    np.save(os.path.join(outdir, "t%d.npy" % rank), np.array([res], dtype=object), allow_pickle=True)


def _tree_worker(rank, world, initfile, outdir):
    os.environ["OMP_NUM_THREADS"] = "2"
    dist.init_process_group("gloo", init_method="file://" + initfile, rank=rank, world_size=world)
    try:
        _tree_rank(rank, world, outdir)
    finally:
        dist.destroy_process_group()


def test_dist_treepm_types_mask_analysis_two_gloo_ranks(ctx):
    """DistTreePM with types, the mask without Type 2 and the analysis hook: the PM part is the single-GPU masked neutrino route's, the
    walk meets test_gpu_dist's oracle bar (relative criterion, OldAcc from this very PM), and overlap on / off give the same bits"""
    import orc
    import common as cm
    import shenqi_amd as sq
    world, N = 2, 48
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_tree_worker, args=(world, os.path.join(tmp, "init"), tmp), nprocs=world, join=True)
        outs = [np.load(os.path.join(tmp, "t%d.npy" % r), allow_pickle=True)[0] for r in range(world)]
    for o in outs:
        assert np.array_equal(o[True], o[False])
        _sums_close(o["power1"], o["power0"])          # floating-point atomics: the sums agree to rounding, nmodes exactly
    rows = np.concatenate([o[True] for o in outs])
    posm_g, types_g = _global_particles(), _global_types()
    key = {tuple(p): i for i, p in enumerate(map(tuple, posm_g[:, :3]))}
    idx = np.array([key[tuple(p)] for p in rows[:, :3]], dtype=np.int64)
    assert len(idx) == NPART and len(set(idx.tolist())) == NPART
    assert np.array_equal(rows[:, 4].astype(np.int64), types_g[idx])
    mref, _, _ = _single_gpu(ctx, N, nu_table(N), NO_TYPE2)
    gpm = rows[:, 11:14]
    assert np.abs(gpm - mref[idx, :3]).max() <= 1e-12 * np.abs(mref[:, :3]).max()
    assert np.abs(rows[:, 14] - mref[idx, 3]).max() <= 1e-12 * np.abs(mref[:, 3]).max()
    # the walk: the oracle's BH pass, then its relative-criterion pass with OldAcc from the BH pass and this PM
    pos, mass = posm_g[:, :3].copy(), posm_g[:, 3].astype(np.float32)
    nodes, first, _ = orc.tree_build(pos, mass, BOX)
    cm.reference_treepar(ErrTolForceAcc=0.005, MaxBHOpeningAngle=0.9, Rcut=6.0, TreeUseBH=1)
    sq.gravshort_set_softenings(BOX / np.cbrt(NPART))
    gp_bh = sq.make_grav_params(BOX, ASMTH, N, G, cm.RHO0)
    a1, _, _ = orc.grav_walk(nodes, first, pos, mass, np.zeros(NPART), gp_bh)
    cm.reference_treepar(ErrTolForceAcc=0.005, MaxBHOpeningAngle=0.9, Rcut=6.0, TreeUseBH=0)
    gp = sq.make_grav_params(BOX, ASMTH, N, G, cm.RHO0)
    a2, _, _ = orc.grav_walk(nodes, first, pos, mass, np.linalg.norm(a1 * G + mref[:, :3], axis=1) / G, gp)
    oacc = a2 * G
    rms = np.sqrt(np.sum((rows[:, 8:11] - oacc[idx]) ** 2) / np.sum(oacc[idx] ** 2))
    print("DistTreePM with types, mask and analysis, 2 ranks: tree rms vs oracle %.3e" % rms)
    assert rms < 1e-3
    cm.reference_treepar()


def test_slab_power_state(ctx):
    """the sums a slab X call leaves are readable until the particle set changes (then SHQ_ERR_STATE again); GpuOps' finish leaves the
    caller's shq_pm_measure_power setting as it found it"""
    from shenqi_amd import capi, dist as sd
    h = ctx.h
    N = 48
    posm = torch.from_numpy(_global_particles()[:2000].copy()).to("cuda:0")
    torch.cuda.synchronize()
    capi.check(capi.hip.shq_particles_set_device(h, C.c_void_p(posm.data_ptr()), 2000, 2000, 0))
    ops = sd.GpuOps(ctx, N, BOX, ASMTH, G, torch.device("cuda", 0))
    zpc = ops.pitch() // 2
    spec = torch.zeros((N, N, zpc), dtype=torch.complex128, device="cuda:0")
    spec[0, 0, 0] = 3.0                                   # x = 0 of the (ky, kz) = 0 line: 3 on every kx, Norm = 9
    kk, pw, nm, norm = ops.xforward(spec, 0, N)
    assert norm == 9.0 and nm.sum() > 0 and pw.sum() > 0
    assert ops.power()[3] == 9.0
    try:
        for setting in (1, 0):
            capi.check(capi.hip.shq_pm_measure_power(h, setting))
            for measure in (False, True):
                ops.xfinish(spec, 0, N, None, measure)
                assert capi.hip.shq_pm_get_measure_power(h) == setting
        capi.check(capi.hip.shq_pm_measure_power(h, 1))
        ops.xforward(spec, 0, N)
        capi.check(capi.hip.shq_particles_set_device(h, C.c_void_p(posm.data_ptr()), 2000, 2000, 0))
        kk, pw, nm, norm = np.zeros(N), np.zeros(N), np.zeros(N, dtype=np.int64), C.c_double()
        assert capi.hip.shq_pm_download_power(h, N, capi.ptr(kk), capi.ptr(pw), capi.ptr(nm), C.byref(norm)) == ERR_STATE
    finally:
        capi.check(capi.hip.shq_pm_measure_power(h, 0))
