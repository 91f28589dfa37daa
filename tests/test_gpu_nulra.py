"""Linear-response neutrinos on the device (csrc/nulra.hip): the device step against the host engine (tests/test_nulra_cpu.py checks that
one against an independent restatement), inside the PM between shq_pm_forward and the finish, and as the analysis hook of a two-rank
DistTreePM step."""
import ctypes as C
import os
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import shenqi_amd as sq  # noqa: E402
from shenqi_amd import capi  # noqa: E402
import nulra_cases as nc  # noqa: E402

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_DEVICE, ERR_STATE = 1, 2, 4
KEYS = ("scalefact", "delta_tot", "delta_nu_init", "kvalue", "delta_nu_last")


def _one_step(nu, st, Time):
    """the history st, then a step at Time on 12 bins k = 2 .. 10, which the state's 10 bins k = 0.01 .. 100 are rebinned from and to"""
    k, nm = nc.bins(12)
    nu.set_state(st)
    raw = nu.delta_nu(float(np.exp(st["scalefact"][-1])))
    nu.step(Time, nc.TIME_TRANSFER, sq.pack_sums(*nc.sums(k, nm, Time)))
    d, kk, info = nu.download()
    return raw, d, kk, info, nu.get_state(), nu.mode_table(16)


@pytest.mark.parametrize("Na", nc.NAS)
@pytest.mark.parametrize("name", nc.COSMOS)
def test_device_step_against_host_engine(ctx, name, Na):
    """The cases of the host test: get_delta_nu_combined over the given history, then one step (which rebins: the history's 10 bins are
    not the sums').  delta_nu, delta_nu_last, delta_tot and the table within sqrt(epsilon) of the host engine; history length and the
    keep-or-discard decision equal; a second device run bit-equal.  Measured worst deviation on an MI355X: 1.0e-15 (hybrid, Na = 2);
    0 to 3.3e-16 elsewhere (the two run the same operations in the same order and differ by the device's exp, log, j0 and cos)."""
    c = nc.cosmo(name)
    st = nc.history(Na)
    Time = 0.6 if Na > 1 else 0.03
    with nc.make(None, c) as host:
        h = _one_step(host, st, Time)
    runs = []
    for _ in range(2):
        with nc.make(ctx, c) as dev:
            runs.append(_one_step(dev, st, Time))
    g = runs[0]
    assert g[3].ia == h[3].ia == Na + 1 and g[3].kept == h[3].kept == 1 and g[3].nk == 10 and g[3].nonzero == 12
    assert g[3].nnodes == h[3].nnodes
    worst = max(nc.rel(g[0], h[0]), nc.rel(g[1], h[1]), nc.rel(g[2], h[2]), nc.rel(g[4]["delta_tot"], h[4]["delta_tot"]), nc.rel(g[5], h[5]))
    print(f"nulra device vs host: {name} Na {Na}: worst {worst:.3e}, {g[3].nnodes} nodes, kernel {g[3].ms[1]:.3f} ms")
    assert worst < nc.GATE
    assert np.array_equal(g[4]["scalefact"], h[4]["scalefact"])
    for a, b in zip(runs[0], runs[1]):
        if isinstance(a, dict):
            assert all(np.array_equal(a[key], b[key]) for key in KEYS)
        elif isinstance(a, np.ndarray):
            assert np.array_equal(a, b)


def _sequence(nu, nbins=24):
    k, nm = nc.bins(nbins, kmin=0.5, kmax=40.0)
    out = []
    for t in nc.TIMES:
        nu.step(t, nc.TIME_TRANSFER, sq.pack_sums(*nc.sums(k, nm, t)))
        d, kk, info = nu.download()
        out.append((info.ia, info.kept, d, nu.get_state()["delta_tot"], nu.mode_table(16)))
    return out


def test_twelve_steps_nk24(ctx):
    """first init from the transfer table and twelve steps under the 0.009 rule on nk = 24: integers equal, values within the gate, two
    device runs bit-equal.  Measured worst deviation: 1.1e-15."""
    c = nc.cosmo("mixed_mpc")
    with nc.make(None, c) as host:
        h = _sequence(host)
    runs = []
    for _ in range(2):
        with nc.make(ctx, c) as dev:
            runs.append(_sequence(dev))
    assert [s[1] for s in h] == [-1, 0, 0, 1, -1, 1, 1, 0, 1, 1, 1, 1]
    worst = 0.0
    for sh, sg, sg2 in zip(h, runs[0], runs[1]):
        assert sh[0] == sg[0] and sh[1] == sg[1]
        assert sg[2].shape == (24,)
        worst = max(worst, nc.rel(sg[2], sh[2]), nc.rel(sg[3], sh[3]), nc.rel(sg[4], sh[4]))
        assert all(np.array_equal(x, y) for x, y in zip(sg[2:], sg2[2:]))
    print(f"nulra device vs host, 12 steps nk 24: worst {worst:.3e}")
    assert worst < nc.GATE


def test_nan_is_a_sticky_device_status(ctx):
    c = nc.cosmo("equal")
    st = nc.history(5)
    st["delta_tot"][3, 2] = np.nan
    k, nm = nc.bins()
    with nc.make(ctx, c) as nu:
        nu.set_state(st)
        nu.try_step(0.6, 0.01, sq.pack_sums(*nc.sums(k, nm, 0.6)))   # may itself return SHQ_OK: it does not wait for the device
        with pytest.raises(capi.ShqError):
            nu.download()
        assert nu.try_step(0.7, 0.01, sq.pack_sums(*nc.sums(k, nm, 0.7))) == ERR_DEVICE
    with nc.make(ctx, c) as nu:   # a new state starts clean
        nu.step(0.01, 0.01, sq.pack_sums(*nc.sums(k, nm, 0.01)))
        nu.download()


# ---- inside the PM ----

def _pm_state(ctx):
    import common as cm
    import orc
    n = 16**3
    pos = cm.random_positions(orc.boost_mt19937_uniform(5, 3 * n), n)
    pman = cm.make_partmanager(pos)
    pv = pman.view()
    capi.check(capi.hip.shq_particles_upload(ctx.h, C.byref(pv)))
    return n, sq.PMParams(32, 0, cm.BOX, 1.5, cm.G)


def _finish(ctx, pmp, n):
    capi.check(capi.hip.shq_pm_run(ctx.h, C.byref(pmp)))
    g, p, phi = np.zeros((n, 3)), np.zeros(n), np.zeros((32, 32, 32))
    capi.check(capi.hip.shq_pm_download(ctx.h, capi.ptr(g), capi.ptr(p)))
    capi.check(capi.hip.shq_pm_download_mesh(ctx.h, 1, capi.ptr(phi)))
    return g, p, phi


def _power(ctx, N):
    kk, power, nmodes, norm = np.zeros(N), np.zeros(N), np.zeros(N, dtype=np.int64), C.c_double()
    capi.check(capi.hip.shq_pm_download_power(ctx.h, N, capi.ptr(kk), capi.ptr(power), capi.ptr(nmodes), C.byref(norm)))
    return kk, power, nmodes, norm.value


def test_inside_the_pm_nmesh32(ctx):
    """shq_pm_forward, shq_nulra_step(sums = NULL), finish against forward, shq_pm_set_mode_factor(the downloaded table), finish: the
    potentials bit-equal; the table within the gate of the host route (shq_pm_download_power, host engine); the error states"""
    h = ctx.h
    c = nc.cosmo("mixed_mpc")
    N = 32
    capi.check(capi.hip.shq_pm_set_debug(h, 1))
    capi.check(capi.hip.shq_pm_set_mode_factor(h, 0, None))
    try:
        n, pmp = _pm_state(ctx)
        plain = _finish(ctx, pmp, n)
        # a step before init
        assert capi.hip.shq_nulra_step(h, 0.01, 0.01, None, 0) == ERR_STATE
        with nc.make(ctx, c, nk_allocated=40) as nu, nc.make(None, c, nk_allocated=40) as host:
            # no pending spectrum
            assert nu.try_step(0.01, 0.01) == ERR_STATE
            for t in (0.01, 0.03):
                capi.check(capi.hip.shq_pm_forward(h, C.byref(pmp)))
                sums = _power(ctx, N)                         # the host route's input
                if t == 0.03:   # wrong Nmesh: reduced sums of another size while this spectrum is pending
                    k10, nm10 = nc.bins()
                    assert nu.try_step(t, 0.01, sq.pack_sums(*nc.sums(k10, nm10, t))) == ERR_INVALID
                nu.step(t, 0.01)
                first = _finish(ctx, pmp, n)
                T = nu.mode_table(N)
                d, kk, info = nu.download()
                host.step(t, 0.01, sq.pack_sums(*sums))
            assert info.ia == 2 and info.kept == 1 and info.nonzero == info.nk and 4 <= info.nk <= N
            # the finish consumed the table and the spectrum
            assert nu.try_step(0.03, 0.01) == ERR_STATE
            capi.check(capi.hip.shq_pm_forward(h, C.byref(pmp)))
            capi.check(capi.hip.shq_pm_set_mode_factor(h, N, capi.ptr(T)))
            second = _finish(ctx, pmp, n)
            Th = host.mode_table(N)
            dh, kkh, ih = host.download()
        for a, b in zip(first, second):
            assert np.array_equal(a, b)
        assert T.shape == (3 * 16 * 16 + 1,) and (T[1:] > 1).all()
        assert np.abs(first[2] - plain[2]).max() > 1e-6 * np.abs(plain[2]).max()      # the factor acted
        worst = max(nc.rel(T, Th), nc.rel(d, dh), nc.rel(kk, kkh))
        print(f"nulra in the PM: table, delta_nu_last and kk against the host route: worst {worst:.3e}; max T - 1 = {T.max() - 1:.3e}")
        assert ih.ia == info.ia and ih.nk == info.nk and worst < nc.GATE
    finally:
        capi.check(capi.hip.shq_pm_set_debug(h, 0))
        capi.check(capi.hip.shq_pm_set_mode_factor(h, 0, None))


def test_host_mirror_gravpm_force_takes_the_object(ctx):
    """sq.gravpm_force(analysis = NuLRA.at(Time, TimeIC)): the mirror's hook steps the resident state on the downloaded sums and gets
    its table; GravPM is that of shq_pm_forward, shq_nulra_step(sums = NULL), shq_pm_run"""
    import common as cm
    import orc
    h = ctx.h
    c = nc.cosmo("mixed_mpc")
    n = 16**3
    pos = cm.random_positions(orc.boost_mt19937_uniform(5, 3 * n), n)
    pman = cm.make_partmanager(pos)
    pm = dict(Asmth=1.5, Nmesh=32, G=cm.G)
    try:
        with nc.make(ctx, c, nk_allocated=40) as nu:
            for t in (0.01, 0.03):
                sq.gravpm_force(ctx, pm, pman, analysis=nu.at(t, 0.01))
            info = nu.info()
            Tm = nu.mode_table(32)
        got = pman.Base["GravPM"].copy()
        pmp = sq.PMParams(32, 0, cm.BOX, 1.5, cm.G)
        pv = pman.view()
        capi.check(capi.hip.shq_particles_upload(h, C.byref(pv)))
        with nc.make(ctx, c, nk_allocated=40) as nu:
            for t in (0.01, 0.03):
                capi.check(capi.hip.shq_pm_forward(h, C.byref(pmp)))
                nu.step(t, 0.01)
                capi.check(capi.hip.shq_pm_run(h, C.byref(pmp)))
            T = nu.mode_table(32)
        want = np.zeros((n, 3))
        capi.check(capi.hip.shq_pm_download(h, capi.ptr(want), None))
    finally:
        capi.check(capi.hip.shq_pm_set_mode_factor(h, 0, None))
    assert info.ia == 2 and info.kept == 1
    assert nc.rel(Tm, T) < nc.GATE and (T[1:] > 1).all()
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max() and np.abs(want).max() > 0


# ---- two ranks sharing the GPU ----

NPART, BOX, G, ASMTH, NMESH = 16**3, 8.0, 43.0071, 1.5, 48
DIST_TIMES = (0.01, 0.03)


def _global_particles():
    import orc
    import common as cm
    pos = cm.random_positions(orc.boost_mt19937_uniform(0, 3 * NPART), NPART)
    return np.concatenate([pos, np.ones((NPART, 1))], axis=1)


def _tree_rank(rank, world, outdir):
    import torch
    from shenqi_amd import dist as sd
    import common as cm
    dev = torch.device("cuda", 0)
    comm = sd.Comm()
    mine = torch.from_numpy(_global_particles()[rank::world].copy()).to(dev)
    cm.reference_treepar(ErrTolForceAcc=0.005, MaxBHOpeningAngle=0.9, Rcut=6.0, TreeUseBH=1)
    sq.gravshort_set_softenings(BOX / np.cbrt(NPART))
    gp = sq.make_grav_params(BOX, ASMTH, NMESH, G, cm.RHO0)
    bounds = sd.balanced_bounds(comm, NMESH, BOX, mine[:, 0])
    ctx = sq.Context(0)
    try:
        drv = sd.DistTreePM(comm, ctx, NMESH, BOX, ASMTH, G, dev, halo_factor=1.3, bounds=bounds)
        local = sd.exchange_to_owner(comm, drv.decomp, mine)
        drv.setup(local, gp.Rcut)
        with nc.make(ctx, nc.cosmo("mixed_mpc"), nk_allocated=64) as nu:
            for t in DIST_TIMES:
                drv.step(gp, analysis=nu.at(t, DIST_TIMES[0]))
            acc, pot, gpm, ppot = drv.download()
            T = nu.mode_table(NMESH)
            d, kk, info = nu.download()
        res = dict(local=drv.local.cpu().numpy(), gpm=gpm, ppot=ppot, T=T, d=d, kk=kk, ia=info.ia)
    finally:
        ctx.close()
    np.save(os.path.join(outdir, "nu%d.npy" % rank), np.array([res], dtype=object), allow_pickle=True)


def _tree_worker(rank, world, initfile, outdir):
    import torch.distributed as dist
    os.environ["OMP_NUM_THREADS"] = "2"
    dist.init_process_group("gloo", init_method="file://" + initfile, rank=rank, world_size=world)
    try:
        _tree_rank(rank, world, outdir)
    finally:
        dist.destroy_process_group()


def test_dist_treepm_with_nulra_two_gloo_ranks(ctx):
    """DistTreePM.step(analysis = NuLRA) on two ranks: every rank's engine is fed the all-reduced sums, so the table and the state are
    the same on both to the bit; GravPM is the single-GPU route's (forward, shq_nulra_step on the context's own sums, finish)"""
    import math
    import torch.multiprocessing as mp
    import common as cm
    world = 2
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_tree_worker, args=(world, os.path.join(tmp, "init"), tmp), nprocs=world, join=True)
        outs = [np.load(os.path.join(tmp, "nu%d.npy" % r), allow_pickle=True)[0] for r in range(world)]
    for key in ("T", "d", "kk"):
        assert np.array_equal(outs[0][key], outs[1][key]), key
    assert outs[0]["ia"] == outs[1]["ia"] == 2
    posm = _global_particles()
    key = {tuple(p): i for i, p in enumerate(map(tuple, posm[:, :3]))}
    rows = np.concatenate([o["local"] for o in outs])
    idx = np.array([key[tuple(p)] for p in rows[:, :3]], dtype=np.int64)
    assert len(set(idx.tolist())) == NPART
    h = ctx.h
    capi.check(capi.hip.shq_pm_set_deposit_log2scale(h, 61 - math.frexp(float(posm[:, 3].sum()))[1]))
    try:
        pman = cm.make_partmanager(posm[:, :3].copy())
        pman.Base["Mass"] = posm[:, 3]
        pv = pman.view()
        capi.check(capi.hip.shq_particles_upload(h, C.byref(pv)))
        pmp = sq.PMParams(NMESH, 0, BOX, ASMTH, G)
        with nc.make(ctx, nc.cosmo("mixed_mpc"), nk_allocated=64) as nu:
            for t in DIST_TIMES:
                capi.check(capi.hip.shq_pm_forward(h, C.byref(pmp)))
                nu.step(t, DIST_TIMES[0])
                capi.check(capi.hip.shq_pm_run(h, C.byref(pmp)))
            T = nu.mode_table(NMESH)
        g, p = np.zeros((NPART, 3)), np.zeros(NPART)
        capi.check(capi.hip.shq_pm_download(h, capi.ptr(g), capi.ptr(p)))
    finally:
        capi.check(capi.hip.shq_pm_set_deposit_log2scale(h, -1))
        capi.check(capi.hip.shq_pm_set_mode_factor(h, 0, None))
    assert nc.rel(outs[0]["T"], T) < nc.GATE and (T[1:] > 1).all()
    gpm = np.concatenate([o["gpm"] for o in outs])
    ppot = np.concatenate([o["ppot"] for o in outs])
    assert np.abs(gpm - g[idx]).max() <= 1e-12 * np.abs(g).max()
    assert np.abs(ppot - p[idx]).max() <= 1e-12 * np.abs(p).max()
