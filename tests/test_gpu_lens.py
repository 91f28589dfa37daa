"""The lensing potential planes on the device (shq_lens_planes: write_plane's compute, plane.cpp:511-600, with cutPlaneGaussianGrid,
lenstools.cpp:233-319, and the PM neutrino correction, plane.cpp:355-475) against the numpy restatement (lens_restated.py): counts and
num_particles_plane exactly, planes to 1e-12 of max|plane|.  Then the per-rank contract (two ranks, two x-slabs), the resident route,
particle order, determinism, no interference with the PM, and bad input.  Every test restores what it changes on the shared context."""
import ctypes as C

import numpy as np
import pytest

import shenqi_amd as sq
from shenqi_amd import capi
import common as cm
import lens_restated as lr

pytestmark = pytest.mark.gpu

ERR_INVALID = 1
BOX = 1000.0
COSMO = dict(atime=0.5, comoving_distance=1.3e6, HubbleParam=0.7, omega_source=0.28)


def _restore(ctx):
    capi.check(capi.hip.shq_set_inputs_current(ctx.h, 0))
    capi.check(capi.hip.shq_pm_set_mode_factor(ctx.h, 0, None))
    capi.check(capi.hip.shq_pm_set_deposit_types(ctx.h, capi.ALL_TYPES))
    capi.check(capi.hip.shq_pm_set_mesh_scrub(ctx.h, 1))
    capi.check(capi.hip.shq_pm_set_deposit_log2scale(ctx.h, -1))


@pytest.fixture
def lctx(ctx):
    _restore(ctx)
    try:
        yield ctx
    finally:
        _restore(ctx)


def _edges(R, cuts, th, off):
    """coordinates on the bins' edges and next to them: 0, L, k L / R, cut +- th / 2, shifted by the offset"""
    v = [0.0, BOX] + [k * BOX / R for k in range(0, R + 1, max(R // 8, 1))] + [c - th / 2 for c in cuts] + [c + th / 2 for c in cuts]
    v = np.array(v)
    v = np.concatenate([v, np.nextafter(v, -np.inf), np.nextafter(v, np.inf)])
    return v


def _particles(N, seed=3, R=256, cuts=(), th=BOX, off=(0.0, 0.0, 0.0), nedge=3000):
    """N^3 dark matter (half of it in compact halos) and N^3 gas next to it, some Type 2; swallowed and garbage particles here and there;
    nedge particles whose coordinates sit on bin edges (offset added).  Returns (pman, pos, flags, types)."""
    rng = np.random.default_rng(seed)
    n = N ** 3
    nh = max(n // 2, 1)
    centres = rng.uniform(0, BOX, (64, 3))
    dm = np.concatenate([centres[rng.integers(0, 64, nh)] + rng.normal(0, 0.01 * BOX, (nh, 3)), rng.uniform(0, BOX, (n - nh, 3))])
    gas = dm + rng.normal(0, 0.2 * BOX / N, dm.shape)
    e = _edges(R, cuts, th, off)
    edge = e[rng.integers(0, len(e), (nedge, 3))] + np.asarray(off)
    pos = np.concatenate([np.mod(np.concatenate([dm, gas]), BOX) + np.asarray(off), edge])
    m = len(pos)
    types = np.concatenate([np.ones(n), np.zeros(n), np.ones(nedge)]).astype(np.uint8)
    types[rng.random(m) < 0.05] = 2
    flags = np.zeros(m, np.uint8)
    flags[rng.random(m) < 0.02] |= 1           # garbage: counted
    flags[rng.random(m) < 0.02] |= 2           # swallowed: skipped
    flags |= (rng.integers(0, 16, m) << 4).astype(np.uint8) & 0xF8   # other bits of the flag byte (Generation): ignored
    pman = sq.PartManager(m, BOX)
    pman.Base["Pos"], pman.Base["Type"], pman.Base["Flags"] = pos, types, flags
    pman.Base["Mass"] = 1.0
    return pman, pos, flags, types


def _cosmo(ntot):
    return dict(COSMO, num_particles_tot=int(ntot))


def _device(ctx, pman, p, c, nu=None):
    return sq.lens_planes(ctx, pman, p["Resolution"], p["Normals"], CutPoints=p.get("CutPoints"), Thickness=p.get("Thickness", 0.0),
                          CurrentParticleOffset=p.get("CurrentParticleOffset", (0.0, 0.0, 0.0)), exclude_type2=p.get("exclude_type2", 0),
                          atime=c["atime"], comoving_distance=c["comoving_distance"], HubbleParam=c["HubbleParam"],
                          omega_source=c["omega_source"], num_particles_tot=c["num_particles_tot"], nu=nu)


def _compare(got, ref):
    planes, npl, counts = got
    rplanes, rnpl, rcounts = ref
    assert planes.shape == rplanes.shape
    assert np.array_equal(counts, rcounts)
    assert np.array_equal(npl, rnpl)
    scale = np.abs(rplanes).max()
    assert scale > 0
    assert np.abs(planes - rplanes).max() <= 1e-12 * scale, np.abs(planes - rplanes).max() / scale


CASES = [  # (N, R, Normals, CutPoints, Thickness, offset, exclude_type2)
    (64, 256, [0, 1, 2], [125.0, 500.0, 875.0], 250.0, (0.0, 0.0, 0.0), 0),
    (32, 250, [2, 2, 0], [100.0, 150.0, 990.0], 200.0, (13.5, -250.25, 1000.0), 1),   # repeated normal, overlapping cuts, a wrap
    (32, 45, [1], None, 0.0, (0.0, 0.0, 0.0), 1),                                     # default cut and thickness, odd R
    (16, 2, [0, 2], [500.0], 300.0, (-7.0, 0.0, 3.0), 0),
    (32, 128, [1, 0], None, 250.0, (0.0, 0.0, 0.0), 0),                               # default cuts of a given thickness
]


@pytest.mark.parametrize("N,R,normals,cuts,th,off,excl", CASES)
def test_parity_with_the_restatement(lctx, N, R, normals, cuts, th, off, excl):
    ecuts = cuts if cuts else lr.default_cuts(BOX, th)[1]
    pman, pos, flags, types = _particles(N, R=R, cuts=ecuts, th=th if th > 0 else BOX, off=off)
    ntot = int(lr.is_active(flags, types, excl).sum())
    assert sq.lens_count_active(lctx, pman, excl) == ntot
    p = dict(BoxSize=BOX, Resolution=R, Normals=normals, CutPoints=cuts, Thickness=th, CurrentParticleOffset=off, exclude_type2=excl)
    c = _cosmo(ntot)
    got = _device(lctx, pman, p, c)
    ref = lr.lens_planes(pos, flags, types, p, c)
    _compare(got, ref)
    assert got[1].min() > 0


def _numesh(N, x0, nx, seed=5):
    rng = np.random.default_rng(seed)
    g = np.arange(N) / N
    full = rng.normal(0, 1, (N, N, N)) + 3 * np.sin(2 * np.pi * g)[:, None, None] + 2 * g[None, :, None] ** 2   # anisotropic
    return dict(Nmesh=N, x0=x0, real=np.ascontiguousarray(full[x0:x0 + nx]), inv_fft_norm=1.0 / N ** 3, mean_mass_cell=0.37), full


@pytest.mark.parametrize("Nmesh,R,normals,cuts,th", [(32, 48, [0, 1, 2], [100.0, 600.0], 250.0), (48, 40, [1, 2, 1], [990.0], 90.0),
                                                     (32, 64, [2, 0], None, 0.0)])
def test_correction_parity(lctx, Nmesh, R, normals, cuts, th):
    ecuts = cuts if cuts else [BOX / 2]
    pman, pos, flags, types = _particles(16, seed=8, R=R, cuts=ecuts, th=th if th > 0 else BOX, nedge=500)
    ntot = int(lr.is_active(flags, types, 0).sum())
    p = dict(BoxSize=BOX, Resolution=R, Normals=normals, CutPoints=cuts, Thickness=th)
    nu, _ = _numesh(Nmesh, 0, Nmesh)
    c = _cosmo(ntot)
    got = _device(lctx, pman, p, c, nu=nu)
    ref = lr.lens_planes(pos, flags, types, p, c, nu=nu)
    _compare(got, ref)
    # the correction is there: the planes differ from the particle-only planes by more than the tolerance
    bare = lr.lens_planes(pos, flags, types, p, c)[0]
    assert np.abs(ref[0] - bare).max() > 1e-6 * np.abs(ref[0]).max()


def test_correction_from_pm_apply(lctx):
    """the binding's chain: a spectrum through shq_pm_apply (SHQ_TF_RADIAL, zero_mode 1) gives the unscaled real mesh"""
    N = 32
    rng = np.random.default_rng(4)
    dens = rng.random((N, N, N))
    spec = np.zeros(N * N * (N // 2 + 1) * 2)
    capi.check(capi.hip.shq_fft_r2c(lctx.h, N, capi.ptr(dens), capi.ptr(spec)))
    T = 0.05 * np.exp(-np.arange(3 * (N // 2) ** 2 + 1) / 40.0)
    tf = capi.PMTransfer(0, 0, 1, 0, T.ctypes.data_as(C.c_void_p))
    real = np.zeros((N, N, N))
    capi.check(capi.hip.shq_pm_apply(lctx.h, N, capi.ptr(spec), C.byref(tf), capi.ptr(real)))
    nu = dict(Nmesh=N, x0=0, real=real, inv_fft_norm=1.0 / N ** 3, mean_mass_cell=dens.mean())
    pman, pos, flags, types = _particles(16, seed=2, R=64, cuts=[300.0], th=200.0, nedge=200)
    ntot = int(lr.is_active(flags, types, 0).sum())
    p = dict(BoxSize=BOX, Resolution=64, Normals=[0, 1, 2], CutPoints=[300.0], Thickness=200.0)
    c = _cosmo(ntot)
    _compare(_device(lctx, pman, p, c, nu=nu), lr.lens_planes(pos, flags, types, p, c, nu=nu))


def test_two_ranks_and_two_slabs_sum_to_the_whole(lctx):
    N, R = 48, 96
    pman, pos, flags, types = _particles(24, seed=6, R=R, cuts=[250.0, 700.0], th=300.0, nedge=1000)
    ntot = int(lr.is_active(flags, types, 0).sum())
    p = dict(BoxSize=BOX, Resolution=R, Normals=[0, 1, 2], CutPoints=[250.0, 700.0], Thickness=300.0)
    c = _cosmo(ntot)
    nu_all, full = _numesh(N, 0, N)
    whole = _device(lctx, pman, p, c, nu=nu_all)
    half = len(pos) // 2
    parts = []
    for sl, (x0, nx) in ((slice(0, half), (0, 20)), (slice(half, None), (20, N - 20))):
        pm = sq.PartManager(len(pos[sl]), BOX)
        pm.Base["Pos"], pm.Base["Type"], pm.Base["Flags"] = pos[sl], types[sl], flags[sl]
        nu = dict(nu_all, x0=x0, real=np.ascontiguousarray(full[x0:x0 + nx]))
        parts.append(_device(lctx, pm, p, c, nu=nu))
    assert np.array_equal(parts[0][2].astype(np.int64) + parts[1][2], whole[2].astype(np.int64))
    assert np.array_equal(parts[0][1] + parts[1][1], whole[1])
    scale = np.abs(whole[0]).max()
    assert np.abs(parts[0][0] + parts[1][0] - whole[0]).max() <= 1e-12 * scale


def test_resident_route_order_and_determinism(lctx):
    pman, pos, flags, types = _particles(32, seed=12, R=128, cuts=[400.0, 450.0], th=120.0)
    p = dict(BoxSize=BOX, Resolution=128, Normals=[0, 1, 2], CutPoints=[400.0, 450.0], Thickness=120.0)
    c = _cosmo(12345)
    nu, _ = _numesh(32, 0, 32)
    a = _device(lctx, pman, p, c, nu=nu)
    b = _device(lctx, pman, p, c, nu=nu)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    # the resident set: the same bits, nothing uploaded
    pv = pman.view()
    capi.check(capi.hip.shq_particles_upload(lctx.h, C.byref(pv)))
    capi.check(capi.hip.shq_set_inputs_current(lctx.h, 1))
    r = _device(lctx, pman, p, c, nu=nu)
    assert sq.lens_count_active(lctx, pman, 0) == int(lr.is_active(flags, types, 0).sum())
    capi.check(capi.hip.shq_set_inputs_current(lctx.h, 0))
    for x, y in zip(a, r):
        assert np.array_equal(x, y)
    # a permuted particle order
    perm = np.random.default_rng(0).permutation(len(pos))
    pm2 = sq.PartManager(len(pos), BOX)
    pm2.Base["Pos"], pm2.Base["Type"], pm2.Base["Flags"] = pos[perm], types[perm], flags[perm]
    q = _device(lctx, pm2, p, c, nu=nu)
    for x, y in zip(a, q):
        assert np.array_equal(x, y)


def test_no_interference_with_a_pending_spectrum(lctx):
    ctx = lctx
    n, L, nmesh = 40000, cm.BOX, 48
    pos = cm.random_positions(np.random.default_rng(3).random(3 * n), n)
    pman = cm.make_partmanager(pos)
    pman.Base["Type"] = np.where(np.arange(n) % 7 == 0, 2, np.where(np.arange(n) % 2 == 0, 0, 1))
    pmp = sq.PMParams(nmesh, 0, L, 1.5, cm.G)
    T = 1.0 + 0.3 * np.exp(-np.arange(3 * (nmesh // 2) ** 2 + 1) / 36.0)
    capi.check(capi.hip.shq_pm_set_deposit_log2scale(ctx.h, 40))
    capi.check(capi.hip.shq_pm_set_deposit_types(ctx.h, 0b11))

    def run(with_lens):
        pv = pman.view()
        capi.check(capi.hip.shq_particles_upload(ctx.h, C.byref(pv)))
        capi.check(capi.hip.shq_pm_forward(ctx.h, C.byref(pmp)))
        z0 = C.c_int(-1)
        capi.check(capi.hip.shq_pm_mesh_prezeroed(ctx.h, C.byref(z0)))
        if with_lens:
            capi.check(capi.hip.shq_set_inputs_current(ctx.h, 1))
            sq.lens_planes(ctx, pman, 64, [0, 1, 2], CutPoints=[2.0, 6.0], Thickness=2.0, exclude_type2=True, num_particles_tot=n,
                           nu=dict(Nmesh=16, x0=0, real=np.ones((16, 16, 16)), inv_fft_norm=1.0, mean_mass_cell=1.0))
            capi.check(capi.hip.shq_set_inputs_current(ctx.h, 0))
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
    got = run(True)
    assert np.array_equal(ref[0], got[0]) and np.array_equal(ref[1], got[1])


def test_bad_input_is_refused_before_anything_is_written(lctx):
    pman, pos, flags, types = _particles(8, nedge=10)
    pv = pman.view()
    R = 8
    normals = np.array([0, 2], np.int32)
    cuts = np.array([500.0])
    real = np.zeros((4, 16, 16))

    def call(R=R, normals=normals, ntot=100, omega=0.3, nu=None):
        lp = capi.LensParams()
        lp.Resolution, lp.ncuts, lp.nnormals, lp.exclude_type2 = R, len(cuts), len(normals), 0
        lp.CutPoints, lp.Normals = capi.ptr(cuts), capi.ptr(normals)
        lp.Thickness, lp.BoxSize = 200.0, BOX
        lc = capi.LensCosmo(0.5, 1e6, 0.7, omega, ntot)
        planes = np.full((1, len(normals), max(R, 1), max(R, 1)), 7.0)
        npl = np.full((1, len(normals)), 7, np.int64)
        cnt = np.full((1, len(normals), max(R, 1), max(R, 1)), 7, np.uint32)
        rc = capi.hip.shq_lens_planes(lctx.h, C.byref(lp), C.byref(lc), C.byref(pv), C.byref(nu) if nu is not None else None,
                                      capi.ptr(planes), capi.ptr(npl), capi.ptr(cnt))
        untouched = np.all(planes == 7.0) and np.all(npl == 7) and np.all(cnt == 7)
        return rc, untouched

    def numesh(N, x0, nx):
        return capi.LensNuMesh(N, x0, nx, 0, 1.0, 1.0, real.ctypes.data_as(C.c_void_p))

    bad = [dict(normals=np.array([0, 3], np.int32)), dict(normals=np.array([-1], np.int32)), dict(R=1), dict(R=0),
           dict(ntot=0), dict(ntot=-5), dict(omega=0.0), dict(omega=-0.1),
           dict(nu=numesh(1, 0, 1)), dict(nu=numesh(16, -1, 4)), dict(nu=numesh(16, 0, 0)), dict(nu=numesh(16, 14, 4))]
    for kw in bad:
        rc, untouched = call(**kw)
        assert rc == ERR_INVALID and untouched, kw
    rc, untouched = call(nu=numesh(16, 12, 4))
    assert rc == 0 and not untouched
