"""The excursion-set reionisation on the device (shq_uvbg_calculate: calculate_uvbg + petapm_reion, uvbg.cpp:474-597,
petapm.cpp:495-685) against the numpy restatement (uvbg_restated.py), and its promises: no stars, determinism, no interference with
the PM's state, bad input.  Every test restores what it changes on the shared context."""
import ctypes as C

import numpy as np
import pytest

import shenqi_amd as sq
from shenqi_amd import capi
import common as cm
import uvbg_restated as ur

pytestmark = pytest.mark.gpu

ERR_INVALID = 1
BOX = 20000.0                     # kpc/h
UNITS = dict(UnitLength_in_cm=3.085678e21, UnitMass_in_g=1.989e43, UnitTime_in_s=3.085678e16)
COSMO = dict(Time=0.1, Omega0=0.3, OmegaBaryon=0.045, HubbleParam=0.7, RhoCrit=3 * 0.1 ** 2 / (8 * np.pi * 43007.1),
             hubble=0.1 * np.sqrt(0.3 / 0.1 ** 3 + 0.7), **UNITS)


def _restore(ctx):
    capi.check(capi.hip.shq_set_inputs_current(ctx.h, 0))
    capi.check(capi.hip.shq_uvbg_keep_grids(ctx.h, 0))
    capi.check(capi.hip.shq_pm_set_mode_factor(ctx.h, 0, None))
    capi.check(capi.hip.shq_pm_set_deposit_types(ctx.h, capi.ALL_TYPES))
    capi.check(capi.hip.shq_pm_set_mesh_scrub(ctx.h, 1))
    capi.check(capi.hip.shq_pm_set_deposit_log2scale(ctx.h, -1))
    capi.check(capi.hip.shq_treepm_set_fuse(ctx.h, 0))


@pytest.fixture
def uctx(ctx):
    _restore(ctx)
    try:
        yield ctx
    finally:
        _restore(ctx)


def _params(N, ftype=0, rtom=0, use_sfr=0, **kw):
    p = dict(ReionRBubbleMax=20340.0, ReionRBubbleMin=406.8, ReionDeltaRFactor=1.1, ReionFilterType=ftype, RtoMFilterType=rtom,
             ReionGammaHaloBias=2.0, ReionNionPhotPerBary=4000.0, AlphaUV=3.0, EscapeFractionNorm=0.2, EscapeFractionScaling=0.5,
             ReionUseParticleSFR=use_sfr, ReionSFRTimescale=0.1, UVBGdim=N, BoxSize=BOX)
    p.update(kw)
    return p


def _structs(p, cp):
    up, uc = capi.UvbgParams(), capi.UvbgCosmo()
    for k, v in p.items():
        setattr(up, k, v)
    for k, v in cp.items():
        setattr(uc, k, v)
    return up, uc


def _particles(N, seed=5, stars=True):
    """a perturbed grid of DM (Type 1) and gas (Type 0), N^3 each, and star clusters (Type 4) of several strengths, so that bubbles of
    several sizes form and some cells end partly ionised.  f_esc holds halo masses (fof.c's), Sfr a spread of rates."""
    rng = np.random.default_rng(seed)
    g = (np.stack(np.meshgrid(*[np.arange(N)] * 3, indexing="ij"), -1).reshape(-1, 3) + 0.5) * (BOX / N)
    dm = g + rng.normal(0, 0.25 * BOX / N, g.shape)
    gas = g + 0.3 * BOX / N + rng.normal(0, 0.25 * BOX / N, g.shape)
    parts = [dm, gas]
    types = [np.full(len(dm), 1), np.full(len(gas), 0)]
    mtot = COSMO["Omega0"] * COSMO["RhoCrit"] * BOX ** 3
    mass = [np.full(len(dm), 0.85 * mtot / len(dm)), np.full(len(gas), 0.15 * mtot / len(gas))]
    if stars:
        for k, strength in enumerate((3e-3, 1e-2, 3e-2, 1e-1, 3e-1, 1.0)):
            c = rng.uniform(0, BOX, 3)
            m = 12 + 6 * k
            parts.append(c + rng.normal(0, 0.6 * BOX / N, (m, 3)))
            types.append(np.full(m, 4))
            mass.append(np.full(m, strength / m * 0.01))
    pos = np.mod(np.concatenate(parts), BOX)
    types = np.concatenate(types).astype(np.uint8)
    mass = np.concatenate(mass).astype(np.float32)
    n = len(pos)
    fesc = np.where(rng.random(n) < 0.2, 0.0, 10 ** rng.uniform(-3, 2, n))
    sfr = np.where((types == 0) & (rng.random(n) < 0.3), 10 ** rng.uniform(-4, 0, n), 0.0)
    local_J21 = rng.uniform(0, 1, n)
    zreion = np.where(rng.random(n) < 0.9, -1.0, 9.5)
    return pos, types, mass, fesc, sfr, local_J21, zreion


def _pman(pos, types, mass, box=BOX):
    pm = cm.make_partmanager(pos, box=box)
    pm.Base["Type"] = types
    pm.Base["Mass"] = mass
    return pm


def _device(ctx, p, cp, pman, fesc, sfr, lj, zr):
    up, uc = _structs(p, cp)
    fesc, lj, zr = fesc.copy(), lj.copy(), zr.copy()
    vol, mw, nr, J21, xHI = sq.calculate_uvbg(ctx, pman, up, uc, fesc, sfr.copy(), lj, zr, keep_grids=True)
    return dict(vol=vol, mass=mw, nradii=nr, J21=J21, xHI=xHI, fesc=fesc, local_J21=lj, zreion=zr)


def _ulps(a, b):
    return np.abs(np.asarray(a, np.float32).view(np.int32).astype(np.int64) - np.asarray(b, np.float32).view(np.int32).astype(np.int64))


CASES = [  # (Nmesh, ReionFilterType, RtoMFilterType, ReionUseParticleSFR); 36 is off the bespoke list (hipFFT route)
    (32, 0, 0, 0), (32, 1, 1, 1), (32, 2, 0, 1), (48, 0, 1, 1), (48, 1, 0, 0), (48, 2, 1, 0),
    (64, 0, 0, 1), (64, 1, 1, 0), (64, 2, 1, 1), (128, 0, 1, 0), (36, 2, 0, 1), (36, 0, 1, 0),
]


@pytest.mark.parametrize("N,ftype,rtom,use_sfr", CASES)
def test_parity_with_the_restatement(uctx, N, ftype, rtom, use_sfr):
    pos, types, mass, fesc, sfr, lj, zr = _particles(N)
    p = _params(N, ftype, rtom, use_sfr)
    got = _device(uctx, p, COSMO, _pman(pos, types, mass), fesc, sfr, lj, zr)
    ref = ur.calculate_uvbg(p, COSMO, pos, mass, types, fesc, sfr, lj, zr)
    near = ref["near"]
    assert got["nradii"] == ref["nradii"]
    # the set must exercise every branch: ionised cells, partial ones, neutral ones; every cell receives mass
    ion = ref["xHI"] == 0
    assert ion.sum() > 0 and ((ref["xHI"] > 0) & (ref["xHI"] < 1)).sum() > 0 and (ref["xHI"] == 1).sum() > 0
    # the ionisation decision: the same in every cell whose f_coll_stars never came within 1e-12 of the threshold (listed)
    flip = (ion != (got["xHI"] == 0)) & ~near
    assert not flip.any(), np.argwhere(flip)[:10]
    # J21 and xHI within 1 float ulp elsewhere (the fixed-point deposit and the transforms round differently from double CIC and numpy).
    # J21 at the noise floor is the exception: a cell ionised far from any star-forming gas records the transforms' rounding noise of
    # the SFR field (1e-16 of its peak, clamped at 0 when negative), in the reference as well; there the rule is |dJ21| <= 1e-12 max J21
    ok = ~near
    floor = 1e-12 * float(ref["J21"].max())
    jbad = (_ulps(got["J21"], ref["J21"]) > 1) & (np.abs(got["J21"].astype(np.float64) - ref["J21"]) > floor)
    assert not jbad[ok].any(), (np.argwhere(jbad & ok)[:10], got["J21"][jbad & ok][:10], ref["J21"][jbad & ok][:10])
    assert _ulps(got["xHI"], ref["xHI"])[ok].max() <= 1
    print(f"N {N}: {int(near.sum())} cells near the threshold; J21 equal in {np.mean(got['J21'] == ref['J21']):.6f}, "
          f"xHI in {np.mean(got['xHI'] == ref['xHI']):.6f} of the cells")
    assert abs(got["vol"] - ref["vol"]) <= 1e-12 and abs(got["mass"] - ref["mass"]) <= 1e-12
    # particles: fesc within pow's rounding, local_J21 within a float ulp, zreion exact - except particles touching a listed cell
    assert np.allclose(got["fesc"], ref["fesc"], rtol=4e-16, atol=0)
    pnear = near.reshape(-1)[ref["cells"]].any(axis=1)
    gas = (types == 0) & ~pnear
    lbad = (_ulps(got["local_J21"], ref["local_J21"]) > 1) & (np.abs(got["local_J21"] - ref["local_J21"]) > floor)
    assert not lbad[gas].any()
    # zreion: exact, except where the particle's largest J21 is at the noise floor (0 on one side, 1e-16 on the other)
    zok = ~pnear & (ref["local_J21"] > floor)
    zok |= ~pnear & (types != 0)
    assert np.array_equal(got["zreion"][zok], ref["zreion"][zok])
    assert np.array_equal(got["zreion"][types != 0], zr[types != 0])
    assert np.array_equal(got["local_J21"][types != 0], lj[types != 0])       # only gas is written
    assert (got["zreion"] != zr).sum() > 0


def test_no_stars(uctx):
    N = 32
    pos, types, mass, fesc, sfr, lj, zr = _particles(N, stars=False)
    got = _device(uctx, _params(N), COSMO, _pman(pos, types, mass), fesc, sfr, lj, zr)
    assert np.all(got["xHI"] == 1) and np.all(got["J21"] == 0)
    assert np.all(got["local_J21"][types == 0] == 0)
    assert np.array_equal(got["zreion"], zr)
    assert got["vol"] == 1.0 and abs(got["mass"] - 1.0) <= 1e-15


def test_determinism_and_particle_order(uctx):
    N = 48
    pos, types, mass, fesc, sfr, lj, zr = _particles(N, seed=9)
    p = _params(N, 0, 0, 1)
    a = _device(uctx, p, COSMO, _pman(pos, types, mass), fesc, sfr, lj, zr)
    b = _device(uctx, p, COSMO, _pman(pos, types, mass), fesc, sfr, lj, zr)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    perm = np.random.default_rng(1).permutation(len(pos))
    c = _device(uctx, p, COSMO, _pman(pos[perm], types[perm], mass[perm]), fesc[perm], sfr[perm], lj[perm], zr[perm])
    for k in ("J21", "xHI", "vol", "mass", "nradii"):
        assert np.array_equal(np.asarray(a[k]), np.asarray(c[k])), k
    for k in ("fesc", "local_J21", "zreion"):
        assert np.array_equal(a[k][perm], c[k]), k


def test_resident_positions(uctx):
    """shq_set_inputs_current(SHQ_CURRENT_PARTICLES) with this very view resident: the same results as the staged call"""
    N = 32
    pos, types, mass, fesc, sfr, lj, zr = _particles(N, seed=4)
    p = _params(N, 2, 1, 1)
    pman = _pman(pos, types, mass)
    a = _device(uctx, p, COSMO, pman, fesc, sfr, lj, zr)
    pv = pman.view()
    capi.check(capi.hip.shq_particles_upload(uctx.h, C.byref(pv)))
    capi.check(capi.hip.shq_set_inputs_current(uctx.h, 1))
    b = _device(uctx, p, COSMO, pman, fesc, sfr, lj, zr)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def _uvbg_on(ctx, pman, n, box):
    """a uvbg call on the resident set (box-sized mesh, stars among the particles)"""
    types = np.asarray(pman.Base["Type"]).copy()
    rng = np.random.default_rng(2)
    fesc = rng.uniform(0, 5, n)
    p = _params(32, 0, 0, 1, BoxSize=box, ReionRBubbleMax=box, ReionRBubbleMin=box / 100)
    up, uc = _structs(p, COSMO)
    capi.check(capi.hip.shq_set_inputs_current(ctx.h, 1))
    sq.calculate_uvbg(ctx, pman, up, uc, fesc, rng.uniform(0, 1, n), np.zeros(n), np.full(n, -1.0))
    capi.check(capi.hip.shq_set_inputs_current(ctx.h, 0))
    return types


def test_no_interference_with_a_pending_spectrum(uctx):
    ctx = uctx
    n, L, nmesh = 40000, cm.BOX, 48
    pos = cm.random_positions(np.random.default_rng(3).random(3 * n), n)
    pman = cm.make_partmanager(pos)
    pman.Base["Type"] = np.where(np.arange(n) % 7 == 0, 4, np.where(np.arange(n) % 2 == 0, 0, 1))
    pmp = sq.PMParams(nmesh, 0, L, 1.5, cm.G)
    T = 1.0 + 0.3 * np.exp(-np.arange(3 * (nmesh // 2) ** 2 + 1) / 36.0)
    capi.check(capi.hip.shq_pm_set_deposit_log2scale(ctx.h, 40))

    def run(with_uvbg):
        pv = pman.view()
        capi.check(capi.hip.shq_particles_upload(ctx.h, C.byref(pv)))
        capi.check(capi.hip.shq_pm_forward(ctx.h, C.byref(pmp)))
        z0 = C.c_int(-1)
        capi.check(capi.hip.shq_pm_mesh_prezeroed(ctx.h, C.byref(z0)))
        if with_uvbg:
            _uvbg_on(ctx, pman, n, L)
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


def test_no_interference_with_a_prestarted_pm(uctx):
    ctx = uctx
    n, L, nmesh = 32**3, 1.0, 64
    pos = sq.synth_positions("cluster", n, L=L)
    pos = pos[sq.morton_order(pos, L)]
    pman = cm.make_partmanager(pos, box=L)
    pman.Base["Type"] = np.where(np.arange(n) % 5 == 0, 4, 0)
    tree = sq.force_tree_full(pman)
    sq.set_gravshort_treepar(ErrTolForceAcc=0.005, BHOpeningAngle=0.175, MaxBHOpeningAngle=0.9, TreeUseBH=0, Rcut=6.0)
    sq.gravshort_set_softenings(L / 32)
    gp = sq.make_grav_params(L, 1.5, nmesh, cm.G, cm.RHO0)
    pmp = sq.PMParams(nmesh, 0, L, 1.5, cm.G)

    def run(with_uvbg):
        pv, tv = pman.view(), tree.view()
        capi.check(capi.hip.shq_particles_upload(ctx.h, C.byref(pv)))
        capi.check(capi.hip.shq_tree_upload(ctx.h, C.byref(tv)))
        capi.check(capi.hip.shq_pm_start(ctx.h, C.byref(pmp), gp.G))
        if with_uvbg:
            _uvbg_on(ctx, pman, n, L)
        capi.check(capi.hip.shq_treepm_step(ctx.h, C.byref(pmp), C.byref(gp), 1, sq.WALK_EXACT))
        g = np.zeros((n, 3)); pp = np.zeros(n)
        capi.check(capi.hip.shq_pm_download(ctx.h, capi.ptr(g), capi.ptr(pp)))
        acc = np.zeros((n, 3)); pot = np.zeros(n); nint = np.zeros(n, dtype=np.int64)
        capi.check(capi.hip.shq_grav_short_download(ctx.h, capi.ptr(acc), capi.ptr(pot), capi.ptr(nint), C.byref(sq.WalkStats())))
        return g, pp, acc, pot, nint

    ref = run(False)
    got = run(True)
    for a, b in zip(ref, got):
        assert np.array_equal(a, b)


def test_negative_escape_fraction_is_refused(uctx):
    N = 32
    pos, types, mass, fesc, sfr, lj, zr = _particles(N)
    up, uc = _structs(_params(N, EscapeFractionNorm=-0.2), COSMO)
    pman = _pman(pos, types, mass)
    f, l, z = fesc.copy(), lj.copy(), zr.copy()
    pv = pman.view()
    res = capi.UvbgResult()
    rc = capi.hip.shq_uvbg_calculate(uctx.h, C.byref(up), C.byref(uc), C.byref(pv), capi.ptr(f), capi.ptr(sfr), capi.ptr(l), capi.ptr(z),
                                     C.byref(res))
    assert rc == ERR_INVALID
    assert np.array_equal(f, fesc) and np.array_equal(l, lj) and np.array_equal(z, zr)
