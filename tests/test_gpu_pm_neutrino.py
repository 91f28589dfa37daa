"""The PM with linear-response massive neutrinos (MassiveNuLinRespOn, gravpm.cpp:76-85, 308-321, 412-435) and the hybrid-neutrino deposit
mask (gravpm.cpp:84-85, 459-464): shq_pm_forward stops the PM between its halves, the caller's factor T[k2] multiplies the modes before
the Green's function, and the next shq_pm_run / shq_treepm_step finishes it.  Every test restores what it changes on the shared context."""
import ctypes as C

import numpy as np
import pytest

import shenqi_amd as sq
from shenqi_amd import capi
import orc
import common as cm

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE = 1, 4
NO_TYPE2 = capi.ALL_TYPES & ~(1 << 2)


def _restore(ctx):
    h = ctx.h
    capi.check(capi.hip.shq_pm_measure_power(h, 0))
    capi.check(capi.hip.shq_pm_set_mode_factor(h, 0, None))
    capi.check(capi.hip.shq_pm_set_deposit_types(h, capi.ALL_TYPES))
    capi.check(capi.hip.shq_pm_set_fft_transposed(h, 1))
    capi.check(capi.hip.shq_pm_set_mesh_scrub(h, 1))
    capi.check(capi.hip.shq_pm_set_debug(h, 0))
    capi.check(capi.hip.shq_pm_set_deposit_log2scale(h, -1))


@pytest.fixture
def pmctx(ctx):
    _restore(ctx)
    try:
        yield ctx
    finally:
        _restore(ctx)


def _k2(N):
    k1 = np.fft.fftfreq(N, 1.0 / N).astype(np.int64)   # petapm_mesh_to_k
    k1[N // 2] = N // 2
    kx, ky, kz = np.meshgrid(k1, k1, np.arange(N // 2 + 1, dtype=np.int64), indexing="ij")
    return kx, ky, kz, kx * kx + ky * ky + kz * kz


def _invsinc2(k, N):
    t = k * np.pi / N
    s = np.where(np.abs(t) < 1e-5, 1.0 - t**2 / 6 + t**4 / 120, np.sin(t) / np.where(t == 0, 1.0, t))
    return 1.0 / (s * s)


def _table(N, amp=0.3, k0=6.0):
    """a factor in the shape of 1 + nu_prefac nu_spline(log k): T = 1 + amp exp(-k2 / k0^2)"""
    k2 = np.arange(3 * (N // 2) ** 2 + 1, dtype=np.float64)
    return 1.0 + amp * np.exp(-k2 / k0**2)


def _restated_potential(rho, N, T, Asmth=1.5, G=cm.G, L=cm.BOX):
    """irfftn(rfftn(rho) T green), unscaled: potential_transfer (gravpm.cpp:378-444) with the neutrino factor in front, zero mode removed"""
    kx, ky, kz, k2 = _k2(N)
    dk = np.fft.rfftn(rho)
    if T is not None:
        dk = dk * np.where(k2 > 0, T[k2], 1.0)
    asmth2 = ((2 * np.pi) * Asmth / N) ** 2
    f = _invsinc2(kx, N) * _invsinc2(ky, N) * _invsinc2(kz, N)
    with np.errstate(divide="ignore", invalid="ignore"):
        fac = (-G / (np.pi * L)) * (np.exp(-k2 * asmth2) / k2) * f * f
    fac[k2 == 0] = 0.0
    return np.fft.irfftn(dk * fac, s=(N, N, N), axes=(0, 1, 2), norm="forward")


def _restated_readout(phi, pos, N, L=cm.BOX):
    """readout_potential / readout_force (gravpm.cpp:489-500) with the 4-point difference the library applies in real space"""
    tmp = pos / (L / N)
    fl = np.floor(tmp)
    res = tmp - fl
    ic = fl.astype(np.int64) % N
    ffac = -(N / L)
    c1, c2 = 2.0 / 3.0, 1.0 / 12.0
    g = np.zeros((len(pos), 3))
    pot = np.zeros(len(pos))

    def at(dx, dy, dz):
        return phi[(ic[:, 0] + dx) % N, (ic[:, 1] + dy) % N, (ic[:, 2] + dz) % N]

    for c in range(8):
        a, b, e = c & 1, (c >> 1) & 1, (c >> 2) & 1
        w = (res[:, 0] if a else 1 - res[:, 0]) * (res[:, 1] if b else 1 - res[:, 1]) * (res[:, 2] if e else 1 - res[:, 2])
        pot += w * at(a, b, e)
        g[:, 0] += w * (ffac * (c1 * (at(a + 1, b, e) - at(a - 1, b, e)) - c2 * (at(a + 2, b, e) - at(a - 2, b, e))))
        g[:, 1] += w * (ffac * (c1 * (at(a, b + 1, e) - at(a, b - 1, e)) - c2 * (at(a, b + 2, e) - at(a, b - 2, e))))
        g[:, 2] += w * (ffac * (c1 * (at(a, b, e + 1) - at(a, b, e - 1)) - c2 * (at(a, b, e + 2) - at(a, b, e - 2))))
    return g, pot


def _restated_power(rho, N, T=None):
    """orc.power_spectrum's sums of w |T delta|^2 f^2 (powerspectrum_add_mode after potential_transfer's nufac, gravpm.cpp:426-430)"""
    kx, ky, kz, k2 = _k2(N)
    dk = np.fft.rfftn(rho)
    if T is not None:
        dk = dk * np.where(k2 > 0, T[k2], 1.0)
    m = dk.real**2 + dk.imag**2
    f = _invsinc2(kx, N) * _invsinc2(ky, N) * _invsinc2(kz, N)
    binsperunit = (N - 1) / np.log(np.sqrt(3) * N / 2.0)
    sel = k2 > 0
    kint = np.floor(binsperunit * np.log(k2[sel].astype(np.float64)) / 2.0).astype(np.int64)
    ok = kint < N
    w = np.where((kz[sel] == 0) | (kz[sel] == N // 2), 1, 2)[ok]
    kint = kint[ok]
    power = np.bincount(kint, weights=w * m[sel][ok] * f[sel][ok] ** 2, minlength=N)
    kk = np.bincount(kint, weights=w * np.sqrt(k2[sel][ok].astype(np.float64)), minlength=N)
    nmodes = np.bincount(kint, weights=w, minlength=N).astype(np.int64)
    return kk, power, nmodes, float(m[0, 0, 0])


def _upload(ctx, pos, types=None, mass=None):
    pman = cm.make_partmanager(pos)
    if types is not None:
        pman.Base["Type"] = types
    if mass is not None:
        pman.Base["Mass"] = mass
    pv = pman.view()
    capi.check(capi.hip.shq_particles_upload(ctx.h, C.byref(pv)))
    return pman


def _pm(ctx, pmp, n, N=None):
    """shq_pm_run and its results; the potential mesh too when N is given (shq_pm_set_debug(1) must be on)"""
    capi.check(capi.hip.shq_pm_run(ctx.h, C.byref(pmp)))
    g = np.zeros((n, 3)); p = np.zeros(n)
    capi.check(capi.hip.shq_pm_download(ctx.h, capi.ptr(g), capi.ptr(p)))
    if N is None:
        return g, p, None
    phi = np.zeros((N, N, N))
    capi.check(capi.hip.shq_pm_download_mesh(ctx.h, 1, capi.ptr(phi)))
    return g, p, phi


def _power(ctx, N):
    kk = np.zeros(N); power = np.zeros(N); nmodes = np.zeros(N, dtype=np.int64); norm = C.c_double()
    capi.check(capi.hip.shq_pm_download_power(ctx.h, N, capi.ptr(kk), capi.ptr(power), capi.ptr(nmodes), C.byref(norm)))
    return kk, power, nmodes, norm.value


def _neutrino(ctx, pmp, n, T, N=None):
    """forward, the sums, the table, finish: the reference-side binding of gravpm_force with MassiveNuLinRespOn"""
    capi.check(capi.hip.shq_pm_forward(ctx.h, C.byref(pmp)))
    sums = _power(ctx, pmp.Nmesh)
    capi.check(capi.hip.shq_pm_set_mode_factor(ctx.h, pmp.Nmesh, capi.ptr(T)))
    return _pm(ctx, pmp, n, N) + (sums,)


def _route(ctx, route):
    capi.check(capi.hip.shq_pm_set_fft_transposed(ctx.h, 0 if route == "inplace" else 1))


def _random_set(n, seed=3):
    return cm.random_positions(orc.boost_mt19937_uniform(seed, 3 * n), n)


@pytest.mark.parametrize("route,nmesh", [("transposed", 48), ("transposed", 128), ("transposed", 384), ("hipfft", 36), ("inplace", 48)])
def test_unit_factor_gives_the_plain_pm(pmctx, route, nmesh):
    """T = 1 through forward + finish: the plain shq_pm_run's GravPM, PM potential and potential mesh bit for bit on the transposing pipeline
    (v * 1.0 is exact, the split X pass does the fused pass's arithmetic); within 1e-12 on the split routes (hipFFT size, in-place pipeline).
    A finish without a table is T = 1 as well."""
    ctx = pmctx
    n = 20**3 + 11
    pos = _random_set(n)
    _upload(ctx, pos)
    _route(ctx, route)
    small = nmesh <= 128
    capi.check(capi.hip.shq_pm_set_debug(ctx.h, 1 if small else 0))
    pmp = sq.PMParams(nmesh, 0, cm.BOX, 1.5, cm.G)
    N = nmesh if small else None
    g0, p0, phi0 = _pm(ctx, pmp, n, N)
    ones = np.ones(3 * (nmesh // 2) ** 2 + 1)
    g1, p1, phi1, _ = _neutrino(ctx, pmp, n, ones, N)
    capi.check(capi.hip.shq_pm_forward(ctx.h, C.byref(pmp)))          # no table
    g2, p2, phi2 = _pm(ctx, pmp, n, N)
    for g, p, phi in ((g1, p1, phi1), (g2, p2, phi2)):
        if route == "transposed":
            assert np.array_equal(g, g0) and np.array_equal(p, p0)
            if small:
                assert np.array_equal(phi, phi0)
        else:
            assert np.abs(g - g0).max() <= 1e-12 * np.abs(g0).max()
            assert np.abs(p - p0).max() <= 1e-12 * np.abs(p0).max()
            assert np.abs(phi - phi0).max() <= 1e-12 * np.abs(phi0).max()


@pytest.mark.parametrize("route,nmesh", [("transposed", 48), ("hipfft", 36), ("inplace", 48)])
def test_factor_multiplies_the_modes_before_the_green_function(pmctx, route, nmesh):
    """A real factor: the potential mesh is irfftn(rfftn(rho) T green) (the restatement checked against the oracle's potential at T = 1),
    GravPM changes and is the readout of that mesh; the P(k) sums of the forward are the density's, those of a measuring finish the
    multiplied density's (potential_transfer's, gravpm.cpp:426-430)."""
    ctx = pmctx
    n = 16**3
    pos = sq.synth_positions("cluster", n, L=cm.BOX)
    pman = _upload(ctx, pos)
    mass = pman.Base["Mass"]
    _route(ctx, route)
    capi.check(capi.hip.shq_pm_set_debug(ctx.h, 1))
    pmp = sq.PMParams(nmesh, 0, cm.BOX, 1.5, cm.G)
    g0, _, phi0 = _pm(ctx, pmp, n, nmesh)
    rho = np.zeros((nmesh,) * 3)
    capi.check(capi.hip.shq_pm_download_mesh(ctx.h, 0, capi.ptr(rho)))
    e = 61 - int(np.frexp(float(mass.astype(np.float64).sum()))[1])
    _, _, orho, ophi = orc.pm_force(pos, mass, nmesh, cm.BOX, 1.5, cm.G, fixed_point_log2scale=e, want_mesh=True)
    assert np.array_equal(rho, orho)
    ones_phi = _restated_potential(rho, nmesh, None)
    assert np.abs(ones_phi - ophi).max() <= 1e-12 * np.abs(ophi).max()          # the restatement is the oracle's potential_transfer
    assert np.abs(phi0 - ones_phi).max() <= 1e-12 * np.abs(ones_phi).max()

    T = _table(nmesh)
    capi.check(capi.hip.shq_pm_measure_power(ctx.h, 1))
    g1, p1, phi1, fwd = _neutrino(ctx, pmp, n, T, nmesh)
    fin = _power(ctx, nmesh)
    want = _restated_potential(rho, nmesh, T)
    assert np.abs(phi1 - want).max() <= 1e-12 * np.abs(want).max()
    assert np.abs(g1 - g0).max() > 1e-3 * np.abs(g0).max()                       # the factor changed the forces ...
    og, op = _restated_readout(want, pos, nmesh)
    assert np.abs(g1 - og).max() <= 1e-11 * np.abs(og).max()                     # ... into the readout of the multiplied potential
    assert np.abs(p1 - op).max() <= 1e-11 * np.abs(op).max()
    for got, ref in ((fwd, orc.power_spectrum(rho, nmesh)), (fwd, _restated_power(rho, nmesh)), (fin, _restated_power(rho, nmesh, T))):
        kk, power, nmodes, norm = got
        okk, opower, onmodes, onorm = ref
        assert np.array_equal(nmodes, onmodes) and nmodes.sum() > 0
        assert abs(norm - onorm) < 1e-10 * onorm
        assert np.abs(kk - okk).max() < 1e-10 * okk.max()
        assert np.abs(power - opower).max() < 1e-9 * opower.max()
    assert np.abs(fin[1] - fwd[1]).max() > 1e-3 * fwd[1].max()


def test_forward_sums_without_measure_power_on_a_larger_mesh(pmctx):
    """shq_pm_forward's sums at Nmesh 192 (the X forward half's histograms of many workgroups) with shq_pm_measure_power off"""
    ctx = pmctx
    n, N = 32**3, 192
    _upload(ctx, sq.synth_positions("cluster", n, L=cm.BOX))
    capi.check(capi.hip.shq_pm_set_debug(ctx.h, 1))
    pmp = sq.PMParams(N, 0, cm.BOX, 1.5, cm.G)
    capi.check(capi.hip.shq_pm_forward(ctx.h, C.byref(pmp)))
    kk, power, nmodes, norm = _power(ctx, N)
    capi.check(capi.hip.shq_pm_run(ctx.h, C.byref(pmp)))
    rho = np.zeros((N, N, N))
    capi.check(capi.hip.shq_pm_download_mesh(ctx.h, 0, capi.ptr(rho)))
    okk, opower, onmodes, onorm = orc.power_spectrum(rho, N)
    assert np.array_equal(nmodes, onmodes)
    assert abs(norm - onorm) < 1e-10 * onorm
    assert np.abs(kk - okk).max() < 1e-10 * okk.max()
    assert np.abs(power - opower).max() < 1e-9 * opower.max()


@pytest.mark.parametrize("route,nmesh", [("transposed", 48), ("hipfft", 36), ("inplace", 48)])
def test_deposit_type_mask(pmctx, route, nmesh):
    """Without Type 2 in the mask (hybrid_nu_tracer): GravPM, PM potential and potential mesh bit-identical to an all-types run with the Type-2
    masses zero (fixed-point deposit: exact); Type 2 is still read out; shq_pm_forward honours the mask; without a Type field the mask is
    refused."""
    ctx = pmctx
    n = 20**3 + 11
    pos = _random_set(n, seed=7)
    types = np.random.default_rng(2).choice(np.array([0, 1, 2, 4], dtype=np.uint8), n)
    _route(ctx, route)
    capi.check(capi.hip.shq_pm_set_debug(ctx.h, 1))
    capi.check(capi.hip.shq_pm_set_deposit_log2scale(ctx.h, 40))       # the same fixed-point scale for both mass sums
    pmp = sq.PMParams(nmesh, 0, cm.BOX, 1.5, cm.G)
    _upload(ctx, pos, types)
    ga, pa, phia = _pm(ctx, pmp, n, nmesh)
    capi.check(capi.hip.shq_pm_set_deposit_types(ctx.h, NO_TYPE2))
    g, p, phi = _pm(ctx, pmp, n, nmesh)
    capi.check(capi.hip.shq_pm_forward(ctx.h, C.byref(pmp)))
    gf, pf, phif = _pm(ctx, pmp, n, nmesh)
    capi.check(capi.hip.shq_pm_set_deposit_types(ctx.h, capi.ALL_TYPES))
    _upload(ctx, pos, types, mass=np.where(types == 2, 0.0, 1.0).astype(np.float32))
    gz, pz, phiz = _pm(ctx, pmp, n, nmesh)
    capi.check(capi.hip.shq_pm_forward(ctx.h, C.byref(pmp)))           # (the in-place pipeline's forward + finish is the split route)
    gzf, pzf, phizf = _pm(ctx, pmp, n, nmesh)
    for a, b in ((g, gz), (p, pz), (phi, phiz), (gf, gzf), (pf, pzf), (phif, phizf)):
        assert np.array_equal(a, b)
    t2 = types == 2
    assert np.all(np.abs(g[t2]).sum(axis=1) > 0)                          # tracers still get their GravPM
    assert np.abs(g - ga).max() > 1e-3 * np.abs(ga).max()
    # a view without the Type field: the mask cannot be honoured
    pman = cm.make_partmanager(pos)
    pv = pman.view()
    pv.off_type = C.c_size_t(-1).value
    capi.check(capi.hip.shq_particles_upload(ctx.h, C.byref(pv)))
    capi.check(capi.hip.shq_pm_set_deposit_types(ctx.h, NO_TYPE2))
    assert capi.hip.shq_pm_run(ctx.h, C.byref(pmp)) == ERR_STATE
    assert capi.hip.shq_pm_forward(ctx.h, C.byref(pmp)) == ERR_STATE
    capi.check(capi.hip.shq_pm_set_deposit_types(ctx.h, capi.ALL_TYPES))
    capi.check(capi.hip.shq_pm_run(ctx.h, C.byref(pmp)))


def _resident_setup(ctx):
    n, L, nmesh = 64**3, 1.0, 96
    pos = sq.synth_positions("cluster", n, L=L)
    pos = pos[sq.morton_order(pos, L)]
    pman = cm.make_partmanager(pos, box=L)
    tree = sq.force_tree_full(pman)
    sq.set_gravshort_treepar(ErrTolForceAcc=0.005, BHOpeningAngle=0.175, MaxBHOpeningAngle=0.9, TreeUseBH=0, Rcut=6.0)
    sq.gravshort_set_softenings(L / 64)
    gp = sq.make_grav_params(L, 1.5, nmesh, cm.G, cm.RHO0)
    pmp = sq.PMParams(nmesh, 0, L, 1.5, cm.G)
    rng = np.random.default_rng(11)
    pman.Base["FullTreeGravAccel"] = rng.standard_normal((n, 3)) * 50.0
    pman.Base["GravPM"] = rng.standard_normal((n, 3))

    def start():
        # the views point into pman's and tree's arrays: made here, so that this closure keeps their owners alive
        pv, tv = pman.view(), tree.view()
        capi.check(capi.hip.shq_particles_upload(ctx.h, C.byref(pv)))
        capi.check(capi.hip.shq_tree_upload(ctx.h, C.byref(tv)))

    def results():
        g = np.zeros((n, 3)); pp = np.zeros(n)
        capi.check(capi.hip.shq_pm_download(ctx.h, capi.ptr(g), capi.ptr(pp)))
        acc = np.zeros((n, 3)); pot = np.zeros(n); nint = np.zeros(n, dtype=np.int64)
        capi.check(capi.hip.shq_grav_short_download(ctx.h, capi.ptr(acc), capi.ptr(pot), capi.ptr(nint), C.byref(sq.WalkStats())))
        return g, pp, acc, pot, nint

    def forward(T):
        capi.check(capi.hip.shq_pm_forward(ctx.h, C.byref(pmp)))
        _power(ctx, nmesh)
        capi.check(capi.hip.shq_pm_set_mode_factor(ctx.h, nmesh, capi.ptr(T)))

    return n, nmesh, gp, pmp, start, results, forward, pman


def test_resident_step_finishes_the_pending_spectrum(pmctx):
    """forward, table, shq_treepm_step against forward, table, shq_pm_run + shq_grav_refresh_oldacc + shq_grav_short_run: GravPM, PM potential,
    forces, potentials and interaction counts bit for bit, with the readout in the walk's prologue and without"""
    ctx = pmctx
    n, nmesh, gp, pmp, start, results, forward, _ = _resident_setup(ctx)
    T = _table(nmesh)
    start()
    forward(T)
    capi.check(capi.hip.shq_pm_run(ctx.h, C.byref(pmp)))
    capi.check(capi.hip.shq_grav_refresh_oldacc(ctx.h, gp.G))
    capi.check(capi.hip.shq_grav_short_run(ctx.h, C.byref(gp), None, 0, 1, sq.WALK_EXACT))
    ref = results()
    start()
    capi.check(capi.hip.shq_pm_run(ctx.h, C.byref(pmp)))
    assert np.abs(results()[0] - ref[0]).max() > 1e-3 * np.abs(ref[0]).max()    # the factor is in ref
    fused = C.c_int(-1)
    try:
        for want in (1, 0):
            start()
            capi.check(capi.hip.shq_treepm_set_fuse(ctx.h, want))
            forward(T)
            capi.check(capi.hip.shq_treepm_step(ctx.h, C.byref(pmp), C.byref(gp), 1, sq.WALK_EXACT))
            capi.check(capi.hip.shq_treepm_last_fused(ctx.h, C.byref(fused)))
            assert fused.value == want
            for a, b, name in zip(results(), ref, ("GravPM", "PM potential", "acc", "pot", "ninteractions")):
                assert np.array_equal(a, b), (want, name, float(np.abs(a - b).max()))
    finally:
        capi.check(capi.hip.shq_treepm_set_fuse(ctx.h, 0))


def test_pending_spectrum_state_rules(pmctx):
    """the finish wants the forward's params; a drift, an upload, an FFT seam call and shq_pm_start discard the spectrum (the next
    shq_pm_run is a plain PM); a walk between forward and finish leaves it alone (no mesh scrub); a table of another Nmesh is invalid; the
    finish consumes the table"""
    ctx = pmctx
    n, nmesh, gp, pmp, start, results, forward, pman = _resident_setup(ctx)
    T = _table(nmesh)
    h = ctx.h

    def pm():
        return _pm(ctx, pmp, n)[:2]

    def prezeroed():
        z = C.c_int(-1)
        capi.check(capi.hip.shq_pm_mesh_prezeroed(h, C.byref(z)))
        return z.value

    start()
    plain = pm()
    forward(T)
    nu = pm()
    assert np.abs(nu[0] - plain[0]).max() > 1e-3 * np.abs(plain[0]).max()
    # no spectrum pending: no table
    assert capi.hip.shq_pm_set_mode_factor(h, nmesh, capi.ptr(T)) == ERR_STATE
    # other params
    capi.check(capi.hip.shq_pm_forward(h, C.byref(pmp)))
    assert capi.hip.shq_pm_set_mode_factor(h, nmesh + 2, capi.ptr(_table(nmesh + 2))) == ERR_INVALID
    capi.check(capi.hip.shq_pm_set_mode_factor(h, nmesh, capi.ptr(T)))
    for other in (sq.PMParams(nmesh, 0, 2.0, 1.5, cm.G), sq.PMParams(nmesh, 0, 1.0, 1.25, cm.G), sq.PMParams(nmesh, 0, 1.0, 1.5, 2 * cm.G),
                  sq.PMParams(nmesh + 2, 0, 1.0, 1.5, cm.G)):
        assert capi.hip.shq_pm_run(h, C.byref(other)) == ERR_STATE
    assert all(np.array_equal(a, b) for a, b in zip(pm(), nu))            # still pending, with its table
    # the finish consumed the table: a forward and a finish without one are the plain PM
    assert capi.hip.shq_pm_set_mode_factor(h, nmesh, capi.ptr(T)) == ERR_STATE
    capi.check(capi.hip.shq_pm_forward(h, C.byref(pmp)))
    assert all(np.array_equal(a, b) for a, b in zip(pm(), plain))
    # discarded by: a particle upload, a drift, the FFT seam, shq_pm_start
    real = np.random.default_rng(5).standard_normal((nmesh, nmesh, nmesh))
    comp = np.zeros((nmesh, nmesh, nmesh // 2 + 1, 2))
    for what in ("upload", "drift", "fft", "start"):
        start()
        if what == "drift":
            pv = pman.view()
            capi.check(capi.hip.shq_dynamics_upload(h, C.byref(pv)))
        forward(T)
        if what == "upload":
            start()
        elif what == "drift":
            capi.check(capi.hip.shq_drift(h, 0.0, 1.0, None))
        elif what == "fft":
            capi.check(capi.hip.shq_fft_r2c(h, nmesh, capi.ptr(real), capi.ptr(comp)))
        else:
            capi.check(capi.hip.shq_pm_start(h, C.byref(pmp), 0.0))
        assert capi.hip.shq_pm_set_mode_factor(h, nmesh, capi.ptr(T)) == ERR_STATE, what
        assert all(np.array_equal(a, b) for a, b in zip(pm(), plain)), what
    # a production-size walk between forward and finish does not scrub the pending spectrum
    start()
    capi.check(capi.hip.shq_grav_refresh_oldacc(h, gp.G))
    capi.check(capi.hip.shq_pm_run(h, C.byref(pmp)))
    capi.check(capi.hip.shq_grav_short_run(h, C.byref(gp), None, 0, 1, sq.WALK_EXACT))
    assert prezeroed() == 1                                                 # this walk carries the scrub ...
    forward(T)
    capi.check(capi.hip.shq_grav_short_run(h, C.byref(gp), None, 0, 1, sq.WALK_EXACT))
    assert prezeroed() == 0                                                 # ... this one, with a spectrum pending, does not
    assert all(np.array_equal(a, b) for a, b in zip(pm(), nu))


def test_two_runs_with_one_table_give_the_same_bits(pmctx):
    """forward + table + finish twice: identical GravPM, PM potential and potential mesh (the P(k) sums, floating-point atomics as
    shq_pm_measure_power's, are not bit-reproducible and not compared here)"""
    ctx = pmctx
    n, N = 20**3 + 11, 96
    _upload(ctx, _random_set(n, seed=9))
    capi.check(capi.hip.shq_pm_set_debug(ctx.h, 1))
    pmp = sq.PMParams(N, 0, cm.BOX, 1.5, cm.G)
    T = _table(N)
    a = _neutrino(ctx, pmp, n, T, N)[:3]
    b = _neutrino(ctx, pmp, n, T, N)[:3]
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_host_mirror_gravpm_force_with_an_analysis_hook(pmctx):
    """gravpm_force of the host mirror with petapm's global_analysis hook and the deposit mask: the hook sees the density's P(k) sums and its
    table reaches the potential; without a hook the call is today's"""
    ctx = pmctx
    n, N = 16**3, 48
    pos = sq.synth_positions("cluster", n, L=cm.BOX)
    types = np.random.default_rng(4).choice(np.array([1, 2], dtype=np.uint8), n)
    pman = cm.make_partmanager(pos)
    pman.Base["Type"] = types
    pm = dict(Asmth=1.5, Nmesh=N, G=cm.G)
    sq.gravpm_force(ctx, pm, pman)
    plain = pman.Base["GravPM"].copy()
    seen = {}
    T = _table(N)

    def analysis(kk, power, nmodes, norm):
        seen["nmodes"] = nmodes
        return T

    pman.Base["Potential"] = 0
    sq.gravpm_force(ctx, pm, pman, analysis=analysis, deposit_types=NO_TYPE2)
    hooked = pman.Base["GravPM"].copy()
    # the same through the C-ABI
    pmp = sq.PMParams(N, 0, cm.BOX, 1.5, cm.G)
    pv = pman.view()
    capi.check(capi.hip.shq_particles_upload(ctx.h, C.byref(pv)))
    capi.check(capi.hip.shq_pm_set_deposit_types(ctx.h, NO_TYPE2))
    g, _, _, sums = _neutrino(ctx, pmp, n, T)
    assert np.array_equal(hooked, g)
    assert np.array_equal(seen["nmodes"], sums[2])
    assert np.abs(hooked - plain).max() > 1e-3 * np.abs(plain).max()
    with pytest.raises(Exception):
        sq.gravpm_force(ctx, pm, pman, analysis=lambda *a: 1 / 0)
