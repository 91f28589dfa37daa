"""Radiative cooling on the device (shq_cooling_eval, shq_cooling; csrc/cooling.hip driving csrc/cooling_math.hpp) against the reference's
recorded DoCooling table, against the same engine on the host (shq_cooling_eval_host, which test_cooling_cpu.py holds bit-equal to the
Python restatement) and against the restatement's cooling_direct.  Every test restores what it changes on the shared context."""
import ctypes as C
import functools

import numpy as np
import pytest

import shenqi_amd as sq
from shenqi_amd import capi
import common as cm
import cooling_restated as cr
import cooling_cases as cc

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE = 1, 4
EPS = 2.0 ** -52
# Device against host engine, the random set (cooling_cases.random_case, seed 20261018, 4133 particles).
# Hard, derived: two bisections that part on one sign test both end within the solver's 1e-6 bracket of the same root, and the fixed
# point's ITERCONV is 1e-6: |u_dev - u_host| <= 2.5e-6 u and |ne_dev - ne_host| <= 2.5e-6 for every particle.
HARD = 2.5e-6
# Tight, measured on an MI355X: the largest deviation once the 0.1 % largest are set aside, |u_dev - u_host| in units of 2^-52 u and
# |ne_dev - ne_host| in units of 2^-52.  The bracket's ends and the bisection's midpoints are exact IEEE arithmetic on u_old, so u moves
# only where a sign test parts; ne carries libm's ulps through the fixed point.  Measured: u 0 for all 4133 particles (bit-equal, the
# engine-step counts too), ne 1.562 outside the 0.1 % (15.62 at most; 1.0 % of the particles differ at all).  The bounds are 8 x these.
# Host only, seed 20261018: a second host run with every log / exp / pow / log10 result moved by one ulp in alternating sign
# (SHQ_COOL_NUDGE) agrees with the first within the hard bound for all 4133 and in u bit for bit for all; in ne 24.4 % differ, by 25.25
# outside the 0.1 % (31.6 at most), so only 97.1 % lie within the tight ne bound.  No seed changes that: the hook moves every libm result
# by a whole ulp, which is coarser than what the card's libm does (its ne deviations are 16 times smaller), so the tight ne bound,
# set as 8 x the card's own figure, is below what the hook can meet.  The share is recorded here as it is.
TIGHT_U_MEASURED = 0.0
TIGHT_NE_MEASURED = 1.562
TIGHT_U_BOUND = 8 * TIGHT_U_MEASURED
TIGHT_NE_BOUND = 8 * TIGHT_NE_MEASURED
OUTLIER_SHARE = 1e-3


def _restore(ctx):
    capi.check(capi.hip.shq_set_inputs_current(ctx.h, 0))
    sq.cooling_set_refill(ctx, 1)


@pytest.fixture
def cctx(ctx):
    _restore(ctx)
    try:
        yield ctx
    finally:
        _restore(ctx)


def _eval(ctx, which, what, n=None):
    case, (rho, u, ne, Z, heiii, dt), mes = cc.grid_case() if which == "grid" else cc.random_case()
    s = slice(0, n)
    sq.cooling_set_tables(ctx, case.tables())
    return sq.cooling_eval(ctx, what, rho[s], u[s], ne[s], case.uvbg(), case.redshift, Z=Z[s], heiii=heiii[s], dt=dt[s], min_egy_spec=mes, lmfp_heat=case.lmfp_heat)


def _deviations(dev, host):
    """(u deviations in 2^-52 u, ne deviations in 2^-52)"""
    return np.abs(dev[0] - host[0]) / (EPS * np.abs(host[0])), np.abs(dev[1] - host[1]) / EPS


def _outside_share(d):
    """the largest deviation once the OUTLIER_SHARE largest are set aside"""
    keep = len(d) - int(np.floor(OUTLIER_SHARE * len(d)))
    return float(np.sort(d)[keep - 1])


# ---- (1) the reference's grid ------------------------------------------------------------------------------------------------------------

def test_grid_meets_recorded_tables(cctx):
    """400 particles = 6.25 waves; DoCooling and GetCoolingTime against tests/test_cooling.cpp's tables at its own gates"""
    unew, _, st, _ = _eval(cctx, "grid", "UNEW")
    tcool, _, st2, _ = _eval(cctx, "grid", "TCOOL")
    assert np.all(st == capi.COOL_OK) and np.all(st2 == capi.COOL_OK)
    assert cc.within_reference_gates(unew=unew)
    assert cc.within_reference_gates(tcool=tcool)


# ---- (2) launch shapes ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 65, 4096 + 37])
def test_launch_shapes(cctx, n):
    """less than a wave, a wave and one lane, and 4133: three workgroups' shares, every lane refilled many times, a ragged end"""
    a = _eval(cctx, "random", "UNEW", n)
    b = _eval(cctx, "random", "UNEW", n)
    sq.cooling_set_refill(cctx, 0)
    c = _eval(cctx, "random", "UNEW", n)
    host = [x[:n] for x in cc.host_result("random", "UNEW")]
    assert np.all(a[2] == capi.COOL_OK)
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x, y)     # two runs
        assert np.array_equal(x, z)     # refill on and off
    assert np.all(np.abs(a[0] - host[0]) <= HARD * host[0]) and np.all(np.abs(a[1] - host[1]) <= HARD)
    ms, steps = sq.cooling_last_kernel(cctx)
    assert ms > 0 and steps == int(c[3].sum())


# ---- (3) device against the host engine ----------------------------------------------------------------------------------------------------

def test_device_against_host_engine(cctx):
    dev = _eval(cctx, "random", "UNEW")
    host = cc.host_result("random", "UNEW")
    du, dne = _deviations(dev, host)
    print(f"cooling device vs host: u outside the share {_outside_share(du):.4g}, max {du.max():.4g} (2^-52 u); ne outside the share {_outside_share(dne):.4g}, "
          f"max {dne.max():.4g} (2^-52); beyond tight u {np.mean(du > TIGHT_U_BOUND):.5f} ne {np.mean(dne > TIGHT_NE_BOUND):.5f}; "
          f"steps equal {np.mean(dev[3] == host[3]):.5f}")
    assert np.all(dev[2] == capi.COOL_OK)
    assert np.all(np.abs(dev[0] - host[0]) <= HARD * host[0]) and np.all(np.abs(dev[1] - host[1]) <= HARD)
    assert np.mean(du > TIGHT_U_BOUND) <= OUTLIER_SHARE and np.mean(dne > TIGHT_NE_BOUND) <= OUTLIER_SHARE


@pytest.mark.parametrize("what", ["TCOOL", "NH0", "HE0", "HEP", "HEPP", "TEMP", "LAMBDANET"])
def test_queries_against_host_engine(cctx, what):
    """the single-evaluation queries on the first 300 particles: one fixed point, no bisection, so only libm's ulps and the fixed
    point's 1e-6 stand between the two"""
    n = 300
    dev = _eval(cctx, "random", what, n)
    host = [x[:n] for x in cc.host_result("random", what)]
    assert np.all(dev[2] == capi.COOL_OK)
    scale = np.maximum(np.abs(host[0]), 1e-300)
    ok = np.abs(dev[0] - host[0]) <= 10 * HARD * scale
    if what == "LAMBDANET":     # heating minus cooling cancels near equilibrium: measure against the larger of the two inputs' scale
        ok |= np.abs(dev[0] - host[0]) <= 10 * HARD * np.abs(host[0]).max()
    assert np.all(ok), (what, np.flatnonzero(~ok)[:5])
    assert np.all(np.abs(dev[1] - host[1]) <= HARD)


# ---- (4) - (6) shq_cooling end to end ------------------------------------------------------------------------------------------------------

NGRID = 12
BOXSIZE = 20000.0
SFR = dict(StarformationOn=1, PhysDensThresh=None, OverDensThresh=None, HIReionTemp=2e4, MinGasTemp=100.0, temp_to_u=None)


@functools.lru_cache(maxsize=None)
def _particles():
    """2 x 12^3 particles: gas and dark matter interleaved at random, a garbage row, a zero-mass row, wind particles, dense gas above the
    star-formation threshold, one particle above 1e9 K and one with Density = 0"""
    case, _, _ = cc.random_case()
    un = case.units
    rng = np.random.default_rng(412)
    ngas = NGRID ** 3
    n = 2 * ngas
    redshift = case.redshift
    a3inv = (1 + redshift) ** 3
    types = rng.permutation(np.concatenate([np.zeros(ngas, np.uint8), np.ones(ngas, np.uint8)]))
    P = np.zeros(n, dtype=capi.PARTICLE_DTYPE)
    P["Type"] = types
    P["Pos"] = rng.random((n, 3)) * BOXSIZE
    gi = np.flatnonzero(types == 0)
    # the wrap cells of the Zreion table on each face: below the first node's cell and in the last one
    for f in range(3):
        P["Pos"][gi[10 + f], f] = 1e-3 * BOXSIZE
        P["Pos"][gi[20 + f], f] = (1 - 1e-3) * BOXSIZE
    P["Mass"] = rng.uniform(0.8, 1.2, n).astype(np.float32)
    P["Hsml"] = BOXSIZE / NGRID
    P["Vel"] = rng.normal(size=(n, 3))
    P["TimeBinHydro"] = rng.integers(15, 20, n)           # bin 15 carries dt = 0 below
    P["PI"][gi] = rng.permutation(ngas)
    P["Flags"][gi[rng.random(ngas) < 0.5]] |= 4           # HeIIIionized
    P["Flags"][gi[3]] |= 1                                 # garbage
    P["Mass"][gi[4]] = 0                                   # Mass <= 0
    S = np.zeros(ngas, dtype=capi.SPH_DTYPE)
    nphys = 10.0 ** rng.uniform(-7, 0.5, ngas)
    S["Density"] = nphys * cr.PROTONMASS / un.density_in_phys_cgs / a3inv
    temp = 10.0 ** rng.uniform(2.5, 7.5, ngas)
    mu = 4.0 / (1 + 3 * cr.HYDROGEN_MASSFRAC)
    u = temp * cr.BOLTZMANN / (cr.GAMMA_MINUS1 * cr.PROTONMASS * mu) / un.uu_in_cgs
    S["Entropy"] = u / np.array([cr.entropy_to_u(float(d), a3inv) for d in S["Density"]])
    S["Ne"] = rng.uniform(0, 1.2, ngas)
    S["Metallicity"] = rng.uniform(0, 0.05, ngas)
    S["Sfr"] = rng.uniform(0.1, 1.0, ngas)
    S["DelayTime"] = np.where(rng.random(ngas) < 0.1, 0.3, 0.0)
    hot, empty = P["PI"][gi[5]], P["PI"][gi[6]]
    S["Density"][hot] = np.median(S["Density"])             # not star-forming: it has to reach the cooling
    S["Entropy"][hot] = 3e9 / temp[hot] * u[hot] / cr.entropy_to_u(float(S["Density"][hot]), a3inv)
    S["Density"][empty] = 0.0
    S["DelayTime"][[hot, empty]] = 0.0
    P["TimeBinHydro"][[gi[5], gi[6]]] = 15                 # lastred = redshift: never inside the reionisation bump
    for a in (P, S):
        a.setflags(write=False)
    return P, S, int(gi[5]), int(gi[6])


def _step(case, mode, J21=None, zre=None):
    P, S, _, _ = _particles()
    un = case.units
    st = capi.CoolingStep()
    st.redshift, st.a3inv, st.hubble = case.redshift, (1 + case.redshift) ** 3, 0.35
    for b in range(capi.TIMEBINS + 1):
        st.kf.dloga_for_bin[b] = 0.0 if b <= 15 else 2e-5 * 2.0 ** (b - 16)
        st.lastred_for_bin[b] = case.redshift + (0.0 if b <= 15 else 0.02 * 2.0 ** (b - 16))
    for k, v in case.uv.items():
        setattr(st.GlobalUVBG, k, v)
    st.uvbg_mode, st.StarformationOn = mode, 1
    mu = 4.0 / (1 + 3 * cr.HYDROGEN_MASSFRAC)
    st.temp_to_u = cr.BOLTZMANN / (cr.GAMMA_MINUS1 * cr.PROTONMASS) / un.uu_in_cgs
    st.HIReionTemp, st.MinGasTemp, st.lmfp_heat = SFR["HIReionTemp"], SFR["MinGasTemp"], case.lmfp_heat
    st.CurrentParticleOffset[:] = [0.25 * BOXSIZE, -0.125 * BOXSIZE, 0.0]
    st.PhysDensThresh = float(np.quantile(S["Density"], 0.9)) * st.a3inv
    st.OverDensThresh = float(np.quantile(S["Density"], 0.02))
    if mode == capi.COOL_UVBG_J21:
        st._keep = (np.ascontiguousarray(J21), np.ascontiguousarray(zre))
        st.local_J21, st.zreion = st._keep[0].ctypes.data, st._keep[1].ctypes.data
        st.J21_coeffs[:] = [1.1e-12, 0.0, 6.0e-13, 7.0e-12, 0.0, 8.0e-12]
        A, Cf = cr.self_shield_factors(case.cp, case.redshift)
        st.ss_greyopac_factor, st.ss_fbar_factor = A, Cf
    return st


@functools.lru_cache(maxsize=None)
def _zreion_table():
    """5^3, smooth, around the step's redshift: some cells reionise later (rates zero), some inside [redshift, lastred), some before"""
    i = np.arange(5)
    x, y, z = np.meshgrid(i, i, i, indexing="ij")
    t = 3.0 + 0.1 * np.sin(1.3 * x + 0.4) * np.cos(0.9 * y) + 0.03 * z
    t.setflags(write=False)
    return t


def _restated_cooling(case, st, mode, active, mask=None, J21=None, zre=None):
    """cooling_and_starformation's classification and cooling_direct over the active list, in Python"""
    P0, S0, _, _ = _particles()
    P, S = P0.copy(), S0.copy()
    sfr = dict(StarformationOn=st.StarformationOn, PhysDensThresh=st.PhysDensThresh, OverDensThresh=st.OverDensThresh, HIReionTemp=st.HIReionTemp,
               MinGasTemp=st.MinGasTemp, temp_to_u=st.temp_to_u)
    ztab = dict(nside=5, boxsize=BOXSIZE, values=[float(v) for v in _zreion_table().ravel()])
    eeqos, cooled, deferred, bad, bumped = [], [], [], [], 0
    off = list(st.CurrentParticleOffset)
    for i in (range(len(P)) if active is None else active):
        i = int(i)
        if P["Type"][i] != 0 or (P["Flags"][i] & 1) or P["Mass"][i] <= 0:
            continue
        pi = P["PI"][i]
        on = int(mask[i]) if mask is not None else cr.on_eeqos(sfr, float(S["Density"][pi]), float(S["DelayTime"][pi]), st.a3inv)
        if on:
            eeqos.append(i)
            continue
        b = int(P["TimeBinHydro"][i])
        uv = cr.local_uvbg(case.cp, mode, st.redshift, case.uv, [float(v) for v in P["Pos"][i]], off, ztab, None if J21 is None else float(J21[pi]),
                           None if zre is None else float(zre[pi]), list(st.J21_coeffs))
        case.net.left_table = False
        try:
            if not (S["Density"][pi] > 0):
                raise ValueError
            ent, ne, bump = cr.cooling_direct(case.cool, sfr, st.redshift, st.a3inv, st.hubble, st.kf.dloga_for_bin[b], st.lastred_for_bin[b], float(S["Density"][pi]),
                                              float(S["Entropy"][pi]), float(S["Ne"][pi]), float(S["Metallicity"][pi]), int(bool(P["Flags"][i] & 4)), uv)
        except ValueError:
            bad.append(i)
            continue
        if case.net.left_table:
            deferred.append(i)
            continue
        bumped += bump
        S["Entropy"][pi], S["Ne"][pi], S["Sfr"][pi] = ent, ne, 0
        cooled.append(i)
    return S, eeqos, cooled, deferred, bad, bumped


def _same_records(a, b):
    """field by field: the records have padding bytes that a copy does not carry"""
    return all(np.array_equal(a[name], b[name]) for name in a.dtype.names)


def _run_cooling(ctx, case, st, active, mask=None, **tab_kw):
    P0, S0, _, _ = _particles()
    pman = sq.PartManager(len(P0), BOXSIZE)
    pman.Base[:] = P0
    S = S0.copy()
    sq.cooling_set_tables(ctx, case.tables(**tab_kw))
    res, eeqos, deferred = sq.cooling(ctx, pman, S, st, active=active, on_eeqos=mask)
    assert _same_records(pman.Base, P0)          # the particle records are never written
    return pman, S, res, eeqos, deferred


def _check_against_restated(S, rS, cooled, P):
    pi = P["PI"][np.array(cooled, dtype=np.int64)]
    untouched = np.ones(len(S), dtype=bool)
    untouched[pi] = False
    _, S0, _, _ = _particles()
    assert _same_records(S[untouched], S0[untouched])         # skipped, eeqos, deferred and bad rows: bit-unchanged
    assert np.all(S["Sfr"][pi] == 0)
    assert np.all(np.abs(S["Entropy"][pi] - rS["Entropy"][pi]) <= HARD * rS["Entropy"][pi])
    assert np.all(np.abs(S["Ne"][pi] - rS["Ne"][pi]) <= HARD)
    for name in S.dtype.names:
        if name not in ("Entropy", "Ne", "Sfr"):
            assert np.array_equal(S[name], S0[name]), name
    return np.abs(S["Entropy"][pi] - rS["Entropy"][pi]) / (EPS * rS["Entropy"][pi]), np.abs(S["Ne"][pi] - rS["Ne"][pi]) / EPS


@pytest.mark.parametrize("listed", [False, True])
def test_cooling_end_to_end(cctx, listed):
    """the Zreion-table mode with the reionisation bump, all particles or a shuffled list of two thirds of them; the statuses"""
    case, _, _ = cc.random_case()
    P, S0, i_hot, i_empty = _particles()
    st = _step(case, capi.COOL_UVBG_ZREION)
    active = None
    if listed:
        active = np.ascontiguousarray(np.random.default_rng(5).permutation(len(P))[:2 * len(P) // 3].astype(np.int32))
        active = np.concatenate([active[(active != i_hot) & (active != i_empty)], [i_hot, i_empty]]).astype(np.int32)
    tab = dict(zreion=_zreion_table(), zreion_boxsize=BOXSIZE)
    rS, r_eeqos, r_cooled, r_deferred, r_bad, r_bumped = _restated_cooling(case, st, capi.COOL_UVBG_ZREION, active)
    assert r_bumped > 20 and len(r_eeqos) > 20 and r_deferred == [i_hot] and r_bad == [i_empty]
    pman, S, res, eeqos, deferred = _run_cooling(cctx, case, st, active, **tab)
    assert list(eeqos) == r_eeqos and list(deferred) == r_deferred
    assert list(res.n_status) == [len(r_cooled), 1, 1, 0] and res.n_eeqos == len(r_eeqos) and res.n_deferred == 1
    cnt = len(P) if active is None else len(active)
    assert res.n_skipped == cnt - len(r_cooled) - len(r_eeqos) - 2 and res.steps > 0 and res.kernel_ms > 0
    du, dne = _check_against_restated(S, rS, r_cooled, P)
    # the bounds of the random set, with the entropy's own exp / log (enttou, twice) on top of u's: measured 2.0 of these units at most
    assert np.mean(du > 8 * 2.0) <= OUTLIER_SHARE and np.mean(dne > TIGHT_NE_BOUND) <= OUTLIER_SHARE
    print(f"cooling end to end: Entropy outside the share {_outside_share(du):.4g} max {du.max():.4g}; Ne outside the share {_outside_share(dne):.4g} max {dne.max():.4g}")
    # the context's copy of the entropies equals the caller's records
    ent = sq.entropy_download(cctx, len(P))
    gas = np.flatnonzero(P["Type"] == 0)
    assert np.array_equal(ent[gas], S["Entropy"][P["PI"][gas]])
    # a second call under shq_set_inputs_current starts from the results of the first, as the reference's next step would
    capi.check(capi.hip.shq_set_inputs_current(cctx.h, capi.CURRENT_PARTICLES | capi.CURRENT_SPH))
    S1 = S.copy()
    res2, eeqos2, _ = sq.cooling(cctx, pman, S, st, active=active)
    capi.check(capi.hip.shq_set_inputs_current(cctx.h, 0))
    S2 = S1.copy()
    sq.cooling(cctx, pman, S2, st, active=active)
    assert _same_records(S, S2) and list(eeqos2) == r_eeqos


def test_cooling_with_caller_mask(cctx):
    case, _, _ = cc.random_case()
    P, S0, i_hot, i_empty = _particles()
    st = _step(case, capi.COOL_UVBG_GLOBAL)
    rng = np.random.default_rng(8)
    mask = (rng.random(len(P)) < 0.3).astype(np.uint8)
    mask[[i_hot, i_empty]] = 0
    rS, r_eeqos, r_cooled, r_deferred, r_bad, _ = _restated_cooling(case, st, capi.COOL_UVBG_GLOBAL, None, mask=mask)
    pman, S, res, eeqos, deferred = _run_cooling(cctx, case, st, None, mask=mask)
    assert list(eeqos) == r_eeqos and list(deferred) == r_deferred == [i_hot]
    assert res.n_status[capi.COOL_BADINPUT] == 1 and res.n_status[capi.COOL_OK] == len(r_cooled)
    _check_against_restated(S, rS, r_cooled, P)


# ---- (5) the tables -----------------------------------------------------------------------------------------------------------------------

def test_j21_mode(cctx):
    """get_local_UVBG_from_J21: local_J21 = 0 for a fifth of the slots, 1e-3 .. 1e2 for the rest"""
    case, _, _ = cc.random_case()
    P, S0, i_hot, i_empty = _particles()
    rng = np.random.default_rng(21)
    J21 = np.where(rng.random(len(S0)) < 0.2, 0.0, 10.0 ** rng.uniform(-3, 2, len(S0)))
    zre = rng.uniform(2.9, 3.3, len(S0))
    st = _step(case, capi.COOL_UVBG_J21, J21, zre)
    rS, r_eeqos, r_cooled, r_deferred, r_bad, r_bumped = _restated_cooling(case, st, capi.COOL_UVBG_J21, None, J21=J21, zre=zre)
    assert r_bumped > 20
    pman, S, res, eeqos, deferred = _run_cooling(cctx, case, st, None)
    assert list(eeqos) == r_eeqos and list(deferred) == r_deferred and res.n_status[capi.COOL_OK] == len(r_cooled)
    _check_against_restated(S, rS, r_cooled, P)


@pytest.mark.parametrize("redshift", [1.5, 3.0, 5.0])
def test_metal_table(cctx, redshift):
    """TableMetalCoolingRate with the clamps at both ends of each axis: the redshift below, inside and above the table, densities and
    temperatures of the random set on all three sides; device against the host engine (which test_cooling_cpu.py holds to the restatement)"""
    case, (rho, u, ne, Z, heiii, dt), mes = cc.metal_case()
    n = 600
    s = slice(0, n)
    Zs = Z[s] * 20      # up to solar, so that the table matters
    t = case.tables()
    uv = case.uvbg()
    host = sq.cooling_eval_host(t, "LAMBDANET", rho[s], u[s], ne[s], uv, redshift, Z=Zs, heiii=heiii[s], lmfp_heat=case.lmfp_heat)
    nometal = sq.cooling_eval_host(cc.random_case()[0].tables(), "LAMBDANET", rho[s], u[s], ne[s], uv, redshift, Z=Zs, heiii=heiii[s], lmfp_heat=case.lmfp_heat)
    assert np.mean(host[0] != nometal[0]) > 0.9
    sq.cooling_set_tables(cctx, t)
    dev = sq.cooling_eval(cctx, "LAMBDANET", rho[s], u[s], ne[s], uv, redshift, Z=Zs, heiii=heiii[s], lmfp_heat=case.lmfp_heat)
    assert np.all(dev[2] == capi.COOL_OK)
    assert np.all(np.abs(dev[0] - host[0]) <= 10 * HARD * np.maximum(np.abs(host[0]), np.abs(host[0]).max() * 1e-6))
    dev = sq.cooling_eval(cctx, "UNEW", rho[s], u[s], ne[s], uv, redshift, Z=Zs, heiii=heiii[s], dt=dt[s], min_egy_spec=mes, lmfp_heat=case.lmfp_heat)
    host = sq.cooling_eval_host(t, "UNEW", rho[s], u[s], ne[s], uv, redshift, Z=Zs, heiii=heiii[s], dt=dt[s], min_egy_spec=mes, lmfp_heat=case.lmfp_heat)
    assert np.all(np.abs(dev[0] - host[0]) <= HARD * host[0]) and np.all(np.abs(dev[1] - host[1]) <= HARD)


# ---- (7) bad arguments ----------------------------------------------------------------------------------------------------------------------

def test_bad_arguments_and_no_interference(cctx):
    case, (rho, u, ne, Z, heiii, dt), mes = cc.random_case()
    P0, S0, _, _ = _particles()
    pman = sq.PartManager(len(P0), BOXSIZE)
    pman.Base[:] = P0
    S = S0.copy()
    pv, sv = pman.view(), capi.sph_view(S)
    kf = sq.KickFactors()
    for b in range(capi.TIMEBINS + 1):
        kf.dloga_for_bin[b] = 1e-3 * 2.0 ** (b - 16) if b > 0 else 0.0

    def winds():
        Sw = S0.copy()
        capi.check(capi.hip.shq_winds_evolve(cctx.h, C.byref(pv), C.byref(capi.sph_view(Sw)), None, len(P0), 8.0, 0.3, float(np.median(S0["Density"])), 0.25, C.byref(kf)))
        return Sw

    before = winds()
    st = _step(case, capi.COOL_UVBG_GLOBAL)
    f = S.dtype.fields
    cf = capi.CoolingFields(f["Ne"][1], f["Metallicity"][1], f["Sfr"][1], f["DelayTime"][1])
    res = capi.CoolingResult()
    lists = np.zeros(len(P0), dtype=np.int32)

    def call(h, pv_, sv_, nlist, st_=st):
        return capi.hip.shq_cooling(h, pv_, sv_, C.byref(cf), None, nlist, C.byref(st_), None, capi.ptr(lists), len(lists), capi.ptr(lists), len(lists), C.byref(res))

    with sq.Context(0) as fresh:        # a context that never had tables
        assert call(fresh.h, C.byref(pv), C.byref(sv), len(P0)) == ERR_STATE
        assert capi.hip.shq_cooling_eval(fresh.h, 0, 4, capi.ptr(rho[:4].copy()), capi.ptr(u[:4].copy()), capi.ptr(ne[:4].copy()), None, None, capi.ptr(dt[:4].copy()),
                                         C.byref(case.uvbg()), 3.0, 0.0, 0.0, capi.ptr(np.zeros(4)), capi.ptr(np.zeros(4, dtype=np.int32)), None) == ERR_STATE
    sq.cooling_set_tables(cctx, case.tables())
    assert call(cctx.h, None, C.byref(sv), len(P0)) == ERR_INVALID
    assert call(cctx.h, C.byref(pv), None, len(P0)) == ERR_INVALID
    assert call(cctx.h, C.byref(pv), C.byref(sv), -1) == ERR_INVALID
    assert call(cctx.h, C.byref(pv), C.byref(sv), len(P0), _step(case, capi.COOL_UVBG_ZREION)) == ERR_STATE     # no Zreion table set
    assert _same_records(S, S0)
    bad = case.tables()
    bad.cooling = 5
    assert capi.hip.shq_cooling_set_tables(cctx.h, C.byref(bad)) == ERR_INVALID
    assert call(cctx.h, C.byref(pv), C.byref(sv), len(P0)) == 0           # the tables of before the refused call still stand
    after = winds()
    assert _same_records(before, after)
