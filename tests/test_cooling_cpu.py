"""Radiative cooling without a GPU: (1) the Python restatement (cooling_restated.py) passes the reference's own gates, (2) the library's
host engine (shq_cooling_eval_host, csrc/cooling_math.hpp driven in a plain loop) equals the restatement bit for bit on the same tables,
for every query, with equal evaluation counts, and (3) the engine alone meets the reference's recorded DoCooling table."""
import math

import numpy as np
import pytest

import shenqi_amd as sq
from shenqi_amd import capi
import cooling_restated as cr
import cooling_cases as cc

G = cc.GOLDEN


def _close(a, b, tol):
    """Boost's tt::tolerance: relative to both"""
    return abs(a - b) <= tol * min(abs(a), abs(b))


# ---- (1) the restatement against the reference's gates -----------------------------------------------------------------------------------

def test_restated_uvbg_values():
    cp = cr.CoolPar()
    tc = cr.TreeCool()
    hi = cr.get_global_UVBG(cp, tc, 16)
    assert hi["epsH0"] == 0 and hi["gJH0"] == 0 and hi["self_shield_dens"] > 1e8
    for z, key in ((0.0, "uvbg_z0"), (3.0, "uvbg_z3")):
        uv = cr.get_global_UVBG(cp, tc, z)
        for k, want in G[key].items():
            assert _close(uv[k], want, G["uvbg_tol"]), (z, k, uv[k], want)


def test_restated_rate_network():
    """test_rate_network (tests/test_cooling_rates.cpp:119-168)"""
    cp = cr.CoolPar()
    net = cr.Network(cp)
    uv = cr.get_global_UVBG(cp, cr.TreeCool(), 2)
    for dens, he, tol in ((1e-6, 0.24, 3e-5), (1e-6, 0.12, 3e-5), (1e-5, 0.24, 3e-4), (1e-4, 0.24, 2e-3)):
        ne, _ = net.get_equilib_ne(dens, 200. * 1e10, he, uv, 1)
        assert _close(ne / (dens * (1 - he)), 1 + 2 * he / (1 - he) / 4, tol)
    ne = 1.
    temp, ne = net.get_temp(1e-4, 200. * 1e10, 0.24, uv, ne)
    assert 9500 < temp < 9510
    t4, ne = net.get_temp(1e-4, 400. * 1e10, 0.24, uv, ne)
    t2, ne = net.get_temp(1e-4, 200. * 1e10, 0.24, uv, ne)
    assert _close(t4, 2 * t2, 1e-3)
    t1, ne = net.get_temp(1, 200. * 1e10, 0.24, uv, ne)
    assert _close(t1, 14700, 200.)
    for dens in (1e-5, 1e-6, 1e-7):
        x, ne = net.get_neutral_fraction_phys_cgs(dens, 200. * 1e10, 0.24, uv, ne)
        assert _close(x, dens * 0.3113, 1e-3)
    x, ne = net.get_neutral_fraction_phys_cgs(1, 100., 0.24, uv, ne)
    assert x > 0.95
    x, ne = net.get_neutral_fraction_phys_cgs(0.1, 100. * 1e10, 0.24, uv, ne)
    assert 0.735 < x < 0.75
    net0 = cr.Network(cr.CoolPar(SelfShieldingOn=0))
    x, ne = net0.get_neutral_fraction_phys_cgs(1, 100. * 1e10, 0.24, uv, ne)
    assert x < 0.25
    x, ne = net0.get_neutral_fraction_phys_cgs(0.1, 100. * 1e10, 0.24, uv, ne)
    assert x < 0.05


def test_restated_heatingcooling_rate():
    """test_heatingcooling_rate (:172-251)"""
    h = G["heatingcooling"]
    cp = cr.CoolPar(recomb=cr.Cen92, cooling=cr.KWH92, SelfShieldingOn=0)
    net = cr.Network(cp)
    un = cr.Units(h["HubbleParam"])
    egyhot = h["egyhot"] * un.uu_in_cgs
    dens = h["dens"] * (un.density_in_phys_cgs / cr.PROTONMASS)
    lam, ne = net.get_heatingcooling_rate(dens, egyhot, 1 - cr.HYDROGEN_MASSFRAC, 0, 0, cr.make_uvbg(), 1.0)
    assert _close(egyhot / (-lam) / un.tt_in_s, h["tcool"], h["tol"])
    uv = cr.get_global_UVBG(cp, cr.TreeCool(), 0)
    assert uv["epsHep"] > 0 and uv["gJHe0"] > 0
    dens /= 100
    lam, ne = net.get_heatingcooling_rate(dens, egyhot / 10., 1 - cr.HYDROGEN_MASSFRAC, 0, 0, uv, ne)
    assert _close(lam, h["lambda_uvb"], h["tol"])
    lam, ne = net.get_heatingcooling_rate(dens / 2.5, egyhot / 10., 1 - cr.HYDROGEN_MASSFRAC, 0, 0, uv, ne)
    assert lam > 0
    net1 = cr.Network(cr.CoolPar(recomb=cr.Cen92, cooling=cr.KWH92, SelfShieldingOn=1))
    lam, ne = net1.get_heatingcooling_rate(dens * 1.5, egyhot / 10., 1 - cr.HYDROGEN_MASSFRAC, 0, 0, uv, ne)
    assert not lam > 0 and _close(lam, h["lambda_selfshield"], h["tol"])


def test_restated_docooling_grid():
    """testDoCooling (tests/test_cooling.cpp:154-237)"""
    case, (rho, u, ne, Z, heiii, dt), mes = cc.grid_case()
    g = G["docooling"]
    for k in ("epsH0", "epsHe0", "epsHep"):
        assert _close(case.uv[k], G["uvbg_z0"][k], 1e-5)
    p = g["tcool_point"]
    assert _close(case.cool.GetCoolingTime(0, p["u"], p["rho"], case.uv, 1.0, 0)[0], p["value"], p["tol"])
    p = g["unew_point"]
    assert _close(case.cool.DoCooling(0, p["u"], p["rho"], p["dt"], case.uv, 1.0, 0, mes, 1)[0], p["value"], p["tol"])
    unew = case.restated("UNEW", rho, u, ne, Z, heiii, dt, mes)[0]
    tcool = case.restated("TCOOL", rho, u, ne, Z, heiii, dt, mes)[0]
    assert not np.isnan(unew).any()
    assert cc.within_reference_gates(unew=unew)
    assert cc.within_reference_gates(tcool=tcool)


# ---- (2) the host engine against the restatement, same tables, bit for bit ---------------------------------------------------------------

@pytest.mark.parametrize("what", cr.WHATS)
@pytest.mark.parametrize("which", ["grid", "random"])
def test_host_engine_equals_restatement(which, what):
    case, (rho, u, ne, Z, heiii, dt), mes = cc.grid_case() if which == "grid" else cc.random_case()
    out, neo, status, steps = cc.host_result(which, what)
    r_out, r_ne, r_ev, r_left = case.restated(what, rho, u, ne, Z, heiii, dt, mes)
    # none of these particles leaves the table (the restatement would then have evaluated a fit the library does not have)
    assert not r_left.any() and np.all(status == capi.COOL_OK)
    assert np.array_equal(steps, r_ev)
    assert np.array_equal(out.view(np.uint64), r_out.view(np.uint64)), np.nonzero(out != r_out)[0][:8]
    if what in ("NH0", "HE0", "HEP", "HEPP"):
        assert np.array_equal(neo, ne)        # ne is an input only
    else:
        assert np.array_equal(neo.view(np.uint64), r_ne.view(np.uint64))


@pytest.mark.parametrize("redshift", [1.5, 3.0, 5.0])
def test_host_engine_metal_table(redshift):
    """TableMetalCoolingRate with the clamps at both ends of each axis: the redshift below, inside and above the table, the random set's
    densities and temperatures on all three sides of the other two axes"""
    case, (rho, u, ne, Z, heiii, dt), mes = cc.metal_case()
    s = slice(0, 400)
    Zs = Z[s] * 20      # up to solar, so that the table matters
    lognh = np.log10(rho[s] * case.units.density_in_phys_cgs / cr.PROTONMASS * 0.76)
    assert (lognh < -6).any() and (lognh > -1).any() and ((lognh > -6) & (lognh < -1)).any()
    host = sq.cooling_eval_host(case.tables(), "LAMBDANET", rho[s], u[s], ne[s], case.uvbg(), redshift, Z=Zs, heiii=heiii[s], lmfp_heat=case.lmfp_heat)
    plain = sq.cooling_eval_host(cc.random_case()[0].tables(), "LAMBDANET", rho[s], u[s], ne[s], case.uvbg(), redshift, Z=Zs, heiii=heiii[s], lmfp_heat=case.lmfp_heat)
    assert np.mean(host[0] != plain[0]) > 0.9
    temp = sq.cooling_eval_host(case.tables(), "TEMP", rho[s], u[s], ne[s], case.uvbg(), redshift)[0]
    assert (temp < 10 ** 3.5).any() and (temp > 10 ** 6.5).any()
    old = case.redshift
    try:
        case.redshift = redshift
        r = case.restated("LAMBDANET", rho[s], u[s], ne[s], Zs, heiii[s], np.zeros(400), mes)
    finally:
        case.redshift = old
    assert np.array_equal(r[0].view(np.uint64), host[0].view(np.uint64)) and np.array_equal(r[2], host[3])


def test_host_engine_threads_do_not_matter():
    case, (rho, u, ne, Z, heiii, dt), mes = cc.random_case()
    a = cc.host_result("random", "UNEW")
    b = sq.cooling_eval_host(case.tables(), "UNEW", rho, u, ne, case.uvbg(), case.redshift, Z=Z, heiii=heiii, dt=dt, min_egy_spec=mes, lmfp_heat=case.lmfp_heat, nthreads=1)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


# ---- (3) the engine against the reference's recorded values, nothing in between ----------------------------------------------------------

def test_host_engine_meets_recorded_tables():
    unew = cc.host_result("grid", "UNEW")[0]
    tcool = cc.host_result("grid", "TCOOL")[0]
    assert cc.within_reference_gates(unew=unew)
    assert cc.within_reference_gates(tcool=tcool)


# ---- statuses and arguments ----------------------------------------------------------------------------------------------------------------

def test_host_engine_statuses():
    case, (rho, u, ne, Z, heiii, dt), mes = cc.random_case()
    un = case.units
    mu = 0.6
    u_hot = 3e9 * cr.BOLTZMANN / (cr.GAMMA_MINUS1 * cr.PROTONMASS * mu) / un.uu_in_cgs      # T > 1e9 K: off the table
    rho4 = np.array([rho[0], rho[1], 0.0, rho[3], rho[4]])
    u4 = np.array([u[0], u_hot, u[2], np.nan, -1.0])
    ne4 = np.array([1.0, 1.0, 1.0, 1.0, 1.0])
    out, neo, status, steps = sq.cooling_eval_host(case.tables(), "UNEW", rho4, u4, ne4, case.uvbg(), case.redshift, Z=0.0, heiii=0, dt=2e-3, min_egy_spec=mes)
    assert list(status) == [capi.COOL_OK, capi.COOL_DEFERRED, capi.COOL_BADINPUT, capi.COOL_BADINPUT, capi.COOL_BADINPUT]
    assert np.isfinite(out[0]) and np.isnan(out[1:]).all()
    assert np.array_equal(neo[1:], ne4[1:])
    # the restatement leaves the table for the same particle
    assert case.cool.query("UNEW", case.redshift, float(u4[1]), float(rho4[1]), 2e-3, case.uv, 1.0, 0.0, mes, 0)[3]


def test_host_engine_bad_arguments():
    case, (rho, u, ne, Z, heiii, dt), mes = cc.random_case()
    t = case.tables()
    with pytest.raises(sq.ShqError):
        sq.cooling_eval_host(t, "UNEW", rho[:4], u[:4], 1.0, case.uvbg(), 3.0)             # UNEW without dt
    bad = case.tables()
    bad.cooling = 7
    with pytest.raises(sq.ShqError):
        sq.cooling_eval_host(bad, "TCOOL", rho[:4], u[:4], 1.0, case.uvbg(), 3.0)
    tab = np.array(case.net.tab)
    tab[5, 17] = math.inf
    with pytest.raises(sq.ShqError):
        sq.cooling_eval_host(sq.cooling_tables(tab), "TCOOL", rho[:4], u[:4], 1.0, case.uvbg(), 3.0)
