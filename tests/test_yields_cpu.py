"""The restatement of metal_return's host part (tests/yields_restated.py) held to the reference's own gates
(libgadget/tests/test_metal_return.cpp:12-64), and the cubic-Hermite age interpolation the device uses against quad of 1 / (a H).
The host-compiled maxmassfrac of shq_yields_init needs a context (a device): that check is in tests/test_gpu_yields.py."""
import math

import numpy as np
import pytest
from scipy.integrate import quad

import yields_restated as yr

COSMO = dict(Hubble=0.1, Omega0=0.2814, OmegaR=8.5e-5, UnitTime_in_s=3.08568e16)      # H0 = 0.1 h / internal time: kpc / (km / s) units


@pytest.fixture(scope="module")
def T():
    return yr.Tables()


@pytest.fixture(scope="module")
def imf_norm(T):
    return yr.compute_imf_norm(T)


def test_imf_norm(imf_norm):
    assert abs(imf_norm / 0.936976167457 - 1) < 1e-2


def test_yield_gates(T, imf_norm):
    agb = yr.compute_agb_yield(T, T.agb_mass_interp, 0.01, 1, 40)
    agb2 = yr.compute_agb_yield(T, T.agb_mass_interp, 0.01, 1, T.SNAGBSWITCH)
    assert abs(agb / agb2 - 1) < 1e-3

    def chabrier_mass(m):       # the test file's own integrand: natural log below 1, where the library has log10; only [0.28, 1] feels it
        imf = 0.852464 / m * math.exp(-(math.log(m / 0.079) / 0.69) ** 2 / 2) if m <= 1 else 0.237912 * m ** -2.3
        return m * imf
    agbmax = quad(chabrier_mass, T.raw["agb_total_mass"][0], T.SNAGBSWITCH, points=[1.0], epsrel=1e-12)[0]
    sniimax = quad(chabrier_mass, T.SNAGBSWITCH, T.snii_masses[-1], epsrel=1e-12)[0]
    snii = yr.compute_snii_yield(T, T.snii_mass_interp, 0.01, 1, 40)
    sn1a = yr.sn1a_number(0, 1500, 0.679, 1.3e-3) * T.sn1a_total_metals
    assert sn1a < 1.3e-3
    assert agb < agbmax and snii < sniimax
    assert (snii + sn1a + agb) / imf_norm < 1


def test_mass_bin_limits(T):
    lo1, hi1 = yr.find_mass_bin_limits(T, 0, 30, 0.02)
    lo2, hi2 = yr.find_mass_bin_limits(T, 30, 60, 0.02)
    los, his = yr.find_mass_bin_limits(T, 0, 60, 0.02)
    assert abs(lo1 / hi2 - 1) < 1e-2
    assert abs(los / lo2 - 1) < 1e-2
    assert abs(his / hi1 - 1) < 1e-2 and hi1 == T.MAXMASS


def test_lifetime_decreases_on_the_bracket(T):
    """what makes the device's segment inversion the unique root: strictly decreasing in mass on [1, 40] at any (clamped) metallicity"""
    masses = np.concatenate([T.lifetime_masses[(T.lifetime_masses >= 0.6) & (T.lifetime_masses <= 40)], np.linspace(1, 40, 400)])
    masses.sort()
    for Z in np.linspace(T.lifetime_metallicity[0], T.lifetime_metallicity[-1], 60):
        life = np.array([T.lifetime_interp.eval(Z, m) for m in masses])
        assert (np.diff(life)[np.diff(masses) > 0] < 0).all()


def test_closed_form_of_one_integral(T):
    """the fact the product rests on, stated independently of it: over [1.3, 8] at Z = 0.01 the agb_total_mass integral is the sum over
    mass segments of the antiderivative of (alpha + beta m) 0.237912 m^-2.3"""
    Z, lo, hi = 0.01, 1.3, 8.0
    I = T.agb_mass_interp
    edges = [lo] + [m for m in I.ys if lo < m < hi] + [hi]
    total = 0.0
    for a, b in zip(edges[:-1], edges[1:]):
        w = lambda m: I.eval(Z, min(m, I.ys[-1])) * (m / min(m, I.ys[-1]))      # noqa: E731
        beta = (w(b) - w(a)) / (b - a)
        alpha = w(a) - beta * a
        F = lambda m: alpha * m ** -1.3 / -1.3 + beta * m ** -0.3 / -0.3        # noqa: E731
        total += 0.237912 * (F(b) - F(a))
    ref = yr.compute_agb_yield(T, I, Z, lo, hi)
    assert abs(total / ref - 1) < 1e-13


def hermite_age(loga0, dloga, Tt, dT, f, a):
    """the interpolant the device integrates (csrc/yields_math.hpp), in plain numpy: T(a) - T(f)"""
    def at(x):
        s = (math.log(x) - loga0) / dloga
        k = min(max(int(math.floor(s)), 0), len(Tt) - 2)
        u = s - k
        m0, m1 = dT[k] * dloga, dT[k + 1] * dloga
        return ((2 * u**3 - 3 * u**2 + 1) * Tt[k] + (u**3 - 2 * u**2 + u) * m0 + (-2 * u**3 + 3 * u**2) * Tt[k + 1] + (u**3 - u**2) * m1)
    return at(a) - at(f)


def test_hermite_age_table():
    """n = 4096 nodes over a in [0.005, 1]: the interpolated age against quad of 1 / (a H), relative to the age; measured 1.9e-13"""
    import shenqi_amd as sq
    n = 4096
    loga0, dloga, Tt, dT = sq.cosmic_time_table(lambda a: yr.hubble_function(COSMO, a), 0.005, 1.0, n, COSMO["UnitTime_in_s"])
    rng = np.random.default_rng(3)
    worst = 0.0
    for _ in range(300):
        f = math.exp(rng.uniform(math.log(0.0051), math.log(0.95)))
        a = min(1.0, f * math.exp(rng.uniform(0.02, 3.0)))
        ref = yr.atime_to_myr(COSMO, f, a)
        worst = max(worst, abs(hermite_age(loga0, dloga, Tt, dT, f, a) / ref - 1))
    print("hermite age, n = 4096: max relative error", worst)
    assert worst <= 1e-10
