"""The star population of tests/test_gpu_yields.py (and of tools/time_yields.py, which tiles it): every branch of metal_return_init by
construction.  Ages are set through FormationTime (float32) by inverting the cosmic-time table; the oracle then takes its ages by quad
from the float32 values, so nothing here needs to be exact."""
import math

import numpy as np

import yields_restated as yr
from shenqi_amd import capi

COSMO = dict(Hubble=0.1, Omega0=0.2814, OmegaR=8.5e-5, UnitTime_in_s=3.08568e16)
HUBBLEPARAM, SN1AN0, ATIME = 0.679, 1.3e-3, 1.0
TABLE = dict(amin=0.1, amax=1.0, n=8192)


def time_table():
    import shenqi_amd as sq
    return sq.cosmic_time_table(lambda a: yr.hubble_function(COSMO, a), TABLE["amin"], TABLE["amax"], TABLE["n"], COSMO["UnitTime_in_s"])


def special_metallicities(T):
    """below, at, between and above the nodes of each of the three metallicity axes, and exactly 0"""
    out = [0.0]
    for ax in (T.lifetime_metallicity, T.agb_metallicities, T.snii_metallicities):
        out += list(ax) + list(0.5 * (ax[1:] + ax[:-1])) + [0.3 * ax[0], 1.7 * ax[-1]]
    return np.array(out)


def population(T, tt, mmf, seed, nstar=3000, ngas=600, ndm=400):
    """(P, S, active, kinds, ages): particle records, star slots, an active list that mixes all types and leaves some stars out, the
    construction group of every slot, and the oracle's age of every slot (quad of 1 / (a H) from the float32 FormationTime)"""
    rng = np.random.default_rng(seed)
    loga0, dloga, Tt, _ = tt
    lna = loga0 + dloga * np.arange(len(Tt))
    tnow = np.interp(math.log(ATIME), lna, Tt)
    age_max = tnow - np.interp(math.log(0.1005), lna, Tt)

    def formation(age):          # scale factor at which a star of this age formed
        return np.exp(np.interp(tnow - np.asarray(age, dtype=np.float64), Tt, lna))
    zs = special_metallicities(T)
    Z = np.where(rng.random(nstar) < 0.5, rng.choice(zs, nstar), rng.uniform(0, 0.06, nstar))
    age, last, tmrfrac = np.zeros(nstar), np.zeros(nstar), rng.uniform(0, 0.2, nstar)
    life = lambda z, m: T.lifetime_interp.eval(min(max(z, T.lifetime_metallicity[0]), T.lifetime_metallicity[-1]), m) / 1e6      # noqa: E731
    kinds = np.empty(nstar, dtype="U8")
    c = 0

    def take(k, name):
        nonlocal c
        sl = slice(c, c + k)
        kinds[sl] = name
        c += k
        return sl
    s = take(500, "young")           # nothing has died: younger than life(MAXMASS)
    age[s] = rng.uniform(0.05, 4.2, 500)
    last[s] = age[s] * rng.choice([0.0, 0.5], 500)
    s = take(300, "old")             # everything dies: older than life(agb_masses[0]) at low metallicity
    Z[s] = rng.choice([0.0, 0.0001, 0.0004, 0.001, 0.003], 300)
    age[s] = rng.uniform(7200, age_max, 300)
    last[s] = age[s] * rng.choice([0.0, 0.3, 0.9, 0.999], 300)
    s = take(20, "same")             # LastEnrichmentMyr == age (as a float): masshigh = masslow
    age[s] = np.exp(rng.uniform(math.log(6), math.log(6000), 20))
    last[s] = np.nan                 # filled below from the float32 age
    s = take(200, "straddle")        # bins across the AGB table edge (7.5), the switch (8) and the SNII table edge (13)
    for i in range(s.start, s.stop):
        mlo, mhi = [(rng.uniform(6.5, 7.4), rng.uniform(7.6, 7.9)), (rng.uniform(7.6, 7.9), rng.uniform(8.1, 12)), (rng.uniform(8.5, 12.5), rng.uniform(13.5, 30)),
                    (rng.uniform(2, 7), rng.uniform(14, 39))][i % 4]
        age[i], last[i] = life(Z[i], mlo), life(Z[i], mhi)
    s = take(200, "narrow")          # bins 1e-3 Myr wide
    age[s] = np.exp(rng.uniform(math.log(5.5), math.log(200), 200))
    last[s] = age[s] - 1e-3
    s = take(200, "sn1a")            # either side of 40 Myr, where SN Ia switches on
    age[s] = rng.uniform(38, 42, 200)
    last[s] = np.where(rng.random(200) < 0.5, rng.uniform(30, 38, 200), age[s] - rng.uniform(0.01, 0.5, 200))
    s = take(240, "clamp")           # TotalMassReturned at the maxmassfrac clamp: work left, none left, already beyond it
    age[s] = np.exp(rng.uniform(math.log(300), math.log(9000), 240))
    last[s] = age[s] * rng.choice([0.0, 0.05], 240)
    tmrfrac[s] = mmf - np.tile([0.01, 1e-4, -0.02], 80)
    s = take(nstar - c, "generic")   # LastEnrichmentMyr before and after life(MAXMASS)
    age[s] = np.exp(rng.uniform(math.log(4.5), math.log(age_max), s.stop - s.start))
    last[s] = age[s] * rng.choice([0.0, 0.01, 0.5, 0.9, 0.99, 0.999, 0.9995, 0.9999], s.stop - s.start, p=[0.04, 0.04, 0.04, 0.04, 0.04, 0.3, 0.3, 0.2])

    S = np.zeros(nstar, dtype=capi.STAR_DTYPE)
    S["FormationTime"] = formation(age).astype(np.float32)
    S["Metallicity"] = Z
    ages = np.array([yr.atime_to_myr(COSMO, float(f), ATIME) for f in S["FormationTime"]])      # the oracle's ages, by slot
    S["LastEnrichmentMyr"] = np.where(np.isnan(last), ages, last).astype(np.float32)
    n = nstar + ngas + ndm
    types = np.concatenate([np.full(nstar, 4, np.uint8), np.zeros(ngas, np.uint8), np.ones(ndm, np.uint8)])
    perm = rng.permutation(n)
    P = np.zeros(n, dtype=capi.PARTICLE_DTYPE)
    P["Type"] = types[perm]
    P["Mass"] = rng.uniform(0.5, 1.5, n).astype(np.float32)
    P["ID"] = np.arange(n) + 1
    isstar = P["Type"] == 4
    P["PI"][isstar] = rng.permutation(nstar)                  # PI is permuted
    P["PI"][P["Type"] == 0] = rng.permutation(ngas)
    mass_of_slot = np.zeros(nstar)
    mass_of_slot[P["PI"][isstar]] = P["Mass"][isstar]
    S["TotalMassReturned"] = tmrfrac / (1 - tmrfrac) * mass_of_slot
    active = rng.permutation(n)[: int(0.9 * n)].astype(np.int32)
    return P, S, active, kinds, ages
