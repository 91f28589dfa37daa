"""Plain-Python restatement of the host part of metal_return() (libgadget/metal_return.cpp:157-462, 539-569): the same branch structure,
but roots by scipy.optimize.brentq at machine level, integrals by scipy.integrate.quad with break points at the table nodes, and ages by
quad of 1 / (a H).  It deliberately shares no closed form with the product (csrc/yields_math.hpp): what the reference approximates to
1e-4 (integrals) and 5e-3 (roots) is evaluated here to ~1e-13, so that the device's exact segment sums can be held to 1e-12.

Tables come from tests/golden/metal_yield_tables.npz (tools/extract_yield_tables.py), laid out value[mass index * nmet + metal index]."""
import math
import os
from bisect import bisect_right

import numpy as np
from scipy.integrate import quad
from scipy.optimize import brentq

HUBBLE = 3.2407789e-18          # h / s
SEC_PER_MEGAYEAR = 3.155e13
NMETALS = 9
EPSREL = 1e-13

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metal_yield_tables.npz")


class Bilinear2D:
    """utils/interp.hpp:9-28: xs = metallicities, ys = masses, zs[j * nx + i]; no clamp of tx, ty (extrapolates)"""

    def __init__(self, xs, ys, zs):
        self.xs, self.ys, self.zs = [float(v) for v in xs], [float(v) for v in ys], [float(v) for v in zs]
        self.nx, self.ny = len(self.xs), len(self.ys)

    def eval(self, x, y):
        xs, ys, zs, nx = self.xs, self.ys, self.zs, self.nx
        i = max(0, min(bisect_right(xs, x) - 1, nx - 2))
        j = max(0, min(bisect_right(ys, y) - 1, self.ny - 2))
        tx = (x - xs[i]) / (xs[i + 1] - xs[i])
        ty = (y - ys[j]) / (ys[j + 1] - ys[j])
        return ((1.0 - tx) * (1.0 - ty) * zs[j * nx + i] + tx * (1.0 - ty) * zs[j * nx + i + 1]
                + (1.0 - tx) * ty * zs[(j + 1) * nx + i] + tx * ty * zs[(j + 1) * nx + i + 1])


class Tables:
    def __init__(self, path=GOLDEN):
        d = np.load(path)
        self.raw = {k: np.ascontiguousarray(d[k], dtype=np.float64) for k in d.files}
        r = self.raw
        self.MAXMASS, self.MINMASS, self.SNAGBSWITCH = r["MAXMASS"].item(), r["MINMASS"].item(), r["SNAGBSWITCH"].item()
        self.lifetime_metallicity, self.lifetime_masses = r["lifetime_metallicity"], r["lifetime_masses"]
        self.agb_masses, self.agb_metallicities = r["agb_masses"], r["agb_metallicities"]
        self.snii_masses, self.snii_metallicities = r["snii_masses"], r["snii_metallicities"]
        self.sn1a_total_metals, self.sn1a_yields = r["sn1a_total_metals"].item(), r["sn1a_yields"]
        self.lifetime_interp = Bilinear2D(r["lifetime_metallicity"], r["lifetime_masses"], r["lifetime"])
        agb = lambda z: Bilinear2D(r["agb_metallicities"], r["agb_masses"], z)        # noqa: E731
        snii = lambda z: Bilinear2D(r["snii_metallicities"], r["snii_masses"], z)     # noqa: E731
        self.agb_mass_interp, self.agb_metallicity_interp = agb(r["agb_total_mass"]), agb(r["agb_total_metals"])
        self.agb_metals_interp = [agb(r["agb_yield"][i]) for i in range(NMETALS)]
        self.snii_mass_interp, self.snii_metallicity_interp = snii(r["snii_total_mass"]), snii(r["snii_total_metals"])
        self.snii_metals_interp = [snii(r["snii_yield"][i]) for i in range(NMETALS)]


def chabrier_imf(mass):
    """:159-167"""
    if mass <= 1:
        return 0.852464 / mass * math.exp(-(math.log10(mass / 0.079) / 0.69) ** 2 / 2)
    return 0.237912 * mass ** -2.3


def compute_imf_norm(T):
    """:287-294"""
    f = lambda m: m * chabrier_imf(m)      # noqa: E731
    return quad(f, T.MINMASS, 1.0, epsrel=EPSREL, epsabs=0)[0] + quad(f, 1.0, T.MAXMASS, epsrel=EPSREL, epsabs=0)[0]


def hubble_function(cos, a):
    """flat LCDM + radiation, in internal units (cos["Hubble"] = H0 in 1 / internal time)"""
    return cos["Hubble"] * math.sqrt(cos["Omega0"] / a**3 + cos["OmegaR"] / a**4 + (1 - cos["Omega0"] - cos["OmegaR"]))


def atime_to_myr(cos, a1, a2):
    """:170-178"""
    return quad(lambda a: 1 / (hubble_function(cos, a) * a), a1, a2, epsrel=EPSREL, epsabs=0)[0] * cos["UnitTime_in_s"] / SEC_PER_MEGAYEAR


def massendlife(T, mass, stellarmetal, dtfind):
    """:190-195"""
    return T.lifetime_interp.eval(stellarmetal, mass) / 1e6 - dtfind


def do_rootfinding(T, stellarmetal, dtfind, lo, hi):
    """:198-207, the bracket solved to machine precision"""
    return brentq(lambda m: massendlife(T, m, stellarmetal, dtfind), lo, hi, xtol=1e-300, rtol=4 * np.finfo(float).eps, maxiter=500)


def find_mass_bin_limits(T, dtstart, dtend, stellarmetal, margins=None):
    """:215-254.  margins (a list) collects |value| / scale of every branch condition evaluated, for the test's fairness check"""
    stellarmetal = min(max(stellarmetal, T.lifetime_metallicity[0]), T.lifetime_metallicity[-1])

    def cond(mass, dtfind):
        v = massendlife(T, mass, stellarmetal, dtfind)
        if margins is not None:
            margins.append(abs(v) / max(abs(dtfind), abs(v + dtfind)))
        return v
    if cond(T.MAXMASS, dtend) >= 0:
        return T.MAXMASS, T.MAXMASS
    if cond(T.agb_masses[0], dtend) <= 0:
        masslow = T.lifetime_masses[0]
    else:
        masslow = do_rootfinding(T, stellarmetal, dtend, T.agb_masses[0], T.MAXMASS)
    if cond(T.MAXMASS, dtstart) >= 0:
        masshigh = T.MAXMASS
    elif cond(masslow, dtstart) <= 0:
        masshigh = masslow
    else:
        masshigh = do_rootfinding(T, stellarmetal, dtstart, masslow, T.MAXMASS)
    return masslow, masshigh


def imf_integral(interp, metallicity, masslow, masshigh):
    """chabrier_imf_integ (:267-282) integrated over [masslow, masshigh], break points at the table's mass nodes"""
    y0, y1 = interp.ys[0], interp.ys[-1]

    def integrand(mass):
        intpmass = min(max(mass, y0), y1)
        return interp.eval(metallicity, intpmass) * (mass / intpmass) * chabrier_imf(mass)
    pts = [y for y in interp.ys if masslow < y < masshigh]
    if 1.0 not in pts and masslow < 1.0 < masshigh:
        pts.append(1.0)
    return quad(integrand, masslow, masshigh, points=pts or None, epsrel=EPSREL, epsabs=0, limit=200)[0]


def compute_agb_yield(T, interp, stellarmetal, masslow, masshigh):
    """:316-340"""
    masshigh = min(masshigh, T.SNAGBSWITCH)
    masslow = max(masslow, T.agb_masses[0])
    stellarmetal = max(min(stellarmetal, T.agb_metallicities[-1]), T.agb_metallicities[0])
    if masslow >= masshigh:
        return 0.0
    return imf_integral(interp, stellarmetal, masslow, masshigh)


def compute_snii_yield(T, interp, stellarmetal, masslow, masshigh):
    """:342-366"""
    masshigh = min(masshigh, T.snii_masses[-1])
    masslow = max(masslow, T.SNAGBSWITCH)
    stellarmetal = max(min(stellarmetal, T.snii_metallicities[-1]), T.snii_metallicities[0])
    if masslow >= masshigh:
        return 0.0
    return imf_integral(interp, stellarmetal, masslow, masshigh)


def sn1a_number(dtmyrstart, dtmyrend, hub, Sn1aN0):
    """:298-313"""
    sn1aindex, tau8msun = 1.12, 40.0
    if dtmyrend < tau8msun:
        return 0.0
    dtmyrstart = max(dtmyrstart, tau8msun)
    totalSN1a = 1 - (1 / (hub * HUBBLE * SEC_PER_MEGAYEAR) / tau8msun) ** (1 - sn1aindex)
    return Sn1aN0 / totalSN1a * ((dtmyrstart / tau8msun) ** (1 - sn1aindex) - (dtmyrend / tau8msun) ** (1 - sn1aindex))


def mass_yield(T, dtstart, dtend, stellarmetal, hub, Sn1aN0, imf_norm, masslow, masshigh):
    """:369-382"""
    agb = compute_agb_yield(T, T.agb_mass_interp, stellarmetal, masslow, masshigh)
    snii = compute_snii_yield(T, T.snii_mass_interp, stellarmetal, masslow, masshigh)
    return (agb + snii) / imf_norm + sn1a_number(dtstart, dtend, hub, Sn1aN0) * T.sn1a_total_metals


def metal_yield(T, dtstart, dtend, stellarmetal, hub, Sn1aN0, imf_norm, masslow, masshigh):
    """:385-407: (MetalGenerated, MetalYields[NMETALS]) as fractions of the initial SSP"""
    total = (compute_agb_yield(T, T.agb_metallicity_interp, stellarmetal, masslow, masshigh)
             + compute_snii_yield(T, T.snii_metallicity_interp, stellarmetal, masslow, masshigh)) / imf_norm
    species = np.zeros(NMETALS)
    for i in range(NMETALS):
        species[i] = (compute_agb_yield(T, T.agb_metals_interp[i], stellarmetal, masslow, masshigh)
                      + compute_snii_yield(T, T.snii_metals_interp[i], stellarmetal, masslow, masshigh)) / imf_norm
    n1a = sn1a_number(dtstart, dtend, hub, Sn1aN0)
    species += n1a * T.sn1a_yields
    return total + n1a * T.sn1a_total_metals, species


def maxmassfrac(T, hub, Sn1aN0, imf_norm):
    """:425"""
    return mass_yield(T, 0, 1 / (hub * HUBBLE * SEC_PER_MEGAYEAR), T.snii_metallicities[-1], hub, Sn1aN0, imf_norm, T.agb_masses[0], T.MAXMASS)


class FullRangeScales:
    """per yield quantity, the same table integral taken over the table's full mass range (AGB [agb_masses[0], SNAGBSWITCH], SNII
    [SNAGBSWITCH, last SNII node]) as a fraction of the SSP: the scale of the antiderivative, in which the tests' bounds are stated.
    The tables are linear in metallicity between nodes, so the integrals at the nodes (quad, once) interpolate exactly."""

    def __init__(self, T, imf_norm):
        self.T, self.imf_norm = T, imf_norm
        lo, hi = T.agb_masses[0], T.MAXMASS
        ia = [T.agb_mass_interp, T.agb_metallicity_interp] + T.agb_metals_interp
        isn = [T.snii_mass_interp, T.snii_metallicity_interp] + T.snii_metals_interp
        self.agb = np.array([[compute_agb_yield(T, t, z, lo, hi) for z in T.agb_metallicities] for t in ia])
        self.snii = np.array([[compute_snii_yield(T, t, z, lo, hi) for z in T.snii_metallicities] for t in isn])

    def __call__(self, stellarmetal):
        """(mass, metal, species[NMETALS]) at this metallicity: |AGB part| + |SNII part|, over imf_norm"""
        T = self.T
        za = min(max(stellarmetal, T.agb_metallicities[0]), T.agb_metallicities[-1])
        zs = min(max(stellarmetal, T.snii_metallicities[0]), T.snii_metallicities[-1])
        a = np.array([np.interp(za, T.agb_metallicities, row) for row in self.agb])
        b = np.array([np.interp(zs, T.snii_metallicities, row) for row in self.snii])
        s = (np.abs(a) + np.abs(b)) / self.imf_norm
        return s[0], s[1], s[2:]


def metal_return_init(T, P, S, active, cos, atime, hub, Sn1aN0, imf_norm, ages=None):
    """metal_return_init (:410-462) + the queue of metals_haswork (:123-132) + metal_return_copy's yields (:539-569).
    P: particle records (Type, PI, Mass float32); S: star slots (FormationTime, LastEnrichmentMyr float32; TotalMassReturned, Metallicity);
    S["LastEnrichmentMyr"] is rewritten as the reference does.  ages: precomputed StellarAges by slot (else quad per star).
    Returns a dict of the slot arrays, the queue, the queue arrays and the bookkeeping the tests compare."""
    nslot = len(S)
    out = dict(StellarAges=np.zeros(nslot), LowDyingMass=np.zeros(nslot), HighDyingMass=np.zeros(nslot), MassReturn=np.zeros(nslot),
               clamped=np.zeros(nslot, bool), rewritten=np.zeros(nslot, bool), margins=[], haswork_margin=[], clamp_margin=[])
    mmf = maxmassfrac(T, hub, Sn1aN0, imf_norm)
    out["maxmassfrac"] = mmf
    idx = np.arange(len(P)) if active is None else np.asarray(active)

    def haswork(i):
        pi = int(P["PI"][i])
        thr = 1e-3 * (float(P["Mass"][i]) + float(S["TotalMassReturned"][pi]))
        mr = out["MassReturn"][pi]
        if mr != 0:
            out["haswork_margin"].append(abs(mr - thr) / thr)
        return not mr < thr
    queue = []
    for i in idx:
        i = int(i)
        if P["Type"][i] != 4:
            continue
        slot = int(P["PI"][i])
        age = atime_to_myr(cos, float(S["FormationTime"][slot]), atime) if ages is None else float(ages[slot])
        out["StellarAges"][slot] = age
        tmr, Z, last = float(S["TotalMassReturned"][slot]), float(S["Metallicity"][slot]), float(S["LastEnrichmentMyr"][slot])
        initialmass = float(P["Mass"][i]) + tmr
        lo, hi = find_mass_bin_limits(T, last, age, Z, out["margins"])
        out["LowDyingMass"][slot], out["HighDyingMass"][slot] = lo, hi
        mr = initialmass * mass_yield(T, last, age, Z, hub, Sn1aN0, imf_norm, lo, hi)
        out["MassReturn"][slot] = mr
        out["clamp_margin"].append(abs(tmr + mr - initialmass * mmf) / (initialmass * mmf))
        if tmr + mr > initialmass * mmf:
            out["clamped"][slot] = True
            out["MassReturn"][slot] = max(initialmass * mmf - tmr, 0.0)
            if not haswork(i):
                S["LastEnrichmentMyr"][slot] = age
                out["rewritten"][slot] = True
                last = float(S["LastEnrichmentMyr"][slot])
        if haswork(i):
            queue.append(i)
    nq = len(queue)
    out["queue"] = np.array(queue, dtype=np.int32)
    out["MassGenerated"], out["MetalGenerated"], out["MetalSpeciesGenerated"] = np.zeros(nq), np.zeros(nq), np.zeros((nq, NMETALS))
    for k, i in enumerate(queue):
        slot = int(P["PI"][i])
        initialmass = float(P["Mass"][i]) + float(S["TotalMassReturned"][slot])
        tot, species = metal_yield(T, float(S["LastEnrichmentMyr"][slot]), out["StellarAges"][slot], float(S["Metallicity"][slot]), hub, Sn1aN0, imf_norm,
                                   out["LowDyingMass"][slot], out["HighDyingMass"][slot])
        out["MassGenerated"][k] = out["MassReturn"][slot]
        out["MetalGenerated"][k] = max(initialmass * tot, 0.0)
        out["MetalSpeciesGenerated"][k] = np.maximum(species * initialmass, 0.0)
    return out
