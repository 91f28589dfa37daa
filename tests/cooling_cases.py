"""Shared inputs of the cooling tests (test_cooling_cpu.py, test_gpu_cooling.py): the reference's 20 x 20 DoCooling grid with its own
parameters, and the random particle set.  Everything is computed once and handed out read-only."""
import functools
import json
import math
import os

import numpy as np

import shenqi_amd as sq
import cooling_restated as cr

GOLDEN = json.load(open(os.path.join(cr.GOLDEN, "ref_docooling_tables.json")))


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


class Case:
    """one parameter set: the restatement's objects and the library's structs over the same tables"""

    def __init__(self, cp, units, redshift, lmfp_heat=0.0, metal=None, uvbg=None):
        self.cp, self.units, self.redshift, self.lmfp_heat = cp, units, redshift, lmfp_heat
        self.net = cr.Network(cp, metal=None if metal is None else dict(dims=list(metal[0].shape), min=list(metal[1]), max=list(metal[2]),
                                                                           values=[float(x) for x in metal[0].ravel()]))
        self.net.tab.setflags(write=False)
        self.cool = cr.Cooling(self.net, units, lmfp_heat)
        self.uv = cr.get_global_UVBG(cp, cr.TreeCool(), redshift) if uvbg is None else uvbg
        self.metal = metal

    def tables(self, **kw):
        cp, un = self.cp, self.units
        m = {} if self.metal is None else dict(metal=self.metal[0], metal_min=self.metal[1], metal_max=self.metal[2])
        m.update(kw)
        return sq.cooling_tables(self.net.tab, cooling=cp.cooling, SelfShieldingOn=cp.SelfShieldingOn, MinGasTemp=cp.MinGasTemp, CMBTemperature=cp.CMBTemperature,
                                 HeliumHeatOn=cp.HeliumHeatOn, HeliumHeatThresh=cp.HeliumHeatThresh, HeliumHeatAmp=cp.HeliumHeatAmp, HeliumHeatExp=cp.HeliumHeatExp,
                                 rho_crit_baryon=cp.rho_crit_baryon, fBar=cp.fBar, density_in_phys_cgs=un.density_in_phys_cgs, uu_in_cgs=un.uu_in_cgs,
                                 tt_in_s=un.tt_in_s, **m)

    def uvbg(self, uv=None):
        return sq.cooling_uvbg(**(self.uv if uv is None else uv))

    def restated(self, what, rho, u, ne, Z, heiii, dt, min_egy_spec, uv=None):
        """the restatement over arrays: (out, ne, evaluations, left the table)"""
        n = len(rho)
        out, neo, ev, left = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=bool)
        uv = self.uv if uv is None else uv
        for k in range(n):
            out[k], neo[k], ev[k], left[k] = self.cool.query(what, self.redshift, float(u[k]), float(rho[k]), float(dt[k]), uv, float(ne[k]), float(Z[k]),
                                                             min_egy_spec, int(heiii[k]))
        return out, neo, ev, left


@functools.lru_cache(maxsize=None)
def grid_case():
    """testDoCooling's setup (libgadget/tests/test_cooling.cpp:154-237): KWH92 / Cen92, no self-shielding, z = 0, dt = 0.2"""
    cp = cr.CoolPar(recomb=cr.Cen92, cooling=cr.KWH92, SelfShieldingOn=0, MinGasTemp=0.0,
                    rho_crit_baryon=0.045 * 3.0 * (0.7 * cr.HUBBLE) ** 2 / (8.0 * math.pi * cr.GRAVITY))
    case = Case(cp, cr.Units(0.7), 0.0)
    g = GOLDEN["docooling"]
    N = g["nstep"]
    rho = np.array([math.exp(math.log(g["dmin"]) + i * (math.log(g["dmax"]) - math.log(g["dmin"])) / 1. / N) for i in range(N) for j in range(N)])
    u = np.array([math.exp(math.log(g["umin"]) + j * (math.log(g["umax"]) - math.log(g["umin"])) / 1. / N) for i in range(N) for j in range(N)])
    meanweight = 4.0 / (1 + 3 * cr.HYDROGEN_MASSFRAC)
    min_egy_spec = 1 / meanweight * (1.0 / cr.GAMMA_MINUS1) * (cr.BOLTZMANN / cr.PROTONMASS) * 1 / case.units.uu_in_cgs
    n = N * N
    arrays = _ro(rho, u, np.ones(n), np.zeros(n), np.ones(n, dtype=np.uint8), np.full(n, g["dt"]))
    return case, arrays, min_egy_spec


def within_reference_gates(unew=None, tcool=None):
    """testDoCooling's two assertions (:230-232) on the 400 recorded values; the tolerance is relative to the smaller of the two, as Boost's"""
    g = GOLDEN["docooling"]
    ok = True
    if unew is not None:
        ref = np.array(g["unew_table"])
        ok &= bool(np.all(np.abs(unew - ref) <= g["unew_tol"] * np.minimum(np.abs(unew), np.abs(ref))))
    if tcool is not None:
        ref = np.array(g["tcool_table"])
        exempt = np.abs(1 / (1e-20 + tcool) - 1. / (1e-20 + ref)) < 1    # "if(fabs(1/(1e-20 + tcool) - 1./(1e-20 + tcool_table)) >= 1)" tests
        ok &= bool(np.all(exempt | (np.abs(tcool - ref) <= g["tcool_tol"] * np.minimum(np.abs(tcool), np.abs(ref)))))
    return ok


# The random set's seed was chosen on the CPU: with it the host engine agrees with a second host run in which every log / exp / pow
# result is moved by one ulp in alternating sign (SHQ_COOL_NUDGE) within the hard bound for every particle, see test_gpu_cooling.py.
RANDOM_SEED = 20261018
RANDOM_N = 4133
RANDOM_LMFP = 1e-5          # erg / s / g: of the order of the photoheating of mean-density gas, so the HeIII flag matters
RANDOM_DT = (0.0, 2e-4, 2e-3, 2e-2)


@functools.lru_cache(maxsize=None)
def random_case(n=RANDOM_N, seed=RANDOM_SEED):
    """Sherwood / Verner96, self-shielding on, the global UVB at z = 3; log-uniform physical density 1e-8 .. 10 cm^-3 and energy
    equivalent to 1e2 .. 1e8 K, Z in 0 .. 0.05, mixed HeIII flags and time bins (one with dt = 0)"""
    cp = cr.CoolPar()
    case = Case(cp, cr.Units(0.7), 3.0, RANDOM_LMFP)
    un = case.units
    rng = np.random.default_rng(seed)
    nphys = 10.0 ** rng.uniform(-8, 1, n)
    rho = nphys * cr.PROTONMASS / un.density_in_phys_cgs
    temp = 10.0 ** rng.uniform(2, 8, n)
    mu = 4.0 / (1 + 3 * cr.HYDROGEN_MASSFRAC)      # neutral gas
    u = temp * cr.BOLTZMANN / (cr.GAMMA_MINUS1 * cr.PROTONMASS * mu) / un.uu_in_cgs
    ne = rng.uniform(0, 1.2, n)
    ne[rng.random(n) < 0.05] = 0.0
    Z = rng.uniform(0, 0.05, n)
    heiii = (rng.random(n) < 0.5).astype(np.uint8)
    dt = np.array(RANDOM_DT)[rng.integers(0, len(RANDOM_DT), n)]
    min_egy_spec = cr.BOLTZMANN / (cr.GAMMA_MINUS1 * cr.PROTONMASS) / un.uu_in_cgs / mu * cp.MinGasTemp
    return case, _ro(rho, u, ne, Z, heiii, dt), min_egy_spec


@functools.lru_cache(maxsize=None)
def host_result(which, what):
    """shq_cooling_eval_host on the grid or the random set, once"""
    case, (rho, u, ne, Z, heiii, dt), mes = grid_case() if which == "grid" else random_case()
    r = sq.cooling_eval_host(case.tables(), what, rho, u, ne, case.uvbg(), case.redshift, Z=Z, heiii=heiii, dt=dt, min_egy_spec=mes, lmfp_heat=case.lmfp_heat)
    return _ro(*r)


@functools.lru_cache(maxsize=None)
def metal_case():
    """the random set with a smooth positive 3 x 4 x 5 metal table over (z, log10 nH, log10 T) whose axes end inside the particles' range
    on both sides: the cloudy table of the reference is 4 MB and needs a reader the tests do not have"""
    base, arrays, mes = random_case()
    i, j, k = np.meshgrid(np.arange(3), np.arange(4), np.arange(5), indexing="ij")
    table = 1e-23 * (1.0 + 0.5 * i + 0.3 * np.sin(j) ** 2 + 0.2 * k * k)
    table.setflags(write=False)
    case = Case(base.cp, base.units, base.redshift, base.lmfp_heat, metal=(table, (2.0, -6.0, 3.5), (4.0, -1.0, 6.5)))
    return case, arrays, mes
