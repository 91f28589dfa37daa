"""Independent restatement of the reference's radiative cooling (libgadget/cooling_rates.cpp, cooling.cpp, cooling_uvfluc.cpp,
sfr_eff.cpp:430-517) in plain Python: the rate fits, init_cooling_rates' tables, get_global_UVBG, the rate network, DoCooling and
cooling_direct, written from the reference's formulas as the nested loops they are there.  Every per-particle operation goes through the
`math` module (glibc's libm, as the C code) in the reference's order of operations, so a C engine that restates the same arithmetic must
agree bit for bit.  Also builds the 14 x 1000 table block the tests hand to the library."""
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# physconst.h
GRAVITY = 6.672e-8
RAD_CONST = 7.565e-15
BOLTZMANN = 1.38066e-16
BOLEVK = 8.61734e-5
eVinergs = 1.60218e-12
LIGHTCGS = 2.99792458e10
PROTONMASS = 1.6726e-24
ELECTRONMASS = 9.10953e-28
THOMPSON = 6.65245e-25
HUBBLE = 3.2407789e-18
GAMMA = 5.0 / 3.0
GAMMA_MINUS1 = GAMMA - 1
HYDROGEN_MASSFRAC = 0.76

Cen92, Verner96, Badnell06 = 0, 1, 2
KWH92, Enzo2Nyx, Sherwood = 0, 1, 2

NRECOMBTAB = 1000
RECOMBTMAX = math.log(1e9)
RECOMBTMIN = 0
MAXITER = 1000
ITERCONV = 1e-6

sqrt, exp, log, log10, pow_ = math.sqrt, math.exp, math.log, math.log10, math.pow


class CoolPar:
    """struct cooling_params with the reference's test defaults (tests/test_cooling_rates.cpp:33-48)"""

    def __init__(self, **kw):
        self.recomb = Verner96
        self.cooling = Sherwood
        self.SelfShieldingOn = 1
        self.PhotoIonizationOn = 1
        self.fBar = 0.17
        self.PhotoIonizeFactor = 1.0
        self.CMBTemperature = 2.7255
        self.MinGasTemp = 100.0
        self.UVRedshiftThreshold = -1.0
        self.HeliumHeatOn = 0
        self.HeliumHeatThresh = 10.0
        self.HeliumHeatAmp = 1.0
        self.HeliumHeatExp = 0.0
        self.rho_crit_baryon = 0.17 * 0.3 * 3.0 * (0.7 * HUBBLE) ** 2 / (8.0 * math.pi * GRAVITY)
        for k, v in kw.items():
            assert hasattr(self, k), k
            setattr(self, k, v)


# ---- the fits (cooling_rates.cpp:326-496, 735-905) -------------------------------------------------------------------------------------

def _verner96(temp, aa, bb, temp0, temp1):
    s0 = sqrt(temp / temp0)
    s1 = sqrt(temp / temp1)
    return aa / (s0 * pow_(1 + s0, 1 - bb) * pow_(1 + s1, 1 + bb))


def recomb_alphaHp(cp, temp):
    if cp.recomb == Cen92:
        return 8.4e-11 / sqrt(temp) / pow_(temp / 1000, 0.2) / (1 + pow_(temp / 1e6, 0.7))
    if cp.recomb == Verner96:
        return _verner96(temp, 7.982e-11, 0.748, 3.148, 7.036e+05)
    return _verner96(temp, 8.318e-11, 0.7472, 2.965, 7.001e5)


def _verner96_alphaHep(temp):
    low = _verner96(temp, 3.294e-11, 0.6910, 1.554e+01, 3.676e+07)
    high = _verner96(temp, 9.356e-10, 0.7892, 4.266e-02, 4.677e+06)
    swtmp, deltat = 7e5, 1e5
    upper, lower = swtmp + deltat, swtmp - deltat
    interp = (low * (upper - temp) + high * (temp - lower)) / (2 * deltat)
    return (temp < lower) * low + (temp > upper) * high + (upper > temp) * (temp > lower) * interp


def recomb_alphaHep(cp, temp):
    if cp.recomb == Cen92:
        return 1.5e-10 / pow_(temp, 0.6353)
    if cp.recomb == Verner96:
        return _verner96_alphaHep(temp)
    return _verner96(temp, 1.818E-10, 0.7492, 10.17, 2.786e6)


def recomb_alphad(cp, temp):
    if cp.recomb == Cen92:
        return 1.9e-3 / pow_(temp, 1.5) * exp(-4.7e5 / temp) * (1 + 0.3 * exp(-9.4e4 / temp))
    return 1.23e-3 / pow_(temp, 1.5) * exp(-4.72e5 / temp) * (1 + 0.3 * exp(-9.4e4 / temp))


def recomb_alphaHepd(cp, temp):
    return recomb_alphad(cp, temp) + recomb_alphaHep(cp, temp)


def recomb_alphaHepp(cp, temp):
    if cp.recomb == Cen92:
        return 4 * recomb_alphaHp(cp, temp)
    if cp.recomb == Verner96:
        return _verner96(temp, 1.891e-10, 0.7524, 9.370, 2.774e6)
    return _verner96(temp, 5.235E-11, 0.6988 + 0.0829 * exp(-1.682e5 / temp), 7.301, 4.475e6)


def _voronov96(temp, dE, PP, AA, XX, KK):
    UU = dE / (BOLEVK * temp)
    return AA * (1 + PP * sqrt(UU)) / (XX + UU) * pow_(UU, KK) * exp(-UU)


def recomb_GammaeH0(cp, temp):
    if cp.recomb == Cen92:
        return 5.85e-11 * sqrt(temp) * exp(-157809.1 / temp) / (1 + sqrt(temp / 1e5))
    return _voronov96(temp, 13.6, 0, 0.291e-07, 0.232, 0.39)


def recomb_GammaeHe0(cp, temp):
    if cp.recomb == Cen92:
        return 2.38e-11 * sqrt(temp) * exp(-285335.4 / temp) / (1 + sqrt(temp / 1e5))
    return _voronov96(temp, 24.6, 0, 0.175e-07, 0.180, 0.35)


def recomb_GammaeHep(cp, temp):
    if cp.recomb == Cen92:
        return 5.68e-12 * sqrt(temp) * exp(-631515.0 / temp) / (1 + sqrt(temp / 1e5))
    return _voronov96(temp, 54.4, 1, 0.205e-08, 0.265, 0.25)


def _t5(cp, temp):
    t0 = 1e5 if cp.cooling == KWH92 else 5e7
    return 1 + sqrt(temp / t0)


def cool_CollisionalH0(cp, temp):
    if cp.cooling == Enzo2Nyx:
        y = log(temp)
        Ryd = 2.1798741e-11
        tot = -0.75 / BOLTZMANN * Ryd / temp
        lowT = [213.7913, 113.9492, 25.06062, 2.762755, 0.1515352, 3.290382e-3]
        highT = [271.25446, 98.019455, 14.00728, 0.9780842, 3.356289e-2, 4.553323e-4]
        for j in range(6):
            tot += ((temp < 1e5) * lowT[j] + (temp >= 1e5) * highT[j]) * pow_(-y, j)
        return 1e-20 * exp(tot)
    return 7.5e-19 * exp(-118348.0 / temp) / _t5(cp, temp) + 13.5984 * eVinergs * recomb_GammaeH0(cp, temp)


def cool_CollisionalHe0(cp, temp):
    return 9.1e-27 * pow_(temp, -0.1687) * exp(-473638 / temp) / _t5(cp, temp) + 24.5874 * eVinergs * recomb_GammaeHe0(cp, temp)


def cool_CollisionalHeP(cp, temp):
    return 5.54e-17 * pow_(temp, -0.397) * exp(-473638. / temp) / _t5(cp, temp) + 54.417760 * eVinergs * recomb_GammaeHep(cp, temp)


def cool_RecombHp(cp, temp):
    if cp.cooling == Enzo2Nyx:
        return 2.851e-27 * sqrt(temp) * (5.914 - 0.5 * log(temp) + 0.01184 * pow_(temp, 1. / 3))
    return 0.75 * BOLTZMANN * temp * recomb_alphaHp(cp, temp)


def cool_RecombHeP(cp, temp):
    return 0.75 * BOLTZMANN * temp * recomb_alphaHep(cp, temp) + 6.526e-11 * recomb_alphad(cp, temp)


def cool_RecombHePP(cp, temp):
    if cp.cooling == Enzo2Nyx:
        return 1.140e-26 * sqrt(temp) * (6.607 - 0.5 * log(temp) + 7.459e-3 * pow_(temp, 1. / 3))
    return 0.75 * BOLTZMANN * temp * recomb_alphaHepp(cp, temp)


def cool_FreeFree(cp, temp, zz):
    if cp.cooling == Enzo2Nyx:
        lt = 2 * log10(temp / zz)
        if lt <= log10(3.2e5):
            gff = (0.79464 + 0.1243 * lt)
        else:
            gff = (2.13164 - 0.1240 * lt)
    else:
        gff = 1.1 + 0.34 * exp(-pow_(5.5 - log10(temp), 2) / 3.)
    return 1.426e-27 * sqrt(temp) * float(zz * zz) * gff


def cool_InverseCompton(cp, temp, redshift):
    tcmb_red = cp.CMBTemperature * (1 + redshift)
    return 4 * THOMPSON * RAD_CONST / (ELECTRONMASS * LIGHTCGS) * pow_(tcmb_red, 4) * BOLTZMANN * (temp - tcmb_red)


def cool_he_reion_factor(cp, nHcgs, helium, redshift):
    if not cp.HeliumHeatOn:
        return 1.
    rho = PROTONMASS * nHcgs / (1 - helium)
    overden = rho / (cp.rho_crit_baryon * pow_(1 + redshift, 3.0))
    if overden >= cp.HeliumHeatThresh:
        overden = cp.HeliumHeatThresh
    return cp.HeliumHeatAmp * pow_(overden, cp.HeliumHeatExp)


# rows of temp_tab (cooling_rates.cpp:989-1003)
ROW_FUNCS = [None, recomb_GammaeH0, recomb_GammaeHe0, recomb_GammaeHep, recomb_alphaHp, recomb_alphaHepd, recomb_alphaHepp,
             cool_CollisionalH0, cool_CollisionalHe0, cool_CollisionalHeP, cool_RecombHp, cool_RecombHeP, cool_RecombHePP,
             lambda cp, t: cool_FreeFree(cp, t, 1)]
R_GammaH0, R_GammaHe0, R_GammaHep, R_alphaHp, R_alphaHep, R_alphaHepp = 1, 2, 3, 4, 5, 6
R_collisH0, R_collisHe0, R_collisHeP, R_recombHp, R_recombHeP, R_recombHePP, R_freefree1 = 7, 8, 9, 10, 11, 12, 13


def build_rate_tables(cp):
    """init_cooling_rates' temp_tab (:1005-1024): [14][NRECOMBTAB], row 0 the log temperatures"""
    tab = np.zeros((14, NRECOMBTAB))
    for i in range(NRECOMBTAB):
        tab[0, i] = RECOMBTMIN + (RECOMBTMAX - RECOMBTMIN) * i / NRECOMBTAB
        tt = exp(tab[0, i])
        for r in range(1, 14):
            tab[r, i] = ROW_FUNCS[r](cp, tt)
    return tab


# ---- the UV background (:69-83, 113-270) -----------------------------------------------------------------------------------------------

def get_interp_data(xdata, ydata, xval):
    if xval > xdata[-1]:
        return xdata[-1]
    if xval < xdata[0]:
        return xdata[0]
    i = int(np.searchsorted(xdata, xval, side="right"))   # std::upper_bound
    return lerp(ydata[i - 1], ydata[i], (xval - xdata[i - 1]) / (xdata[i] - xdata[i - 1]))


def lerp(a, b, t):
    """std::lerp of libstdc++ for finite arguments"""
    if (a <= 0 and b >= 0) or (a >= 0 and b <= 0):
        return t * b + (1 - t) * a
    if t == 1:
        return b
    x = a + t * (b - a)
    if (t > 1) == (b > a):
        return x if b < x else b
    return x if b > x else b


class TreeCool:
    def __init__(self, path=None):
        path = path or os.path.join(GOLDEN, "TREECOOL_ep_2018p")
        rows = np.array([[float(x) for x in line.split()] for line in open(path) if line.strip()])
        self.log1z = [float(x) for x in rows[:, 0]]
        self.cols = [[log10(x) for x in rows[:, c]] for c in range(1, 7)]   # Gamma HI, HeI, HeII, Eps HI, HeI, HeII

    def photo_rate(self, cp, redshift, c):
        if not cp.PhotoIonizationOn:
            return 0.0
        log1z = log10(1 + redshift)
        if len(self.log1z) < 2 or log1z >= self.log1z[-1]:
            return 0.0
        return pow_(10, get_interp_data(self.log1z, self.cols[c], log1z)) * cp.PhotoIonizeFactor


GRAYOPAC_Z = [0., 1., 2., 3., 4., 5.]
GRAYOPAC_Y = [2.59e-18, 2.37e-18, 2.27e-18, 2.15e-18, 2.02e-18, 1.94e-18]


def self_shield_factors(cp, redshift):
    """the two constant factors of get_self_shield_dens (:226-235)"""
    greyopac = get_interp_data(GRAYOPAC_Z, GRAYOPAC_Y, redshift)
    return pow_(greyopac / 2.49e-18, -2. / 3), pow_(cp.fBar / 0.17, -1. / 3)


def get_self_shield_dens(cp, redshift, gJH0):
    if gJH0 == 0:
        return 1e10
    G12 = gJH0 / 1e-12
    A, C = self_shield_factors(cp, redshift)
    return 6.73e-3 * A * pow_(G12, 2. / 3) * C


def make_uvbg(gJH0=0., gJHep=0., gJHe0=0., epsH0=0., epsHep=0., epsHe0=0., self_shield_dens=0., zreion=0., J_UV=0.):
    return dict(J_UV=J_UV, gJH0=gJH0, gJHep=gJHep, gJHe0=gJHe0, epsH0=epsH0, epsHep=epsHep, epsHe0=epsHe0, self_shield_dens=self_shield_dens, zreion=zreion)


def get_global_UVBG(cp, tc, redshift):
    uv = make_uvbg()
    if not cp.PhotoIonizationOn:
        return uv
    uv["zreion"] = pow_(10, tc.log1z[-1]) - 1
    if cp.UVRedshiftThreshold >= 0.:
        uv["zreion"] = cp.UVRedshiftThreshold
        if redshift > cp.UVRedshiftThreshold:
            return uv
    uv["gJH0"] = tc.photo_rate(cp, redshift, 0)
    uv["gJHe0"] = tc.photo_rate(cp, redshift, 1)
    uv["gJHep"] = tc.photo_rate(cp, redshift, 2)
    uv["epsH0"] = tc.photo_rate(cp, redshift, 3)
    uv["epsHe0"] = tc.photo_rate(cp, redshift, 4)
    uv["epsHep"] = tc.photo_rate(cp, redshift, 5)
    uv["self_shield_dens"] = get_self_shield_dens(cp, redshift, uv["gJH0"])
    return uv


# ---- the network (:293-305, 499-683) ---------------------------------------------------------------------------------------------------

class Network:
    """The per-particle functions over one set of tables.  `evals` counts ne_internal evaluations; `left_table` is set when a lookup fell
    off the table (the reference then evaluates the fit; so does this)."""

    def __init__(self, cp, tab=None, metal=None):
        self.cp = cp
        self.tab = build_rate_tables(cp) if tab is None else tab
        self.rows = [[float(x) for x in self.tab[r]] for r in range(14)]
        self.metal = metal      # dict(dims, min, max, values (flat list)) or None
        self.evals = 0
        self.left_table = False

    def interp(self, logt, row):
        dind = (logt - RECOMBTMIN) / (RECOMBTMAX - RECOMBTMIN) * NRECOMBTAB
        index = int(dind)       # toward zero, as the C cast
        if index < 0 or index >= NRECOMBTAB - 1:
            self.left_table = True
            return ROW_FUNCS[row](self.cp, exp(logt))
        t = self.rows[row]
        return lerp(t[index], t[index + 1], dind - index)

    def self_shield_corr(self, nh, logt, ssdens):
        if not self.cp.SelfShieldingOn or nh < ssdens * 0.01:
            return 1
        T4 = exp(0.17 * (logt - log(1e4)))
        nSSh = 1.003 * ssdens * T4
        return 0.98 * pow_(1 + pow_(nh / nSSh, 1.64), -2.28) + 0.02 * pow_(1 + nh / nSSh, -0.84)

    def nH0_internal(self, logt, ne, uv, photofac):
        alphaHp = self.interp(logt, R_alphaHp)
        GammaeH0 = self.interp(logt, R_GammaH0)
        photorate = 0
        if uv["gJH0"] > 0. and ne > 1e-50:
            photorate = uv["gJH0"] / ne * photofac
        return alphaHp / (alphaHp + GammaeH0 + photorate)

    def nHe_internal(self, nh, logt, ne, uv, photofac):
        alphaHep = self.interp(logt, R_alphaHep)
        alphaHepp = self.interp(logt, R_alphaHepp)
        GammaHe0 = self.interp(logt, R_GammaHe0)
        GammaHep = self.interp(logt, R_GammaHep)
        if uv["gJHe0"] > 0. and ne > 1e-50:
            GammaHe0 += uv["gJHe0"] / ne * photofac
            GammaHep += uv["gJHep"] / ne * photofac
        if GammaHe0 > 1e-50:
            nHep = nh / (1 + alphaHep / GammaHe0 + GammaHep / alphaHepp)
            nHe0 = nHep * alphaHep / GammaHe0
            nHepp = nHep * GammaHep / alphaHepp
        else:
            nHep, nHe0, nHepp = 0, nh, 0
        return nHe0, nHep, nHepp

    def get_temp_internal(self, nebynh, ienergy, helium):
        hy_mass = 1 - helium
        muienergy = 4 / (hy_mass * (3 + 4 * nebynh) + 1) * ienergy
        temp = GAMMA_MINUS1 * PROTONMASS / BOLTZMANN * muienergy
        if temp < self.cp.MinGasTemp:
            return self.cp.MinGasTemp
        return temp

    def ne_internal(self, nh, ienergy, ne, helium, uv):
        self.evals += 1
        yy = helium / 4 / (1 - helium)
        logt = log(self.get_temp_internal(ne / nh, ienergy, helium))
        photofac = self.self_shield_corr(nh, logt, uv["self_shield_dens"])
        nH0 = self.nH0_internal(logt, ne, uv, photofac)
        nHp = 1. - nH0
        if nHp < 0:
            nHp = 0
        nHe0, nHep, nHepp = self.nHe_internal(nh, logt, ne, uv, photofac)
        return nh * nHp + yy * nHep + 2 * yy * nHepp, logt

    def get_equilib_ne(self, density, ienergy, helium, uv, ne_init):
        """returns (ne, logt); raises ArithmeticError where the reference ends the run"""
        nh = density * (1 - helium)
        if ne_init <= 0:
            ne_init = 1.0
        ne0 = ne_init
        logt = None
        for i in range(MAXITER):
            ne1, logt1 = self.ne_internal(nh, ienergy, ne0 * nh, helium, uv)
            ne1 /= nh
            if abs(ne1 - ne0) < ITERCONV:
                logt = logt1
                ne0 = ne1
                break
            ne2, logt1 = self.ne_internal(nh, ienergy, ne1 * nh, helium, uv)
            ne2 /= nh
            d = ne0 + ne2 - 2.0 * ne1
            pp = ne2
            if d > 1e-15 or d < -1e-15:
                pp = ne0 - (ne1 - ne0) * (ne1 - ne0) / d
            ne0 = pp
            if ne0 < 0:
                ne0 = 0
        else:
            raise ArithmeticError("rate network failed to converge")
        if not math.isfinite(ne0):
            raise ArithmeticError("rate network failed to converge")
        return ne0 * nh, logt

    def metal_rate(self, redshift, temp, nHcgs):
        """TableMetalCoolingRate with InterpNLinear<3>::eval (cooling_uvfluc.cpp:321-335, utils/interp.hpp:41-90)"""
        m = self.metal
        if m is None:
            return 0
        x = [redshift, log10(nHcgs), log10(temp)]
        dims = m["dims"]
        strides = [dims[1] * dims[2], dims[2], 1]
        xi, f = [0, 0, 0], [0., 0., 0.]
        for d in range(3):
            step = (m["max"][d] - m["min"][d]) / (dims[d] - 1)
            xd = (x[d] - m["min"][d]) / step
            if x[d] <= m["min"][d]:
                xi[d], f[d] = 0, 0
            elif x[d] >= m["max"][d]:
                xi[d], f[d] = dims[d] - 2, 1
            else:
                xi[d] = math.floor(xd)
                f[d] = xd - xi[d]
        ret = 0
        l0 = sum(strides[d] * xi[d] for d in range(3))
        for i in range(8):
            filt = 1.0
            l = l0
            for d in range(3):
                off = 1 if i & (1 << d) else 0
                filt *= f[d] if off else (1 - f[d])
                l += off * strides[d]
            ret += m["values"][l] * filt
        return ret

    def abundances(self, density, ienergy, helium, uv, ne_init):
        """what get_heatingcooling_rate, get_neutral_fraction_phys_cgs and get_helium_ion_phys_cgs compute after the solve"""
        ne, logt = self.get_equilib_ne(density, ienergy, helium, uv, ne_init)
        nh = density * (1 - helium)
        nebynh = ne / nh
        temp = self.get_temp_internal(nebynh, ienergy, helium)
        photofac = self.self_shield_corr(nh, logt, uv["self_shield_dens"])
        nH0 = self.nH0_internal(logt, ne, uv, photofac)
        nHe0, nHep, nHepp = self.nHe_internal(nh, logt, ne, uv, photofac)
        return ne, nh, nebynh, temp, logt, nH0, nHe0, nHep, nHepp

    def get_heatingcooling_rate(self, density, ienergy, helium, redshift, metallicity, uv, ne_equilib):
        """returns (LambdaNet in erg/s/g, ne/nh)"""
        cp = self.cp
        ne, nh, nebynh, temp, logt, nH0, nHe0, nHep, nHepp = self.abundances(density, ienergy, helium, uv, ne_equilib)
        yy = helium / 4 / (1 - helium)
        nHp = 1. - nH0
        if nHp < 0:
            nHp = 0
        nHep *= yy / nh
        nHe0 *= yy / nh
        nHepp *= yy / nh
        LambdaCollis = nebynh * (self.interp(logt, R_collisH0) * nH0 + self.interp(logt, R_collisHe0) * nHe0 + self.interp(logt, R_collisHeP) * nHep)
        LambdaRecomb = nebynh * (self.interp(logt, R_recombHp) * nHp + self.interp(logt, R_recombHeP) * nHep + self.interp(logt, R_recombHePP) * nHepp)
        cff = self.interp(logt, R_freefree1)
        if cp.cooling == Enzo2Nyx:
            LambdaFF = nebynh * (cff * (nHp + nHep) + cool_FreeFree(cp, temp, 2) * nHepp)
        else:
            LambdaFF = nebynh * (cff * (nHp + nHep) + 4 * cff * nHepp)
        LambdaCmptn = nebynh * cool_InverseCompton(cp, temp, redshift) / nh
        Lambda = LambdaCollis + LambdaRecomb + LambdaFF + LambdaCmptn
        Heat = (nH0 * uv["epsH0"] + nHe0 * uv["epsHe0"] + nHep * uv["epsHep"]) / nh
        Heat *= cool_he_reion_factor(cp, density, helium, redshift)
        MetalCooling = metallicity * self.metal_rate(redshift, temp, nh)
        LambdaNet = Heat - Lambda - MetalCooling
        return LambdaNet * ((1 - helium) * (1 - helium)) * density / PROTONMASS, nebynh

    def get_temp(self, density, ienergy, helium, uv, ne_init):
        ne, logt = self.get_equilib_ne(density, ienergy, helium, uv, ne_init)
        nh = density * (1 - helium)
        return self.get_temp_internal(ne / nh, ienergy, helium), ne / nh

    def get_neutral_fraction_phys_cgs(self, density, ienergy, helium, uv, ne_init):
        r = self.abundances(density, ienergy, helium, uv, ne_init)
        return r[5], r[2]

    def get_helium_ion_phys_cgs(self, ion, density, ienergy, helium, uv, ne_init):
        ne, nh, nebynh, temp, logt, nH0, nHe0, nHep, nHepp = self.abundances(density, ienergy, helium, uv, ne_init)
        yy = helium / 4 / (1 - helium)
        return yy * (nHe0, nHep, nHepp)[ion] / nh


# ---- cooling.cpp:42-163 -----------------------------------------------------------------------------------------------------------------

class Units:
    """struct cooling_units; the defaults are testDoCooling's (tests/test_cooling.cpp:177-195)"""

    def __init__(self, HubbleParam=0.7):
        UnitDensity_in_cgs = 6.76991e-22
        UnitTime_in_s = 3.08568e+16
        UnitMass_in_g = 1.989e+43
        UnitLength_in_cm = 3.08568e+21
        UnitEnergy_in_cgs = UnitMass_in_g * UnitLength_in_cm ** 2 / UnitTime_in_s ** 2
        self.density_in_phys_cgs = UnitDensity_in_cgs * HubbleParam * HubbleParam
        self.uu_in_cgs = UnitEnergy_in_cgs / UnitMass_in_g
        self.tt_in_s = UnitTime_in_s / HubbleParam


class Cooling:
    def __init__(self, net, units, lmfp_heat=0.0):
        self.net = net
        self.units = units
        self.lmfp_heat = lmfp_heat      # get_long_mean_free_path_heating(z) / (rho_crit_baryon (1+z)^3)

    def get_lambdanet(self, rho, u, redshift, Z, uv, ne_guess, heiii):
        lam, ne = self.net.get_heatingcooling_rate(rho, u, 1 - HYDROGEN_MASSFRAC, redshift, Z, uv, ne_guess)
        if not heiii:
            lam += self.lmfp_heat
        return lam, ne

    def DoCooling(self, redshift, u_old, rho, dt, uv, ne_guess, Z, MinEgySpec, heiii):
        """returns (unew in internal units, ne)"""
        cu = self.units
        rho *= cu.density_in_phys_cgs / PROTONMASS
        u_old *= cu.uu_in_cgs
        MinEgySpec *= cu.uu_in_cgs
        if u_old < MinEgySpec:
            u_old = MinEgySpec
        dt *= cu.tt_in_s
        u = u_old
        u_lower = u
        u_upper = u
        ne = ne_guess
        LambdaNet, ne = self.get_lambdanet(rho, u, redshift, Z, uv, ne, heiii)
        if u - u_old - LambdaNet * dt < 0:
            while True:
                u_lower = u_upper
                u_upper *= 1.1
                LambdaNet, ne = self.get_lambdanet(rho, u_upper, redshift, Z, uv, ne, heiii)
                if not (u_upper - u_old - LambdaNet * dt < 0):
                    break
        else:
            while True:
                u_upper = u_lower
                u_lower /= 1.1
                if u_upper <= MinEgySpec:
                    break
                LambdaNet, ne = self.get_lambdanet(rho, u_lower, redshift, Z, uv, ne, heiii)
                if not (u_lower - u_old - LambdaNet * dt > 0):
                    break
        it = 0
        while True:
            u = 0.5 * (u_lower + u_upper)
            if u_upper <= MinEgySpec:
                u = MinEgySpec
                break
            LambdaNet, ne = self.get_lambdanet(rho, u, redshift, Z, uv, ne, heiii)
            if u - u_old - LambdaNet * dt > 0:
                u_upper = u
            else:
                u_lower = u
            du = u_upper - u_lower
            it += 1
            if not (abs(du / u) > 1.0e-6 and it < MAXITER):
                break
        if it >= MAXITER:
            raise ArithmeticError("failed to converge in DoCooling()")
        return u / cu.uu_in_cgs, ne

    def GetCoolingTime(self, redshift, u_old, rho, uv, ne_guess, Z):
        cu = self.units
        rho *= cu.density_in_phys_cgs / PROTONMASS
        u_old *= cu.uu_in_cgs
        LambdaNet, ne = self.net.get_heatingcooling_rate(rho, u_old, 1 - HYDROGEN_MASSFRAC, redshift, Z, uv, ne_guess)
        if LambdaNet >= 0:
            return 0, ne
        return u_old / (-LambdaNet) / cu.tt_in_s, ne

    def query(self, what, redshift, u, rho, dt, uv, ne, Z, MinEgySpec, heiii):
        """one of the library's array-level queries for one particle: (out, ne after, ne_internal evaluations, left the table)"""
        net, cu = self.net, self.units
        net.evals, net.left_table = 0, False
        he = 1 - HYDROGEN_MASSFRAC
        rc, uc = rho * (cu.density_in_phys_cgs / PROTONMASS), u * cu.uu_in_cgs
        if what == "UNEW":
            out, ne = self.DoCooling(redshift, u, rho, dt, uv, ne, Z, MinEgySpec, heiii)
        elif what == "TCOOL":
            out, ne = self.GetCoolingTime(redshift, u, rho, uv, ne, Z)
        elif what == "NH0":
            out = net.get_neutral_fraction_phys_cgs(rc, uc, he, uv, ne)[0]
        elif what in ("HE0", "HEP", "HEPP"):
            out = net.get_helium_ion_phys_cgs(("HE0", "HEP", "HEPP").index(what), rc, uc, he, uv, ne)
        elif what == "TEMP":
            out, ne = net.get_temp(rc, uc, he, uv, ne)
        elif what == "LAMBDANET":
            out, ne = self.get_lambdanet(rc, uc, redshift, Z, uv, ne, heiii)
        else:
            raise ValueError(what)
        return out, ne, net.evals, net.left_table


WHATS = ["UNEW", "TCOOL", "NH0", "HE0", "HEP", "HEPP", "TEMP", "LAMBDANET"]


# ---- sfr_eff.cpp:430-517 and cooling_uvfluc.cpp:142-214 ---------------------------------------------------------------------------------

def entropy_to_u(density, a3inv):
    return exp(GAMMA_MINUS1 * log(density * a3inv)) / GAMMA_MINUS1


def eval_periodic(x, table, nside, boxsize):
    """InterpNLinear<3>::eval_periodic (utils/interp.hpp:93-129) with Min = 0, Max = BoxSize; table [nside]^3 flat, C order"""
    step = (boxsize - 0.0) / (nside - 1)
    xi, f = [0, 0, 0], [0., 0., 0.]
    for d in range(3):
        xd = (x[d] - 0.0) / step
        xi[d] = math.floor(xd)
        f[d] = xd - xi[d]
    ret = 0
    for i in range(8):
        filt = 1.0
        l = 0
        for d in range(3):
            off = 1 if i & (1 << d) else 0
            x1 = (xi[d] + off) % nside
            filt *= f[d] if off else (1 - f[d])
            l = l * nside + x1
        ret += table[l] * filt
    return ret


def local_uvbg(cp, mode, redshift, glob, pos, offset, zreion_table, J21, zre, j21_coeffs):
    """get_local_UVBG; mode 0 global, 1 the Zreion table (dict nside, boxsize, values), 2 J21"""
    if mode == 2:
        uv = make_uvbg(J_UV=J21, zreion=zre)
        uv["gJH0"] = j21_coeffs[0] * J21
        uv["epsH0"] = j21_coeffs[3] * J21 * 1.60218e-12
        uv["gJHe0"] = j21_coeffs[2] * J21
        uv["epsHe0"] = j21_coeffs[5] * J21 * 1.60218e-12
        uv["self_shield_dens"] = get_self_shield_dens(cp, redshift, uv["gJH0"])
        return uv
    if mode == 0:
        return dict(glob)
    z = eval_periodic([pos[d] - offset[d] for d in range(3)], zreion_table["values"], zreion_table["nside"], zreion_table["boxsize"])
    if z < redshift:
        return make_uvbg(self_shield_dens=glob["self_shield_dens"], zreion=z)
    uv = dict(glob)
    uv["zreion"] = z
    return uv


def on_eeqos(sfr, density, delaytime, a3inv):
    """the three clauses of sfreff_on_eeqos (:502-517)"""
    if not sfr["StarformationOn"]:
        return 0
    flag = 0
    if density * a3inv >= sfr["PhysDensThresh"]:
        flag = 1
    if density < sfr["OverDensThresh"]:
        flag = 0
    if delaytime > 0:
        flag = 0
    return flag


def cooling_direct(cool, sfr, redshift, a3inv, hubble, dloga, lastred, density, entropy, ne, Z, heiii, uv):
    """cooling_direct (:430-481) for one particle: (Entropy, Ne, bumped)"""
    dtime = dloga / hubble
    enttou = entropy_to_u(density, a3inv)
    uold = entropy * enttou
    if sfr["HIReionTemp"] > 0 and uv["zreion"] >= redshift and uv["zreion"] < lastred:
        meanweight = 4 / (8 - 6 * (1 - HYDROGEN_MASSFRAC))
        unew = sfr["temp_to_u"] / meanweight * sfr["HIReionTemp"]
        if uold > unew:
            unew = uold
        return unew / enttou, ne, True
    meanweight = 4.0 / (1 + 3 * HYDROGEN_MASSFRAC)
    MinEgySpec = sfr["temp_to_u"] / meanweight * sfr["MinGasTemp"]
    unew, ne = cool.DoCooling(redshift, uold, density * a3inv, dtime, uv, ne, Z, MinEgySpec, heiii)
    return unew / enttou, ne, False
