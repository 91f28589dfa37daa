"""The loops behind the run's log files restated in numpy from the reference's lines, and the cases the stats tests share.

  compute_global_quantities_of_system   libgadget/stats.cpp:235-272 (the loop), :289-361 (rank 0's block)
  write_blackhole_txt                   libgadget/bhinfo.cpp:176-184
  collect_BH_info                       libgadget/bhinfo.cpp:76-151

The loops are restated as per-particle addends: every addend is a handful of IEEE operations in the reference's order, so numpy forms the
same doubles as the reference and as the device (but for the one pow of the gas energy); what the order of a sum may do to it is the
tests' business."""
import functools
import math

import numpy as np

import shenqi_amd as sq
from shenqi_amd import capi
import cooling_restated as cr
import cooling_cases as cc
import startup_restated as st

SEED = 20261020
COUNTS = st.COUNTS                      # nothing, one lane, a wave less and more one, a workgroup and one, four tiles ragged, twenty
TIME = 0.25                             # redshift 3 exactly: the cooling cases' global UVBG
BOXSIZE = 20000.0
OFFSET = (0.25 * BOXSIZE, -0.125 * BOXSIZE, 0.0)
GAMMA_MINUS1 = (5.0 / 3.0) - 1
HYDROGEN_MASSFRAC = 0.76
SPH_DTYPE = st.SPH_REION_DTYPE
J21_COEFFS = (1.1e-12, 0.0, 6.0e-13, 7.0e-12, 0.0, 8.0e-12)
NOT_SWALLOWED = np.uint64(2 ** 64 - 1)  # (MyIDType) -1
COLUMNS = ("Mass", "EnergyPot", "EnergyKin", "Momentum0", "Momentum1", "Momentum2", "AngMomentum0", "AngMomentum1", "AngMomentum2", "CenterOfMass0",
           "CenterOfMass1", "CenterOfMass2")


# ---- stats.cpp:235-272 ------------------------------------------------------------------------------------------------------------------

def energy_addends(P, S, Time):
    """per type t (0..5) and column the addends of the particles of that type in index order, the gas addends of EnergyIntComp[0], the
    gas particles' indices and their get_temp inputs (Density, egyspec, Ne), the type counts and the number of particles of Type > 5"""
    a1 = Time
    a2 = Time * Time
    a3 = Time * Time * Time
    m = P["Mass"].astype(np.float64)
    pos, vel = P["Pos"], P["Vel"]
    col = {}
    col["Mass"] = m
    col["EnergyPot"] = 0.5 * m * P["Potential"] / a1
    col["EnergyKin"] = 0.5 * m * (vel[:, 0] * vel[:, 0] + vel[:, 1] * vel[:, 1] + vel[:, 2] * vel[:, 2]) / a2
    for j in range(3):
        col["Momentum%d" % j] = m * vel[:, j]
        col["CenterOfMass%d" % j] = m * pos[:, j]
    col["AngMomentum0"] = m * (pos[:, 1] * vel[:, 2] - pos[:, 2] * vel[:, 1])
    col["AngMomentum1"] = m * (pos[:, 2] * vel[:, 0] - pos[:, 0] * vel[:, 2])
    col["AngMomentum2"] = m * (pos[:, 0] * vel[:, 1] - pos[:, 1] * vel[:, 0])
    by_type = []
    for t in range(6):
        idx = np.flatnonzero(P["Type"] == t)
        by_type.append({c: [float(x) for x in col[c][idx]] for c in COLUMNS})
    gas = np.flatnonzero(P["Type"] == 0)
    slot = S[P["PI"][gas]]
    with np.errstate(all="ignore"):
        egyspec = slot["Entropy"] / GAMMA_MINUS1 * np.power(slot["Density"] / a3, GAMMA_MINUS1)
    eint = [float(x) for x in m[gas] * egyspec]
    count = [int((P["Type"] == t).sum()) for t in range(6)]
    return dict(by_type=by_type, eint=eint, gas=gas, density=slot["Density"].copy(), egyspec=egyspec, ne=slot["Ne"].copy(), mass=m[gas], count=count,
                n_bad_type=int((P["Type"] > 5).sum()))


# ---- stats.cpp:289-361 ------------------------------------------------------------------------------------------------------------------

def finish(s):
    """rank 0's block on a dict of the summed Comp members (lists; the vectors [6][4]); returns the state as a dict"""
    S = {k: [list(r) if isinstance(r, (list, tuple)) else float(r) for r in s[k]] for k in
         ("MassComp", "EnergyPotComp", "EnergyKinComp", "EnergyIntComp", "TemperatureComp", "MomentumComp", "AngMomentumComp", "CenterOfMassComp")}
    S["EnergyTotComp"] = [0.0] * 6
    for i in range(6):
        S["EnergyTotComp"][i] = S["EnergyKinComp"][i] + S["EnergyPotComp"][i] + S["EnergyIntComp"][i]
    S["Mass"] = S["EnergyKin"] = S["EnergyPot"] = S["EnergyInt"] = S["EnergyTot"] = 0.0
    for i in range(6):
        if S["MassComp"][i] > 0:
            S["TemperatureComp"][i] /= S["MassComp"][i]
    for k in ("Momentum", "AngMomentum", "CenterOfMass"):
        S[k] = [0.0] * 4
    for i in range(6):
        S["Mass"] += S["MassComp"][i]
        S["EnergyKin"] += S["EnergyKinComp"][i]
        S["EnergyPot"] += S["EnergyPotComp"][i]
        S["EnergyInt"] += S["EnergyIntComp"][i]
        S["EnergyTot"] += S["EnergyTotComp"][i]
        for j in range(3):
            S["Momentum"][j] += S["MomentumComp"][i][j]
            S["AngMomentum"][j] += S["AngMomentumComp"][i][j]
            S["CenterOfMass"][j] += S["CenterOfMassComp"][i][j]
    for i in range(6):
        for j in range(3):
            if S["MassComp"][i] > 0:
                S["CenterOfMassComp"][i][j] /= S["MassComp"][i]
    for j in range(3):
        if S["Mass"] > 0:
            S["CenterOfMass"][j] /= S["Mass"]
    for i in range(6):
        for k in ("CenterOfMassComp", "MomentumComp", "AngMomentumComp"):
            S[k][i][3] = 0.0
        for j in range(3):
            for k in ("CenterOfMassComp", "MomentumComp", "AngMomentumComp"):
                S[k][i][3] += S[k][i][j] * S[k][i][j]
        for k in ("CenterOfMassComp", "MomentumComp", "AngMomentumComp"):
            S[k][i][3] = math.sqrt(S[k][i][3]) if S[k][i][3] >= 0 else math.nan
    for k in ("CenterOfMass", "Momentum", "AngMomentum"):
        S[k][3] = 0.0
    for j in range(3):
        for k in ("CenterOfMass", "Momentum", "AngMomentum"):
            S[k][3] += S[k][j] * S[k][j]
    for k in ("CenterOfMass", "Momentum", "AngMomentum"):
        S[k][3] = math.sqrt(S[k][3]) if S[k][3] >= 0 else math.nan
    return S


# ---- bhinfo.cpp ----------------------------------------------------------------------------------------------------------------------------

def bh_totals(B):
    """(count, the addends of Mass, Mdot, Mdot / Mass) over the slots with SwallowID == (MyIDType) -1"""
    live = B[B["SwallowID"] == NOT_SWALLOWED]
    with np.errstate(all="ignore"):
        medd = live["Mdot"] / live["Mass"]
    return len(live), [[float(x) for x in a] for a in (live["Mass"], live["Mdot"], medd)]


PRIV_SCALARS = ("BH_Entropy", "BH_accreted_Mass", "BH_accreted_BHMass", "BH_FeedbackWeightSum", "NumDM", "MgasEnc", "KEflag", "SPH_SwallowID")
PRIV_VECTORS = ("BH_SurroundingGasVel", "BH_accreted_momentum")


def bh_info(P, B, priv, active, atime, offset):
    """collect_BH_info's records for the particles of `active`; priv: the BHPriv arrays by name, a missing one leaves its members zero"""
    info = np.zeros(len(active), dtype=sq.BHINFO_DTYPE)
    size = sq.BHINFO_DTYPE.itemsize - 8
    off = np.asarray(offset, dtype=np.float64)
    for i, p_i in enumerate(active):
        pp = P[p_i]
        assert 0 <= p_i < len(P) and pp["Type"] == 5
        PI = int(pp["PI"])
        bh = B[PI]
        r = info[i]
        r["size1"] = r["size2"] = size
        r["ID"] = pp["ID"]
        for k in ("Mass", "Mdot", "Density", "minTimeBin", "encounter", "MinPot", "SwallowID", "CountProgs", "Mtrack", "KineticFdbkEnergy", "VDisp"):
            r[k] = bh[k]
        for k in PRIV_SCALARS:
            if priv.get(k) is not None:
                r[k] = priv[k][PI]
        for k in PRIV_VECTORS:
            if priv.get(k) is not None:
                r[k] = priv[k][PI]
        r["MinPotPos"] = bh["MinPotPos"] - off
        r["Pos"] = pp["Pos"] - off
        r["BH_DragAccel"] = bh["DragAccel"]
        r["BH_DFAccel"] = bh["DFAccel"]
        r["BH_FullTreeGravAccel"] = pp["FullTreeGravAccel"]
        r["Velocity"] = pp["Vel"]
        r["BH_SurroundingDensity"] = bh["DF_SurroundingDensity"]
        r["BH_SurroundingRmsVel"] = bh["DF_SurroundingRmsVel"]
        r["BH_SurroundingVel"] = bh["DF_SurroundingVel"]
        r["Swallowed"] = (int(pp["Flags"]) >> 1) & 1
        r["Mdyn"] = np.float64(pp["Mass"])
        r["a"] = atime
    return info


# ---- the shared cases ------------------------------------------------------------------------------------------------------------------

def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)


class Case:
    """n particles of types 0..5, interleaved (particle k has type k % 6) or sorted by type, every member filled; gas slots in shuffled PI
    order with three unreferenced slots behind them.  Half of the gas slots hold (Density, egyspec) of internal-unit magnitudes, for
    which get_temp ends on MinGasTemp; the other half cgs-like magnitudes (1e-6 .. 1e2 protons / cm^3, the energy of 10^0.5 .. 10^9.5 K)
    where the network is solved and the hottest leave the rate table (DEFERRED).  From 63 particles on a few slots carry a negative
    Entropy and a zero Density (BADINPUT).  bad_type: one particle of Type 6."""

    def __init__(self, n, order="interleaved", bad_type=False, seed=SEED):
        rng = np.random.default_rng([seed, n, 0 if order == "interleaved" else 1])
        self.n = n
        P = np.zeros(n, dtype=capi.PARTICLE_DTYPE)
        st._fill(rng, P)
        types = (np.arange(n) % 6).astype(np.uint8)
        P["Type"] = types if order == "interleaved" else np.sort(types)
        if bad_type:
            P["Type"][np.flatnonzero(P["Type"] == 3)[1]] = 6
        P["Mass"] = (rng.uniform(0.5, 2.0, n) * 10.0 ** rng.choice([-4.0, 0.0, 5.0], n)).astype(np.float32)
        P["Pos"] = rng.uniform(0, 1, (n, 3)) * BOXSIZE
        gas = np.flatnonzero(P["Type"] == 0)
        ng = len(gas)
        S = np.zeros(ng + 3, dtype=SPH_DTYPE)
        st._fill(rng, S)
        P["PI"][gas] = rng.permutation(ng)
        ns = len(S)
        cgs = rng.random(ns) < 0.5
        dens = np.where(cgs, 10.0 ** rng.uniform(-6, 2, ns), 10.0 ** rng.uniform(-9, -2, ns))
        mu = 4.0 / (1 + 3 * HYDROGEN_MASSFRAC)
        u = np.where(cgs, 10.0 ** rng.uniform(0.5, 9.5, ns) * cr.BOLTZMANN / (GAMMA_MINUS1 * cr.PROTONMASS * mu), 10.0 ** rng.uniform(1, 5, ns))
        S["Density"] = dens
        S["Entropy"] = u * GAMMA_MINUS1 / np.power(dens / (TIME * TIME * TIME), GAMMA_MINUS1)
        S["Ne"] = np.where(rng.random(ns) < 0.1, 0.0, rng.uniform(0, 1.2, ns))
        S["local_J21"] = np.where(rng.random(ns) < 0.2, 0.0, 10.0 ** rng.uniform(-3, 2, ns))
        S["zreion"] = rng.uniform(2.5, 3.5, ns)
        if n >= 63:
            S["Entropy"][1] = -S["Entropy"][1]
            S["Density"][2] = 0.0
        self.P, self.S = P, S
        _ro(P, S)


@functools.lru_cache(maxsize=None)
def case(n, order="interleaved", bad_type=False):
    return Case(n, order, bad_type)


# ---- the temperature reference: the host engine on the restatement's per-particle inputs ---------------------------------------------------

@functools.lru_cache(maxsize=None)
def cooling():
    """the cooling cases' random set: Sherwood / Verner96, self-shielding on, the global UVB at z = 3"""
    return cc.random_case()[0]


@functools.lru_cache(maxsize=None)
def zreion_table():
    i = np.arange(5)
    x, y, z = np.meshgrid(i, i, i, indexing="ij")
    t = 3.0 + 0.1 * np.sin(1.3 * x + 0.4) * np.cos(0.9 * y) + 0.03 * z
    t.setflags(write=False)
    return t


def device_tables():
    """the context's tables: the run's units, which shq_energy_statistics must not apply, and the Zreion table"""
    return cooling().tables(zreion=zreion_table(), zreion_boxsize=BOXSIZE)


def unit_tables():
    """the same tables with units of one, so that shq_cooling_eval_host hands density and energy to the engine as they come: PROTONMASS /
    PROTONMASS and a factor 1.0 are exact"""
    c = cooling()
    cp = c.cp
    return sq.cooling_tables(c.net.tab, cooling=cp.cooling, SelfShieldingOn=cp.SelfShieldingOn, MinGasTemp=cp.MinGasTemp, CMBTemperature=cp.CMBTemperature,
                             HeliumHeatOn=cp.HeliumHeatOn, HeliumHeatThresh=cp.HeliumHeatThresh, HeliumHeatAmp=cp.HeliumHeatAmp, HeliumHeatExp=cp.HeliumHeatExp,
                             rho_crit_baryon=cp.rho_crit_baryon, fBar=cp.fBar, density_in_phys_cgs=cr.PROTONMASS, uu_in_cgs=1.0, tt_in_s=1.0)


def stats_params(mode, want_temperature=True):
    c = cooling()
    A, Cf = cr.self_shield_factors(c.cp, 1.0 / TIME - 1)
    return sq.stats_params(TIME, want_temperature, mode, c.uvbg(), OFFSET, J21_COEFFS, A, Cf)


@functools.lru_cache(maxsize=None)
def temperatures(n, order, mode, bad_type=False):
    """(T, status) per gas particle in index order from shq_cooling_eval_host(TEMP), the particles grouped by their local UVBG since the host
    entry takes one per call; T is NaN where the status is not OK"""
    k = case(n, order, bad_type)
    a = energy_addends(k.P, k.S, TIME)
    c = cooling()
    redshift = 1.0 / TIME - 1
    ztab = dict(nside=5, boxsize=BOXSIZE, values=[float(v) for v in zreion_table().ravel()])
    groups = {}
    for g, i in enumerate(a["gas"]):
        slot = k.S[k.P["PI"][i]]
        uv = cr.local_uvbg(c.cp, mode, redshift, c.uv, [float(v) for v in k.P["Pos"][i]], list(OFFSET), ztab, float(slot["local_J21"]), float(slot["zreion"]),
                           list(J21_COEFFS))
        groups.setdefault(tuple(sorted(uv.items())), []).append(g)
    T, status = np.full(len(a["gas"]), np.nan), np.zeros(len(a["gas"]), dtype=np.int32)
    tables = unit_tables()
    for key, members in groups.items():
        members = np.array(members)
        out, _, stt, _ = sq.cooling_eval_host(tables, "TEMP", a["density"][members], a["egyspec"][members], a["ne"][members], sq.cooling_uvbg(**dict(key)), redshift,
                                              nthreads=1)
        T[members], status[members] = out, stt
    _ro(T, status)
    return T, status


# ---- black holes ------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def bh_slots(n):
    """n black-hole slots, every member filled, a third swallowed"""
    rng = np.random.default_rng([SEED, n, 5])
    B = np.zeros(n, dtype=capi.BH_DTYPE)
    st._fill(rng, B)
    B["Mass"] = 10.0 ** rng.uniform(-5, -1, n)
    B["Mdot"] = 10.0 ** rng.uniform(-9, -3, n)
    B["SwallowID"] = np.where(np.arange(n) % 3 == 1, B["SwallowID"] >> np.uint64(1), NOT_SWALLOWED)
    _ro(B)
    return B


class BhCase:
    """1000 particles, 400 of them black holes at random places, their slots in shuffled PI order with three unreferenced slots behind;
    the BHPriv arrays by slot, SPH_SwallowID (sized by the gas slots in the reference) five entries longer"""

    def __init__(self, n=1000, nbh=400):
        rng = np.random.default_rng([SEED, n, 55])
        P = np.zeros(n, dtype=capi.PARTICLE_DTYPE)
        st._fill(rng, P)
        P["Type"] = rng.choice([0, 1, 4], n).astype(np.uint8)
        self.bh = np.sort(rng.choice(n, nbh, replace=False))
        P["Type"][self.bh] = 5
        P["PI"][self.bh] = rng.permutation(nbh)
        P["Pos"] = rng.uniform(0, 1, (n, 3)) * BOXSIZE
        B = np.zeros(nbh + 3, dtype=capi.BH_DTYPE)
        st._fill(rng, B)
        ns = len(B)
        priv = {k: rng.normal(size=ns) * 10.0 ** rng.uniform(-3, 3, ns) for k in PRIV_SCALARS[:6]}
        priv["KEflag"] = rng.integers(-2, 3, ns).astype(np.int32)
        priv["SPH_SwallowID"] = rng.integers(0, 2 ** 63, ns + 5).astype(np.uint64)
        for k in PRIV_VECTORS:
            priv[k] = rng.normal(size=(ns, 3)) * 100.0
        self.P, self.B, self.priv = P, B, priv
        _ro(P, B, *priv.values())

    def active(self, m):
        """m of the black holes, unordered"""
        return np.random.default_rng([SEED, m, 56]).permutation(self.bh)[:m].astype(np.int32)


@functools.lru_cache(maxsize=None)
def bh_case():
    return BhCase()
