"""Restatement in numpy of the start-up loops of libgadget/init.cpp (check_omega :203-214, check_positions :313-335,
check_smoothing_length :342-359, init()'s loop :119-188, check_density_entropy :363-388) and of set_init_hsml (density2.cpp:164-203),
one particle at a time as the reference writes them, with a counter per branch, and the cases the CPU and GPU tests share."""
import collections
import functools
import math

import numpy as np

from shenqi_amd import capi

SEED = 20261019
COUNTS = (0, 1, 63, 65, 257, 1000, 5000)   # nothing, one lane, a wave less and more one, a workgroup and one, four tiles ragged, twenty
BOXSIZE = 20000.0
GAMMA_MINUS1 = (5.0 / 3.0) - 1
HYDROGEN_MASSFRAC = 0.76
OMEGA, POSITIONS, HSML, INIT = 1, 2, 4, 8
NOFIELD = capi.NOFIELD

# a gas slot of an EXCUR_REION build: local_J21 and zreion behind the members of SPH_DTYPE, and eight bytes no loop owns
_f = capi.SPH_DTYPE.fields
SPH_REION_DTYPE = np.dtype({"names": list(capi.SPH_DTYPE.names) + ["local_J21", "zreion", "spare"],
                            "formats": [_f[k][0] for k in capi.SPH_DTYPE.names] + ["<f8", "<f8", "<u8"],
                            "offsets": [_f[k][1] for k in capi.SPH_DTYPE.names] + [176, 184, 192], "itemsize": 200})


class Params:
    def __init__(self, RestartSnapNum, init_reion, generations=4):
        self.BoxSize = BOXSIZE
        self.MassTable = np.array([0.03, 0.5, 0.25, 0.0, 0.02, 1e-3])
        self.MeanSeparation = np.array([31.25, 62.5, 125.0, 0.0, 40.0, 500.0])
        self.Ti_Current = 0x123456789
        self.generations = generations
        self.RestartSnapNum = RestartSnapNum
        self.init_reion = init_reion


def bytes_copy(a):
    """a copy that keeps the padding bytes between the members (ndarray.copy() of a structured array need not)"""
    return a.view(np.uint8).copy().view(a.dtype)


# ---- the record loops -----------------------------------------------------------------------------------------------------------------

def particles(P, S, B, par, which, counters=None):
    """the loops of `which` over copies of the records: (P, S, B, report dict).  S may carry local_J21 / zreion or not."""
    P, S, B = bytes_copy(P), bytes_copy(S), bytes_copy(B)
    c = collections.Counter() if counters is None else counters
    rep = dict(mass_type=[[] for _ in range(6)], mass_all=[], badmass=0, noutside=0, first_outside=-1, numzero=0, lastzero=-1, numprob=0, lastprob=-1,
               nbad_delaytime=0, first_bad_delaytime=-1)
    has_reion = "local_J21" in S.dtype.names and "zreion" in S.dtype.names
    for i in range(len(P)):
        t = int(P["Type"][i])
        c["type%d" % t] += 1
        if which & OMEGA:
            if P["Mass"][i] == 0:
                gen = int(P["Flags"][i]) >> 4
                if t < 6:
                    P["Mass"][i] = np.float32(par.MassTable[t] * (1. - float(gen) / par.generations))
                rep["badmass"] += 1
                c["recovered"] += 1
            if t < 6:
                rep["mass_type"][t].append(float(P["Mass"][i]))
            rep["mass_all"].append(float(P["Mass"][i]))
        if which & POSITIONS:
            pos = P["Pos"][i]
            out = False
            for j in range(3):
                if pos[j] < 0:
                    c["negative"] += 1
                    out = True
                elif pos[j] > par.BoxSize:
                    c["toolarge"] += 1
                    out = True
                elif not math.isfinite(pos[j]):   # only a NaN gets here: an infinity is negative or too large
                    c["nan"] += 1
                    out = True
                if math.isinf(pos[j]):
                    c["inf"] += 1
            if out:
                rep["noutside"] += 1
                if rep["first_outside"] < 0:
                    rep["first_outside"] = i
            if pos[0] < 1e-35 and pos[1] < 1e-35 and pos[2] < 1e-35:
                rep["numzero"] += 1
                rep["lastzero"] = i
                c["zero"] += 1
        if which & HSML and t in (0, 5):
            h = P["Hsml"][i]
            if h > par.BoxSize or h <= 0:
                c["hsml_large" if h > par.BoxSize else ("hsml_zero" if h == 0 else "hsml_negative")] += 1
                P["Hsml"][i] = par.MeanSeparation[t]
                rep["numprob"] += 1
                rep["lastprob"] = i
        if which & INIT:
            P["Ti_drift"][i] = par.Ti_Current
            pi = int(P["PI"][i])
            if par.RestartSnapNum == -1 and t == 5:
                B["Mass"][pi] = P["Mass"][i]
                c["bh_mass"] += 1
            if t == 4 and P["Hsml"][i] == 0:
                P["Hsml"][i] = 0.1 * par.MeanSeparation[0]
                c["star_hsml"] += 1
            if t == 5:
                B["DFAccel"][pi] = 0
                B["DragAccel"][pi] = 0
            if t != 0:
                continue
            S["HydroAccel"][pi] = 0
            if not math.isfinite(S["DelayTime"][pi]):
                rep["nbad_delaytime"] += 1
                if rep["first_bad_delaytime"] < 0:
                    rep["first_bad_delaytime"] = i
                c["bad_delaytime"] += 1
            S["DtEntropy"][pi] = 0
            if par.RestartSnapNum == -1:
                c["ic"] += 1
                for k in ("Density", "EgyWtDensity", "DhsmlEgyDensityFactor", "Entropy"):
                    S[k][pi] = -1
                S["Ne"][pi] = 1.0
                for k in ("DivVel", "CurlVel", "DelayTime", "Metallicity", "Sfr", "MaxSignalVel"):
                    S[k][pi] = 0
                S["Metals"][pi] = 0
                S["Metals"][pi][0] = np.float32(HYDROGEN_MASSFRAC)
                S["Metals"][pi][1] = np.float32(1 - HYDROGEN_MASSFRAC)
            else:
                c["restart"] += 1
            if not has_reion:
                c["reion_absent"] += 1
            elif par.init_reion:
                S["local_J21"][pi] = 0
                S["zreion"][pi] = -1
                c["reion_on"] += 1
            else:
                c["reion_off"] += 1
    return P, S, B, rep


def check_density_entropy(S, meanbar, MinEgySpec, atime, counters=None):
    """(S after the loop, bad, the slots whose Entropy was raised)"""
    S = bytes_copy(S)
    c = collections.Counter() if counters is None else counters
    a3 = math.pow(atime, 3)
    bad, raised = 0, []
    for i in range(len(S)):
        rho = S["Density"][i]
        if rho <= 0 or not math.isfinite(rho):
            c["density_nonpositive" if rho <= 0 else ("density_nan" if math.isnan(rho) else "density_inf")] += 1
            S["Density"][i] = meanbar
            bad += 1
        e = S["EgyWtDensity"][i]
        if e <= 0 or not math.isfinite(e):
            S["EgyWtDensity"][i] = S["Density"][i]
            c["egy_replaced"] += 1
        minent = GAMMA_MINUS1 * MinEgySpec / math.pow(S["Density"][i] / a3, GAMMA_MINUS1)
        if S["Entropy"][i] < minent:
            S["Entropy"][i] = minent
            raised.append(i)
            c["entropy_below"] += 1
        else:
            c["entropy_above"] += 1
    return S, bad, np.array(raised, dtype=np.int64)


def minent(S, MinEgySpec, atime):
    return GAMMA_MINUS1 * MinEgySpec / np.power(S["Density"] / math.pow(atime, 3), GAMMA_MINUS1)


# ---- set_init_hsml --------------------------------------------------------------------------------------------------------------------

def set_init_hsml(nodes, firstnode, father, P, MeanGasSeparation, DesNumNgb, BoxSize, counters=None):
    """density2.cpp:164-203 on a NODE array numbered from firstnode and the Father array: (Hsml, the node each climb ended on with -1 for
    skipped particles, counts of the conditions "Bad tree moments" and "Bad hsml guess")"""
    c = collections.Counter() if counters is None else counters
    hsml = P["Hsml"].copy()
    out = np.full(len(P), -1, dtype=np.int64)
    badmom = badhsml = 0
    for i in range(len(P)):
        if P["Type"][i] != 0 and P["Type"][i] != 5:
            c["other_type"] += 1
            continue
        if P["Flags"][i] & 1:
            c["garbage"] += 1
            continue
        mass = float(P["Mass"][i])
        no = i
        levels = 0
        while True:
            p = int(nodes["father"][no - firstnode]) if no >= firstnode else int(father[i])
            if p < firstnode:
                c["root_reached" if no >= firstnode else "not_in_tree"] += 1
                break
            no = p
            levels += 1
            if not 10 * DesNumNgb * mass > nodes["mass"][no - firstnode]:
                break
        c["climb%d" % min(levels, 3)] += 1
        h = MeanGasSeparation
        if no >= firstnode:
            nd = nodes[no - firstnode]
            if nd["len"] > BoxSize or nd["mass"] < mass:
                badmom += 1
            testhsml = nd["len"] * math.pow(3.0 / (4 * math.pi) * DesNumNgb * mass / nd["mass"], 1.0 / 3)
            if testhsml < 500. * MeanGasSeparation:
                h = testhsml
            else:
                c["fallback"] += 1
        if h <= 0:
            badhsml += 1
        hsml[i] = h
        out[i] = no
    return hsml, out, badmom, badhsml


# ---- the shared cases -----------------------------------------------------------------------------------------------------------------

def _fill(rng, arr):
    for name in arr.dtype.names:
        ft = arr.dtype.fields[name][0]
        shape = (len(arr),) + ft.shape
        if ft.base.kind == "f":
            arr[name] = (rng.uniform(0.5, 2.0, shape) * 10.0 ** rng.uniform(-3, 3, shape) * rng.choice([-1.0, 1.0], shape)).astype(ft.base)
        elif ft.base.kind == "u":
            arr[name] = rng.integers(0, np.iinfo(ft.base).max, shape, dtype=ft.base, endpoint=True)
        else:
            arr[name] = rng.integers(np.iinfo(ft.base).min, np.iinfo(ft.base).max, shape, dtype=ft.base, endpoint=True)


class Case:
    """n particles of interleaved types 0, 1, 2, 4, 5 (and a few of type 3), gas and black-hole slots in shuffled PI order with three
    unreferenced slots behind them, every member filled.  Masses of three magnitudes, every fifth zero; positions inside the box except
    for the first rows, which carry a negative, a too-large, a NaN and an infinite coordinate and `nzero` positions at the origin; Hsml
    faults (too large, zero, negative, NaN) on gas and black holes, stars with Hsml == 0; DelayTime NaN and infinite on some gas."""

    def __init__(self, n, reion=True, nzero=2, seed=SEED):
        rng = np.random.default_rng([seed, n])
        self.n = n
        P = np.zeros(n, dtype=capi.PARTICLE_DTYPE)
        _fill(rng, P)
        k = np.arange(n)
        P["Type"] = rng.permutation(np.array([0, 1, 2, 4, 5, 0, 1, 0, 5, 4, 3])[k % 11]).astype(np.uint8)
        if n == 1:
            P["Type"] = 0
        P["Flags"] = rng.integers(0, 256, n).astype(np.uint8)
        P["Mass"] = (rng.uniform(0.5, 2.0, n) * 10.0 ** rng.choice([-4.0, 0.0, 5.0], n)).astype(np.float32)
        P["Mass"][rng.permutation(k % 5 == 1)] = 0
        P["Pos"] = rng.uniform(0, 1, (n, 3)) * BOXSIZE
        P["Hsml"] = rng.uniform(1e-3, 0.1, n) * BOXSIZE
        faults = [2 * BOXSIZE, 0.0, -3.0, np.nan, np.nextafter(BOXSIZE, np.inf), BOXSIZE]
        for t in (0, 5):
            idx = np.flatnonzero(P["Type"] == t)
            for j, v in enumerate(faults[:max(len(idx) - 1, 0)]):
                P["Hsml"][idx[-1 - j]] = v
        stars = np.flatnonzero(P["Type"] == 4)
        P["Hsml"][stars[::3]] = 0
        edges = [[-1e-300, 5.0, 6.0], [1.0, np.nextafter(BOXSIZE, np.inf), 2.0], [3.0, 4.0, np.nan], [np.inf, 1.0, 1.0], [BOXSIZE, 0.0, BOXSIZE], [7.0, -np.inf, 8.0]]
        for j, e in enumerate(edges[:max(n - 3, 0)]):
            P["Pos"][3 + 5 * j if 3 + 5 * j < n else j] = e
        for j in range(min(nzero, n)):
            P["Pos"][n - 1 - 7 * j if n > 7 * j else j] = [0.0, 1e-36, 0.0]
        sdt = SPH_REION_DTYPE if reion else capi.SPH_DTYPE
        self.slots = {}
        for t, dt in ((0, sdt), (5, capi.BH_DTYPE)):
            idx = np.flatnonzero(P["Type"] == t)
            S = np.zeros(len(idx) + 3, dtype=dt)
            _fill(rng, S)
            P["PI"][idx] = rng.permutation(len(idx))
            self.slots[t] = S
        S = self.slots[0]
        S["DelayTime"][::7] = np.nan
        S["DelayTime"][3::11] = -np.inf
        self.P, self.S, self.B = P, S, self.slots[5]
        for a in (self.P, self.S, self.B):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def case(n, reion=True, nzero=2):
    return Case(n, reion, nzero)


MODES = {"ic": Params(-1, True), "restart": Params(3, False), "restart_reion": Params(3, True)}
MEANBAR, MINEGYSPEC, ATIME = 3.7e-9, 12.5, 0.25


@functools.lru_cache(maxsize=None)
def entropy_case(n):
    """gas slots for check_density_entropy: Density <= 0, NaN, infinite or fine; EgyWtDensity likewise; Entropy a factor 2 below or above
    its floor (so no rounding of the floor decides the branch)"""
    rng = np.random.default_rng([SEED, n, 7])
    S = np.zeros(n, dtype=capi.SPH_DTYPE)
    _fill(rng, S)
    S["Density"] = np.exp(rng.normal(-18, 3, n))
    k = np.arange(n)
    S["Density"][k % 13 == 2] = 0
    S["Density"][k % 13 == 5] = -1.5
    S["Density"][k % 13 == 7] = np.nan
    S["Density"][k % 13 == 11] = np.inf
    S["EgyWtDensity"] = S["Density"] * rng.uniform(0.9, 1.1, n)
    S["EgyWtDensity"][k % 5 == 1] = 0
    S["EgyWtDensity"][k % 17 == 3] = np.nan
    fixed = S.copy()
    badrho = ~(fixed["Density"] > 0) | ~np.isfinite(fixed["Density"])
    fixed["Density"][badrho] = MEANBAR
    S["Entropy"] = minent(fixed, MINEGYSPEC, ATIME) * np.where(k % 2 == 0, 0.5, 2.0)
    S.setflags(write=False)
    return S


# ---- the particle sets of the smoothing-length tests ----------------------------------------------------------------------------------

def hsml_set(ngas, box=8.0):
    """ngas gas particles at cm.random_positions with two masses a factor 8 apart (so the climbs end on different levels), one of them
    garbage, and behind them a live and a swallowed black hole: (PartManager, SphP, BhP)"""
    import common as cm
    import orc
    import shenqi_amd as sq
    pos = cm.random_positions(orc.boost_mt19937_uniform(11, 3 * (ngas + 2)), ngas + 2, box)
    pman = sq.PartManager(ngas + 2, box)
    P = pman.Base
    P["Pos"] = pos
    P["Mass"] = np.where(np.arange(ngas + 2) % 3 == 0, 8.0, 1.0)
    P["ID"] = np.arange(1, ngas + 3)
    P["Hsml"] = 0.37           # what an untouched particle must keep
    P["Type"][:ngas] = 0
    P["PI"][:ngas] = np.arange(ngas)
    P["Type"][ngas:] = 5
    P["PI"][ngas:] = [0, 1]
    P["Flags"][ngas // 2] = 1   # a garbage gas particle
    P["Flags"][ngas + 1] = 2    # a swallowed black hole: the tree skips it
    SphP = np.zeros(ngas, dtype=capi.SPH_DTYPE)
    SphP["Entropy"] = -1
    SphP["Density"] = -1
    SphP["EgyWtDensity"] = -1
    BhP = np.zeros(2, dtype=sq.BH_SLOT_DTYPE)
    return pman, SphP, BhP


def tree_father(tree, n):
    """ForceTree.Father of a host tree as a numpy array"""
    import ctypes as C
    v = tree.view()
    return np.ctypeslib.as_array(C.cast(v.father, C.POINTER(C.c_int32)), shape=(n,)).copy()
