"""Inputs that take hydro_force() through every branch of its pair term (HydroLocalTreeWalk::ngbiter, hydratree2.hpp:253-378) and
through the symmetric search, where a target depends on neighbours whose radius reaches it from outside its own and the walk knows
of them only by the node hmax.  Shared by test_hydro_brute_cpu.py (oracle against the all-pairs sum of hydro_brute.py) and
test_gpu_hydro_brute.py (device against both).

Every case: BOX 8, unequal masses a float holds exactly, atime 0.1, ArtBulkViscConst 0.75.  The outputs of density() are INPUTS of
the hydro force, so the synthetic cases write them straight into the slots: Density log-normal, EgyWtDensity = Density * ratio with
ratio log-uniform in [0.2, 5], DhsmlEgyDensityFactor in [0.5, 1.5], DivVel normal, CurlVel |normal|, Entropy in [0.5, 2).  The
converged cases (CONVERGED) take them from the device's own density() in test_gpu_hydro_brute.py.

The counters of hydro_brute.hydro, per target (CLAIMS names those a case is there to reach; test_hydro_brute_cpu.py asserts them):
  by_hi_only, by_hj_only, by_both   accepted pairs within the target's radius only / the neighbour's only / both
  wrapped                           accepted pairs across a periodic face
  approaching                       vdotr2 < 0: the viscosity is evaluated
  limiter_bites, limiter_off        the fmin of the viscosity limiter takes its second argument / dloga == 0 switches it off
  contrast_i, contrast_j            the DensityContrastLimit clamp lowers rr1 / rr2
  density_guard                     SPH_DensityPred of the neighbour returns 1e-6 Density
  wind_skipped                      neighbours in reach left out for DelayTime > 0
  coincident                        other gas particles at r2 == 0 (left out, as the reference returns on r2 <= 0)
  f_zero                            DivVel == CurlVel == 0 on either side (the F1 / f2 quotients are 0 / x)

A target must be in a time bin whose drift factor is zero (the reference leaves drifts[] zero for active bins; shq_hydro_force
refuses anything else), so `ragged`, whose lists are drawn from all particles of `drift`, moves the listed particles of drifted
bins to bins 1 and 2."""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np

import shenqi_amd as sq
from shenqi_amd import capi
import orc
import common as cm
import hydro_brute as hb

BOX = cm.BOX
NBINS = capi.TIMEBINS + 1


def kick_tables(scale=0.3, dloga_bins=True):
    """every table non-zero and different per bin: the tables of test_gpu_sph_edges.kick_tables.  dloga_bins False: dloga_for_bin = 0"""
    kf = sq.KickFactors()
    kf.FgravkickB = 0.013 * scale
    for b in range(NBINS):
        kf.gravkicks[b] = scale * 0.02 * (1 + 0.1 * b) * (1 if b % 2 else -1)
        kf.hydrokicks[b] = scale * 0.015 * (1 + 0.07 * b)
        kf.dloga_kick[b] = scale * 0.004 * (b % 5 - 1.5)
        kf.dloga_for_bin[b] = 0.002 * (b + 1) if dloga_bins else 0.0
    return kf


def _uniform(seed, n):
    return np.random.default_rng(seed).uniform(0, BOX, size=(n, 3))


def synthetic(name, pos, hsml, seed, kernel=1, DISPH=1, contrast=100.0, ptype=None, kicked=False):
    """a case with synthetic slot fields.  `kicked`: fields the predictors read (accelerations, DtEntropy, HydroAccel) sized so that
    non-zero kick tables matter, as in test_gpu_sph_edges.gas_setup"""
    n = len(pos)
    rng = np.random.default_rng(2000 + seed)
    c = SimpleNamespace(name=name, n=n, pos=np.ascontiguousarray(pos, dtype=np.float64), kernel=kernel, DISPH=DISPH, contrast=contrast,
                        visc=0.75, atime=0.1, hubble=cm.HUBBLE, box=BOX, kf=None, drifts=None, WindSpeed=0.0,
                        WindFreeTravelDensThresh=0.0, active=None, use_evp=True, subset=None)
    c.type = np.zeros(n, dtype=np.uint8) if ptype is None else np.asarray(ptype, dtype=np.uint8)
    gas = np.flatnonzero(c.type == 0)
    ng = len(gas)
    c.pi = np.zeros(n, dtype=np.int32)
    c.pi[gas] = np.arange(ng)
    c.mass = rng.uniform(0.5, 1.5, size=n).astype(np.float32)
    c.hsml = np.broadcast_to(np.asarray(hsml, dtype=np.float64), (n,)).copy()
    c.vel = rng.normal(size=(n, 3)) * 2.0
    c.treeacc = rng.normal(size=(n, 3)) * 30.0
    c.gravpm = rng.normal(size=(n, 3)) * 10.0
    c.bin_hydro = np.zeros(n, dtype=np.uint8)
    c.bin_grav = np.zeros(n, dtype=np.uint8)
    dens = np.exp(rng.normal(scale=0.5, size=ng))
    c.sph = {"Density": dens, "EgyWtDensity": dens * np.exp(rng.uniform(np.log(0.2), np.log(5.0), size=ng)),
             "DhsmlEgyDensityFactor": rng.uniform(0.5, 1.5, size=ng), "DivVel": rng.normal(size=ng), "CurlVel": np.abs(rng.normal(size=ng)),
             "Entropy": rng.uniform(0.5, 2.0, size=ng), "DtEntropy": rng.normal(size=ng) * (150.0 if kicked else 1.0),
             "HydroAccel": rng.normal(size=(ng, 3)) * 40.0, "DelayTime": np.zeros(ng)}
    c.nslots = ng
    assert np.all((c.pos >= 0) & (c.pos < BOX))
    return c


def variant(c, name, **kw):
    """a copy of a case with some attributes replaced (the arrays are shared: read-only)"""
    v = SimpleNamespace(**vars(c))
    v.name = name
    for k, x in kw.items():
        setattr(v, k, x)
    return v


def evp_of(c):
    """the EntVarPred cache density() would have left: SPH_EntVarPred of every gas slot with the case's kick tables"""
    gas = np.flatnonzero(c.type == 0)
    dk = hb.kick_arrays(c.kf)[3]
    evp = np.zeros(max(c.nslots, 1))
    slot = c.pi[gas]
    evp[slot] = hb.entvar_pred(c.sph["Entropy"][slot], c.sph["DtEntropy"][slot], dk[c.bin_hydro[gas].astype(np.int64)])
    return evp


def state(c):
    """(pman, SphP) of a case"""
    pman = sq.PartManager(c.n, BOX)
    P = pman.Base
    P["Pos"], P["Mass"], P["Vel"], P["Hsml"] = c.pos, c.mass, c.vel, c.hsml
    P["FullTreeGravAccel"], P["GravPM"] = c.treeacc, c.gravpm
    P["TimeBinHydro"], P["TimeBinGravity"] = c.bin_hydro, c.bin_grav
    P["ID"] = np.arange(1, c.n + 1)
    P["Type"], P["PI"] = c.type, c.pi
    SphP = np.zeros(max(c.nslots, 1), dtype=sq.SPH_DTYPE)[:c.nslots]
    for k in hb.SPH_FIELDS:
        SphP[k][:len(c.sph[k])] = c.sph[k]
    return pman, SphP


def hydro_params(c, **over):
    """the hand-filled HydroParams of the C ABI"""
    hp = cm.hydro_params(atime=c.atime, hubble=c.hubble, kernel=c.kernel, DensityIndependentSphOn=c.DISPH,
                         DensityContrastLimit=over.get("contrast", c.contrast), ArtBulkViscConst=c.visc)
    hp.WindSpeed, hp.WindFreeTravelDensThresh = c.WindSpeed, c.WindFreeTravelDensThresh
    drifts = over.get("drifts", c.drifts)
    if drifts is not None:
        for b in range(NBINS):
            hp.drifts[b] = drifts[b]
    if c.kf is not None:
        C.memmove(C.addressof(hp.kf), C.addressof(c.kf), C.sizeof(sq.KickFactors))
    return hp


def host_tree(pman):
    """the project's host tree of the gas with the node hmax force_tree_update_hmax leaves"""
    tree = sq.force_tree_rebuild_mask(pman, sq.GASMASK)
    sq.force_tree_update_hmax(tree, pman)
    return tree


def active_of(c):
    return c.active if c.active is None or len(c.active) else np.zeros(1, dtype=np.int32)[:0]


def gas_targets(c):
    """particle indices of the gas targets of a case, in list order"""
    q = np.arange(c.n) if c.active is None else c.active.astype(np.int64)
    return q[c.type[q] == 0]


def oracle_run(c, tree=None, zero_hmax=False, clear_delay=False, **over):
    """orc.hydro on a case, on the host tree.  `over`: contrast / drifts given to the oracle instead of the case's; zero_hmax:
    Nodes_base["hmax"] zeroed; clear_delay: DelayTime cleared.  Returns (SphState with the results, candidate count)."""
    pman, SphP = state(c)
    if clear_delay:
        SphP["DelayTime"] = 0
    if tree is None:
        tree = host_tree(pman)
    nodes = tree.Nodes_base.copy()
    if zero_hmax:
        nodes["hmax"] = 0
    st = orc.SphState(pman.Base, SphP)
    nint = orc.hydro(nodes, tree.firstnode, st, hydro_params(c, **over), evp_of(c) if c.use_evp else None, active=active_of(c))
    return st, nint


def brute_targets(c):
    return gas_targets(c) if c.subset is None else np.asarray(c.subset, dtype=np.int64)


def brute_run(c):
    """the all-pairs reference of a case for brute_targets(c)"""
    return hb.hydro(c.pos, c.type, c.mass, c.hsml, c.vel, c.treeacc, c.gravpm, c.bin_hydro, c.bin_grav, c.sph, evp_of(c) if c.use_evp else None,
                    c, brute_targets(c), pi=c.pi)


# ---- the synthetic cases -------------------------------------------------------------------------------------------------------

def reach():
    """1024 particles with radii near the mean spacing and 4 giants of 0.3 Box, two of them within 0.01 Box of a corner"""
    n = 1024
    pos = np.concatenate([_uniform(101, n), [[0.03, 7.96, 0.05], [7.95, 7.97, 7.94], [3.1, 4.7, 2.2], [5.9, 1.3, 6.4]]])
    rng = np.random.default_rng(101)
    hsml = np.concatenate([BOX / np.cbrt(n) * rng.uniform(1.0, 1.5, size=n), np.full(4, 0.3 * BOX)])
    c = synthetic("reach", pos, hsml, seed=1)
    c.giants = np.arange(n, n + 4)
    return c


def contrast(limit=100.0, DISPH=1):
    c = synthetic("contrast_%g_%d" % (limit, DISPH), _uniform(102, 512), BOX / 8 * np.random.default_rng(102).uniform(1.0, 1.8, size=512),
                  seed=2, DISPH=DISPH, contrast=limit)
    return c


DRIFTS = np.zeros(NBINS)
DRIFTS[3:8] = (0.03, -0.05, 0.08, -0.02, 0.04)


def drift(use_evp=True, dloga_bins=True):
    """TimeBinHydro 1..5, bins <= 2 active; drift factors of both signs above; 40 inactive particles with DivVel * drift = 2.5 (the
    1e-6 Density guard), |DivVel * drift| <= 0.4 for the rest; kick tables non-zero and different per bin, mixed TimeBinGravity"""
    n = 1024
    rng = np.random.default_rng(103)
    c = synthetic("drift" + ("" if use_evp else "_noevp") + ("" if dloga_bins else "_dloga0"), _uniform(103, n),
                  BOX / 10 * rng.uniform(1.0, 2.2, size=n), seed=3, kicked=True)
    c.bin_hydro = rng.integers(1, 6, size=n).astype(np.uint8)
    c.bin_grav = (c.bin_hydro + rng.integers(0, 3, size=n)).astype(np.uint8)
    c.drifts = DRIFTS.copy()
    c.kf = kick_tables(dloga_bins=dloga_bins)
    c.sph["DivVel"] = np.clip(c.sph["DivVel"] * 2.0, -5.0, 5.0)
    inactive = np.flatnonzero(c.bin_hydro > 2)
    c.guarded = rng.choice(inactive, size=40, replace=False)
    c.sph["DivVel"][c.guarded] = 2.5 / c.drifts[c.bin_hydro[c.guarded]]
    c.active = np.flatnonzero(c.bin_hydro <= 2).astype(np.int32)
    c.use_evp = use_evp
    return c


def kernels(ktype, DISPH):
    rng = np.random.default_rng(110 + ktype)
    return synthetic("kernels_%d_%d" % (ktype, DISPH), _uniform(110 + ktype, 512), BOX / 8 * rng.uniform(1.0, 2.5, size=512), seed=10 + ktype,
                     kernel=ktype, DISPH=DISPH)


def coincident():
    """8 pairs and one triple of bit-equal positions; 16 particles with DivVel = CurlVel = 0"""
    n = 512
    pos = _uniform(104, n)
    rng = np.random.default_rng(104)
    pick = rng.permutation(n)
    for k in range(8):
        pos[pick[2 * k + 1]] = pos[pick[2 * k]]
    pos[pick[17]] = pos[pick[16]]
    pos[pick[18]] = pos[pick[16]]
    c = synthetic("coincident", pos, BOX / 8 * rng.uniform(1.0, 1.8, size=n), seed=4)
    c.twins = pick[:19]
    c.fzero = np.concatenate([pick[:4], pick[100:112]])                # four of them among the coincident ones
    c.sph["DivVel"][c.fzero] = 0
    c.sph["CurlVel"][c.fzero] = 0
    return c


def winds():
    n = 512
    rng = np.random.default_rng(105)
    c = synthetic("winds", _uniform(105, n), BOX / 8 * rng.uniform(1.0, 1.8, size=n), seed=5)
    c.wind = rng.random(n) < 0.1
    c.sph["DelayTime"][c.wind] = rng.uniform(0.1, 1.0, size=c.wind.sum())
    c.WindSpeed, c.WindFreeTravelDensThresh = 3.5, 0.2
    return c


def mixed_types():
    """1000 gas, 19 type-1 and 5 type-5 particles in shuffled order; the non-gas particles carry PI values that are valid gas slots
    (a result written for one of them would land on a gas particle's row); 8 spare slots no particle owns; the list names everybody"""
    n = 1024
    rng = np.random.default_rng(106)
    ptype = np.zeros(n, dtype=np.uint8)
    other = rng.permutation(n)[:24]
    ptype[other[:19]] = 1
    ptype[other[19:]] = 5
    c = synthetic("mixed_types", _uniform(106, n), BOX / 10 * rng.uniform(1.0, 2.0, size=n), seed=6, ptype=ptype)
    c.pi[other] = rng.integers(0, 1000, size=24)
    c.nslots = 1008
    c.active = rng.permutation(n).astype(np.int32)
    return c


def ragged(nactive):
    """the drift inputs with a list of `nactive` entries drawn from all particles, unsorted"""
    c = drift()
    rng = np.random.default_rng(120 + nactive)
    act = rng.permutation(c.n)[:nactive]
    c.name = "ragged%d" % nactive
    move = act[c.bin_hydro[act] > 2]
    c.bin_hydro[move] -= 3                                              # 3, 4, 5 -> 0, 1, 2: zero drift, as a target needs
    c.bin_hydro[move] = np.maximum(c.bin_hydro[move], 1)
    c.sph["DivVel"][c.pi[move]] = np.clip(c.sph["DivVel"][c.pi[move]], -5.0, 5.0)
    c.active = np.ascontiguousarray(act, dtype=np.int32)
    return c


def tiers():
    """the shape of test_heavy_targets_get_a_wave_or_a_workgroup: 32^3 particles, 300 radii x 4 (the wave tier), 3 of them 0.49 Box
    (the workgroup tier).  All are targets; the all-pairs sum is taken for 512: the 3 giants, 61 of the wave tier, 448 others."""
    n1 = 32
    n = n1**3
    rng = np.random.default_rng(1)
    hsml = BOX / n1 * rng.uniform(1.0, 2.0, size=n)
    wave = rng.choice(n, size=300, replace=False)
    hsml[wave] *= 4.0
    giants = wave[:3]
    hsml[giants] = 0.49 * BOX
    c = synthetic("tiers", cm.random_positions(orc.boost_mt19937_uniform(31, 3 * n), n), hsml, seed=7)
    c.giants, c.wave = giants, wave[3:64]
    # random_positions puts a quarter of the particles in the whole box, half in a clump 0.28 wide and a quarter in one 0.07 wide; a
    # target inside a clump has all of it for neighbours (16384 or 8192 pairs), so 16 of each clump and 416 of the rest keep the sum short
    rest = np.setdiff1d(np.arange(n), wave)
    c.ordinary = np.concatenate([rng.choice(rest[rest < n // 4], size=416, replace=False),
                                 rng.choice(rest[(rest >= n // 4) & (rest < 3 * n // 4)], size=16, replace=False),
                                 rng.choice(rest[rest >= 3 * n // 4], size=16, replace=False)])
    c.subset = np.concatenate([c.giants, c.wave, c.ordinary])
    return c


SYNTHETIC = {"reach": reach,
             **{"contrast_%g_1" % lim: (lambda lim=lim: contrast(lim, 1)) for lim in (100.0, 1.0, 0.0, -1.0)},
             **{"contrast_%g_0" % lim: (lambda lim=lim: contrast(lim, 0)) for lim in (100.0, 1.0, -1.0)},
             "drift": drift, "drift_noevp": lambda: drift(use_evp=False), "drift_dloga0": lambda: drift(dloga_bins=False),
             **{"kernels_%d_%d" % (k, d): (lambda k=k, d=d: kernels(k, d)) for k in (1, 2, 4) for d in (0, 1)},
             "coincident": coincident, "winds": winds, "mixed_types": mixed_types,
             **{"ragged%d" % k: (lambda k=k: ragged(k)) for k in (0, 1, 63, 65, 1001)},
             "tiers": tiers}
HEAVY = ("reach", "tiers")                      # run twice on the device: equal bits
CONVERGED = ("tiny_start", "huge_start", "clump_floor", "kernel2", "kernel4", "dynrange", "dynrange_corner")      # of sph_loop_cases

CLAIMS = {"reach": ("by_hj_only", "wrapped", "by_hi_only", "by_both", "approaching"),
          "contrast_1_1": ("contrast_i", "contrast_j"),
          "drift": ("limiter_bites", "density_guard", "approaching"), "drift_noevp": ("limiter_bites", "density_guard"),
          "drift_dloga0": ("limiter_off", "density_guard"),
          "coincident": ("coincident", "f_zero"), "winds": ("wind_skipped",), "mixed_types": ("by_hj_only", "by_hi_only"),
          "ragged1001": ("density_guard", "limiter_bites"), "tiers": ("by_hj_only", "by_hi_only", "wrapped")}


@functools.lru_cache(maxsize=None)
def reference(name):
    """(case, brute result) computed once per process and shared; treat both as read-only"""
    c = SYNTHETIC[name]()
    return c, brute_run(c)
