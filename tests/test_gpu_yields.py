"""Stellar yields on the device (shq_yields_init, shq_metal_yields, shq_metal_return_postprocess; csrc/yields.hip) against the plain-Python
restatement of metal_return.cpp:157-462, 539-569 in tests/yields_restated.py (brentq roots, quad integrals with break points at the
table nodes, ages by quad of 1 / (a H)).

Bounds, fixed before any run: discrete results (queue, clamp branch, rewritten LastEnrichmentMyr) equal; ages and mass limits 1e-12
relative; every yield quantity within 1e-12 x (the same table integral over the table's full mass range) x initialmass.

Measured on an MI355X (seed 2, 3000 stars; the figures are printed by the test): see DESIGN §3.7i."""
import ctypes as C

import numpy as np
import pytest

import shenqi_amd as sq
from shenqi_amd import capi
import yields_restated as yr
import yields_fixtures as yf

pytestmark = pytest.mark.gpu
SEED = 2


@pytest.fixture(scope="module")
def world(ctx):
    """tables uploaded, the population, and the oracle's results for the active list: computed once, never changed"""
    T = yr.Tables()
    imf_norm = yr.compute_imf_norm(T)
    tt = yf.time_table()
    mmf_dev = sq.yields_init(ctx, T.raw, tt, yf.SN1AN0, yf.HUBBLEPARAM, imf_norm)
    mmf = yr.maxmassfrac(T, yf.HUBBLEPARAM, yf.SN1AN0, imf_norm)
    P, S, active, kinds, ages = yf.population(T, tt, mmf, SEED)
    So = S.copy()
    ref = yr.metal_return_init(T, P, So, active, yf.COSMO, yf.ATIME, yf.HUBBLEPARAM, yf.SN1AN0, imf_norm, ages=ages)
    return dict(T=T, imf_norm=imf_norm, tt=tt, mmf=mmf, mmf_dev=mmf_dev, P=P, S=S, So=So, active=active, kinds=kinds, ages=ages, ref=ref,
                scales=yr.FullRangeScales(T, imf_norm))


def run_device(ctx, w, active):
    pman = sq.PartManager(len(w["P"]), 1.0)
    pman.Base[:] = w["P"]
    S = w["S"].copy()
    sentinel = {k: np.full(len(S), -7.0) for k in ("StellarAges", "LowDyingMass", "HighDyingMass", "MassReturn")}
    out = sq.metal_yields(ctx, pman, S, yf.ATIME, active=active, out=sentinel)
    assert np.array_equal(pman.Base, w["P"])              # the particle records are only read
    return out, S


def test_maxmassfrac_of_the_host_compiled_routine(world):
    """shq_yields_init evaluates :425 on the host with the kernel's routine (csrc/yields_math.hpp)"""
    print("maxmassfrac: device-side routine", world["mmf_dev"], "restatement", world["mmf"])
    assert abs(world["mmf_dev"] / world["mmf"] - 1) < 1e-12


def test_population_holds_every_case(world):
    """what the population contains by construction, asserted on the oracle's values; and the fairness condition of the equalities below"""
    w, T, ref, S, kinds = world, world["T"], world["ref"], world["S"], world["kinds"]
    P = w["P"]
    inlist = np.zeros(len(S), bool)
    act = w["active"]
    inlist[P["PI"][act[P["Type"][act] == 4]]] = True
    assert inlist.sum() > 2500 and (~inlist).sum() > 100 and (P["Type"][act] != 4).sum() > 500
    lo, hi, age = ref["LowDyingMass"], ref["HighDyingMass"], ref["StellarAges"]
    sel = lambda k: inlist & (kinds == k)      # noqa: E731
    assert ((lo == T.MAXMASS) & (hi == T.MAXMASS))[sel("young")].all() and sel("young").sum() > 300
    assert (lo[sel("old")] == T.lifetime_masses[0]).all() and sel("old").sum() > 200
    last = S["LastEnrichmentMyr"].astype(np.float64)
    life40 = np.array([T.lifetime_interp.eval(min(max(z, 0.0004), 0.05), 40.0) / 1e6 for z in S["Metallicity"]])
    g = sel("generic")
    assert (last[g] < life40[g]).sum() > 20 and (last[g] > life40[g]).sum() > 500
    same = sel("same")
    assert (S["LastEnrichmentMyr"][same] == age[same].astype(np.float32)).all() and (hi[same] == lo[same]).sum() >= 3
    st = sel("straddle")
    for edge in (7.5, 8.0, 13.0):
        assert ((lo < edge) & (hi > edge))[st].sum() > 30
    nar = sel("narrow")
    assert ((age - last)[nar] < 2e-3).all() and ((hi > lo)[nar]).sum() > 150
    ia = sel("sn1a")
    assert (age[ia] < 40).sum() > 30 and (age[ia] > 40).sum() > 30 and ((last < 40) & (age > 40))[ia].sum() > 10
    Z = S["Metallicity"][inlist]
    for ax in (T.lifetime_metallicity, T.agb_metallicities, T.snii_metallicities):
        assert (Z < ax[0]).any() or ax[0] == 0
        assert (Z > ax[-1]).any() and all((Z == z).any() for z in ax) and all(((Z > a) & (Z < b)).any() for a, b in zip(ax[:-1], ax[1:]))
    assert (Z == 0).sum() > 10
    cl = sel("clamp")
    inq = np.zeros(len(S), bool)
    inq[P["PI"][ref["queue"]]] = True
    assert (ref["clamped"] & inq)[cl].sum() > 30 and (ref["clamped"] & ref["rewritten"])[cl].sum() > 60
    assert (ref["MassReturn"][ref["rewritten"]] < 1e-3).all() and (ref["MassReturn"][cl] == 0).sum() > 30
    # fairness: nobody within 1e-9 relative of the haswork threshold, the clamp condition or a branch condition of find_mass_bin_limits
    assert min(ref["margins"]) > 1e-9 and min(ref["haswork_margin"]) > 1e-9 and min(ref["clamp_margin"]) > 1e-9


def compare(w, out, S_dev, ref, So):
    T, P, S0 = w["T"], w["P"], w["S"]
    q = ref["queue"]
    assert out["queue"].tolist() == q.tolist()
    rewritten = S_dev["LastEnrichmentMyr"] != S0["LastEnrichmentMyr"]
    assert np.array_equal(rewritten, ref["rewritten"] & (So["LastEnrichmentMyr"] != S0["LastEnrichmentMyr"]))
    assert np.array_equal(S_dev["LastEnrichmentMyr"], So["LastEnrichmentMyr"])
    for name in ("FormationTime", "TotalMassReturned", "Metallicity", "Metals"):
        assert np.array_equal(S_dev[name], S0[name])
    done = ref["StellarAges"] != 0                                           # the slots of the list's stars
    for k in ("StellarAges", "LowDyingMass", "HighDyingMass", "MassReturn"):
        assert (out[k][~done] == -7.0).all()                                # slots of stars outside the list are left alone
    err = {k: np.abs(out[k][done] / ref[k][done] - 1).max() for k in ("StellarAges", "LowDyingMass", "HighDyingMass")}
    # the clamp branch: the device's MassReturn is initialmass * maxmassfrac - TotalMassReturned exactly where the oracle took it
    star = np.flatnonzero(P["Type"] == 4)
    init = np.zeros(len(S0))
    init[P["PI"][star]] = P["Mass"][star].astype(np.float64) + S0["TotalMassReturned"][P["PI"][star]]
    clamp_val = np.maximum(init * w["mmf_dev"] - S0["TotalMassReturned"], 0.0)
    # (to rounding: the compiler may contract the product and the difference; an unclamped star stays clamp_margin > 1e-9 below it)
    assert np.array_equal((np.abs(out["MassReturn"] - clamp_val) <= 1e-14 * init)[done], ref["clamped"][done])
    scale = {s: w["scales"](S0["Metallicity"][s]) for s in np.flatnonzero(done)}
    smass = np.array([scale[s][0] for s in np.flatnonzero(done)]) * init[done]
    err["MassReturn"] = (np.abs(out["MassReturn"] - ref["MassReturn"])[done] / smass).max()
    pi = P["PI"][q]
    assert np.array_equal(out["MassGenerated"], out["MassReturn"][pi])
    err["MetalGenerated"] = (np.abs(out["MetalGenerated"] - ref["MetalGenerated"]) / (np.array([scale[s][1] for s in pi]) * init[pi])).max()
    sp = np.array([scale[s][2] for s in pi]) * init[pi, None]
    err["MetalSpeciesGenerated"] = (np.abs(out["MetalSpeciesGenerated"] - ref["MetalSpeciesGenerated"]) / sp).max()
    assert (out["MetalGenerated"] >= 0).all() and (out["MetalSpeciesGenerated"] >= 0).all()
    print("max errors (bound 1e-12):", {k: float(v) for k, v in err.items()})
    assert all(v <= 1e-12 for v in err.values()), err


def test_yields_match_restatement(ctx, world):
    out, S_dev = run_device(ctx, world, world["active"])
    compare(world, out, S_dev, world["ref"], world["So"])


def test_yields_all_particles(ctx, world):
    """active = NULL: every particle; the same per-star values, the queue in particle order"""
    w = world
    out, S_dev = run_device(ctx, w, None)
    ref, P = w["ref"], w["P"]
    inlist = ref["StellarAges"] != 0
    for k in ("StellarAges", "LowDyingMass", "HighDyingMass", "MassReturn"):
        assert (np.abs(out[k][inlist] - ref[k][inlist]) <= 1e-12 * np.abs(ref[k][inlist]) + 1e-12 * (k == "MassReturn")).all() and (out[k] != -7.0).all()
    q = out["queue"]
    assert (np.diff(q) > 0).all() and (P["Type"][q] == 4).all()
    thr = 1e-3 * (P["Mass"][q].astype(np.float64) + w["S"]["TotalMassReturned"][P["PI"][q]])
    assert (out["MassReturn"][P["PI"][q]] >= thr).all()
    listed = set(ref["queue"].tolist())
    mine = [i for i in q.tolist() if inlist[P["PI"][i]]]
    assert set(mine) == listed and sorted(listed) == mine
    pos = {i: k for k, i in enumerate(ref["queue"].tolist())}
    sel = np.array([pos[i] for i in mine])
    at = np.array([k for k, i in enumerate(q.tolist()) if inlist[P["PI"][i]]])
    assert np.abs(out["MetalSpeciesGenerated"][at] - ref["MetalSpeciesGenerated"][sel]).max() <= 1e-12 * ref["MetalSpeciesGenerated"].max()


def test_formation_outside_the_time_table(ctx, world):
    """a star formed before the table's first node: SHQ_ERR_INVALID with the count, outputs untouched, context usable afterwards"""
    w = world
    pman = sq.PartManager(len(w["P"]), 1.0)
    pman.Base[:] = w["P"]
    S = w["S"].copy()
    stars = np.flatnonzero(w["P"]["Type"] == 4)
    S["FormationTime"][w["P"]["PI"][stars[:3]]] = [0.05, 0.0999, 1.5]
    S0 = S.copy()
    sentinel = {k: np.full(len(S), -7.0) for k in ("StellarAges", "LowDyingMass", "HighDyingMass", "MassReturn")}
    with pytest.raises(sq.ShqError) as e:
        sq.metal_yields(ctx, pman, S, yf.ATIME, active=None, out=sentinel)
    assert e.value.status == 1 and e.value.nbad == 3                       # SHQ_ERR_INVALID
    assert all((v == -7.0).all() for v in sentinel.values()) and np.array_equal(S, S0)
    with pytest.raises(sq.ShqError) as e:                                   # atime beyond the table: every star of the list
        sq.metal_yields(ctx, pman, w["S"].copy(), 1.01, active=stars[:10].astype(np.int32), out=sentinel)
    assert e.value.nbad == 10
    out, _ = run_device(ctx, w, w["active"][:200])
    assert (out["StellarAges"] != -7.0).sum() == (w["P"]["Type"][w["active"][:200]] == 4).sum()


def test_chain_yields_density_return_postprocess(ctx, world):
    """shq_metal_yields -> shq_stellar_density -> shq_metal_return -> shq_metal_return_postprocess on the 14^3 gas set-up of
    tests/test_gpu_metal_return.py, against restated yields, the same stellar density and oracle/metal_return.py; that file's tolerances"""
    import common as cm
    from test_gpu_metal_return import setup, omr
    w = world
    pman, G, _, _, _, _, _ = setup(11, nstar=300)
    P = pman.Base
    rng = np.random.default_rng(4)
    nstar = 300
    S = np.zeros(nstar, dtype=capi.STAR_DTYPE)
    S["FormationTime"] = rng.uniform(0.2, 0.995, nstar).astype(np.float32)
    S["Metallicity"] = rng.uniform(0, 0.03, nstar)
    ages = np.array([yr.atime_to_myr(yf.COSMO, float(f), yf.ATIME) for f in S["FormationTime"]])
    S["LastEnrichmentMyr"] = (ages * rng.choice([0.0, 0.5, 0.999], nstar)).astype(np.float32)
    active = np.flatnonzero(rng.random(len(P)) < 0.8).astype(np.int32)
    oP, oG, oS = P.copy(), G.copy(), S.copy()
    ref = yr.metal_return_init(w["T"], oP, oS, active, yf.COSMO, yf.ATIME, yf.HUBBLEPARAM, yf.SN1AN0, w["imf_norm"], ages=ages)
    P0, S0 = P.copy(), S.copy()
    y = sq.metal_yields(ctx, pman, S, yf.ATIME, active=active)
    q = y["queue"]
    assert q.tolist() == ref["queue"].tolist() and 40 < len(q) < 250
    tree = sq.force_tree_rebuild_mask(pman, sq.GASMASK)
    f = capi.SPH_DTYPE.fields
    pv, tv, sv = pman.view(), tree.view(), capi.sph_view(G)
    stp = capi.StellarParams(cm.BOX, 4.0 / 3 * np.pi * 2.0**3, 2.0, 1, 1)
    vol = np.zeros(nstar)
    capi.check(capi.hip.shq_stellar_density(ctx.h, C.byref(tv), C.byref(pv), C.byref(sv), capi.ptr(q), len(q), C.byref(stp), capi.ptr(vol), None))
    oP["Hsml"] = P["Hsml"]                                                  # the same stellar density on both sides
    starvol = np.ascontiguousarray(vol[P["PI"][q]])
    gv = capi.GasMetalView(G.ctypes.data, G.dtype.itemsize, len(G), f["Density"][1], f["Metallicity"][1], f["Metals"][1], 9, 0)
    mret = np.zeros(len(q))
    capi.check(capi.hip.shq_metal_return(ctx.h, C.byref(tv), C.byref(pv), C.byref(gv), capi.ptr(q), len(q), capi.ptr(starvol), capi.ptr(y["MassGenerated"]),
                                         capi.ptr(y["MetalGenerated"]), capi.ptr(y["MetalSpeciesGenerated"]), 4.0, 1, 1, capi.ptr(mret), None))
    sq.metal_return_postprocess(ctx, pman, S, q, mret, y["StellarAges"])
    omass = omr.metal_return(oP, oG, ref["queue"], starvol, ref["MassGenerated"], ref["MetalGenerated"], ref["MetalSpeciesGenerated"], 4.0, 1, 1, cm.BOX)
    pi = P["PI"][q]
    oP["Mass"][q] = (oP["Mass"][q].astype(np.float64) - omass).astype(np.float32)          # metal_return_postprocess (:581-589)
    oS["TotalMassReturned"][pi] += omass
    oS["LastEnrichmentMyr"][pi] = ref["StellarAges"][pi].astype(np.float32)
    same = lambda a, b, tol: np.abs(a.astype(np.float64) - b.astype(np.float64)).max() <= tol * np.abs(b).max()      # noqa: E731
    assert same(P["Mass"], oP["Mass"], 1.2e-7) and same(G["Density"], oG["Density"], 1e-15)
    assert same(G["Metallicity"], oG["Metallicity"], 1e-15) and same(G["Metals"], oG["Metals"], 1.2e-7)
    assert np.abs(mret - omass).max() <= 1e-14 * omass.max()
    assert same(S["TotalMassReturned"], oS["TotalMassReturned"], 1e-14) and np.array_equal(S["LastEnrichmentMyr"], oS["LastEnrichmentMyr"])
    # only the queue's stars changed; their new LastEnrichmentMyr is the age
    notq = np.ones(len(P), bool)
    notq[q] = False
    stars = P["Type"] == 4
    assert np.array_equal(P["Mass"][stars & notq], P0["Mass"][stars & notq])
    assert np.array_equal(S["LastEnrichmentMyr"][pi], y["StellarAges"][pi].astype(np.float32))
    # conservation: gas mass gained = sum of MassReturn = star mass lost, to float rounding of the masses
    gas = (P["Type"] == 0) & ((P["Flags"] & 1) == 0)
    gained = (P["Mass"][gas].astype(np.float64) - P0["Mass"][gas].astype(np.float64)).sum()
    lost = (P0["Mass"][q].astype(np.float64) - P["Mass"][q].astype(np.float64)).sum()
    assert mret.sum() > 0.5
    assert abs(gained - mret.sum()) < 2e-6 * P0["Mass"][gas].sum() and abs(lost - mret.sum()) < 6e-8 * P0["Mass"][q].astype(np.float64).sum()
    assert same(S["TotalMassReturned"][pi] - S0["TotalMassReturned"][pi], mret, 1e-15)
