"""The device's density() with its Hsml loop, on the inputs of sph_loop_cases.py, against the oracle (same decisions: iteration
count, Hsml, node hmax) and against the all-pairs sum of density_brute.py (the sums themselves, per particle).

Every branch of sph_density_post_kernel is taken by some case (test_density_brute_cpu.py counts them on the CPU and shows that no
NumNgb comes within 1e-9 of a decision threshold, so a device that adds in another order still has to take the same decisions);
the wave and workgroup tiers of the walk are entered and left inside the loop; dynrange and dynrange_corner put Hsml at 1e-5 Box
beside coordinates near Box, where the slack of the f32 pre-test of the candidate scan (pre32_bound) is 9 % of Hsml.

Bars.  Hsml: 1e-12 relative per particle.  Density, EgyWtDensity: 1e-11 relative per particle.  DivVel, CurlVel, |GradRho|, DtHsml:
1e-11 of the same quantity formed from the sums of the absolute values of its terms (rounding of <= 2000 terms is <= 2e-13 of that).
DhsmlEgyDensityFactor = 1 / (1 + x)-like: where |f| < 100, to 1e-11 (1 + |f|)^2.

Measured on an MI355X (device iterations, equal to both references'; largest relative deviation of Hsml and of Density per particle):

    case             iter  vs oracle: Hsml, Density   vs all-pairs: Hsml, Density
    alone1            22   0        0                 0        2.2e-16
    alone2            22   0        1.1e-16           0        2.2e-16
    sparse20          11   4.4e-16  8.9e-16           4.4e-16  7.8e-16
    sparse40           9   4.4e-16  6.7e-16           2.2e-16  6.7e-16
    clump_floor       10   5.6e-16  2.1e-15           4.4e-16  1.8e-15
    tiny_start        51   8.9e-16  3.1e-15           7.8e-16  2.0e-15
    huge_start        15   2.2e-15  1.1e-14           2.0e-15  5.1e-15
    kernel2           20   1.1e-15  3.1e-15           1.1e-15  2.6e-15
    kernel4           18   1.5e-15  3.8e-15           1.5e-15  4.0e-15
    bh                13   1.3e-15  3.8e-15           1.0e-15  2.0e-15
    lattice           12   6.7e-16  8.9e-16           6.7e-16  6.7e-16
    dynrange          41   1.1e-15  3.9e-15           8.9e-16  1.9e-15
    dynrange_corner   42   8.9e-16  5.1e-15           6.7e-16  2.2e-15
    kernel2_refloor    1   0        2.2e-15           0        1.7e-15
    tiers_active      11   5.6e-16  1.6e-15
    ragged0/1/63/65/1001   1/7/13/12/13 iterations; <= 1.1e-15, <= 3.2e-15

The signed sums stay below 2e-14 of their scales; the hydro force from the dynrange states below 1.2e-15 of each part's maximum."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import shenqi_amd as sq
from shenqi_amd import capi
import orc
import common as cm
import density_brute as db
import sph_loop_cases as sc

pytestmark = pytest.mark.gpu

BOX = sc.BOX


def run_device(ctx, c):
    """shq_density on a case through the C ABI with the host tree of the gas.  Returns a record of everything it wrote."""
    pman, SphP, BhP = sc.state(c)
    P = pman.Base
    tree = sq.force_tree_rebuild_mask(pman, sq.GASMASK)
    fp = capi.host.shqh_tree_father(tree._h)
    father = np.frombuffer((C.c_char * (4 * c.n)).from_address(fp), dtype=np.int32).copy()
    nodes0 = tree.Nodes_base.copy()
    before = (P.copy(), SphP.copy(), BhP.copy())
    pv, tv, sv, bv = pman.view(), tree.view(), capi.sph_view(SphP), capi.bh_view(BhP)
    evp, gmag = np.zeros(max(len(SphP), 1)), np.full(max(len(SphP), 1), np.nan)
    st = capi.SphStats()
    dp = sc.params(c)
    act = c.active if c.active is None or len(c.active) else np.zeros(1, dtype=np.int32)[:0]
    capi.check(capi.hip.shq_density(ctx.h, C.byref(tv), capi.ptr(tree.Nodes_base), C.byref(pv), C.byref(sv), C.byref(bv), capi.ptr(act),
                                    0 if act is None else len(act), C.byref(dp), capi.ptr(evp), capi.ptr(gmag), C.byref(st)))
    return SimpleNamespace(pman=pman, P=P, SphP=SphP, BhP=BhP, tree=tree, father=father, nodes0=nodes0, before=before, evp=evp,
                              gmag=gmag, stats=st, dp=dp)


def by_particle(c, gasfield, bhfield=None):
    """a gas-slot array as a by-particle array (black-hole rows from `bhfield` or NaN)"""
    ng = c.n - c.nbh
    out = np.full(c.n, np.nan)
    out[:ng] = gasfield[:ng]
    if bhfield is not None and c.nbh:
        out[ng:] = bhfield[:c.nbh]
    return out


def device_fields(c, d):
    return {"Hsml": d.P["Hsml"].copy(), "Density": by_particle(c, d.SphP["Density"], d.BhP["Density"]),
            "EgyWtDensity": by_particle(c, d.SphP["EgyWtDensity"]), "DhsmlEgyDensityFactor": by_particle(c, d.SphP["DhsmlEgyDensityFactor"]),
            "DivVel": by_particle(c, d.SphP["DivVel"], d.BhP["DivVel"]), "CurlVel": by_particle(c, d.SphP["CurlVel"]),
            "GradRho_mag": by_particle(c, d.gmag), "DtHsml": d.P["DtHsml"].copy()}


def oracle_fields(c, st, o):
    return {"Hsml": st.hsml, "Density": by_particle(c, st.density, st.bh_density), "EgyWtDensity": by_particle(c, st.egywtdensity),
            "DhsmlEgyDensityFactor": by_particle(c, st.dhsmlegydensityfactor), "DivVel": by_particle(c, st.divvel, st.bh_divvel),
            "CurlVel": by_particle(c, st.curlvel), "GradRho_mag": by_particle(c, np.linalg.norm(o.gradrho, axis=1)), "DtHsml": st.dthsml}


def targets_of(c):
    q = np.arange(c.n) if c.active is None else c.active.astype(np.int64)
    return q[(c.type[q] == 0) | (c.type[q] == 5)]


def check_against_oracle(c, d):
    """the decisions: iteration count, Hsml, extremes, node hmax, inactive rows, stats.  Returns (oracle state, extras, worst Hsml dev)."""
    st, o = sc.oracle_run(c, tree=(d.nodes0, d.tree.firstnode, d.father))
    q = targets_of(c)
    h = d.P["Hsml"]
    dev = np.abs(h[q] / st.hsml[q] - 1).max() if len(q) else 0.0
    print("%-16s device iterations %d (oracle %d); Hsml vs oracle %.2e" % (c.name, d.stats.niterations, o.niter, dev))
    assert d.stats.niterations == o.niter
    assert d.stats.ntargets == len(q)
    assert np.all(np.abs(h[q] - st.hsml[q]) <= 1e-12 * st.hsml[q])
    for extreme in (BOX, c.MinGasHsml):
        assert np.array_equal(h[q] == extreme, st.hsml[q] == extreme)
    assert np.abs(d.tree.Nodes_base["hmax"] - o.nodes["hmax"]).max() < 1e-12
    idle = np.ones(c.n, dtype=bool)
    idle[q] = False
    P0, S0, B0 = d.before
    assert np.array_equal(d.P[idle], P0[idle])
    ng = c.n - c.nbh
    assert np.array_equal(d.SphP[idle[:ng]], S0[idle[:ng]])
    if c.nbh:
        assert np.array_equal(d.BhP[:c.nbh][idle[ng:]], B0[:c.nbh][idle[ng:]])
    if len(q):
        assert d.stats.hsml_max_tried >= c.hsml[q].max() and d.stats.hsml_max_tried >= h[q].max()
    # EntVarPred is made for every gas particle, active or not
    assert np.abs(d.evp[:ng] - o.evp[:ng]).max() <= 1e-13 * np.abs(o.evp[:ng]).max()
    return st, o, dev


def check_fields(c, got, ref, scales, q, label):
    """the sums, per particle; `scales`: by-particle abs_* arrays.  Returns the worst relative Density deviation."""
    gas = q[c.type[q] == 0]
    worst = {}
    for name, rows in (("Density", q), ("EgyWtDensity", gas)):
        e = np.abs(got[name][rows] / ref[name][rows] - 1)
        worst[name] = e.max() if len(rows) else 0.0
        assert np.all(e < 1e-11), (label, name, worst[name])
    for name, rows in (("DivVel", q), ("CurlVel", gas), ("GradRho_mag", gas), ("DtHsml", q)):
        sca = scales["abs_" + name][rows]
        e = np.abs(got[name][rows] - ref[name][rows])
        ok = sca > 0
        worst[name] = (e[ok] / sca[ok]).max() if ok.any() else 0.0
        assert np.all(e <= 1e-11 * sca), (label, name, worst[name])
    f, rf = got["DhsmlEgyDensityFactor"][gas], ref["DhsmlEgyDensityFactor"][gas]
    ok = np.isfinite(rf) & (np.abs(rf) < 100)
    if len(gas) >= 512:
        assert ok.mean() > 0.75
    assert np.all(np.abs(f[ok] - rf[ok]) < 1e-11 * (1 + np.abs(rf[ok])) ** 2), (label, "DhsmlEgyDensityFactor")
    print("%-16s vs %-9s %s" % (c.name, label, "  ".join("%s %.1e" % kv for kv in worst.items())))
    return worst["Density"]


def check_case(ctx, c, ref=None):
    d = run_device(ctx, c)
    st, o, _ = check_against_oracle(c, d)
    q = targets_of(c)
    got = device_fields(c, d)
    if ref is not None:
        hdev = np.abs(got["Hsml"][q] / ref["Hsml"][q] - 1).max()
        print("%-16s Hsml vs all-pairs %.2e" % (c.name, hdev))
        assert hdev < 1e-12
        assert ref["niterations"] == d.stats.niterations
        check_fields(c, got, ref, ref, q, "all-pairs")
        scales = ref
    else:
        # no all-pairs loop for this case: the scales of the signed sums from one all-pairs pass at the radii the oracle ends with
        one = db.single_pass(c.pos, c.type, c.mass, c.vel, c.entropy, st.hsml, BOX, c.kernel, q)
        scales = {k: np.full(c.n, np.nan) for k in one}
        for k, v in one.items():
            scales[k][q] = v
    if len(q):
        check_fields(c, got, oracle_fields(c, st, o), scales, q, "oracle")
    return d, st, o


@pytest.mark.parametrize("name", list(sc.BRUTE_CASES))
def test_loop_against_oracle_and_all_pairs(ctx, name):
    c, ref = sc.reference(name)
    d, st, o = check_case(ctx, c, ref)
    if name == "huge_start":
        assert ref["npairs_first"].min() > 256          # every target began in the wave tier (NL_CAP) and left it
        assert ref["npairs_first"].max() <= 16384
    if name == "bh":
        ng = c.n - c.nbh
        assert np.all(ref["NumNgb"][ng:] > 1.9 * db.desnumngb(c.kernel))          # the holes converged on DesNumNgbBH


def test_refloor_raises_the_lower_half_only(ctx):
    """a second call from the device's own converged radii with MinGasHsml at their median: one pass, the lower half on the floor,
    the upper half bit-equal"""
    base, _ = sc.reference(sc.REFLOOR_BASE)
    d0 = run_device(ctx, base)
    h0 = d0.P["Hsml"].copy()
    c = sc.refloor(base, h0)
    ref = sc.brute_run(c)
    assert ref["niterations"] == 1 and ref["margin"] >= 1e-9
    assert ref["counters"]["floor_band"] > 0 and ref["counters"]["inband"] > 0
    d, st, o = check_case(ctx, c, ref)
    up = h0 >= c.MinGasHsml
    assert d.stats.niterations == 1 and 0 < up.sum() < c.n
    assert np.array_equal(d.P["Hsml"][up], h0[up])
    assert np.all(d.P["Hsml"][~up] == c.MinGasHsml)


@pytest.mark.parametrize("name", list(sc.ORACLE_CASES))
def test_loop_against_oracle(ctx, name):
    c = sc.ORACLE_CASES[name]()
    d, st, o = check_case(ctx, c)
    if name == "ragged0":
        assert d.stats.niterations == 1 and d.stats.ninteractions == 0
        assert np.array_equal(d.tree.Nodes_base["hmax"], d.nodes0["hmax"])
    if name == "tiers_active":
        assert o.niter > 3                                                    # the restarted targets iterate, the others are done at once
        assert np.all(st.hsml[c.giants] < 0.1 * BOX)                          # and come back from the heavy tiers


@pytest.mark.parametrize("name", ["dynrange", "dynrange_corner"])
def test_hydro_from_the_converged_dynrange_state(ctx, name):
    """hydro_force on the state density() leaves at Hsml = 1e-5 Box against the oracle, with the bars of
    test_heavy_targets_get_a_wave_or_a_workgroup, taken for the clump and for the background separately: the clump's
    accelerations are ten orders of magnitude above the background's"""
    c, ref = sc.reference(name)
    d = run_device(ctx, c)
    assert np.abs(d.P["Hsml"] / ref["Hsml"] - 1).max() < 1e-12
    P, SphP, tree = d.P, d.SphP, d.tree
    sq.force_tree_update_hmax(tree, d.pman)
    sq.set_densitypar(DensityResolutionEta=1.0, MaxNumNgbDeviation=c.dev, DensityKernelType=c.kernel, BlackHoleNgbFactor=2.0,
                      MinGasHsml=c.MinGasHsml)
    sq.set_hydropar(DensityIndependentSphOn=1, DensityContrastLimit=100.0, ArtBulkViscConst=0.75)
    hp = cm.hydro_params(kernel=c.kernel)
    st = orc.SphState(P, SphP, d.BhP)
    onint = orc.hydro(tree.Nodes_base, tree.firstnode, st, hp, d.evp)
    hs = sq.hydro_force(ctx, None, 0.1, cm.HUBBLE, d.evp, None, tree, d.pman, SphP)
    assert hs.ninteractions == onint
    a, oa = SphP["HydroAccel"], st.hydroaccel
    assert np.all(np.isfinite(oa)) and np.all(np.isfinite(a))
    clump = np.arange(c.n) >= 112
    for part, rows in (("background", ~clump), ("clump", clump)):
        ea = np.abs(a[rows] - oa[rows]).max() / np.abs(oa[rows]).max()
        ee = np.abs(SphP["DtEntropy"][rows] - st.dtentropy[rows]).max() / np.abs(st.dtentropy[rows]).max()
        print("%-16s hydro %-10s HydroAccel %.2e  DtEntropy %.2e of the part's maximum" % (name, part, ea, ee))
        assert ea < 1e-10, part
        assert ee < 1e-10, part
    assert np.abs(SphP["MaxSignalVel"] / st.maxsignalvel - 1).max() < 1e-12
