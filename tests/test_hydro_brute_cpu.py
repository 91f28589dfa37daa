"""The oracle's hydro_force() (a restatement of the reference's symmetric tree walk, on the project's host tree with the node hmax
force_tree_update_hmax leaves) against the all-pairs sum of hydro_brute.py, on the synthetic inputs of hydro_cases.py; that no pair
of any case lies within 1e-12 of a radius squared, so a device whose r2 differs in the last bit still has to accept the same pairs;
that every case reaches the branches it claims; and that the cases have teeth: four deliberately wrong oracle runs miss the bars by
five orders of magnitude and more.

Bars, as in test_gpu_hydro_brute.py: HydroAccel (each component) and DtEntropy per particle to 1e-11 of the sum of the absolute values
of the terms; MaxSignalVel to 1e-12 relative.

Measured here (targets and accepted pairs of the all-pairs sum; oracle against all-pairs: the largest |deviation| / abs-sum over the
targets for HydroAccel and DtEntropy, the largest relative deviation of MaxSignalVel; the margin, the smallest |r2 / h^2 - 1| over
all pairs and both radii; host seconds of the all-pairs sum):

    case            targets    pairs   HydroAccel DtEntropy MaxSigVel  margin   seconds
    reach              1028    11448   1.9e-15   1.6e-14   4.4e-16    4.6e-05  0.11
    contrast_100_1      512     7976   1.1e-15   3.2e-15   4.4e-16    3.5e-05  0.04
    contrast_1_1        512     7976   9.8e-16   3.2e-15   4.4e-16    3.5e-05  0.05
    contrast_0_1        512     7976   1.1e-15   3.2e-15   4.4e-16    3.5e-05  0.05
    contrast_-1_1       512     7976   9.4e-16   3.2e-15   4.4e-16    3.5e-05  0.05
    contrast_*_0        512     7976   1.1e-15   3.4e-15   4.4e-16    3.5e-05  0.05
    drift               400    10633   1.6e-15   3.2e-15   3.3e-16    4.3e-05  0.04
    drift_noevp         400    10633   1.6e-15   3.2e-15   3.3e-16    4.3e-05  0.04
    drift_dloga0        400    10633   1.5e-15   2.4e-15   3.3e-16    4.3e-05  0.04
    kernels_1_0 / _1    512    17420   1.2e-15   1.6e-15   4.4e-16    2.8e-06  0.04
    kernels_2_0 / _1    512    18682   1.1e-15   1.9e-15   4.4e-16    3.2e-05  0.04
    kernels_4_0 / _1    512    18634   1.2e-15   2.6e-15   4.4e-16    9.0e-06  0.04
    coincident          512     7896   1.1e-15   9.9e-15   4.4e-16    2.9e-05  0.03
    winds               512     7021   2.5e-15   6.1e-15   7.8e-16    6.8e-05  0.03
    mixed_types        1000    20536   1.2e-15   3.4e-15   4.4e-16    2.5e-05  0.10
    ragged1               1       40   1.4e-16   2.9e-16   2.2e-16    2.9e-03  0.00
    ragged63             63     1738   3.3e-15   2.1e-15   4.4e-16    1.3e-04  0.01
    ragged65             65     1765   1.3e-15   1.0e-15   4.4e-16    1.5e-04  0.01
    ragged1001         1001    26786   7.5e-16   3.6e-15   4.4e-16    8.3e-06  0.11
    tiers               512  1147887   6.5e-15   2.6e-14   4.4e-16    7.4e-07  2.88

Teeth (the same ratios for the wrong runs; the bar is 1e-11): reach with hmax zeroed 4.0e-2 / 1.0 / 0.58; contrast at 1.0 with the
oracle given 100: 1.3 for HydroAccel (DtEntropy holds the viscous term alone and does not see the limit); drift with the oracle's
drifts zeroed 0.98 / 8.4e-2 / 0.19; winds with DelayTime cleared 11 / 83 / 44.
"""
import time

import numpy as np
import pytest

import hydro_brute as hb
import hydro_cases as hc
from density_brute import min_image

MARGIN = 1e-12
BAR, BAR_SIG = 1e-11, 1e-12
TEETH = 1e-6


def by_target(c, st, q):
    """the oracle's results for the particles `q`, by position in q"""
    s = c.pi[q]
    return {"HydroAccel": st.hydroaccel[s], "DtEntropy": st.dtentropy[s], "MaxSignalVel": st.maxsignalvel[s]}


def deviations(got, ref):
    """(worst |dev| / abs-sum of HydroAccel, of DtEntropy, worst relative dev of MaxSignalVel) over the targets of `ref`"""
    def worst(err, sca):
        ok = sca > 0
        assert np.all(err[~ok] == 0)
        return float((err[ok] / sca[ok]).max()) if ok.any() else 0.0
    ea = worst(np.abs(got["HydroAccel"] - ref["HydroAccel"]), ref["abs_HydroAccel"])
    ee = worst(np.abs(got["DtEntropy"] - ref["DtEntropy"]), ref["abs_DtEntropy"])
    es = float(np.abs(got["MaxSignalVel"] / ref["MaxSignalVel"] - 1).max()) if len(ref["MaxSignalVel"]) else 0.0
    return ea, ee, es


def check(got, ref, label):
    assert all(np.all(np.isfinite(got[k])) for k in got), label
    ea, ee, es = deviations(got, ref)
    print("%-16s %-9s HydroAccel %.1e  DtEntropy %.1e  MaxSignalVel %.1e" % (label, "", ea, ee, es))
    assert np.all(np.abs(got["HydroAccel"] - ref["HydroAccel"]) <= BAR * ref["abs_HydroAccel"]), (label, ea)
    assert np.all(np.abs(got["DtEntropy"] - ref["DtEntropy"]) <= BAR * ref["abs_DtEntropy"]), (label, ee)
    assert es <= BAR_SIG, (label, es)
    return ea, ee, es


@pytest.mark.parametrize("name", list(hc.SYNTHETIC))
def test_oracle_matches_all_pairs(name):
    t0 = time.perf_counter()
    c, ref = hc.reference(name)
    t1 = time.perf_counter()
    q = hc.brute_targets(c)
    st, nint = hc.oracle_run(c)
    tot = {k: int(v.sum()) for k, v in ref["counters"].items()}
    print("%-16s targets %d  pairs %d  margin %.2e  all-pairs %.2f s  %s" % (name, len(q), ref["npairs"].sum(), ref["margin"], t1 - t0,
                                                                         {k: v for k, v in tot.items() if v}))
    check(by_target(c, st, q), ref, name)
    assert ref["margin"] >= MARGIN
    for k in hc.CLAIMS.get(name, ()):
        assert tot[k] > 0, k
    if name == "reach":
        g = np.isin(q, c.giants)
        assert np.all(ref["counters"]["by_hi_only"][g] > 50)
        assert np.all(ref["counters"]["wrapped"][np.isin(q, c.giants[:2])] > 100)         # the corner giants reach across the faces
        assert (ref["counters"]["by_hj_only"][~g] > 0).mean() > 0.3                       # the others are reached from outside their own radius
    if name == "contrast_1_1":
        bit = ref["counters"]["contrast_i"] > 0
        assert 0.2 < bit.mean() < 0.8                                                     # the clamp bites on some targets, not on others
        assert np.all(ref["counters"]["contrast_j"] > 0) and np.all(ref["counters"]["contrast_j"] < ref["npairs"])
    if name.startswith("contrast") and name not in hc.CLAIMS:
        assert tot["contrast_i"] == tot["contrast_j"] == 0
    if name.startswith("drift"):
        assert len(q) < 0.5 * c.n and np.all(c.drifts[c.bin_hydro[q]] == 0) and (c.drifts[c.bin_hydro] > 0).any() and (c.drifts[c.bin_hydro] < 0).any()
        assert 20 <= (ref["counters"]["density_guard"] > 0).sum()
    if name == "coincident":
        tw = np.isin(q, c.twins)
        assert np.array_equal(ref["counters"]["coincident"] > 0, tw) and ref["counters"]["coincident"].max() == 2
    if name == "winds":
        w = c.wind[q]
        assert np.all(ref["HydroAccel"][w] == 0) and np.all(ref["DtEntropy"][w] == 0) and np.all(ref["HydroAccel"][~w].any(axis=1))
        windspeed = 2 * 3.5 * c.atime * hb.time_factors(c.atime, c.hubble)[0]
        assert np.all(ref["MaxSignalVel"][w] >= np.cbrt(0.2 / c.sph["Density"][c.pi[q][w]]) * c.atime * windspeed * (1 - 1e-15))
    if name == "mixed_types":
        assert len(q) == 1000 and len(c.active) == c.n and np.any(np.diff(c.active) < 0)
    if name.startswith("ragged"):
        assert len(c.active) == int(name[6:]) and np.all(c.drifts[c.bin_hydro[q]] == 0)
    if name == "tiers":
        cn = ref["counters"]
        ng, nw = len(c.giants), len(c.wave)
        print("tiers: pairs of the giants %s, of the wave tier %d..%d, of the others %d..%d" % (ref["npairs"][:ng], ref["npairs"][ng:ng + nw].min(),
              ref["npairs"][ng:ng + nw].max(), ref["npairs"][ng + nw:].min(), ref["npairs"][ng + nw:].max()))
        assert len(q) == 512 and ng == 3 and nw == 61 and len(c.ordinary) == 448
        assert ref["npairs"][:ng].min() > 8192 and np.all(c.hsml[c.giants] == 0.49 * hc.BOX)
        assert np.median(ref["npairs"][ng:ng + nw]) > 256                                 # more than a lane's list holds (NL_CAP)
        # ordinary targets a giant's radius reaches and their own does not
        o = c.ordinary
        d = np.sqrt((min_image(c.pos[o][:, None, :] - c.pos[c.giants][None, :, :], hc.BOX) ** 2).sum(axis=2))
        from_giant = ((d > c.hsml[o][:, None]) & (d < c.hsml[c.giants][None, :])).any(axis=1)
        assert (from_giant & (cn["by_hj_only"][ng + nw:] > 0)).sum() >= 64
        assert np.array_equal(from_giant, from_giant & (cn["by_hj_only"][ng + nw:] > 0))


def test_every_counter_was_reached():
    total = dict.fromkeys(hb.COUNTERS, 0)
    for name in hc.SYNTHETIC:
        if name != "tiers":
            for k, v in hc.reference(name)[1]["counters"].items():
                total[k] += int(v.sum())
    print(total)
    assert all(total[k] > 0 for k in hb.COUNTERS), total


def test_limit_is_ignored_without_disph():
    """DensityIndependentSphOn = 0: the all-pairs sums do not depend on DensityContrastLimit"""
    base = hc.reference("contrast_100_0")[1]
    for name in ("contrast_1_0", "contrast_-1_0"):
        ref = hc.reference(name)[1]
        for k in ("HydroAccel", "DtEntropy", "MaxSignalVel"):
            assert np.array_equal(ref[k], base[k]), (name, k)
    on = hc.reference("contrast_100_1")[1]
    assert np.array_equal(hc.reference("contrast_0_1")[1]["HydroAccel"], on["HydroAccel"])   # no ratio reaches 100: both leave it as it is
    for name in ("contrast_1_1", "contrast_-1_1"):                                        # the clamp and the switched-off term give other numbers
        assert np.abs(hc.reference(name)[1]["HydroAccel"] - on["HydroAccel"]).max() > 1e-3 * np.abs(on["HydroAccel"]).max(), name


def teeth(name, **wrong):
    c, ref = hc.reference(name)
    q = hc.brute_targets(c)
    st, _ = hc.oracle_run(c, **wrong)
    ea, ee, es = deviations(by_target(c, st, q), ref)
    print("%-16s %-28s HydroAccel %.1e  DtEntropy %.1e  MaxSignalVel %.1e" % (name, ", ".join(wrong), ea, ee, es))
    return ea, ee, es


def test_teeth_reach_with_hmax_zeroed():
    ea, ee, es = teeth("reach", zero_hmax=True)
    assert ea >= TEETH and ee >= TEETH


def test_teeth_contrast_limit_not_applied():
    ea, ee, es = teeth("contrast_1_1", contrast=100.0)
    assert ea >= TEETH


def test_teeth_drifts_zeroed():
    ea, ee, es = teeth("drift", drifts=np.zeros(hc.NBINS))
    assert ea >= TEETH and ee >= TEETH


def test_teeth_wind_neighbours_not_skipped():
    ea, ee, es = teeth("winds", clear_delay=True)
    assert ea >= TEETH and ee >= TEETH
