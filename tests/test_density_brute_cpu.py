"""The oracle's density() with its Hsml loop (a restatement of the reference's tree walk) against the all-pairs sum of
density_brute.py, on the inputs of sph_loop_cases.py: the same number of iterations, Hsml and Density to rounding, every outcome
of density_check_neighbours taken where a case claims it, and every NumNgb far enough from a decision threshold that a device
which adds in another order must take the same decisions.

Measured here (iterations; max relative deviation of Hsml and Density, oracle against all-pairs; the smallest |NumNgb - t| over all
targets and passes for t in {des - dev, des, des + dev}):

    case             iter  Hsml     Density  margin
    alone1            22   0        2.2e-16  22.3
    alone2            22   0        2.2e-16  19.2
    sparse20          11   2.2e-16  6.7e-16  1.2e-2
    sparse40           9   4.4e-16  8.9e-16  1.4e-2
    clump_floor       10   8.9e-16  3.1e-15  2.9e-4
    tiny_start        51   1.0e-15  3.1e-15  5.4e-6
    huge_start        15   2.4e-15  8.4e-15  3.1e-4
    kernel2           20   1.4e-15  2.9e-15  2.6e-5
    kernel4           18   1.2e-15  4.4e-15  3.0e-5
    bh                13   8.9e-16  3.7e-15  7.0e-4
    lattice           12   8.9e-16  7.8e-16  4.4e-6
    dynrange          41   1.1e-15  5.1e-15  2.2e-4
    dynrange_corner   42   8.9e-16  6.2e-15  6.7e-5
    kernel2_refloor    1   0        2.3e-15  2.6e-5

Outcomes counted over the file: bracket_collapse 3, bisect 12 633, bisect_box 50, grow_clamp 43 880, shrink_clamp 6 127,
newton 17 569, floor_R 200, floor_band 261, inband 8 303.

The lattice holds pairs exactly Box / 2 apart in a coordinate (5 cells of 0.8); they lie beyond every radius it tries, which is
what density_brute.density asserts for them."""
import numpy as np
import pytest

import orc
import density_brute as db
import sph_loop_cases as sc

NAMES = list(sc.BRUTE_CASES) + [sc.REFLOOR_BASE + "_refloor"]
MARGIN = 1e-9            # rounding of <= 2000 terms moves NumNgb by <= 2e-13 relative, 1e-11 absolute: a hundred times below this


@pytest.mark.parametrize("ktype", [1, 2, 4])
def test_numpy_kernels_match_the_pinned_kernels(ktype):
    """the piecewise polynomials of density_brute, in f64, against orc.density_kernel (pinned by the reference's golden values) to
    1e-14 relative (measured 4e-16).  Relative to the sum of the absolute values of the polynomial's terms: that is the value itself
    up to a small factor wherever the terms do not cancel, and what the rounding of both sides scales with where they do (dwk of
    the cubic at u = 0, dW at its zero crossing); at the very edge of the support, where (a - q)^p loses the digits of q on both
    sides alike, relative to 1e-3 of the kernel's central value."""
    support = db.KERNELS[ktype][0]
    assert abs(db.desnumngb(ktype) / orc.density_kernel(ktype, 1.0, 0.0)["desnumngb"] - 1) < 1e-14
    worst = 0.0
    for H in (0.37, 1.0, 8.5e-5):
        us = np.concatenate([np.linspace(0, 1, 201)[:-1], np.arange(1, support) / support + 1e-9, [1 - 1e-12]])
        got = db.kernel_values(ktype, np.float64(H), us)
        mag = db.kernel_values(ktype, np.float64(H), us, absolute=True)
        centre = orc.density_kernel(ktype, H, 0.0)["wk"]
        for k, u in enumerate(us):
            ref = orc.density_kernel(ktype, H, float(u))
            assert abs(got[3] / ref["volume"] - 1) < 1e-14
            for j, (name, floor) in enumerate((("wk", centre), ("dwk", centre / H), ("dW", centre / H))):
                err = abs(got[j][k] - ref[name]) / max(mag[j][k], 1e-3 * floor)
                worst = max(worst, err)
                assert err < 1e-14, (name, H, u, got[j][k], ref[name])
    print("kernel %d: worst deviation %.2e" % (ktype, worst))


@pytest.mark.parametrize("name", NAMES)
def test_oracle_loop_matches_all_pairs(name):
    c, ref = sc.reference(name)
    st, o = sc.oracle_run(c)
    gas = c.type == 0
    dens = np.empty(c.n)
    dens[gas] = st.density[:gas.sum()]
    dens[~gas] = st.bh_density[:c.nbh]
    dh = np.abs(st.hsml / ref["Hsml"] - 1).max()
    dd = np.abs(dens / ref["Density"] - 1).max()
    print("%-16s iterations %d / %d  Hsml %.2e  Density %.2e  margin %.2e  %s" %
          (name, o.niter, ref["niterations"], dh, dd, ref["margin"], {k: v for k, v in ref["counters"].items() if v}))
    assert o.niter == ref["niterations"]
    assert dh < 1e-13
    assert dd < 1e-13
    assert ref["margin"] >= MARGIN
    for outcome in sc.CLAIMS[name]:
        assert ref["counters"][outcome] > 0, outcome
    if name.startswith("alone"):
        assert np.all(ref["Hsml"] == sc.BOX) and np.all(st.hsml == sc.BOX)
    if name == "clump_floor":
        assert (ref["Hsml"][-200:] == c.MinGasHsml).sum() >= 190               # the clump ends on the floor, exactly
        assert np.array_equal(ref["Hsml"] == c.MinGasHsml, st.hsml == c.MinGasHsml)
    if name.startswith("sparse"):
        assert ref["Hsml"].max() > 0.5 * sc.BOX
    if name.startswith("dynrange"):
        assert ref["Hsml"].min() < 1.2e-5 * sc.BOX
    if name == "huge_start":
        assert ref["npairs_first"].min() > 256             # every target starts beyond a lane's list (NL_CAP)
    if name.endswith("_refloor"):
        base = sc.reference(name[:-len("_refloor")])[1]["Hsml"]
        up = base >= c.MinGasHsml
        assert ref["niterations"] == 1 and 0 < up.sum() < c.n
        assert np.array_equal(ref["Hsml"][up], base[up]) and np.all(ref["Hsml"][~up] == c.MinGasHsml)
        assert np.array_equal(st.hsml, ref["Hsml"])


def test_every_outcome_was_taken():
    """over the cases of this file each of the nine outcomes of density_check_neighbours occurs"""
    total = dict.fromkeys(db.OUTCOMES, 0)
    for name in NAMES:
        for k, v in sc.reference(name)[1]["counters"].items():
            total[k] += v
    print(total)
    assert all(total[k] > 0 for k in db.OUTCOMES), total


def test_all_fields_match_the_oracle():
    """every field of the postprocess, on the case with black holes: the oracle against the all-pairs sums, each signed sum to 1e-13 of
    the sum of the absolute values of its terms"""
    c, ref = sc.reference("bh")
    st, o = sc.oracle_run(c)
    ng = c.n - c.nbh
    g = slice(0, ng)
    assert np.abs(st.egywtdensity / ref["EgyWtDensity"][g] - 1).max() < 1e-13
    assert np.all(np.abs(st.divvel - ref["DivVel"][g]) < 1e-13 * ref["abs_DivVel"][g])
    assert np.all(np.abs(st.curlvel - ref["CurlVel"][g]) < 1e-13 * ref["abs_CurlVel"][g])
    assert np.all(np.abs(st.dthsml - ref["DtHsml"]) < 1e-13 * ref["abs_DtHsml"])
    assert np.all(np.abs(np.linalg.norm(o.gradrho, axis=1) - ref["GradRho_mag"][g]) < 1e-13 * ref["abs_GradRho_mag"][g])
    assert np.all(np.abs(st.bh_divvel[:c.nbh] - ref["DivVel"][ng:]) < 1e-13 * ref["abs_DivVel"][ng:])
    f, rf = st.dhsmlegydensityfactor, ref["DhsmlEgyDensityFactor"][g]
    ok = np.isfinite(rf) & (np.abs(rf) < 100)
    assert ok.mean() > 0.75
    assert np.all(np.abs(f[ok] - rf[ok]) < 1e-13 * (1 + np.abs(rf[ok])) ** 2)
    assert np.abs(o.evp[:ng] - c.entropy[:ng] ** (1 / db.GAMMA)).max() < 1e-14
