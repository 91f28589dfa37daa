"""Star formation without a GPU: the library's host engine (shq_sfr_eval_host, csrc/sfr_math.hpp driven in a plain loop) equals the
line-by-line Python restatement of sfr_eff.cpp (sfr_restated.py) bit for bit in every output of every mode and in the evaluation
counts; the argument checks; the header's structs against their ctypes mirrors; and the agreement of the host engine with a second
host build whose every libm result is moved by one ulp (SHQ_COOL_NUDGE) in every discrete outcome, with the margins that make the GPU
test's "zero flips" a consequence and not luck."""
import ctypes as C

import numpy as np
import pytest

import shenqi_amd as sq
from shenqi_amd import capi
import sfr_cases as sc

# The smallest relative distance of any particle of the set (sfr_cases.particles, seed 20261018) from each discrete decision that a
# libm result enters, over BHFeedbackUseTcool 0..3, as test_nudged_build_agrees recomputes them:
#   the draw against prob            |draw - prob| / prob                         1.44e-2
#   clause 4 of sfreff_on_eeqos      |unew - 3.2 egyeff| / (3.2 egyeff)           1.14e-3
#   tcool < trelax                   |tcool - trelax| / trelax                    2.71e-3
#   egycurrent > egyeff              |egycurrent - egyeff| / egyeff               1.30e-3
#   egycurrent > 5e6                 |egycurrent - 5e6| / 5e6                     1.50e-2
# The device may differ from the host by 1.5 * 2.5e-5 + 1e-9 relative in these quantities at most (the hard bound derived in
# test_gpu_sfr.py), so a margin above MARGIN_NEEDED cannot flip there.
MARGIN_NEEDED = 1.5 * 2.5e-5 + 1e-9
MARGINS_RECORDED = dict(draw=1.44e-2, clause4=1.14e-3, tcool_vs_trelax=2.71e-3, egycurrent_vs_egyeff=1.30e-3, egycurrent_vs_5e6=1.50e-2)


def _equal(h, r, where=""):
    """a host result against sfr_cases.restated's tuple: statuses, evaluation counts, every row and byte of every OK particle"""
    out, flags, decision, branch, ev, left = r
    # the restatement leaves the table exactly where the library defers (it then evaluates a fit the library does not have)
    assert np.array_equal(h.status == capi.COOL_DEFERRED, left), where
    ok = h.status == capi.COOL_OK
    assert np.array_equal(ok, ~left), where
    assert np.array_equal(h.steps[ok], ev[ok]), where
    for i, name in enumerate(capi.SFR_OUT):
        a, b = h.out[i][ok], out[i][ok]
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (where, name, np.flatnonzero(a.view(np.uint64) != b.view(np.uint64))[:5])
    assert np.array_equal(h.flags[ok], flags[ok]) and np.array_equal(h.decision[ok], decision[ok]) and np.array_equal(h.branch[ok], branch[ok]), where
    # a particle that is not OK is not written
    assert np.isnan(h.out[:, ~ok]).all() and np.all(h.decision[~ok] == 255)


# ---- the host engine against the restatement, bit for bit -----------------------------------------------------------------------------------

@pytest.mark.parametrize("tcool", [0, 1, 2, 3])
def test_starform_equals_restatement(tcool):
    """the dense set with the edge rows under each BHFeedbackUseTcool"""
    par, p = sc.params(BHFeedbackUseTcool=tcool), sc.particles()
    h = sc.host_starform(tcool)
    _equal(h, sc.restated("STARFORM", par, p), f"tcool {tcool}")
    ok = h.status == capi.COOL_OK
    n, ne = len(ok), len(sc.EDGE_ROWS)
    # the set does what it is for: every decision, every branch of find_star_mass, both sides of each test
    assert set(h.decision[ok]) == {0, 1, 2}
    mos, mass = h.mass_of_star[ok], np.asarray(p["Mass"])[ok]
    assert (mos == sc.AVG_BARYON_MASS / 2).any() and (mos == mass).any() and (mass < sc.AVG_BARYON_MASS / 2).any()
    assert ((h.branch[ok] & capi.SFR_B_RELAXED) == 0).any() and ((h.branch[ok] & capi.SFR_B_RELAXED) != 0).any()
    edge = {name: n - ne + i for i, name in enumerate(sc.EDGE_ROWS)}
    k = edge["tsfr_below_dtime"]
    assert h.tsfr[k] == p["dloga"][k] / sc.HUBBLE
    for name in ("in_the_wind", "below_overdensity"):       # data keeps its initial values (:775-784)
        k = edge[name]
        assert (h.branch[k] & capi.SFR_B_ON_EEQOS) == 0 and h.cloudfrac[k] == 0 and h.trelax[k] == par["MaxSfrTimescale"] and h.smr[k] == 0 and h.Ne[k] == 0
    k = edge["deferred_bh_heated"]
    if tcool in (1, 3):
        assert h.status[k] == capi.COOL_DEFERRED
        assert ((h.branch[ok] & capi.SFR_B_TCOOL_WON) != 0).any() and ((h.branch[ok] & capi.SFR_B_TCOOL) != 0).sum() > ((h.branch[ok] & capi.SFR_B_TCOOL_WON) != 0).sum()
        assert ((h.flags[ok] ^ np.asarray(p["flags"])[ok]) == capi.SFR_FLAG_BHHEATED).any()
    else:
        assert np.array_equal(h.flags[ok], np.asarray(p["flags"])[ok])
    if tcool == 2:
        c4 = (h.branch[ok] & capi.SFR_B_CLAUSE4) != 0
        assert ((h.branch[ok][c4] & capi.SFR_B_ON_EEQOS) == 0).any() and ((h.branch[ok][c4] & capi.SFR_B_ON_EEQOS) != 0).any()


@pytest.mark.parametrize("criterion", sc.CRITERIA)
def test_criteria_equal_restatement(criterion):
    par, p = sc.params(StarformationCriterion=criterion), sc.particles()
    h = sc.host("STARFORM", par, p)
    _equal(h, sc.restated("STARFORM", par, p), f"criterion {criterion}")
    base = sc.host_starform(1)
    ok = (h.status == capi.COOL_OK) & (base.smr > 0)
    assert (criterion == 1) == bool(np.array_equal(h.smr[ok], base.smr[ok]))
    if criterion == 13:
        assert (h.smr[ok] == 0).any() and (h.smr[ok] > 0).any()       # convergent flows only


@pytest.mark.parametrize("boost", [0, 1])
def test_boost_equals_restatement(boost):
    par, p = sc.params(BoostSFDenseGas=boost, BoostSFOverDenseFactor=50.0), sc.particles()
    h = sc.host("STARFORM", par, p)
    _equal(h, sc.restated("STARFORM", par, p), f"boost {boost}")
    assert bool(boost) == bool((h.tsfr != sc.host_starform(1).tsfr)[h.status == capi.COOL_OK].any())


def test_quick_lyman_alpha_equals_restatement():
    par, p = sc.params(QuickLymanAlphaProbability=0.5, QuickLymanAlphaTempThresh=1e5), sc.particles()
    h = sc.host("STARFORM", par, p)
    _equal(h, sc.restated("STARFORM", par, p), "quicklya")
    assert np.all(h.status == capi.COOL_OK) and np.all(h.steps == 0) and set(h.decision) == {0, 1}
    hit = h.decision == 1
    assert np.array_equal(h.sm[hit], np.asarray(p["Mass"])[hit]) and np.all(h.sm[~hit] == 0)
    assert np.array_equal(h.Entropy, p["Entropy"]) and np.array_equal(h.Ne, p["Ne"])      # no eeqos physics runs


@pytest.mark.parametrize("tcool", [1, 2])
@pytest.mark.parametrize("what", ["EGYEFF", "NH0", "HE0", "HEP", "HEPP", "ON_EEQOS"])
def test_queries_equal_restatement(what, tcool):
    par, p = sc.params(BHFeedbackUseTcool=tcool), sc.particles()
    h = sc.host(what, par, p)
    _equal(h, sc.restated(what, par, p), f"{what} tcool {tcool}")
    if what == "ON_EEQOS":
        assert np.array_equal((h.branch & capi.SFR_B_ON_EEQOS) != 0, (sc.host_starform(tcool).branch & capi.SFR_B_ON_EEQOS) != 0)


def test_fractions_of_quick_lyman_alpha_gas():
    """QuickLymanAlphaProbability > 0 sends every particle down the standard-gas branch (:550, :583)"""
    par, p = sc.params(QuickLymanAlphaProbability=1.0), sc.subset(sc.particles(), slice(0, 200))
    _equal(sc.host("NH0", par, p), sc.restated("NH0", par, p), "NH0 quicklya")


def test_net_heating_gives_zero_cooling_time():
    """the synthetic strong-heating UVBG as the local one: GetCoolingTime returns 0, y is infinite, cloudfrac 1, trelax 0 and
    exp(-dtime / 0) = 0, all by IEEE arithmetic and without a guard, as in the reference"""
    uv = sc.heating_uvbg()
    p = sc.heating_subset()
    for tcool in (0, 1, 3):
        par = sc.params(BHFeedbackUseTcool=tcool)
        h = sc.host("STARFORM", par, p, local_uv=uv)
        _equal(h, sc.restated("STARFORM", par, p, local_uv=uv), f"heating tcool {tcool}")
        on = (h.status == capi.COOL_OK) & ((h.branch & capi.SFR_B_ON_EEQOS) != 0)
        assert on.sum() > 200 and np.all(h.cloudfrac[on] == 1) and np.all(h.trelax[on] == 0)
        rel = on & ((h.branch & capi.SFR_B_RELAXED) != 0)
        densityfac = h.egycurrent[rel] / np.asarray(p["Entropy"])[rel]
        # the relaxation lands on egyeff = EgySpecCold at once (the bits are _equal's business; densityfac here is a quotient)
        assert np.allclose(h.Entropy[rel] * densityfac, par["EgySpecCold"], rtol=1e-14, atol=0) and np.all(h.egyeff[rel] == par["EgySpecCold"])
    _equal(sc.host("NH0", sc.params(), p, local_uv=uv), sc.restated("NH0", sc.params(), p, local_uv=uv), "heating NH0")


def test_threads_do_not_matter():
    a = sc.host_starform(1)
    b = sc.host("STARFORM", sc.params(BHFeedbackUseTcool=1), sc.particles(), nthreads=1)
    for x, y in zip(a.arrays(), b.arrays()):
        assert np.array_equal(x, y, equal_nan=True)


# ---- arguments and structs ----------------------------------------------------------------------------------------------------------------------

def test_bad_arguments():
    p = sc.subset(sc.particles(), slice(0, 8))
    for crit in (3, 3 | 5, 3 | 21):       # "GradRho not allocated but has SFR_CRITERION_MOLECULAR_H2" (sfr_eff.cpp:822-823)
        with pytest.raises(sq.ShqError):
            sc.host("STARFORM", sc.params(StarformationCriterion=crit), {k: v for k, v in p.items() if k != "GradRho"})
    sc.host("STARFORM", sc.params(StarformationCriterion=5), {k: v for k, v in p.items() if k != "GradRho"})
    with pytest.raises(sq.ShqError):
        sc.host("STARFORM", sc.params(Generations=0), p)
    with pytest.raises(sq.ShqError):
        sc.host("STARFORM", sc.params(BHFeedbackUseTcool=4), p)
    c = sc.case()
    with pytest.raises(sq.ShqError):
        sq.sfr_eval_host(c.tables(), sc.lib_params(sc.params()), "STARFORM", p, c.uvbg(), sc.REDSHIFT, sc.A3INV, sc.HUBBLE, np.zeros(0))


def test_statuses():
    p = {k: np.array(v[:3]) for k, v in sc.particles().items()}
    p["Density"][1], p["Mass"][2] = np.nan, 0.0
    h = sc.host("STARFORM", sc.params(), p)
    assert list(h.status) == [capi.COOL_OK, capi.COOL_BADINPUT, capi.COOL_BADINPUT]
    assert np.isfinite(h.out[:, 0]).all() and np.isnan(h.out[:, 1:]).all()


@pytest.fixture(scope="module")
def nudged(tmp_path_factory):
    return sc.build_nudged(tmp_path_factory.mktemp("sfr_nudged"))


def test_structs_match_header(nudged):
    assert nudged[1] == [C.sizeof(capi.SfrParams), C.sizeof(capi.SfrArrays), C.sizeof(capi.SfrEvalStep), C.sizeof(capi.SfrFields), C.sizeof(capi.SfrResultC)]


# ---- the perturbed build ------------------------------------------------------------------------------------------------------------------------

def test_nudged_build_agrees(nudged):
    """every discrete outcome of every particle, and the margins that protect them"""
    p = sc.particles()
    smallest = {}
    for tcool in range(4):
        par = sc.params(BHFeedbackUseTcool=tcool)
        h = sc.host_starform(tcool)
        nd = sc.host("STARFORM", par, p, entry=nudged[0])
        assert np.array_equal(h.status, nd.status)
        ok = h.status == capi.COOL_OK
        assert not np.array_equal(h.cloudfrac[ok], nd.cloudfrac[ok])      # the hook is in
        for k in ("decision", "branch", "flags"):       # branch: clause 4, egycurrent > egyeff, tcool < trelax, the draw
            assert np.array_equal(getattr(h, k)[ok], getattr(nd, k)[ok]), (tcool, k)
        for k, v in sc.margins(h, p).items():
            smallest[k] = min(smallest.get(k, np.inf), v)
    print("smallest margins:", {k: f"{v:.3g}" for k, v in smallest.items()})
    assert set(smallest) == set(MARGINS_RECORDED)
    for k, v in smallest.items():
        assert v > MARGIN_NEEDED, (k, v)
        assert abs(v / MARGINS_RECORDED[k] - 1) < 0.01, (k, v)      # the record above is this set's
