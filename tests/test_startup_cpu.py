"""Run start-up without a device: the host functions of csrc/startup.hip against hand-computed values, the branch coverage of the
restatements in startup_restated.py (every branch of every loop is reached by the shared cases, asserted by counters), and the restated
set_init_hsml against the host mirror on the same tree."""
import collections
import math

import numpy as np
import pytest

import shenqi_amd as sq
import startup_restated as st


def test_mean_separation_by_hand():
    ms = sq.mean_separation(1000.0, [8, 27, 0, 1000000, 64, 1])
    assert ms[0] == 1000.0 / math.pow(8, 1.0 / 3) and ms[1] == 1000.0 / math.pow(27, 1.0 / 3) and ms[4] == 1000.0 / math.pow(64, 1.0 / 3)
    assert np.allclose(ms, [500.0, 1000.0 / 3, 0.0, 10.0, 250.0, 1000.0], rtol=1e-14)
    assert ms[2] == 0.0    # a type without particles keeps its zero


def test_u_init_by_hand():
    k_over_mp = 1.38066e-16 / 1.6726e-24
    assert abs(k_over_mp / 8.254574e7 - 1) < 1e-6
    uu = 1.0e10
    # neutral gas: molecular weight 4 / (1 + 3 * 0.76) = 1.2195122
    u, T = sq.u_init(100.0, 2.7255, 0.01, uu, 0.0)
    assert T == 100.0 and u == (1.0 / ((5.0 / 3.0) - 1)) * k_over_mp * 100.0 / uu / (4 / (1 + 3 * 0.76))
    assert abs(u / 1.0153126 - 1) < 1e-6          # 1.5 * 8.254574e7 * 100 / 1e10 / 1.2195122
    # full ionisation above 1e4 K: 4 / (8 - 5 * 0.24) = 0.58823529
    u, T = sq.u_init(2.0e4, 2.7255, 0.01, uu, 0.0)
    assert u == (1.0 / ((5.0 / 3.0) - 1)) * k_over_mp * 2.0e4 / uu / (4 / (8 - 5 * (1 - 0.76)))
    assert abs(u / 420.98327 - 1) < 1e-6          # 1.5 * 8.254574e7 * 2e4 / 1e10 / 0.58823529
    # exactly 1e4 K is still neutral
    assert sq.u_init(1.0e4, 2.7255, 0.01, uu, 0.0)[0] == (1.0 / ((5.0 / 3.0) - 1)) * k_over_mp * 1.0e4 / uu / (4 / (1 + 3 * 0.76))
    # the MinEgySpec floor
    assert sq.u_init(100.0, 2.7255, 0.01, uu, 7.5)[0] == 7.5
    assert sq.u_init(100.0, 2.7255, 0.01, uu, 1.0)[0] > 1.0
    # InitGasTemp < 0: CMBTemperature / atime = 272.55 K
    u, T = sq.u_init(-1.0, 2.7255, 0.01, uu, 0.0)
    assert T == 2.7255 / 0.01 and u == sq.u_init(2.7255 / 0.01, 0.0, 1.0, uu, 0.0)[0]
    assert abs(u / 2.7672344 - 1) < 1e-6          # 1.0153126 * 2.7255


def test_omega_verdict_on_both_sides():
    Box, rhocrit, Omega0 = 10.0, 2.0, 0.3
    norm = Box ** 3 * rhocrit     # 2000
    mt = [30.0, 500.0, 0, 0, 10.0, 1.0]
    om, o, bad = sq.check_omega(mt, 0.3 * norm, Box, rhocrit, Omega0)
    assert np.array_equal(om, np.array(mt) / norm) and o == 0.3 and not bad
    assert not sq.check_omega(mt, (0.3 + 0.0009) * norm, Box, rhocrit, Omega0)[2]
    assert sq.check_omega(mt, (0.3 + 0.0011) * norm, Box, rhocrit, Omega0)[2]
    assert not sq.check_omega(mt, (0.3 - 0.0009) * norm, Box, rhocrit, Omega0)[2]
    assert sq.check_omega(mt, (0.3 - 0.0011) * norm, Box, rhocrit, Omega0)[2]
    # the neutrinos followed analytically count only with MassiveNuLinRespOn
    assert sq.check_omega(mt, 0.29 * norm, Box, rhocrit, Omega0, OmegaNu=0.01)[2]
    _, o, bad = sq.check_omega(mt, 0.29 * norm, Box, rhocrit, Omega0, OmegaNu=0.01, MassiveNuLinRespOn=True)
    assert o == 0.29 * norm / norm + 0.01 and not bad
    with pytest.raises(sq.StartupError, match="The mass content is Omega0 = 0.3011,but you specified Omega0 = 0.3 in the parameterfile."):
        sq.check_omega(mt, (0.3 + 0.0011) * norm, Box, rhocrit, Omega0, raise_on=True)


def test_meanbar_by_hand():
    # 0.05 * 3 * (3.2407789e-18 * 0.7)^2 / (8 pi 6.672e-8) = 4.6033e-31 g / cm^3
    m = sq.meanbar(0.05, 0.7)
    assert m == 0.05 * 3 * 3.2407789e-18 * 0.7 * 3.2407789e-18 * 0.7 / (8 * math.pi * 6.672e-8)
    assert abs(m / 4.6033e-31 - 1) < 1e-4


def test_record_loops_reach_every_branch():
    c = collections.Counter()
    for n in st.COUNTS[:-1]:
        for reion in (True, False):
            for mode, par in st.MODES.items():
                k = st.case(n, reion)
                st.particles(k.P, k.S, k.B, par, st.OMEGA | st.POSITIONS | st.HSML | st.INIT, c)
    for nzero in (0, 1):
        k = st.case(65, True, nzero)
        r = st.particles(k.P, k.S, k.B, st.MODES["ic"], st.POSITIONS, c)[3]
        assert r["numzero"] == nzero
    assert st.particles(st.case(257).P, st.case(257).S, st.case(257).B, st.MODES["ic"], st.POSITIONS)[3]["numzero"] == 2
    for b in ("recovered", "type0", "type1", "type2", "type3", "type4", "type5", "negative", "toolarge", "nan", "inf", "zero", "hsml_large", "hsml_zero",
              "hsml_negative", "star_hsml", "bad_delaytime", "ic", "restart", "reion_on", "reion_off", "reion_absent", "bh_mass"):
        assert c[b] > 0, b


def test_density_entropy_cases_reach_every_branch_and_stay_off_the_floor():
    c = collections.Counter()
    for n in st.COUNTS[1:]:
        S = st.entropy_case(n)
        after, bad, raised = st.check_density_entropy(S, st.MEANBAR, st.MINEGYSPEC, st.ATIME, c)
        floor = st.minent(after, st.MINEGYSPEC, st.ATIME)
        assert np.all(np.abs(S["Entropy"] / floor - 1) >= 1e-9)      # no rounding of the floor decides a branch
        assert np.array_equal(raised, np.flatnonzero(S["Entropy"] < floor))
    for b in ("density_nonpositive", "density_nan", "density_inf", "egy_replaced", "entropy_below", "entropy_above"):
        assert c[b] > 0, b


def test_mass_sums_of_the_restatement_mix_three_magnitudes():
    k = st.case(1000)
    rep = st.particles(k.P, k.S, k.B, st.MODES["ic"], st.OMEGA)[3]
    m = np.array(rep["mass_all"])
    assert (m < 1e-2).any() and ((m > 0.1) & (m < 10)).any() and (m > 1e4).any()
    assert rep["badmass"] == 200 and abs(sum(math.fsum(x) for x in rep["mass_type"]) / math.fsum(m) - 1) < 1e-12


def _host_tree(pman):
    sq.set_densitypar(DensityResolutionEta=1.0, MaxNumNgbDeviation=0.5, DensityKernelType=1, BlackHoleNgbFactor=2.0, MinGasHsml=0.006)
    return sq.force_tree_rebuild_mask(pman, sq.GASMASK + sq.BHMASK)


@pytest.mark.parametrize("ngas,mean,expect", [(16 ** 3, 0.5, ("climb2", "climb3", "garbage", "not_in_tree")),
                                             (12, 0.5, ("root_reached", "garbage", "not_in_tree")),
                                             (16 ** 3, 1e-6, ("fallback",))])
def test_set_init_hsml_restated_equals_the_host_mirror(ngas, mean, expect):
    pman, _, _ = st.hsml_set(ngas)
    tree = _host_tree(pman)
    n = pman.NumPart
    c = collections.Counter()
    des = sq.GetNumNgb()
    assert des == 4.0 / 3 * math.pi * 8
    hsml, nodes, badmom, badhsml = st.set_init_hsml(tree.Nodes_base, tree.firstnode, st.tree_father(tree, n), pman.Base, mean, des, pman.BoxSize, c)
    before = pman.Base["Hsml"].copy()
    sq.set_init_hsml(tree, mean, pman)
    assert np.array_equal(pman.Base["Hsml"], hsml)
    for b in expect:
        assert c[b] > 0, (b, c)
    P = pman.Base
    skipped = ((P["Type"] != 0) & (P["Type"] != 5)) | ((P["Flags"] & 1) != 0)
    assert np.array_equal(hsml[skipped], before[skipped]) and np.all(nodes[skipped] == -1)
    assert nodes[n - 1] == n - 1 and hsml[n - 1] == mean        # the swallowed black hole keeps no = i
    if "fallback" in expect:
        live = ~skipped
        assert np.all(hsml[live] == mean) and c["fallback"] == live.sum() - 1
    # the root is 1.001 BoxSize long: the reference's "Bad tree moments" holds for every particle that ends on it, and for no other
    assert badmom == np.sum(nodes == tree.firstnode) >= c["root_reached"]
    if "root_reached" in expect:
        assert badmom > 0
    assert badhsml == 0
