"""The all-pairs restatement of the black-hole walks (bh_brute.py) alone, on the inputs of bh_cases.py: every branch of the two pair
lambdas and the two postprocess kernels of csrc/sph_bh.hip is taken by some case, no floating-point decision comes within 1e-9 of
its threshold (so a device that adds in another order has to take the same decisions), no two hole IDs are consecutive and the
compare-and-swap marks come out the same in five orders, and oracle/blackhole.py (f64, queue order) agrees with the long-double
reference under the bars of bh_cases.compare: integers, flags and IDs equal, floats within 1e-11 of the element's own scale.

Branches no case takes, with the reason no input can take them:
  bh_no_record / fb_bh_no_record (`ob < 0`: a type-5 neighbour without a slot record): the records are collected from every type-5
      particle that is no garbage, and garbage never reaches the pair code (flag_leaf; treewalk.c:943-949).
  fb_other_type (`type != 0` after the hole branch of the feedback pair): only gas and holes pass flag_leaf.
The kernels' task loop with more tasks than workgroups needs more than 262 144 holes in a queue: not reachable at test sizes.

Measured here.  Branches taken over all cases:
  accretion pair: mass_negative 96, wind_decoupled 204, self 2025, bh_no_record 0, bh_far 13854, bh_near_no_neighbour 6,
      encounter 615, flag_reposition 559, flag_nobound 28, bound_yes 14, bound_no 14, gas_outside_kernel 2432, gas_inside_kernel
      84090, seed_off 1985, seed_below 26, seed_reached 14, pacc_no_excess 5536, pacc_no_density 68, pacc_positive 78486,
      draw_hit 6640, draw_miss 77450, mgas_on 2265, mgas_off 81825, no_neighbour 5, timebin_active 340, timebin_inactive 231,
      timebin_bin0 2, timebin_ti0 28, cas_first_larger_id 280, cas_first_inactive 103, cas_replace 10, cas_keep 208, mark_first
      4316, mark_raised 928, mark_kept 1396
  accretion post: density_positive 2022, density_zero 3, norm_positive 2021, norm_zero 1, edd_capped 1074, edd_free 915, edd_off
      36, drag0 1791, drag1 122, drag2 112, ke_off 1977, ke_low_x 10, ke_low_thr 38, ke_accumulate 28, ke_high 20, eps_capped
      24, eps_free 4, ke_release 32, ke_hold 15, vdisp_zero 1
  feedback pair: fb_no_work 378, fb_self 1647, fb_wind_decoupled 135, bh_unmarked 10731, bh_marked_elsewhere 1406, bh_swallowed
      176, fb_bh_no_record 0, othermass_seed_off 164, othermass_imtrack_zero 1, othermass_mtrack 9, othermass_particle 2,
      fb_other_type 0, gas_unmarked_inside 51342, gas_unmarked_outside 1405, mintimebin_lowered 3456, mintimebin_kept 47886,
      heat 50163, heat_no_weight 1, heat_no_energy 107, heat_kinetic_channel 941, heat_zero_mass 130, eeqos_flagged 13807,
      eeqos_not 26969, eeqos_absent 9387, heat_capped 543, heat_capped_by_one 535, heat_capped_by_sum 8, heat_free 15634, kick
      711, kick_no_density 64, kick_nothing_released 166, kick_thermal_channel 50401, gas_marked_elsewhere 14775, gas_swallowed
      3741, channel_thermal 1618, channel_kinetic_hold 6, channel_kinetic_release 23
  feedback post: bhmass_grows 168, bhmass_kept 1479, bhmass_only 1, mass_nothing 474, mtrack_grows 1, mtrack_saturates 14,
      mass_grows 1158, ke_reset 23, ke_kept 1624
Smallest margins over all cases:
  ngb_radius 1.1e-05, rmerge 2.8e-03, kernel 1.6e-05, bound 9.6e-01, draw 5.7e-05, excess 3.1e-03, seed 3.1e-02, seed_sum
  6.0e-01, eddington 1.2e-04, edd_ratio 1.3e-02, lam_x 1.8e-02, epsilon 5.0e-01, ke_thresh 4.5e-02, max_u 4.2e-08
oracle/blackhole.py against the reference, worst deviation per quantity over all cases in units of the bar (1e-11 of the scale):
  Vel 1.1e-03, Entropy 1.1e-04, Mdot 3.7e-05, Mass 1.6e-05, Mtrack 0.0e+00, KFE 1.6e-06, Drag 5.5e-05, fws 1.4e-03, bhEnt
  1.8e-03, gasvel 2.5e-03, Mgas 0.0e+00, accM 1.7e-05, accBH 0.0e+00, accmom 3.7e-05
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import bh_brute as bb  # noqa: E402
import bh_cases as bc  # noqa: E402

MARGIN = 1e-9            # the bar of test_ngbsums_brute_cpu.py: rounding of <= 2000 terms moves a sum by <= 2e-13 of its scale
UNREACHABLE = {"accretion": ("bh_no_record",), "feedback": ("fb_bh_no_record", "fb_other_type")}


def tally(name):
    _, acc, fb = bc.reference(name)
    return {k: acc.tally[k] + fb.tally[k] for k in bb.BRANCHES}


def margins(name):
    _, acc, fb = bc.reference(name)
    return {k: min(acc.margins.get(k, np.inf), fb.margins.get(k, np.inf)) for k in bb.MARGINS}


@pytest.mark.parametrize("name", bc.NAMES)
def test_oracle_matches_all_pairs(name):
    c, acc, fb = bc.reference(name)
    w = bc.compare(c, (acc, fb), bc.oracle_run(c))
    m = margins(name)
    print(bc.line(c, w, "oracle"), " margins", {k: "%.1e" % v for k, v in m.items() if np.isfinite(v)})
    for k, v in m.items():
        assert v >= MARGIN, (name, k, v)
    assert acc.marks_order_free, (name, "the compare-and-swap marks depend on the order")
    hid = np.sort(c.P["ID"][c.bh].astype(np.int64))
    assert np.all(np.diff(hid) > 1), (name, "consecutive hole IDs")


def test_every_reachable_branch_is_taken():
    total = dict.fromkeys(bb.BRANCHES, 0)
    low = dict.fromkeys(bb.MARGINS, np.inf)
    for name in bc.NAMES:
        for k, v in tally(name).items():
            total[k] += v
        for k, v in margins(name).items():
            low[k] = min(low[k], v)
    print("branches", total)
    print("margins", {k: "%.1e" % v for k, v in low.items()})
    assert all(len(v) <= 2 for v in UNREACHABLE.values())
    never = sum(UNREACHABLE.values(), ())
    for k in bb.BRANCHES:
        if k in never:
            assert total[k] == 0, (k, "is reached after all: take it off the list")
        else:
            assert total[k] > 0, k
    assert all(np.isfinite(v) for v in low.values()), low


def test_what_the_cases_are_there_for():
    """each case reaches what its docstring promises"""
    t = tally
    assert sorted(len(bc.reference(n)[0].queue) for n in ("single", "q63", "q64", "q65", "q257", "uniform")) == [1, 63, 64, 65, 257, 700]
    u = t("uniform")
    for k in ("encounter", "draw_hit", "draw_miss", "edd_capped", "edd_free", "heat", "gas_swallowed", "bh_swallowed", "gas_outside_kernel"):
        assert u[k] > 0, k
    lo = t("lonely")
    assert lo["no_neighbour"] >= 3 and lo["norm_zero"] >= 1 and lo["density_zero"] >= 1
    c, acc, _ = bc.reference("tiny")
    assert c.P["Hsml"][c.queue].min() < 1.01e-5 * bc.BOX and t("tiny")["gas_inside_kernel"] >= 6
    tiny_q = np.flatnonzero(c.P["Hsml"][c.queue] < 2e-4)
    assert len(tiny_q) == 6 and np.all(acc.work["BH_FeedbackWeightSum"][c.P["PI"][c.queue[tiny_q]]] > 0)
    w = t("wrap")
    assert w["encounter"] >= 16 and w["bh_swallowed"] >= 6 and w["cas_replace"] + w["cas_keep"] > 0
    c, acc, _ = bc.reference("wrap")
    far = [np.abs(c.P["Pos"][row] - c.P["Pos"][c.queue[tq]]).max() > bc.BOX / 2 for row, tq, kind, _ in acc.marks]
    assert sum(far) >= 12                                   # marks that reach across a face by construction
    c, acc, _ = bc.reference("lanes")
    assert acc.nngb.max() > 400 and acc.nngb[1::2].max() < 20 and acc.nngb[0::2].min() > 256
    o = t("other_hsml")
    assert o["bh_near_no_neighbour"] >= 6 and o["encounter"] >= 6 and o["gas_outside_kernel"] > 0
    c, acc, _ = bc.reference("other_hsml")
    only_theirs = [(row, tq) for row, tq, kind, _ in acc.marks if kind == 0 and
                   np.linalg.norm(bc.min_image(c.P["Pos"][row] - c.P["Pos"][c.queue[tq]], bc.BOX)) > c.P["Hsml"][c.queue[tq]]]
    assert len(only_theirs) >= 1                            # a hole marked by one whose own Hsml does not reach it
    ch = t("chain")
    for k in ("cas_first_larger_id", "cas_first_inactive", "cas_replace", "cas_keep", "mark_raised", "mark_kept", "bh_marked_elsewhere", "fb_no_work",
              "gas_marked_elsewhere", "timebin_inactive", "timebin_active"):
        assert ch[k] > 0, k
    c, acc, fb = bc.reference("chain")
    marked_by_marked = [b for b in np.flatnonzero(acc.work["BH_SwallowID"]) if
                        acc.work["BH_SwallowID"][c.P["PI"][np.flatnonzero(c.P["ID"] == acc.work["BH_SwallowID"][b] - 1)[0]]] != 0]
    assert len(marked_by_marked) >= 1
    b = t("bound")
    assert b["bound_yes"] > 0 and b["bound_no"] > 0 and b["timebin_bin0"] > 0 and b["flag_reposition"] == 0 and b["flag_nobound"] == 0
    assert t("bound_off")["flag_nobound"] > 0 and t("bound_off")["bound_yes"] + t("bound_off")["bound_no"] == 0
    assert t("bound_ti0")["flag_reposition"] > 0 and t("bound_ti0")["timebin_ti0"] > 0
    s = t("seed")
    for k in ("seed_below", "seed_reached", "mtrack_grows", "mtrack_saturates", "mass_grows", "othermass_mtrack", "othermass_particle",
              "othermass_imtrack_zero", "bhmass_only", "pacc_no_excess"):
        assert s[k] > 0, k
    assert t("eddington_drag0")["drag0"] > 0 and t("eddington_drag1")["drag1"] > 0 and t("eddington_drag2")["drag2"] > 0
    for n in ("eddington_drag0", "eddington_drag1", "eddington_drag2"):
        assert t(n)["edd_capped"] > 0 and t(n)["edd_free"] > 0, n
    assert t("eddington_off")["edd_off"] == 36 and t("eddington_off")["edd_capped"] == 0
    k_ = t("kinetic")
    for k in ("ke_low_x", "ke_low_thr", "ke_accumulate", "ke_high", "eps_capped", "eps_free", "ke_release", "ke_hold", "vdisp_zero", "kick",
              "kick_no_density", "kick_nothing_released", "heat_kinetic_channel", "heat", "ke_reset", "ke_kept", "channel_thermal"):
        assert k_[k] > 0, k
    c, acc, _ = bc.reference("kinetic")
    assert set(np.unique(acc.work["KEflag"][c.P["PI"][c.queue]])) == {0, 1, 2}
    th = t("thermal")
    for k in ("heat_capped_by_one", "heat_capped_by_sum", "heat_free", "heat_no_energy", "heat_zero_mass", "heat_no_weight", "eeqos_flagged",
              "eeqos_not"):
        assert th[k] > 0, k
    assert t("decoupled")["wind_decoupled"] > 0 and t("decoupled")["fb_wind_decoupled"] > 0 and t("decoupled")["eeqos_absent"] > 0
    f = t("flagged")
    assert f["mass_negative"] > 0 and f["bh_swallowed"] >= 1
    c, acc, fb = bc.reference("flagged")
    again = [r for r in fb.effects if r[2] == 0 and r[0] in c.swallowed]
    assert len(again) >= 1                                  # a hole swallowed before the call, still in the tree, is swallowed again
    for kt in (1, 2, 4):
        assert bc.reference("k%d" % kt)[0].prm.DensityKernelType == kt and t("k%d" % kt)["heat"] > 0


def test_the_flags_matter():
    """the flagged case's results differ measurably from the same input with nothing flagged"""
    c, acc, fb = bc.reference("flagged")
    assert len(c.garbage) > 0 and len(c.retype) > 0 and len(c.negmass) > 0 and len(c.swallowed) == 6
    pacc, pfb = bc.brute_run(c, flagged=False)
    slots = c.P["PI"][c.queue]
    a, b = acc.work["BH_FeedbackWeightSum"][slots], pacc.work["BH_FeedbackWeightSum"][slots]
    differs = np.abs(a - b) > 1e-6 * np.abs(b)
    print("holes whose weight sum changes: %d of %d" % (differs.sum(), len(differs)))
    assert differs.mean() > 0.25
    assert fb.counts[0] != pfb.counts[0] and not np.array_equal(fb.S["Entropy"], pfb.S["Entropy"])
    # the walk does not look at the Swallowed flag (treewalk.c:943-949): passing the swallowed holes over gives other marks and counts
    dacc, dfb = bc.brute_run(c, drop_swallowed=True)
    assert not np.array_equal(acc.work["BH_SwallowID"], dacc.work["BH_SwallowID"])
    assert not np.array_equal(acc.B["encounter"], dacc.B["encounter"])
    assert not np.array_equal(fb.B["CountProgs"], dfb.B["CountProgs"]) and fb.counts[1] > dfb.counts[1]


def test_the_bars_bite():
    """compare() refuses one Mdot off by 1e-10 of its scale, one gas entropy off by 1e-10, one mark off by one, one flag bit and
    one minTimeBin off by one"""
    c, acc, fb = bc.reference("q63")
    slots = c.P["PI"][c.queue]

    def refused(change):
        got = bc.oracle_run(c)
        bc.compare(c, (acc, fb), got)
        change(got)
        with pytest.raises(AssertionError):
            bc.compare(c, (acc, fb), got)

    b = slots[np.argmax(acc.B["Mdot"][slots] > 0)]

    def mdot(got):
        got["acc"]["B"]["Mdot"][b] += 1e-10 * acc.scale["B.Mdot"][b]
    s = int(np.argmax(fb.scale["S.Entropy"] > 0))

    def entropy(got):
        got["fb"]["S"]["Entropy"][s] += 1e-10 * fb.scale["S.Entropy"][s]

    def mark(got):
        k = int(np.flatnonzero(got["acc"]["work"]["SPH_SwallowID"])[0])
        got["acc"]["work"]["SPH_SwallowID"][k] += 1

    def flag(got):
        got["fb"]["P"]["Flags"][c.gas[3]] ^= 8

    def mintimebin(got):
        got["fb"]["B"]["minTimeBin"][slots[0]] += 1
    assert acc.B["Mdot"][b] > 0 and fb.scale["S.Entropy"][s] > 0
    for change in (mdot, entropy, mark, flag, mintimebin):
        refused(change)
