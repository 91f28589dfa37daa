"""The all-pairs restatements of ngbsums_brute.py alone, on the inputs of ngbsums_cases.py: every branch of the radius loops and of the
exits is taken by some case, no decision comes within 1e-9 of its threshold (so a device that adds in another order has to take the
same decisions), and the oracle's tree walks (orc.stellar_density, orc.wind_veldisp, orc.bh_veldisp, orc.bh_dynfric on the host tree)
agree with the all-pairs sums: pass counts as integers, the rest to the bars of ngbsums_cases.compare.  The oracle's wind loop
returns no neighbour counts; its DMRadius, which ngb_narrow_down forms from the counts of every pass, is compared instead, and
the counts of bh_veldisp are compared as integers.

Branches no case takes, with the reason no input can take them:
  stellar L0_noslope: Left == 0 after the update means Ngb[0] >= 33, and the kernel-weighted count grows strictly with the radius once
      it is positive, so the slope between the first two radii is positive (or maxcmpte == 1 and the slope is Ngb[0] / r0^3 > 0).
  stellar clamp_L: the radius of the count nearest to 33 lies below Left only where two counts tie (the first of equal distances is
      kept), and kernel-weighted counts tie only at zero; ten empty radii in a closed bracket need more than 33 weighted neighbours
      to enter within its last eleventh in volume, i.e. beyond 0.969 R, where the cubic spline gives 21.3 (1 - r / R)^3 each:
      over 50 000 gas particles within 3 % in distance, more than a case holds (the other kernels vanish faster at the edge).
  wind open_cap: with integer counts and 40 wanted the extrapolated volume hs^3 + (40 - n) / slope is at most (5 + 39) / 6 of the open
      bracket's, below the 64 hs^3 of the cap.

Measured here.  The oracle agrees with the all-pairs sums to 1.2e-14 in Hsml and DMRadius and to 3.5e-15 of its scale in every sum;
the pass counts are equal (2 - 12).  Branches taken over all cases:
  stellar  closed 2897, open_extrap 1031, open_cap 101, open_noslope 262, clamp_R 2, L0_first 211, L0_slope 2, band 1799, collapse 63,
           redo 2429
  wind     closed 3325, open_extrap 1243, open_noslope 942, clamp_R 234, L0_first 240, L0_slope 7, L0_noslope 4, clamp_L 264,
           band 1432, collapse 42, collapse_box 20, redo 4016, vd_positive 1429, vd_not_positive 65
  bhvd     written 496, no_dm 16, vd_not_positive 64
  dynfric  minpot_lowered 428, minpot_kept 546, dens_positive 680, dens_zero 34
Smallest margins: stellar radius 1.6e-7, count 3.6e-5, close 1.0e-8, band 4.2e-4, collapse 3.3e-3; wind radius 1.7e-8 (the lattice),
collapse 1.7e-2; bhvd radius 3.6e-6; dynfric radius 6.6e-7, potential 6.6e-4; R is never nearer than 1 % to 0.99 Box.
"""
import numpy as np
import pytest

import orc
import ngbsums_brute as nb
import ngbsums_cases as nc

MARGIN = 1e-9            # the bar of test_density_brute_cpu.py: rounding of <= 2000 terms moves a sum by <= 2e-13 of its scale
UNREACHABLE = {"stellar": ("L0_noslope", "clamp_L"), "wind": ("open_cap",), "bhvd": (), "dynfric": ()}
BRANCHES = {"stellar": nb.STELLAR_BRANCHES, "wind": nb.WIND_BRANCHES, "bhvd": nb.BHVD_BRANCHES, "dynfric": nb.DYNFRIC_BRANCHES}
ALL = [n for op in nc.OPS for n in nc.NAMES[op]]


def oracle_run(c):
    """the oracle's tree walk of a case on the host tree, in the layout of ngbsums_cases.compare"""
    import shenqi_amd as sq
    pman, SphP, kf = nc.state(c)
    P = pman.Base
    tree = sq.force_tree_rebuild_mask(pman, nc.tree_mask(c))
    nc.apply_changes(c, P)
    st = orc.SphState(P, SphP)
    nodes, first = tree.Nodes_base, tree.firstnode
    if c.op == "stellar":
        rc, vol, niter, _ = orc.stellar_density(nodes, first, st, c.queue, nc.BOX, nc.des_num_ngb(c), c.dev, c.weighting, c.kernel)
        assert rc == 0
        return dict(Hsml=st.hsml[c.queue], StarVolumeSPH=vol[c.queue], niterations=niter)
    if c.op == "wind":
        rc, vd, dm, niter = orc.wind_veldisp(nodes, first, st, c.queue, nc.BOX, kf, c.Time, c.hubble)
        assert rc == 0
        return dict(VDisp=vd, DMRadius=dm, niterations=niter)
    if c.op == "bhvd":
        out, vd = orc.bh_veldisp(nodes, first, st, c.queue, nc.BOX, kf)
        return dict(NumDM=out[:, 0], V1sumDM=out[:, 1:4], V2sumDM=out[:, 4], VDisp=vd)
    raw = orc.bh_dynfric(nodes, first, st, P["Potential"], c.queue, nc.BOX, kf, c.method, c.kernel, nc.tree_mask(c))
    mp, mpp, mpv = nc.initial_minpot(c)
    upd = np.zeros(c.nslots, dtype=np.int32)
    s = c.slot[c.queue]
    better = mp[s] > raw[:, 0]
    mp[s[better]], mpp[s[better]], mpv[s[better]], upd[s[better]] = raw[better, 0], raw[better, 1:4], raw[better, 4:7], 1
    got = dict(MinPot=mp, MinPotPos=mpp, MinPotVel=mpv, updated=upd)
    if c.method > 0:
        d = raw[:, 7]
        pz = d > 0
        dd = np.where(pz, d, 1.0)
        got.update(Density=d, Vel=np.where(pz[:, None], raw[:, 8:11] / dd[:, None], raw[:, 8:11]),
                   RmsVel=np.where(pz, np.sqrt(raw[:, 11] / dd), raw[:, 11]))
    return got


@pytest.mark.parametrize("name", ALL)
def test_oracle_matches_all_pairs(name):
    c, ref = nc.reference(name)
    w = nc.compare(c, ref, oracle_run(c))
    taken = {k: v for k, v in ref["tally"].items() if v}
    print(nc.line(c, ref, w, "oracle"), " margins", {k: "%.1e" % v for k, v in ref["margins"].items()}, taken)
    for k, v in ref["margins"].items():
        assert v >= MARGIN, (name, k, v)


@pytest.mark.parametrize("op", nc.OPS)
def test_every_reachable_branch_is_taken(op):
    total = dict.fromkeys(BRANCHES[op], 0)
    for name in nc.NAMES[op]:
        for k, v in nc.reference(name)[1]["tally"].items():
            total[k] += v
    print(op, total)
    assert len(UNREACHABLE[op]) <= 2
    for k in BRANCHES[op]:
        if k in UNREACHABLE[op]:
            assert total[k] == 0, (k, "is reached after all: take it off the list")
        else:
            assert total[k] > 0, (op, k)


def test_what_the_cases_are_there_for():
    """each case reaches what its docstring promises"""
    t = lambda name: nc.reference(name)[1]["tally"]                                 # noqa: E731
    for k in ("open_extrap", "open_noslope", "L0_first", "L0_slope", "clamp_L", "band"):
        assert t("wind_uniform")[k] > 0, k
    assert t("wind_lattice")["collapse"] > 0
    assert t("wind_sparse")["clamp_R"] > 0 and t("stellar_sparse")["clamp_R"] > 0
    c, ref = nc.reference("wind_few30")
    assert ref["tally"]["collapse_box"] == c.nt and np.all(ref["Right"] == nc.BOX) and np.all(ref["NumDM"] < 40)
    assert sum(t(n)["open_cap"] for n in nc.NAMES["stellar"]) > 0
    assert t("stellar_narrow")["collapse"] == 63 and t("stellar_narrow")["band"] == 0
    assert t("wind_clump")["L0_noslope"] > 0
    for op in ("stellar", "wind"):
        c, ref = nc.reference(op + "_tiny")
        final = ref["Hsml"] if op == "stellar" else ref["DMRadius"]
        assert c.hsml[c.queue].max() < 2e-5 * nc.BOX and final.min() < 1e-3
    # lane lists: more accepted neighbours than a lane's list holds (NL_CAP = 256), beside lanes with a handful
    for op in nc.OPS:
        n = nc.reference(op + "_lanes")[1]["npairs_first"]
        assert n.max() > 380 and (op in ("bhvd", "dynfric") or n.min() < 20), (op, n.min(), n.max())
    assert t("wind_still")["vd_not_positive"] == 65 and t("wind_still")["vd_positive"] == 0
    assert t("bhvd_still")["vd_not_positive"] == 63
    assert t("bhvd_uniform")["no_dm"] == 10 and t("bhvd_uniform")["written"] > 200
    for k in (1, 2, 4):
        for m in (1, 2):
            assert t("dynfric_k%d_m%d" % (k, m))["dens_zero"] >= 3 and t("dynfric_k%d_m%d" % (k, m))["dens_positive"] > 50
    assert sorted(len(nc.reference(n)[0].queue) for n in ("stellar_single", "stellar_lattice", "stellar_clump", "stellar_sparse",
                                                          "stellar_uniform")) == [1, 63, 65, 257, 700]


@pytest.mark.parametrize("name", [n for n in ALL if "flagged" in n])
def test_the_flags_matter(name):
    """the sums with the marked and retyped particles passed over differ measurably from the sums with them"""
    c, ref = nc.reference(name)
    assert len(c.garbage) > 0 and len(c.retype) > 0
    plain = nc.brute_run(c, flagged=False)
    key = {"stellar": "StarVolumeSPH", "wind": "VDisp", "bhvd": "V2sumDM", "dynfric": "raw_minpot"}[c.op]
    differs = ref[key] != plain[key]
    print(name, "targets whose %s changes: %d of %d" % (key, differs.sum(), len(differs)))
    # the lowest potential changes only where the marked particle was the lowest of its neighbourhood: the case marks it for 30 holes
    assert differs.sum() >= 10 if c.op == "dynfric" else differs.mean() > 0.25
    if c.op == "dynfric" and c.method > 0:
        assert np.mean(np.abs(ref["dens"] - plain["dens"]) > 1e-6 * plain["dens"]) > 0.25


def test_the_bars_bite():
    """compare() refuses a radius off by 1e-8, a sum off by 1e-10 of its scale, a count off by one and a MinPot of other bits"""
    def refused(name, key, change):
        c, ref = nc.reference(name)
        got = oracle_run(c)
        nc.compare(c, ref, got)
        got[key] = change(got[key].copy())
        with pytest.raises(AssertionError):
            nc.compare(c, ref, got)

    def scaled(f):
        def change(a):
            a[0] *= f
            return a
        return change

    refused("stellar_single", "Hsml", scaled(1 + 1e-8))
    refused("stellar_single", "StarVolumeSPH", scaled(1 + 1e-10))
    refused("wind_single", "VDisp", scaled(1 + 1e-10))
    refused("bhvd_single", "NumDM", lambda a: a + 1)
    refused("bhvd_single", "V2sumDM", scaled(1 + 1e-10))
    refused("dynfric_single", "Density", scaled(1 + 1e-10))
    refused("dynfric_k1_m1", "MinPot", scaled(1 + 1e-15))
