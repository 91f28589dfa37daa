"""The device's hydro_force() on the inputs of hydro_cases.py against the all-pairs sum of hydro_brute.py (no tree, no node hmax, no
cull: a neighbour counts because it is in the table) and against the oracle (same walk: the candidate counts agree as integers).

Synthetic cases write the outputs of density() straight into the slots and call shq_hydro_force with hand-filled HydroParams; the
converged cases run the device's density() with its Hsml loop on the inputs of sph_loop_cases.py, then force_tree_update_hmax, and
give the device's own fields to the device's hydro force, to the oracle and to the all-pairs sum alike: there the radii have just
changed by orders of magnitude, so a stale hmax or a stale leaf radius would lose neighbours.

Bars.  HydroAccel (each component) and DtEntropy, per particle: |got - ref| <= 1e-11 of the sum of the absolute values of the terms
(N terms cost <= N u of that sum, the device's pair term <= 32 u per term; N <= 32768 gives 3.7e-12).  MaxSignalVel: 1e-12 relative.
Bit-equal where stated: rows the call does not own, DensityIndependentSphOn = 0 at any DensityContrastLimit, a second run.

Host time of the all-pairs sums (test_hydro_brute_cpu.py lists it per case): at most 0.11 s each, `tiers` 2.9 s; the converged
cases sum all pairs of 512 to 1024 particles in 0.1 s.

Measured on an MI355X (the largest |deviation| / abs-sum over the targets for HydroAccel and DtEntropy and the largest relative
deviation of MaxSignalVel, against the all-pairs sum | against the oracle):

    case              all-pairs: HydroAccel DtEntropy MaxSigVel   oracle: HydroAccel DtEntropy MaxSigVel
    reach                        2.1e-15   3.1e-14   4.4e-16              2.5e-15   3.0e-14   4.4e-16
    contrast_100_1               1.4e-15   2.8e-15   3.3e-16              2.4e-15   4.2e-15   4.4e-16
    contrast_1_1                 1.7e-15   2.8e-15   3.3e-16              2.2e-15   4.2e-15   4.4e-16
    contrast_0_1                 1.4e-15   2.8e-15   3.3e-16              2.4e-15   4.2e-15   4.4e-16
    contrast_-1_1                1.8e-15   2.8e-15   3.3e-16              2.4e-15   4.2e-15   4.4e-16
    contrast_*_0                 1.7e-15   2.6e-15   4.4e-16              2.7e-15   3.9e-15   4.4e-16
    drift                        1.6e-15   4.2e-15   4.4e-16              1.5e-15   4.2e-15   4.4e-16
    drift_noevp                  1.6e-15   4.2e-15   4.4e-16              1.5e-15   4.2e-15   4.4e-16
    drift_dloga0                 1.7e-15   5.8e-15   4.4e-16              1.4e-15   3.4e-15   4.4e-16
    kernels_1_0 / _1             1.1e-15   1.5e-15   4.4e-16              1.5e-15   2.8e-15   4.4e-16
    kernels_2_0 / _1             1.3e-15   1.9e-15   4.4e-16              2.0e-15   3.8e-15   4.4e-16
    kernels_4_0 / _1             1.9e-15   2.1e-15   4.4e-16              1.3e-15   2.4e-15   4.4e-16
    coincident                   1.3e-15   4.6e-14   4.4e-16              1.5e-15   5.6e-14   4.4e-16
    winds                        1.7e-15   9.9e-15   4.4e-16              2.4e-15   9.1e-15   6.7e-16
    mixed_types                  1.0e-15   6.0e-15   4.4e-16              1.2e-15   7.4e-15   4.4e-16
    ragged1/63/65/1001           <= 1.2e-15 3.9e-15  4.4e-16              <= 2.4e-15 6.2e-15  4.4e-16
    tiers                        7.4e-15   2.5e-14   4.4e-16              6.5e-15   5.1e-14   4.4e-16
    tiny_start                   1.8e-15   2.1e-15   1.1e-15              2.3e-15   3.0e-15   1.1e-15
    huge_start                   8.6e-16   1.4e-15   3.3e-16              1.9e-15   1.9e-15   4.4e-16
    clump_floor                  8.9e-16   1.8e-15   3.3e-16              8.5e-16   2.6e-15   4.4e-16
    kernel2                      1.9e-15   3.3e-15   3.3e-16              2.3e-15   2.7e-15   3.3e-16
    kernel4                      1.1e-15   1.6e-15   2.2e-16              1.4e-15   1.6e-15   3.3e-16
    dynrange                     8.2e-16   1.7e-15   3.3e-16              1.6e-15   2.6e-15   3.3e-16
    dynrange_corner              3.7e-15   1.6e-15   1.3e-15              3.8e-15   3.3e-15   1.3e-15

The margins of the converged cases (device radii): between 2.2e-06 and 4.9e-05.  No case came within two orders of a bar.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import shenqi_amd as sq
from shenqi_amd import capi
import orc
import common as cm
import hydro_brute as hb
import hydro_cases as hc
import sph_loop_cases as sc
from test_gpu_sph_loop import run_device as run_density

pytestmark = pytest.mark.gpu

BAR, BAR_SIG = 1e-11, 1e-12
OUT = ("HydroAccel", "DtEntropy", "MaxSignalVel")


def hydro_call(ctx, pman, tree, SphP, active, hp, evp):
    """shq_hydro_force through the C ABI; results land in SphP.  Returns the SphStats."""
    pv, tv, sv = pman.view(), tree.view(), capi.sph_view(SphP)
    st = capi.SphStats()
    capi.check(capi.hip.shq_hydro_force(ctx.h, C.byref(tv), C.byref(pv), C.byref(sv), capi.ptr(active), 0 if active is None else len(active),
                                        C.byref(hp), capi.ptr(evp), C.byref(st)))
    return st


def run_device(ctx, c, **over):
    pman, SphP = hc.state(c)
    tree = hc.host_tree(pman)
    before = (pman.Base.copy(), SphP.copy())
    st = hydro_call(ctx, pman, tree, SphP, hc.active_of(c), hc.hydro_params(c, **over), hc.evp_of(c) if c.use_evp else None)
    return SimpleNamespace(pman=pman, P=pman.Base, SphP=SphP, tree=tree, before=before, stats=st)


def rows(SphP, slots):
    return {k: SphP[k][slots].copy() for k in OUT}


def compare(got, ref, scale, label, name):
    """per particle against `ref` at the bars, relative to the abs-sums of `scale`.  Returns the three worst ratios."""
    assert all(np.all(np.isfinite(got[k])) for k in OUT), (name, label)
    worst = []
    for k in OUT[:2]:
        err, sca = np.abs(got[k] - ref[k]), scale["abs_" + k]
        ok = sca > 0
        worst.append(float((err[ok] / sca[ok]).max()) if ok.any() else 0.0)
        assert np.all(err <= BAR * sca), (name, label, k, worst[-1])
    es = float(np.abs(got["MaxSignalVel"] / ref["MaxSignalVel"] - 1).max()) if len(ref["MaxSignalVel"]) else 0.0
    print("%-18s vs %-9s HydroAccel %.1e  DtEntropy %.1e  MaxSignalVel %.1e" % (name, label, worst[0], worst[1], es))
    assert es <= BAR_SIG, (name, label, es)
    return worst + [es]


def check_untouched(c, d):
    """every particle row, and every slot no gas target owns, is bit-equal to its value before the call; an owned slot changes in
    HydroAccel, DtEntropy and MaxSignalVel only"""
    P0, S0 = d.before
    assert np.array_equal(d.P, P0)
    q = hc.gas_targets(c)
    idle = np.ones(c.nslots, dtype=bool)
    idle[c.pi[q]] = False
    assert np.array_equal(d.SphP[idle], S0[idle])
    for k in d.SphP.dtype.names:
        if k not in OUT:
            assert np.array_equal(d.SphP[k], S0[k], equal_nan=True), k


def check_case(ctx, name):
    c, ref = hc.reference(name)
    d = run_device(ctx, c)
    st, onint = hc.oracle_run(c, tree=d.tree)
    q = hc.gas_targets(c)
    assert d.stats.ntargets == len(q)
    assert d.stats.ninteractions == onint
    check_untouched(c, d)
    qb = hc.brute_targets(c)
    compare(rows(d.SphP, c.pi[qb]), ref, ref, "all-pairs", name)
    # against the oracle: the targets of the all-pairs sum at the same bars (its abs-sums are the scale); where that sum covers a
    # subset only, every target at the bars of the existing oracle comparisons
    o = {"HydroAccel": st.hydroaccel[c.pi[qb]], "DtEntropy": st.dtentropy[c.pi[qb]], "MaxSignalVel": st.maxsignalvel[c.pi[qb]]}
    compare(rows(d.SphP, c.pi[qb]), o, ref, "oracle", name)
    if c.subset is not None and len(q):
        s = c.pi[q]
        a, oa = d.SphP["HydroAccel"][s], st.hydroaccel[s]
        assert np.abs(a - oa).max() < 1e-10 * np.abs(oa).max()                            # the bars of the existing oracle comparisons
        assert np.abs(d.SphP["DtEntropy"][s] - st.dtentropy[s]).max() < 1e-10 * np.abs(st.dtentropy[s]).max()
        assert np.abs(d.SphP["MaxSignalVel"][s] / st.maxsignalvel[s] - 1).max() < 1e-12
    return c, ref, d


NAMES = [n for n in hc.SYNTHETIC if not (n.startswith("contrast") and n.endswith("_0"))]      # those: test_contrast_limit_is_ignored_without_disph


@pytest.mark.parametrize("name", NAMES)
def test_device_matches_all_pairs_and_oracle(ctx, name):
    c, ref, d = check_case(ctx, name)
    q = hc.brute_targets(c)
    if name in hc.HEAVY:                                                                  # fixed assignment of candidates to threads
        d2 = run_device(ctx, c)
        for k in OUT:
            assert np.array_equal(d2.SphP[k], d.SphP[k]), k
    if name == "coincident":
        assert np.all(np.isfinite(d.SphP["HydroAccel"])) and np.all(np.isfinite(d.SphP["DtEntropy"])) and np.all(np.isfinite(d.SphP["MaxSignalVel"]))
        assert ref["counters"]["coincident"].sum() == 22
    if name == "winds":
        w = c.wind[q]
        assert np.all(d.SphP["HydroAccel"][c.pi[q][w]] == 0) and np.all(d.SphP["DtEntropy"][c.pi[q][w]] == 0)
    if name == "ragged0":
        assert d.stats.ninteractions == 0 and np.array_equal(d.SphP, d.before[1])
    if name == "drift":
        # EntVarPred = NULL: the device predicts per particle what the cache held; same numbers to rounding
        c2, _ = hc.reference("drift_noevp")
        d2 = run_device(ctx, c2)
        s = c.pi[q]
        assert np.abs(d2.SphP["HydroAccel"][s] - d.SphP["HydroAccel"][s]).max() < 1e-12 * np.abs(d.SphP["HydroAccel"][s]).max()


def test_contrast_limit_is_ignored_without_disph(ctx):
    """DensityIndependentSphOn = 0 at DensityContrastLimit 100, 1 and -1: against the all-pairs sum, and the same bits thrice"""
    outs = []
    for name in ("contrast_100_0", "contrast_1_0", "contrast_-1_0"):
        c, ref, d = check_case(ctx, name)
        outs.append(d.SphP.copy())
    for o in outs[1:]:
        assert np.array_equal(o, outs[0])


def test_contrast_branches_differ(ctx):
    """with DensityIndependentSphOn = 1 the clamp (1.0) and the switched-off grad-h term (-1) change the device's numbers, and a
    limit no ratio reaches (100) gives the bits of no limit at all (0)"""
    out = {}
    for lim in (100.0, 1.0, 0.0, -1.0):
        c, _ = hc.reference("contrast_%g_1" % lim)
        out[lim] = run_device(ctx, c).SphP["HydroAccel"].copy()
    assert np.array_equal(out[0.0], out[100.0])
    for lim in (1.0, -1.0):
        assert np.abs(out[lim] - out[100.0]).max() > 1e-3 * np.abs(out[100.0]).max()


def test_drifted_target_is_refused(ctx):
    """a target in a bin with a non-zero drift factor: the reference's query takes its densities un-drifted, the walk reads the
    drifted record, so shq_hydro_force refuses the call with an argument error and writes nothing"""
    c, _ = hc.reference("drift")
    bad = hc.variant(c, "drift_bad", active=np.concatenate([c.active[:5], np.flatnonzero(c.bin_hydro > 2)[:1].astype(np.int32)]))
    pman, SphP = hc.state(bad)
    tree = hc.host_tree(pman)
    S0 = SphP.copy()
    with pytest.raises(sq.ShqError, match="drift"):
        hydro_call(ctx, pman, tree, SphP, bad.active, hc.hydro_params(bad), hc.evp_of(bad))
    assert np.array_equal(SphP, S0)
    # the same list with that particle's drift factor zero is served, and the next legal call works as before
    ok = hc.variant(bad, "drift_ok", drifts=np.zeros(hc.NBINS))
    hydro_call(ctx, pman, tree, SphP, ok.active, hc.hydro_params(ok), hc.evp_of(ok))
    assert not np.array_equal(SphP, S0)


@pytest.mark.parametrize("name", hc.CONVERGED)
def test_converged_state_against_all_pairs(ctx, name):
    """density() with its Hsml loop on the device, force_tree_update_hmax, then hydro_force from the device's own fields"""
    c0, dref = sc.reference(name)
    d = run_density(ctx, c0)
    assert np.abs(d.P["Hsml"] / dref["Hsml"] - 1).max() < 1e-12
    sq.force_tree_update_hmax(d.tree, d.pman)
    P, SphP = d.P, d.SphP
    c = SimpleNamespace(box=sc.BOX, kernel=c0.kernel, DISPH=1, contrast=100.0, visc=0.75, atime=0.1, hubble=cm.HUBBLE, kf=None, drifts=None,
                        WindSpeed=0.0, WindFreeTravelDensThresh=0.0)
    hp = cm.hydro_params(kernel=c0.kernel)
    sph = {k: SphP[k].copy() for k in hb.SPH_FIELDS}
    hsml = P["Hsml"].copy()
    q = np.arange(c0.n)
    ref = hb.hydro(c0.pos, c0.type, c0.mass, hsml, c0.vel, np.zeros((c0.n, 3)), np.zeros((c0.n, 3)), P["TimeBinHydro"], P["TimeBinGravity"],
                   sph, d.evp, c, q)
    print("%-18s pairs %d..%d  margin %.2e  Hsml %.2e..%.2e" % (name, ref["npairs"].min(), ref["npairs"].max(), ref["margin"], hsml.min(), hsml.max()))
    assert ref["margin"] >= 1e-12
    st = orc.SphState(P, SphP, d.BhP)
    onint = orc.hydro(d.tree.Nodes_base, d.tree.firstnode, st, hp, d.evp)
    S0 = SphP.copy()
    gs = hydro_call(ctx, d.pman, d.tree, SphP, None, hp, d.evp)
    assert gs.ninteractions == onint and gs.ntargets == c0.n
    for k in SphP.dtype.names:
        if k not in OUT:
            assert np.array_equal(SphP[k], S0[k], equal_nan=True), k
    compare(rows(SphP, q), ref, ref, "all-pairs", name)
    compare(rows(SphP, q), {"HydroAccel": st.hydroaccel, "DtEntropy": st.dtentropy, "MaxSignalVel": st.maxsignalvel}, ref, "oracle", name)
