"""The device's shq_stellar_density, shq_wind_veldisp, shq_bh_veldisp and shq_bh_dynfric through the C ABI with the host tree, on the
inputs of ngbsums_cases.py, against the all-pairs sums of ngbsums_brute.py: no tree, no oracle, so a cull error the oracle and
the device share would show.  test_ngbsums_brute_cpu.py shows on the CPU that the cases take every reachable branch of the radius
loops and exits and that no decision comes within 1e-9 of its threshold.

Bars (ngbsums_cases.compare).  Integers equal: stats.niterations, stats.ntargets, NumDM.  Hsml, and hsml_max_tried against the largest
radius of the reference: 1e-9 relative (the radii go through pow()); hsml_max_tried never below an Hsml written.  StarVolumeSPH, the
first and second moments, the friction sums: per target within 1e-11 of the sum of the absolute values of the terms.  3 VDisp^2:
within 1e-11 of V2sum / num (the variance is a difference; the bulk-velocity cases cancel five digits).  MinPot, MinPotPos,
MinPotVel, updated: the same bits.  Rows of particles in no queue, of swallowed holes and of the exits that write nothing keep the
sentinel put there.  After each case the same context reruns a small case of ANOTHER operator and gets the bits of its first run
(the operators share their leaf-order scratch arrays).

Measured on an MI355X (passes; worst deviation of each quantity in units of its bar's scale):

    stellar_uniform700   passes  5  Hsml 5.6e-15  StarVolumeSPH 6.8e-16  hsml_max_tried 0.0e+00
    stellar_uniform1     passes  2  Hsml 0.0e+00  StarVolumeSPH 1.8e-16  hsml_max_tried 2.2e-16
    stellar_lattice      passes  3  Hsml 7.3e-15  StarVolumeSPH 4.2e-16  hsml_max_tried 1.1e-16
    stellar_clump        passes  7  Hsml 1.1e-15  StarVolumeSPH 7.1e-16  hsml_max_tried 1.1e-16
    stellar_sparse60     passes  5  Hsml 8.2e-15  StarVolumeSPH 6.4e-16  hsml_max_tried 0.0e+00
    stellar_tiny         passes  3  Hsml 1.8e-15  StarVolumeSPH 3.9e-16  hsml_max_tried 0.0e+00
    stellar_wrap         passes  3  Hsml 4.4e-16  StarVolumeSPH 4.1e-16  hsml_max_tried 2.2e-16
    stellar_lanes        passes  4  Hsml 5.3e-15  StarVolumeSPH 7.7e-16  hsml_max_tried 0.0e+00
    stellar_flagged      passes  5  Hsml 4.4e-15  StarVolumeSPH 7.2e-16  hsml_max_tried 0.0e+00
    stellar_narrow       passes  6  Hsml 1.8e-15  StarVolumeSPH 5.1e-16  hsml_max_tried 0.0e+00
    stellar_k1_w0        passes  4  Hsml 4.7e-15  StarVolumeSPH 5.5e-16  hsml_max_tried 1.1e-16
    stellar_k1_w1        passes  4  Hsml 2.1e-15  StarVolumeSPH 8.6e-16  hsml_max_tried 0.0e+00
    stellar_k2_w0        passes  5  Hsml 2.7e-15  StarVolumeSPH 7.0e-16  hsml_max_tried 0.0e+00
    stellar_k2_w1        passes  5  Hsml 4.0e-15  StarVolumeSPH 2.3e-15  hsml_max_tried 0.0e+00
    stellar_k4_w0        passes  5  Hsml 1.8e-15  StarVolumeSPH 7.8e-16  hsml_max_tried 2.2e-16
    stellar_k4_w1        passes  4  Hsml 2.9e-15  StarVolumeSPH 1.9e-15  hsml_max_tried 1.1e-16
    wind_uniform700      passes 10  VDisp 1.1e-15
    wind_uniform1        passes  2  VDisp 5.8e-17
    wind_lattice         passes 12  VDisp 9.1e-16
    wind_clump           passes  8  VDisp 7.4e-16
    wind_sparse60        passes 10  VDisp 1.1e-15
    wind_tiny            passes  8  VDisp 9.2e-16
    wind_wrap            passes  8  VDisp 7.6e-16
    wind_lanes           passes  9  VDisp 1.2e-15
    wind_flagged         passes  9  VDisp 9.5e-16
    wind_few30           passes 12  VDisp 9.0e-16
    wind_still           passes  8  VDisp 0.0e+00
    bhvd_uniform257      VDisp 1.6e-15  V1sumDM 8.6e-16  V2sumDM 1.5e-15
    bhvd_still           VDisp 0.0e+00  V1sumDM 0.0e+00  V2sumDM 0.0e+00
    bhvd_uniform1        VDisp 1.4e-15  V1sumDM 2.3e-16  V2sumDM 1.0e-15
    bhvd_wrap            VDisp 1.3e-15  V1sumDM 0.0e+00  V2sumDM 1.3e-15
    bhvd_lanes           VDisp 3.4e-15  V1sumDM 1.6e-15  V2sumDM 3.2e-15
    bhvd_flagged         VDisp 2.0e-15  V1sumDM 1.1e-15  V2sumDM 1.3e-15
    dynfric_k1_m0        MinPot, MinPotPos, MinPotVel, updated: equal bits
    dynfric_k1_m1        Density 7.6e-16  Vel 7.1e-16  RmsVel 9.9e-16
    dynfric_k1_m2        Density 6.0e-16  Vel 5.2e-16  RmsVel 1.6e-15
    dynfric_k2_m0        MinPot, MinPotPos, MinPotVel, updated: equal bits
    dynfric_k2_m1        Density 9.7e-16  Vel 1.4e-15  RmsVel 1.1e-15
    dynfric_k2_m2        Density 9.1e-16  Vel 1.3e-15  RmsVel 1.3e-15
    dynfric_k4_m0        MinPot, MinPotPos, MinPotVel, updated: equal bits
    dynfric_k4_m1        Density 9.3e-16  Vel 2.1e-15  RmsVel 1.2e-15
    dynfric_k4_m2        Density 9.1e-16  Vel 6.7e-16  RmsVel 1.6e-15
    dynfric_uniform1     Density 1.2e-16  Vel 3.2e-16  RmsVel 2.2e-16
    dynfric_wrap         Density 6.3e-16  Vel 1.0e-15  RmsVel 1.1e-15
    dynfric_lanes        Density 1.6e-15  Vel 1.0e-15  RmsVel 3.3e-15
    dynfric_flagged_m0   MinPot, MinPotPos, MinPotVel, updated: equal bits
    dynfric_flagged_m1   Density 1.0e-15  Vel 7.4e-16  RmsVel 1.5e-15
    dynfric_flagged_m2   Density 1.8e-15  Vel 9.0e-16  RmsVel 1.7e-15

The MinPot arrays of every friction case are the same bits, and every rerun of a small case gave the bits of its first run.
"""
import ctypes as C

import numpy as np
import pytest

import shenqi_amd as sq
from shenqi_amd import capi
import ngbsums_cases as nc

pytestmark = pytest.mark.gpu

BOX = nc.BOX
SENT = -7.25                 # what the output rows hold before a call
ALL = [n for op in nc.OPS for n in nc.NAMES[op]]
NEXT_OP = {"stellar": "wind", "wind": "bhvd", "bhvd": "dynfric", "dynfric": "stellar"}
_first_bits = {}


def run_device(ctx, c):
    """one call of the case's operator; returns (results in the layout of ngbsums_cases.compare, every array the call could write)"""
    pman, SphP, kf = nc.state(c)
    P = pman.Base
    tree = sq.force_tree_rebuild_mask(pman, nc.tree_mask(c))
    nc.apply_changes(c, P)
    pv, tv = pman.view(), tree.view()
    slots = c.slot[c.queue]
    stats = capi.SphStats()
    before = P.copy()
    if c.op == "stellar":
        sv = capi.sph_view(SphP)
        sp = capi.StellarParams(BOX, nc.des_num_ngb(c), c.dev, c.weighting, c.kernel)
        vol = np.full(c.nslots, SENT)
        capi.check(capi.hip.shq_stellar_density(ctx.h, C.byref(tv), C.byref(pv), C.byref(sv), capi.ptr(c.queue), len(c.queue), C.byref(sp),
                                                capi.ptr(vol), C.byref(stats)))
        got = dict(Hsml=P["Hsml"][c.queue].copy(), StarVolumeSPH=vol[slots], niterations=stats.niterations,
                   hsml_max_tried=stats.hsml_max_tried)
        raw = dict(vol=vol, Hsml=P["Hsml"].copy())
        rest = np.setdiff1d(np.arange(c.n), c.queue)
        assert np.array_equal(P["Hsml"][rest], before["Hsml"][rest])                       # gas, idle stars
        assert np.all(vol[np.setdiff1d(np.arange(c.nslots), slots)] == SENT)
    elif c.op == "wind":
        vd = np.full(c.nslots, SENT)
        capi.check(capi.hip.shq_wind_veldisp(ctx.h, C.byref(tv), C.byref(pv), capi.ptr(c.queue), len(c.queue), C.byref(kf), c.Time, c.hubble,
                                             capi.ptr(vd), C.byref(stats)))
        v = vd[slots]
        got = dict(VDisp=np.where(v == SENT, np.nan, v), niterations=stats.niterations)
        raw = dict(vd=vd)
        assert np.all(vd[np.setdiff1d(np.arange(c.nslots), slots)] == SENT)
    elif c.op == "bhvd":
        num, v1, v2, vd = np.full(c.nslots, SENT), np.full((c.nslots, 3), SENT), np.full(c.nslots, SENT), np.full(c.nslots, SENT)
        capi.check(capi.hip.shq_bh_veldisp(ctx.h, C.byref(tv), C.byref(pv), capi.ptr(c.active), len(c.active), C.byref(kf), capi.ptr(num),
                                           capi.ptr(v1), capi.ptr(v2), capi.ptr(vd)))
        v = vd[slots]
        got = dict(NumDM=num[slots], V1sumDM=v1[slots], V2sumDM=v2[slots], VDisp=np.where(v == SENT, np.nan, v))
        raw = dict(num=num, v1=v1, v2=v2, vd=vd)
        idle = np.setdiff1d(np.arange(c.nslots), slots)                                    # idle and swallowed holes
        assert len(idle) >= 5 and all(np.all(a[idle] == SENT) for a in (num, v1, v2, vd))
    else:
        mp, mpp, mpv = nc.initial_minpot(c)
        upd = np.zeros(c.nslots, dtype=np.int32)
        dens, dvel, drms = np.full(c.nslots, SENT), np.full((c.nslots, 3), SENT), np.full(c.nslots, SENT)
        out = capi.BhDynFricOut(capi.ptr(mp), capi.ptr(mpp), capi.ptr(mpv), capi.ptr(upd), capi.ptr(dens), capi.ptr(dvel), capi.ptr(drms))
        capi.check(capi.hip.shq_bh_dynfric(ctx.h, C.byref(tv), C.byref(pv), capi.ptr(c.queue), len(c.queue), C.byref(kf), c.method, c.kernel,
                                           nc.tree_mask(c), C.byref(out)))
        got = dict(MinPot=mp, MinPotPos=mpp, MinPotVel=mpv, updated=upd, Density=dens[slots], Vel=dvel[slots], RmsVel=drms[slots])
        raw = dict(mp=mp, mpp=mpp, mpv=mpv, upd=upd, dens=dens, dvel=dvel, drms=drms)
        idle = np.setdiff1d(np.arange(c.nslots), slots) if c.method > 0 else np.arange(c.nslots)
        assert all(np.all(a[idle] == SENT) for a in (dens, dvel, drms))
    if c.op in ("stellar", "wind"):
        assert stats.ntargets == len(c.queue)
    keep = [k for k in P.dtype.names if k != "Hsml"]
    assert all(np.array_equal(P[k], before[k]) for k in keep)                              # nothing but Hsml is written back
    return got, raw


def rerun_small(ctx, op):
    """a small case of `op` on the same context: the bits of its first run in this session"""
    c, _ = nc.reference(nc.SMALL[op])
    _, raw = run_device(ctx, c)
    first = _first_bits.setdefault(op, raw)
    for k in raw:
        assert np.array_equal(raw[k], first[k], equal_nan=True), (op, k, "differs from its first run on this context")


@pytest.mark.parametrize("name", ALL)
def test_device_matches_all_pairs(ctx, name):
    c, ref = nc.reference(name)
    got, raw = run_device(ctx, c)
    w = nc.compare(c, ref, got)
    print(nc.line(c, ref, w, "device"))
    if c.op in ("wind", "bhvd"):
        # the exits: rows of targets whose variance is not positive, or that have no neighbour, keep the sentinel
        quiet = ~np.isfinite(ref["VDisp"])
        assert np.all(raw["vd"][c.slot[c.queue[quiet]]] == SENT)
        if "still" in name:
            assert quiet.all()
    if name == "bhvd_uniform":
        assert np.all(got["NumDM"][np.isin(c.queue, c.lonely)] == 0) and np.all(raw["vd"][c.slot[c.lonely]] == SENT)
        assert np.all(raw["num"][c.slot[c.swallowed]] == SENT)
    if c.op == "dynfric" and c.method > 0 and hasattr(c, "lonely"):
        lone = np.isin(c.queue, c.lonely)
        assert np.all(got["Density"][lone] == 0) and np.all(got["Vel"][lone] == 0) and np.all(got["RmsVel"][lone] == 0)
    if name.endswith("_lanes"):
        assert ref["npairs_first"].max() > 256                 # NL_CAP: the lane list was flushed in the middle of the walk
    rerun_small(ctx, NEXT_OP[c.op])


def test_few_neighbours_end_at_the_box(ctx):
    """30 dark-matter particles, 40 wanted: every bracket collapses at R = Box after 12 passes, the call succeeds and writes the
    dispersion of all 30"""
    c, ref = nc.reference("wind_few30")
    got, _ = run_device(ctx, c)
    assert np.all(ref["NumDM"] < 40) and np.all(ref["Right"] == BOX) and np.all(np.isfinite(got["VDisp"]))
    assert got["niterations"] == ref["niterations"]
