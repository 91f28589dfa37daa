"""The device's black-hole accretion and feedback walks (csrc/sph_bh.hip) on the inputs of bh_cases.py against the all-pairs
long-double reference of bh_brute.py, in both routes: one-shot (shq_bh_accretion, shq_bh_feedback through the C ABI on the host tree)
and in parts (shq_bh_accretion_marks / _marks_resolve / _feedback_effects / _effects_apply on one rank with every row local).  No
tree and no oracle in the yardstick, so an error the oracle and the device share would show.  test_bh_brute_cpu.py shows on the CPU
that the cases take every reachable branch and that no decision comes within 1e-9 of its threshold.

Bars (bh_cases.compare), the same for both routes and for the oracle.  Equal: both mark arrays, encounter, KEflag, CountProgs,
minTimeBin, SwallowID, SwallowTime, every flag byte, ReverseLink, the two swallow counts, Type, and every field no call writes.
Floats: per element within 1e-11 of the element's own scale from the reference; an element nothing wrote (rows no hole of the queue
reaches, sentinels included) keeps its bits.  The float particle mass: the float rounding of the reference's value or its
neighbour.  The two emitted lists equal the reference's record by record, heat and kick values within the bar of their scale.
Between the routes, what does not depend on an arrival order is the same bits: marks, flags, counts, every hole-side sum and
slot field, the holes' Vel and Mass.  After each case the same context reruns a small case of a neighbour-sum operator and gets the
bits of its first run (the walks share s_nlist2, flag_leaf and the leaf-order arrays).
The kernels' task loop with more tasks than workgroups needs more than 262 144 holes in a queue: not reachable at test sizes.

Measured on an MI355X (worst deviation of each quantity in units of its bar):

    uniform          one-shot Vel 3.6e-05  Entropy 6.6e-05  Mdot 3.1e-05  Mass 1.6e-05  fws 6.9e-05  bhEnt 8.4e-05  gasvel 8.7e-05  accmom 3.7e-05
    uniform          parts    Vel 3.6e-05  Entropy 6.6e-05  Mdot 3.1e-05  Mass 1.6e-05  fws 6.9e-05  bhEnt 8.4e-05  gasvel 8.7e-05  accmom 3.7e-05  heat 1.7e-02
    single           one-shot Vel 4.1e-06  Entropy 2.2e-05  Mdot 5.5e-06  fws 3.9e-05  bhEnt 2.0e-05  gasvel 2.6e-05  accmom 4.6e-06
    single           parts    Vel 4.1e-06  Entropy 2.2e-05  Mdot 5.5e-06  fws 3.9e-05  bhEnt 2.0e-05  gasvel 2.6e-05  accmom 4.6e-06  heat 1.6e-03
    q63              one-shot Vel 2.7e-05  Entropy 4.4e-05  Mdot 2.8e-05  fws 7.6e-05  bhEnt 6.3e-05  gasvel 4.6e-05  accmom 3.6e-05
    q63              parts    Vel 2.7e-05  Entropy 6.3e-05  Mdot 2.8e-05  fws 7.6e-05  bhEnt 6.3e-05  gasvel 4.6e-05  accmom 3.6e-05  heat 6.8e-02
    q64              one-shot Vel 2.2e-05  Entropy 6.1e-05  Mdot 1.6e-05  fws 3.9e-05  bhEnt 5.9e-05  gasvel 4.9e-05  accmom 2.1e-05
    q64              parts    Vel 2.2e-05  Entropy 6.1e-05  Mdot 1.6e-05  fws 3.9e-05  bhEnt 5.9e-05  gasvel 4.9e-05  accmom 2.1e-05  heat 1.8e-02
    q65              one-shot Vel 2.9e-05  Entropy 4.3e-05  Mdot 2.1e-05  fws 6.6e-05  bhEnt 6.7e-05  gasvel 5.0e-05  accmom 2.1e-05
    q65              parts    Vel 2.9e-05  Entropy 5.7e-05  Mdot 2.1e-05  fws 6.6e-05  bhEnt 6.7e-05  gasvel 5.0e-05  accmom 2.1e-05  heat 8.7e-03
    q257             one-shot Vel 3.1e-05  Entropy 7.8e-05  Mdot 3.2e-05  fws 6.8e-05  bhEnt 5.9e-05  gasvel 4.6e-05  accmom 2.5e-05
    q257             parts    Vel 3.1e-05  Entropy 1.1e-04  Mdot 3.2e-05  fws 6.8e-05  bhEnt 5.9e-05  gasvel 4.6e-05  accmom 2.5e-05  heat 5.0e-02
    lonely           one-shot Vel 1.6e-05  Entropy 2.9e-05  Mdot 1.5e-05  Drag 1.6e-05  fws 3.6e-05  bhEnt 4.7e-05  gasvel 2.9e-05  accmom 2.0e-05
    lonely           parts    Vel 1.6e-05  Entropy 4.4e-05  Mdot 1.5e-05  Drag 1.6e-05  fws 3.6e-05  bhEnt 4.7e-05  gasvel 2.9e-05  accmom 2.0e-05  heat 1.1e-03
    tiny             one-shot Vel 2.0e-05  Entropy 4.4e-05  Mdot 4.6e-05  fws 4.9e-05  bhEnt 5.5e-05  gasvel 4.8e-05  accmom 1.7e-05
    tiny             parts    Vel 2.0e-05  Entropy 4.4e-05  Mdot 4.6e-05  fws 4.9e-05  bhEnt 5.5e-05  gasvel 4.8e-05  accmom 1.7e-05  heat 1.2e-02
    wrap             one-shot Vel 1.8e-05  Entropy 6.5e-05  Mdot 2.1e-05  fws 4.9e-05  bhEnt 5.7e-05  gasvel 2.8e-05  accmom 1.6e-05
    wrap             parts    Vel 1.8e-05  Entropy 5.5e-05  Mdot 2.1e-05  fws 4.9e-05  bhEnt 5.7e-05  gasvel 2.8e-05  accmom 1.6e-05  heat 9.3e-03
    lanes            one-shot Vel 2.9e-05  Entropy 8.6e-05  Mdot 2.6e-05  Drag 5.5e-05  fws 1.4e-03  bhEnt 1.8e-03  gasvel 2.5e-03  accmom 2.2e-05
    lanes            parts    Vel 2.9e-05  Entropy 9.1e-05  Mdot 2.6e-05  Drag 5.5e-05  fws 1.4e-03  bhEnt 1.8e-03  gasvel 2.5e-03  accmom 2.2e-05  heat 1.3e-01
    other_hsml       one-shot Vel 1.9e-05  Entropy 4.4e-05  Mdot 1.5e-05  fws 5.7e-04  bhEnt 5.5e-04  gasvel 6.1e-04  accmom 2.0e-05
    other_hsml       parts    Vel 1.9e-05  Entropy 4.4e-05  Mdot 1.5e-05  fws 5.7e-04  bhEnt 5.5e-04  gasvel 6.1e-04  accmom 2.0e-05  heat 1.1e-02
    chain            one-shot Vel 3.5e-05  Entropy 4.2e-05  Mdot 1.6e-05  Mass 1.2e-05  fws 4.4e-05  bhEnt 8.4e-05  gasvel 4.8e-05  accmom 2.2e-05
    chain            parts    Vel 3.5e-05  Entropy 4.2e-05  Mdot 1.6e-05  Mass 1.2e-05  fws 4.4e-05  bhEnt 8.4e-05  gasvel 4.8e-05  accmom 2.2e-05  heat 7.3e-03
    bound            one-shot Vel 3.0e-05  Entropy 4.4e-05  Mdot 1.9e-05  fws 5.5e-05  bhEnt 6.1e-05  gasvel 3.5e-05  accmom 1.8e-05
    bound            parts    Vel 3.0e-05  Entropy 4.4e-05  Mdot 1.9e-05  fws 5.5e-05  bhEnt 6.1e-05  gasvel 3.5e-05  accmom 1.8e-05  heat 3.9e-02
    bound_off        one-shot Vel 1.3e-05  Entropy 4.3e-05  Mdot 1.9e-05  fws 5.5e-05  bhEnt 6.1e-05  gasvel 3.5e-05  accmom 1.8e-05
    bound_off        parts    Vel 1.3e-05  Entropy 3.9e-05  Mdot 1.9e-05  fws 5.5e-05  bhEnt 6.1e-05  gasvel 3.5e-05  accmom 1.8e-05  heat 3.9e-02
    bound_ti0        one-shot Vel 2.0e-05  Entropy 4.3e-05  Mdot 1.9e-05  fws 5.5e-05  bhEnt 6.1e-05  gasvel 3.5e-05  accmom 1.8e-05
    bound_ti0        parts    Vel 2.0e-05  Entropy 4.1e-05  Mdot 1.9e-05  fws 5.5e-05  bhEnt 6.1e-05  gasvel 3.5e-05  accmom 1.8e-05  heat 3.9e-02
    seed             one-shot Vel 1.5e-05  Entropy 3.3e-05  Mdot 2.7e-05  Drag 2.8e-05  fws 3.9e-05  bhEnt 5.0e-05  gasvel 3.2e-05  accmom 1.7e-05
    seed             parts    Vel 1.5e-05  Entropy 3.3e-05  Mdot 2.7e-05  Drag 2.8e-05  fws 3.9e-05  bhEnt 5.0e-05  gasvel 3.2e-05  accmom 1.7e-05  heat 5.5e-03
    eddington_drag0  one-shot Vel 2.5e-05  Entropy 3.9e-05  Mdot 1.8e-05  fws 3.8e-05  bhEnt 6.3e-05  gasvel 4.2e-05  accmom 2.1e-05
    eddington_drag0  parts    Vel 2.5e-05  Entropy 4.0e-05  Mdot 1.8e-05  fws 3.8e-05  bhEnt 6.3e-05  gasvel 4.2e-05  accmom 2.1e-05  heat 4.9e-03
    eddington_drag1  one-shot Vel 2.1e-05  Entropy 4.3e-05  Mdot 2.9e-05  Drag 2.7e-05  fws 5.2e-05  bhEnt 6.8e-05  gasvel 3.2e-05  accmom 1.9e-05
    eddington_drag1  parts    Vel 2.1e-05  Entropy 4.4e-05  Mdot 2.9e-05  Drag 2.7e-05  fws 5.2e-05  bhEnt 6.8e-05  gasvel 3.2e-05  accmom 1.9e-05  heat 8.5e-03
    eddington_drag2  one-shot Vel 2.3e-05  Entropy 3.5e-05  Mdot 2.6e-05  Drag 3.8e-05  fws 5.3e-05  bhEnt 5.5e-05  gasvel 4.7e-05  accmom 2.0e-05
    eddington_drag2  parts    Vel 2.3e-05  Entropy 3.9e-05  Mdot 2.6e-05  Drag 3.8e-05  fws 5.3e-05  bhEnt 5.5e-05  gasvel 4.7e-05  accmom 2.0e-05  heat 8.7e-02
    eddington_off    one-shot Vel 2.1e-05  Entropy 3.9e-05  Mdot 2.1e-05  fws 6.9e-05  bhEnt 7.9e-05  gasvel 5.3e-05  accmom 2.2e-05
    eddington_off    parts    Vel 2.1e-05  Entropy 4.2e-05  Mdot 2.1e-05  fws 6.9e-05  bhEnt 7.9e-05  gasvel 5.3e-05  accmom 2.2e-05  heat 5.8e-03
    kinetic          one-shot Vel 1.1e-03  Entropy 2.4e-05  Mdot 2.7e-05  KFE 1.1e-05  fws 7.0e-05  bhEnt 6.2e-05  gasvel 7.1e-05  accmom 2.1e-05
    kinetic          parts    Vel 1.1e-03  Entropy 2.4e-05  Mdot 2.7e-05  KFE 1.1e-05  fws 7.0e-05  bhEnt 6.2e-05  gasvel 7.1e-05  accmom 2.1e-05  heat 7.2e-03  kick 3.0e-02
    thermal          one-shot Vel 3.6e-05  Entropy 6.6e-05  Mdot 2.0e-05  fws 7.3e-05  bhEnt 7.9e-05  gasvel 4.1e-05  accmom 2.0e-05
    thermal          parts    Vel 3.6e-05  Entropy 5.7e-05  Mdot 2.0e-05  fws 7.3e-05  bhEnt 7.9e-05  gasvel 4.1e-05  accmom 2.0e-05  heat 5.0e-02
    decoupled        one-shot Vel 3.1e-05  Entropy 2.5e-05  Mdot 2.5e-05  fws 6.4e-05  bhEnt 5.0e-05  gasvel 4.6e-05  accmom 2.0e-05
    decoupled        parts    Vel 3.1e-05  Entropy 2.5e-05  Mdot 2.5e-05  fws 6.4e-05  bhEnt 5.0e-05  gasvel 4.6e-05  accmom 2.0e-05  heat 3.7e-02
    flagged          one-shot Vel 2.3e-05  Entropy 4.4e-05  Mdot 1.9e-05  fws 4.0e-05  bhEnt 5.6e-05  gasvel 3.7e-05  accmom 2.5e-05
    flagged          parts    Vel 2.3e-05  Entropy 4.3e-05  Mdot 1.9e-05  fws 4.0e-05  bhEnt 5.6e-05  gasvel 3.7e-05  accmom 2.5e-05  heat 6.6e-03
    k1               one-shot Vel 2.0e-05  Entropy 5.2e-05  Mdot 2.0e-05  fws 5.4e-05  bhEnt 5.8e-05  gasvel 4.7e-05  accmom 3.0e-05
    k1               parts    Vel 2.0e-05  Entropy 6.2e-05  Mdot 2.0e-05  fws 5.4e-05  bhEnt 5.8e-05  gasvel 4.7e-05  accmom 3.0e-05  heat 3.3e-02
    k2               one-shot Vel 2.2e-05  Entropy 4.2e-05  Mdot 2.2e-05  fws 5.1e-05  bhEnt 6.9e-05  gasvel 5.3e-05  accmom 2.4e-05
    k2               parts    Vel 2.2e-05  Entropy 4.4e-05  Mdot 2.2e-05  fws 5.1e-05  bhEnt 6.9e-05  gasvel 5.3e-05  accmom 2.4e-05  heat 2.0e-02
    k4               one-shot Vel 3.3e-05  Entropy 4.2e-05  Mdot 1.9e-05  fws 6.1e-05  bhEnt 5.8e-05  gasvel 4.6e-05  accmom 2.7e-05
    k4               parts    Vel 3.3e-05  Entropy 4.3e-05  Mdot 1.9e-05  fws 6.1e-05  bhEnt 5.8e-05  gasvel 4.6e-05  accmom 2.7e-05  heat 9.2e-02

Quantities that are the reference's bits in every element (Mtrack, MgasEnc, the accreted masses, ...) are left out of a line.  In every
case the two routes gave the same bits in everything no arrival order enters, and every rerun of a neighbour-sum case gave the bits
of its first run.  Before the host code of shq_bh_feedback and shq_bh_effects_apply was mended, the `flagged` case failed in both
routes on encounter, SwallowID, SwallowTime and the count of swallowed holes of the holes that carried the Swallowed flag already.
"""
import ctypes as C

import numpy as np
import pytest

import shenqi_amd as sq
from shenqi_amd import capi
from shenqi_amd import dist as sd
import bh_cases as bc
import test_gpu_ngbsums_brute as tn

pytestmark = pytest.mark.gpu

OTHER = ("stellar", "wind", "bhvd", "dynfric")
_device_error = []           # a case that ended in a device error: no later case starts anything on the card


def _work(w):
    return capi.BhWork(*[w[k].ctypes.data for k, _ in capi.BhWork._fields_])


def run_oneshot(ctx, c):
    """shq_bh_accretion then shq_bh_feedback on the tree as it was built, the particles as they are now"""
    pman, S, B, kf = bc.state(c)
    P = pman.Base
    tree = sq.force_tree_rebuild_mask(pman, sq.GASMASK + sq.BHMASK)
    sq.force_tree_update_hmax(tree, pman)
    bc.apply_changes(c, P)
    ids = np.ascontiguousarray(P["ID"])
    w = bc.work_arrays(c)
    cw, cp = _work(w), bc.params(c)
    pv, tv, sv, bv = pman.view(), tree.view(), capi.sph_view(S), capi.bh_slot_view(B)
    capi.check(capi.hip.shq_bh_accretion(ctx.h, C.byref(tv), C.byref(pv), C.byref(sv), C.byref(bv), capi.ptr(ids), capi.ptr(c.queue), len(c.queue), C.byref(kf),
                                         C.byref(cp), c.Ti, capi.ptr(c.rnd), len(c.rnd), C.byref(cw)))
    acc = bc.snapshot(P, S, B, w, None)
    ns, nb = C.c_int64(), C.c_int64()
    capi.check(capi.hip.shq_bh_feedback(ctx.h, C.byref(tv), C.byref(pv), C.byref(sv), C.byref(bv), capi.ptr(ids), capi.ptr(c.queue), len(c.queue), C.byref(kf),
                                        C.byref(cp), c.maxpart, capi.ptr(c.rnd), len(c.rnd), None if c.eeqos is None else capi.ptr(c.eeqos), C.byref(cw),
                                        C.byref(ns), C.byref(nb)))
    return dict(acc=acc, fb=bc.snapshot(P, S, B, w, (ns.value, nb.value)))


class CaseOps(sd.GpuBhOps):
    """GpuBhOps walking the tree of the case as it was BUILT, with the particles as they are now"""

    def __init__(self, ctx, c):
        super().__init__(ctx, bc.BOX)
        self.c = c

    def _tree(self, Pall):
        if self._walkset is None or self._walkset[0] is not Pall:
            pman = sd.records_pman(sq, self.L, self.c.P)
            tree = sq.force_tree_rebuild_mask(pman, sq.GASMASK + sq.BHMASK)
            sq.force_tree_update_hmax(tree, pman)
            self._walkset = (Pall, pman, tree)
        pman, tree = self._walkset[1:]
        pman.Base[:] = Pall
        return pman, tree


def run_parts(ctx, c):
    """the four parts on one rank, every row local; returns (snapshots, marks, effects)"""
    ops = CaseOps(ctx, c)
    P, S, B, kf = c.P.copy(), c.S.copy(), c.B.copy(), bc.kick_factors(c)
    bc.apply_changes(c, P)
    w = bc.work_arrays(c)
    none = np.zeros(0, dtype=np.int32)
    marks, counts = ops.accretion_marks(P, S, B, len(P), c.queue, none, none, 1, 0, 0, kf, c.prm, c.Ti, c.rnd, w)
    assert counts[0] == len(marks)
    ops.marks_resolve(P, marks, c.Ti, len(S), len(B), w)
    acc = bc.snapshot(P, S, B, w, None)
    effects, counts = ops.feedback_effects(P, S, B, len(P), c.queue, none, none, 1, 0, 0, kf, c.prm, c.rnd, w)
    assert counts[0] == len(effects)
    swallowed = ops.effects_apply(P, S, B, effects, c.prm, c.maxpart, c.rnd, c.eeqos, w)
    return dict(acc=acc, fb=bc.snapshot(P, S, B, w, tuple(swallowed))), marks, effects


def same_bits_across_routes(c, a, b):
    """what no arrival order enters: everything but the gas entropy and the gas velocities"""
    holes = c.P["Type"] == 5
    for stage in ("acc", "fb"):
        x, y = a[stage], b[stage]
        assert x["counts"] == y["counts"], (c.name, stage)
        for rec in ("P", "S", "B"):
            for k in x[rec].dtype.names:                      # field by field: the records' padding is not initialised
                if (rec, k) in (("S", "Entropy"), ("P", "Vel")):
                    continue
                assert np.array_equal(x[rec][k], y[rec][k], equal_nan=True), (c.name, stage, rec, k)
        assert np.array_equal(x["P"]["Vel"][holes], y["P"]["Vel"][holes]), (c.name, stage, "Vel of the holes")
        for k in x["work"]:
            assert np.array_equal(x["work"][k], y["work"][k]), (c.name, stage, k)


@pytest.mark.parametrize("name", bc.NAMES)
def test_device_matches_all_pairs(ctx, name):
    assert not _device_error, "case %s ended in a device error: nothing more is started" % _device_error[0]
    c, acc, fb = bc.reference(name)
    try:
        one = run_oneshot(ctx, c)
        parts, marks, effects = run_parts(ctx, c)
    except sq.ShqError:
        _device_error.append(name)
        raise
    errors, lines = [], []

    def check(who, f):
        try:
            w = f()
            if w is not None:
                lines.append(bc.line(c, w, who))
        except AssertionError as e:                          # every check of a case is made before the case fails
            errors.append("%s: %s" % (who, str(e)[:600]))

    def parts_checks():
        w = bc.compare(c, (acc, fb), parts)
        w.update(bc.compare_records(c, (acc, fb), marks, effects))
        return w
    check("one-shot", lambda: bc.compare(c, (acc, fb), one))
    check("parts", parts_checks)
    check("routes", lambda: same_bits_across_routes(c, one, parts))
    print("\n".join(lines))
    if name == "lanes":
        assert acc.nngb.max() > 256                          # NL_CAP: a lane's list was flushed in the middle of the walk
    try:
        tn.rerun_small(ctx, OTHER[bc.NAMES.index(name) % 4])
    except sq.ShqError:
        _device_error.append(name)
        raise
    assert not errors, errors
