"""GPU parity tests of metal_return's treewalk (shq_metal_return, csrc/sph_winds.hip) against the restatement of
libgadget/metal_return.cpp:573-667 in oracle/metal_return.py: stars in queue order, the reference's float / double arithmetic, so the
comparison is exact up to the last bit of the kernel weight.  No reference fixture exists for the walk (parity unpinned); mass and metal conservation are checked beside it."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import shenqi_amd as sq
from shenqi_amd import capi
import common as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import metal_return as omr  # noqa: E402

pytestmark = pytest.mark.gpu


def setup(seed, ngrid=14, nstar=300, nq=120, hscale=1.0):
    rng = np.random.default_rng(seed)
    ngas = ngrid**3
    sp = cm.BOX / ngrid
    gas = np.mod(cm.grid_positions(ngrid) + rng.normal(size=(ngas, 3)) * 0.3 * sp, cm.BOX)
    stars = rng.random((nstar, 3)) * cm.BOX
    stars[:40] = gas[rng.integers(0, ngas, 40)] + rng.normal(size=(40, 3)) * 0.2 * sp      # crowded: several stars feed the same gas
    stars[40] = gas[17]                                                                   # r2 = 0: that particle is skipped
    pos = np.mod(np.concatenate([gas, stars, rng.random((100, 3)) * cm.BOX]), cm.BOX)
    n = len(pos)
    types = np.concatenate([np.zeros(ngas, np.uint8), np.full(nstar, 4, np.uint8), np.ones(100, np.uint8)])
    perm = rng.permutation(n)
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n)
    pos, types = pos[perm], types[perm]
    pman = sq.PartManager(n, cm.BOX)
    P = pman.Base
    P["Pos"], P["Type"] = pos, types
    P["Mass"] = rng.uniform(0.8, 1.2, n).astype(np.float32)
    P["ID"] = np.arange(n) + 1
    P["Hsml"] = sp * rng.uniform(1.0, 2.0, n) * hscale
    isgas, isstar = types == 0, types == 4
    P["PI"][isgas] = rng.permutation(ngas)
    P["PI"][isstar] = rng.permutation(nstar)
    gi = np.flatnonzero(isgas)
    P["Flags"][gi[:6]] |= 1
    P["Mass"][gi[10:40]] = 3.9                               # close to MaxGasMass = 4: some of these refuse the return
    S = np.zeros(ngas, dtype=capi.SPH_DTYPE)
    S["Density"] = rng.uniform(0.5, 2.0, ngas) * ngas / cm.BOX**3
    S["Metallicity"] = rng.uniform(0, 0.02, ngas)
    S["Metals"] = rng.uniform(0, 2e-3, (ngas, 9)).astype(np.float32)
    queue = np.ascontiguousarray(rng.permutation(inv[ngas + np.arange(nq)]).astype(np.int32))
    starvol = rng.uniform(20, 60, nq) * (cm.BOX**3 / ngas)
    massgen = rng.uniform(0.0, 0.3, nq)
    massgen[:3] = 0
    metalgen = massgen * rng.uniform(0.01, 0.05, nq)
    species = (metalgen[:, None] * rng.dirichlet(np.ones(9), nq)).copy()
    return pman, S, queue, starvol, massgen, metalgen, species


@pytest.mark.parametrize("sphw,kt,hscale", [(1, 1, 1.0), (0, 1, 1.0), (1, 2, 1.0), (1, 4, 1.0), (0, 1, 2.4)])
def test_metal_return_equals_serial_loop(ctx, sphw, kt, hscale):
    pman, S, queue, starvol, massgen, metalgen, species = setup(5 + kt + sphw, hscale=hscale)
    if hscale > 1:
        starvol = starvol * hscale**3                         # more neighbours share the same return
    P = pman.Base
    tree = sq.force_tree_rebuild_mask(pman, sq.GASMASK)
    oP, oS = P.copy(), S.copy()
    omass = omr.metal_return(oP, oS, queue, starvol, massgen, metalgen, species, 4.0, sphw, kt, cm.BOX)
    P0, S0 = P.copy(), S.copy()
    f = capi.SPH_DTYPE.fields
    gv = capi.GasMetalView(S.ctypes.data, S.dtype.itemsize, len(S), f["Density"][1], f["Metallicity"][1], f["Metals"][1], 9, 0)
    pv, tv = pman.view(), tree.view()
    mret = np.full(len(queue), -1.0)
    npairs = C.c_int64()
    capi.check(capi.hip.shq_metal_return(ctx.h, C.byref(tv), C.byref(pv), C.byref(gv), capi.ptr(queue), len(queue), capi.ptr(starvol), capi.ptr(massgen),
                                         capi.ptr(metalgen), capi.ptr(species), 4.0, sphw, kt, capi.ptr(mret), C.byref(npairs)))
    assert npairs.value > 20 * len(queue) // 4
    # same order, same float / double arithmetic; the kernel weight is products on the device and pow() in the reference (and the
    # restatement): a last-bit difference there shows as one ulp in a few hundred of the doubles and, rarely, of a float
    same = lambda a, b, tol: np.abs(a.astype(np.float64) - b.astype(np.float64)).max() <= tol * np.abs(b).max()      # noqa: E731
    assert same(P["Mass"], oP["Mass"], 1.2e-7) and same(S["Density"], oS["Density"], 1e-15)
    assert same(S["Metallicity"], oS["Metallicity"], 1e-15) and same(S["Metals"], oS["Metals"], 1.2e-7)
    assert (P["Mass"] != oP["Mass"]).sum() <= 2 and np.array_equal(S["Metallicity"] != S0["Metallicity"], oS["Metallicity"] != S0["Metallicity"])
    if not sphw:                                             # no kernel weight: nothing to differ in
        assert np.array_equal(P["Mass"], oP["Mass"]) and np.array_equal(S["Density"], oS["Density"])
        assert np.array_equal(S["Metallicity"], oS["Metallicity"]) and np.array_equal(S["Metals"], oS["Metals"])
    assert np.abs(mret - omass).max() <= 1e-14 * omass.max()
    # conservation: what the stars gave away arrived in the gas (float masses: to float precision), metals likewise
    gas = (P["Type"] == 0) & ((P["Flags"] & 1) == 0)
    gained = (P["Mass"][gas].astype(np.float64) - P0["Mass"][gas].astype(np.float64)).sum()
    assert abs(gained - mret.sum()) < 2e-6 * P0["Mass"][gas].sum() and mret.sum() > 1
    pi = P["PI"][gas]
    z1 = (S["Metallicity"][pi] * P["Mass"][gas]).sum()
    z0 = (S0["Metallicity"][pi] * P0["Mass"][gas]).sum()
    assert z1 > z0 and (mret >= 0).all() and (mret[:0] == 0).all()
    # volume = Mass / Density is what the reference keeps fixed
    vol0 = P0["Mass"][gas] / S0["Density"][pi]
    vol1 = P["Mass"][gas] / S["Density"][pi]
    assert np.abs(vol1 / vol0 - 1).max() < 5e-7
    heavy = gas & (P0["Mass"] == np.float32(3.9))
    assert (P["Mass"][heavy] <= 4.0).all() and (P["Mass"][heavy] > P0["Mass"][heavy]).any()
    if hscale == 1:
        assert (P["Mass"][heavy] == P0["Mass"][heavy]).any()      # some refused a return that would have lifted them over MaxGasMass
    # untouched: everything that is not gas
    assert np.array_equal(P["Mass"][~gas], P0["Mass"][~gas])


def test_many_stars_span_several_workgroups(ctx):
    """1000 stars: 16 waves in 4 workgroups of the emit kernel, ~16 000 triples through the sorts"""
    pman, S, queue, starvol, massgen, metalgen, species = setup(21, ngrid=24, nstar=1500, nq=1000)
    P = pman.Base
    tree = sq.force_tree_rebuild_mask(pman, sq.GASMASK)
    oP, oS = P.copy(), S.copy()
    omass = omr.metal_return(oP, oS, queue, starvol, massgen, metalgen, species, 4.0, 0, 1, cm.BOX)
    f = capi.SPH_DTYPE.fields
    gv = capi.GasMetalView(S.ctypes.data, S.dtype.itemsize, len(S), f["Density"][1], f["Metallicity"][1], f["Metals"][1], 9, 0)
    pv, tv = pman.view(), tree.view()
    mret = np.zeros(len(queue))
    npairs = C.c_int64()
    capi.check(capi.hip.shq_metal_return(ctx.h, C.byref(tv), C.byref(pv), C.byref(gv), capi.ptr(queue), len(queue), capi.ptr(starvol), capi.ptr(massgen),
                                         capi.ptr(metalgen), capi.ptr(species), 4.0, 0, 1, capi.ptr(mret), C.byref(npairs)))
    assert npairs.value > 10000
    assert np.array_equal(P["Mass"], oP["Mass"]) and np.array_equal(S["Density"], oS["Density"])
    assert np.array_equal(S["Metallicity"], oS["Metallicity"]) and np.array_equal(S["Metals"], oS["Metals"])
    assert np.abs(mret - omass).max() <= 1e-14 * omass.max()


def test_metal_return_errors_and_empty(ctx):
    pman, S, queue, starvol, massgen, metalgen, species = setup(9, ngrid=8, nstar=60, nq=10)
    P = pman.Base
    tree = sq.force_tree_rebuild_mask(pman, sq.GASMASK)
    f = capi.SPH_DTYPE.fields
    gv = capi.GasMetalView(S.ctypes.data, S.dtype.itemsize, len(S), f["Density"][1], f["Metallicity"][1], f["Metals"][1], 9, 0)
    pv, tv = pman.view(), tree.view()
    mret = np.zeros(len(queue))

    def call(q, sv, gview=gv):
        return capi.hip.shq_metal_return(ctx.h, C.byref(tv), C.byref(pv), C.byref(gview), capi.ptr(q), len(q), capi.ptr(sv), capi.ptr(massgen), capi.ptr(metalgen),
                                         capi.ptr(species), 4.0, 1, 1, capi.ptr(mret), None)
    sv0 = starvol.copy()
    sv0[2] = 0
    with pytest.raises(sq.ShqError):                       # "StarVolumeSPH 0 hsml ..."
        capi.check(call(queue, sv0))
    gasq = np.flatnonzero(P["Type"] == 0)[:3].astype(np.int32)
    with pytest.raises(sq.ShqError):
        capi.check(call(gasq, starvol))
    bad = capi.GasMetalView(S.ctypes.data, S.dtype.itemsize, len(S), f["Density"][1], f["Metallicity"][1], f["Metals"][1], 7, 0)
    with pytest.raises(sq.ShqError):
        capi.check(call(queue, starvol, bad))
    P0 = P.copy()
    capi.check(call(queue[:0].copy(), starvol))
    assert np.array_equal(P["Mass"], P0["Mass"])
