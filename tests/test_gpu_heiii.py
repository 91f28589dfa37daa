"""Helium reionisation on the device (shq_heiii_reionization: turn_on_quasars, cooling_qso_lightup.cpp:489-596) against the numpy
restatement (heiii_restated.py) fed the catalogue shq_fof leaves on the device: flag bytes bit for bit, Entropy to 1e-14, the FdHelium
lines and the result exactly.  Sizes: one bubble, a stop inside a batch, three or more batches, the flash, negative radii on the
host-built gas tree, 2 x 64^3.  Then two calls in a row on the context's copies, determinism and bad input."""
import ctypes as C

import numpy as np
import pytest

import shenqi_amd as sq
from shenqi_amd import capi
import heiii_restated as hr

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE = 1, 4
BOX = 20000.0


def _particles(N, nhalo, seed=11):
    """N^3 dark matter (half of it in nhalo compact halos) and N^3 gas next to it; some gas is garbage, some converted to Type 5,
    some already ionised; other flag bits (Swallowed, BHHeated, Generation) set here and there"""
    rng = np.random.default_rng(seed)
    n = N ** 3
    sep = BOX / N
    centres = rng.uniform(0, BOX, (nhalo, 3))
    nin = n // 2
    h = rng.integers(0, nhalo, nin)
    dm = np.concatenate([centres[h] + rng.normal(0, 0.12 * sep, (nin, 3)), rng.uniform(0, BOX, (n - nin, 3))])
    gas = dm + rng.normal(0, 0.05 * sep, dm.shape)
    pos = np.mod(np.concatenate([dm, gas]), BOX)
    types = np.concatenate([np.ones(n, np.uint8), np.zeros(n, np.uint8)])
    perm = rng.permutation(2 * n)
    pos, types = pos[perm], types[perm]
    gas_idx = np.flatnonzero(types == 0)
    conv = rng.choice(gas_idx, max(n // 200, 2), replace=False)
    types[conv] = 5
    pman = sq.PartManager(2 * n, BOX)
    P = pman.Base
    P["Pos"], P["Type"], P["Mass"] = pos, types, np.where(types == 0, 0.2, 1.0).astype(np.float32)
    P["ID"] = rng.permutation(2 * n).astype(np.uint64) + 1
    P["Hsml"] = sep
    P["PI"][gas_idx] = np.arange(len(gas_idx))
    P["PI"][conv] = 0
    flags = (rng.integers(0, 16, 2 * n) << 4).astype(np.uint8)          # Generation
    flags |= np.where(rng.random(2 * n) < 0.1, 8, 0).astype(np.uint8)  # BHHeated
    live_gas = np.flatnonzero(types == 0)
    flags[rng.choice(live_gas, max(n // 100, 2), replace=False)] |= 1  # garbage gas
    flags[rng.choice(live_gas, max(n // 50, 2), replace=False)] |= 4   # already HeIII
    flags[conv[:1]] |= 2                                                # a swallowed hole
    P["Flags"] = flags
    S = np.zeros(len(gas_idx), dtype=capi.SPH_DTYPE)
    S["Density"] = rng.uniform(0.5, 50.0, len(S))
    S["Entropy"] = rng.uniform(1.0, 10.0, len(S))
    return pman, S, int(len(gas_idx))


def _fof(ctx, pman, S, N):
    pv, sv = pman.view(), capi.sph_view(S)
    capi.check(capi.hip.shq_set_inputs_current(ctx.h, 0))
    capi.check(capi.hip.shq_particles_upload(ctx.h, C.byref(pv)))
    sq.dynamics_upload(ctx, pman)
    capi.check(capi.hip.shq_sph_state_upload(ctx.h, C.byref(pv), C.byref(sv)))
    fp = capi.FofParams(BOX, 0.2 * BOX / N, 2, 1 + 16 + 32, 8, 0)
    ng = C.c_int64()
    ids = np.ascontiguousarray(pman.Base["ID"])
    capi.check(capi.hip.shq_fof(ctx.h, C.byref(fp), capi.ptr(ids), None, None, C.byref(ng)))
    groups = np.zeros(ng.value, dtype=capi.FOF_GROUP_DTYPE)
    capi.check(capi.hip.shq_fof_groups_download(ctx.h, capi.ptr(groups), len(groups)))
    return groups


def _params(ngas, **kw):
    p = dict(BoxSize=BOX, atime=0.25, qso_candidate_min_mass=0.0, qso_candidate_max_mass=1e30, mean_bubble=2000.0, var_bubble=0.0,
             heIIIreion_finish_frac=0.995, desired_ion_frac=0.9, qso_inst_heating=2e-12, uu_in_cgs=1e10, OmegaBaryon=0.045,
             HubbleParam=0.7, CurrentParticleOffset=(1234.5, -777.25, 20001.0), n_gas_tot=ngas)
    p.update(kw)
    return p


def _struct(p):
    s = capi.HeiiiParams()
    for k, v in p.items():
        if k == "CurrentParticleOffset":
            for d in range(3):
                s.CurrentParticleOffset[d] = v[d]
        else:
            setattr(s, k, v)
    return s


def _restated(pman, S, groups, rnd, p, tree=None, stop_after=None):
    P = pman.Base
    return hr.turn_on_quasars(P["Pos"], P["Type"], P["Flags"], P["PI"], S["Density"], S["Entropy"], groups, rnd, p,
                              hr.host_tree(tree, pman.NumPart) if tree is not None else None, stop_after=stop_after)


def _compare(pman, S, res, log, want):
    flags, entropy, wlog, wres = want
    assert np.array_equal(pman.Base["Flags"], flags), np.flatnonzero(pman.Base["Flags"] != flags)[:10]
    assert np.all(np.abs(S["Entropy"] - entropy) <= 1e-14 * np.abs(entropy))
    assert len(log) == len(wlog) == wres["n_iterations"]
    for row, (g, pos, frac, nion) in zip(log, wlog):
        assert int(row["group"]) == g and tuple(float(x) for x in row["pos"]) == pos
        assert float(row["ionfrac"]) == frac and int(row["n_ionized"]) == nion
    got = dict(init_ionfrac=res.init_ionfrac, final_ionfrac=res.final_ionfrac, n_candidates=res.n_candidates, n_iterations=res.n_iterations,
               n_flash=res.n_flash, n_ionized=res.n_ionized)
    assert got == wres


def _stats(ctx):
    st = capi.HeiiiStats()
    capi.check(capi.hip.shq_heiii_last_stats(ctx.h, C.byref(st)))
    return st


def _case(ctx, N, nhalo, rnd_seed=5, tree=False, current=True, trajectory_stop=None, **kw):
    pman, S, ngas = _particles(N, nhalo)
    groups = _fof(ctx, pman, S, N)
    rnd = np.random.default_rng(rnd_seed).random(4096)
    p = _params(ngas, **kw)
    gtree = sq.force_tree_rebuild_mask(pman, sq.GASMASK | sq.BHMASK) if tree else None
    if trajectory_stop is not None:   # a target the loop reaches exactly at this iteration (or the first one after it that ionises)
        _, _, tlog, _ = _restated(pman, S, groups, rnd, dict(p, desired_ion_frac=0.99), gtree, stop_after=trajectory_stop + 40)
        k = next(i for i in range(trajectory_stop, len(tlog)) if tlog[i][3] > 0)
        p["desired_ion_frac"] = tlog[k][2]
    want = _restated(pman, S, groups, rnd, p, gtree)
    flags0 = pman.Base["Flags"].copy()
    if current:
        capi.check(capi.hip.shq_set_inputs_current(ctx.h, capi_current()))
    try:
        res, log = sq.heiii_reionization(ctx, pman, S, _struct(p), rnd, gtree)
    finally:
        capi.check(capi.hip.shq_set_inputs_current(ctx.h, 0))
    _compare(pman, S, res, log, want)
    assert np.array_equal(pman.Base["Flags"] & ~np.uint8(4), flags0 & ~np.uint8(4))   # nothing but the HeIII bit changes
    return pman, S, groups, rnd, p, res, log, gtree


def capi_current():
    return 1 | 2   # SHQ_CURRENT_PARTICLES | SHQ_CURRENT_SPH


def test_heiii_one_bubble(ctx):
    pman, S, ngas = _particles(16, 120)
    init = np.count_nonzero((pman.Base["Type"] == 0) & (pman.Base["Flags"] & 4 != 0)) / ngas
    _, _, _, _, _, res, log, _ = _case(ctx, 16, 120, desired_ion_frac=init + 1e-9, current=False)
    assert res.n_ionized > 0 and int(log[-1]["n_ionized"]) > 0 and sum(int(r["n_ionized"]) > 0 for r in log) == 1
    assert _stats(ctx).nsweeps == 1


def test_heiii_stop_inside_a_batch(ctx):
    _, _, groups, _, _, res, log, _ = _case(ctx, 16, 120, trajectory_stop=45, qso_candidate_min_mass=10.0)
    assert 45 <= res.n_iterations < 32 + 64 and _stats(ctx).nsweeps == 2
    assert res.n_candidates == np.count_nonzero(groups["Mass"] >= 10.0)


def test_heiii_three_batches_to_the_end_of_the_list(ctx):
    _, _, groups, _, _, res, log, _ = _case(ctx, 16, 160, mean_bubble=700.0, qso_candidate_min_mass=2.0)
    st = _stats(ctx)
    assert res.n_iterations > 96 and st.nsweeps >= 3
    assert res.final_ionfrac < 0.9 and res.n_iterations == res.n_candidates - 1   # the list ran out; the last one never lit
    assert any(int(r["group"]) == -1 for r in log)


def test_heiii_flash(ctx):
    pman, _, _ = _particles(16, 120)
    ngas = int(np.count_nonzero(pman.Base["Type"] == 0))      # the slots of the converted particles no longer counted: all gas flashed = 1
    _, _, _, _, _, res, log, _ = _case(ctx, 16, 120, desired_ion_frac=0.999, n_gas_tot=ngas)
    assert res.n_flash > 0 and res.init_ionfrac == 1.0 and res.n_candidates == 0 and len(log) == 0
    # with the converted particles' slots still counted the flashed box stays below the target: the quasars run after the flash
    _, _, _, _, _, res, log, _ = _case(ctx, 16, 120, desired_ion_frac=0.999)
    assert res.n_flash > 0 and res.init_ionfrac < 0.999 and res.n_candidates > 0 and len(log) > 0


def test_heiii_negative_radii_on_the_gas_tree(ctx):
    pman, S, groups, rnd, p, res, log, gtree = _case(ctx, 16, 120, tree=True, mean_bubble=800.0, var_bubble=1.0e6, trajectory_stop=40)
    # some lit bubbles had a negative radius: the draws of the restatement again
    R = [hr.gaussian_rng(800.0, 1000.0, int(groups["MinID"][int(r["group"])]), rnd) for r in log if int(r["group"]) >= 0]
    assert sum(x < 0 for x in R) >= 3 and sum(x > 0 for x in R) >= 3


def test_heiii_two_calls_continue_on_the_context_copies(ctx):
    """the second call (next step, larger target) with shq_set_inputs_current: no upload, so what the first call flagged and heated must
    be in the context's copies for the second to match the restatement continued from the first's output"""
    pman, S, ngas = _particles(16, 120, seed=12)
    groups = _fof(ctx, pman, S, 16)
    rnd = np.random.default_rng(9).random(4096)
    capi.check(capi.hip.shq_set_inputs_current(ctx.h, capi_current()))
    try:
        for atime, target in ((0.25, 0.3), (0.26, 0.6)):
            p = _params(ngas, atime=atime, desired_ion_frac=target)
            want = _restated(pman, S, groups, rnd, p)
            res, log = sq.heiii_reionization(ctx, pman, S, _struct(p), rnd)
            _compare(pman, S, res, log, want)
            assert res.n_ionized > 0
    finally:
        capi.check(capi.hip.shq_set_inputs_current(ctx.h, 0))


def test_heiii_deterministic(ctx):
    out = []
    for _ in range(2):
        pman, S, _, _, _, res, log, _ = _case(ctx, 16, 120, trajectory_stop=50, var_bubble=4.0e5, tree=True)
        out.append((pman.Base["Flags"].copy(), S["Entropy"].copy(), log.copy(), res.n_ionized, res.final_ionfrac))
    a, b = out
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3:] == b[3:]


def test_heiii_at_2x64cubed(ctx):
    _, _, _, _, _, res, log, _ = _case(ctx, 64, 1000, mean_bubble=600.0, trajectory_stop=150)
    assert res.n_iterations >= 150 and _stats(ctx).nsweeps >= 3 and res.n_ionized > 1000


def test_heiii_bad_input(ctx):
    pman, S, ngas = _particles(8, 20)
    rnd = np.random.default_rng(1).random(256)
    pv, sv = pman.view(), capi.sph_view(S)
    capi.check(capi.hip.shq_set_inputs_current(ctx.h, 0))
    capi.check(capi.hip.shq_particles_upload(ctx.h, C.byref(pv)))   # a new particle set: no catalogue
    res, nlog = capi.HeiiiResult(), C.c_int64()

    def call(p, tree=None, S_=S):
        return capi.hip.shq_heiii_reionization(ctx.h, C.byref(_struct(p)), C.byref(pman.view()), C.byref(capi.sph_view(S_)),
                                               C.byref(tree.view()) if tree is not None else None, capi.ptr(rnd), len(rnd), None, 0,
                                               C.byref(nlog), C.byref(res))
    assert call(_params(ngas)) == ERR_STATE
    _fof(ctx, pman, S, 8)
    assert call(_params(ngas, var_bubble=1e4)) == ERR_INVALID                    # a positive variance needs the gas tree
    flags0 = pman.Base["Flags"].copy()
    assert call(_params(ngas), S_=S[:-3]) == ERR_INVALID                          # gas particles with PI outside the slots
    assert np.array_equal(pman.Base["Flags"], flags0)
