"""Glass making on the device (shq_glass_evolve: glass_evolve, libgenic/glass.cpp:76-360) against the numpy restatement
(glass_restated.py): one force, every one of 14 steps from the device's own state, composition and determinism bit for bit, the
statistics and the double-counted spectrum, two species in one call, bad input, no interference with the context's residents, and the
hand-over to the displacement call.  Every test restores what it changes on the shared context.

The bars.  The three force meshes of device and restatement agree to BAR = 1e-11 max|mesh|, the bar of
test_pm_apply_other_petapm_clients and test_gpu_zeldovich.py for the same transfer + c2r.  A difference that small can flip each of the
eight float roundings of the gather by one float ulp of the running sum, which max|mesh| bounds: per component
    |dDisp| <= (8 * 2^-23 + 1e-11) max|force mesh|.
A kick multiplies that by hdt and adds a float ulp of |Vel|; a drift multiplies by dt."""
import ctypes as C
import math

import numpy as np
import pytest

import shenqi_amd as sq
from shenqi_amd import capi
import common as cm
import glass_restated as gr

pytestmark = pytest.mark.gpu

ERR_INVALID = 1
BAR = 1e-11
L = 1.0


def _disp_bar(meshes):
    return (8 * 2.0**-23 + BAR) * max(float(np.abs(m).max()) for m in meshes)


def _ulp32(x):
    return float(np.spacing(np.float32(np.abs(x).max())))


def _input(Ngrid, seed, outside=True):
    """setup_glass's positions, some particles pushed out of the box on both sides"""
    pos = sq.glass_setup_positions(Ngrid, L, 0.0, seed)
    if outside:
        pos[::7] += L
        pos[3::11, 1] -= 2 * L
        pos[5::13, 2] += 3 * L
    return pos


def _zero_vel(n):
    return np.zeros((n, 3), dtype=np.float32)


@pytest.mark.parametrize("Ngrid,N", [(16, 32), (32, 64), (12, 18)])
def test_one_force_against_restatement(ctx, Ngrid, N):
    pos = _input(Ngrid, 100 + N)
    assert (pos < 0).any() and (pos >= L).any()
    n = len(pos)
    mass = np.ones(n, dtype=np.float32)
    out = sq.glass_evolve(ctx, N, L, pos, _zero_vel(n), mass, nsteps=0)
    assert np.array_equal(out["Pos"], pos) and not out["Vel"].any() and out["steps"] == []
    ref, meshes, _ = gr.glass_force(pos, mass, N, L)
    bar = _disp_bar(meshes)
    err = np.abs(out["Disp"].astype(np.float64) - ref.astype(np.float64)).max()
    same = float((out["Disp"] == ref).mean())
    print(f"Ngrid {Ngrid} Nmesh {N}: max |dDisp| {err:.3e} (bar {bar:.3e}), bit-equal components {100 * same:.2f} %")
    assert out["Disp"].dtype == np.float32 and err <= bar


def test_every_step_from_the_device_state(ctx):
    """for s = 0 .. 13: the device's state after s steps, one restated step from exactly that state, against the device's state after
    s + 1 steps.  The closing force is compared at the DEVICE's drifted positions, and the closing kick takes the device's Disp, so
    that the comparison holds no derivative of the force field: Vel and Pos carry only the opening Disp's bar through kick and drift."""
    Ngrid, N = 16, 32
    pos = _input(Ngrid, 7)
    n = len(pos)
    mass = np.ones(n, dtype=np.float32)
    vel = _zero_vel(n)
    worst = dict(disp=0.0, vel=0.0, pos=0.0)
    for s in range(14):
        out = sq.glass_evolve(ctx, N, L, pos, vel, mass, nsteps=1, spectra=True)
        d0, m0, _ = gr.glass_force(pos, mass, N, L)
        bar0 = _disp_bar(m0)
        v1 = gr.kick(vel, d0)
        bar_v1 = bar0 * gr.HDT + _ulp32(v1)
        p1 = gr.drift(pos, v1)
        bar_p = bar_v1 * gr.DT + 2 * float(np.spacing(np.abs(p1).max()))
        e = np.abs(out["Pos"] - p1).max()
        worst["pos"] = max(worst["pos"], e / bar_p)
        assert e <= bar_p, (s, e, bar_p)
        d1, m1, ps = gr.glass_force(out["Pos"], mass, N, L, spectrum=True)
        bar1 = _disp_bar(m1)
        e = np.abs(out["Disp"].astype(np.float64) - d1).max()
        worst["disp"] = max(worst["disp"], e / bar1)
        assert e <= bar1, (s, e, bar1)
        v2 = gr.kick(v1, out["Disp"])
        bar_v2 = bar_v1 * abs(1 - gr.HDT) + 2 * _ulp32(v2)
        e = np.abs(out["Vel"].astype(np.float64) - v2).max()
        worst["vel"] = max(worst["vel"], e / bar_v2)
        assert e <= bar_v2, (s, e, bar_v2)
        # statistics on the device's own Disp and Vel: 3 n non-negative terms in any order
        fs, vs = gr.glass_stats(out["Disp"], out["Vel"])
        tol = 3 * (3 * n) * 2.0**-53
        st = out["steps"][0]
        assert abs(st["force_std"] / fs - 1) <= tol and abs(st["vel_std"] / vs - 1) <= tol
        assert (st["t_f"], st["t_v"], st["t_x"]) == (gr.HDT, gr.DT, gr.HDT + gr.HDT)
        # the spectrum of this step's force, restated on the device's positions
        kk, power, nmodes, norm = ps
        nz = nmodes > 0
        anyorder = 3 * (N**3) * 2.0**-53
        assert np.array_equal(out["nmodes"][0], nmodes) and nmodes.sum() == 2 * (N**3 - 1)
        assert np.abs(out["kk"][0][nz] / kk[nz] - 1).max() <= 1e-11 + anyorder
        assert np.abs(out["power"][0][nz] / power[nz] - 1).max() <= 1e-11 + anyorder
        assert not out["power"][0][~nz].any() and abs(out["norm"][0] / norm - 1) <= 1e-11 + anyorder
        pos, vel = out["Pos"], out["Vel"]
    print("worst error / bar over 14 steps:", {k: round(v, 4) for k, v in worst.items()})


def test_composition_determinism_permutation(ctx):
    Ngrid, N = 16, 32
    pos = _input(Ngrid, 21)
    n = len(pos)
    mass = np.ones(n, dtype=np.float32)
    full = sq.glass_evolve(ctx, N, L, pos, _zero_vel(n), mass, nsteps=14, spectra=True)
    again = sq.glass_evolve(ctx, N, L, pos, _zero_vel(n), mass, nsteps=14)
    for k in ("Pos", "Vel", "Disp"):
        assert np.array_equal(full[k], again[k]), k
    assert [s["t_x"] for s in full["steps"]] == [s["t_x"] for s in again["steps"]]
    a = sq.glass_evolve(ctx, N, L, pos, _zero_vel(n), mass, nsteps=5)
    b = sq.glass_evolve(ctx, N, L, a["Pos"], a["Vel"], mass, nsteps=9)
    for k in ("Pos", "Vel", "Disp"):
        assert np.array_equal(full[k], b[k]), k
    c = dict(Pos=pos, Vel=_zero_vel(n))
    for _ in range(14):
        c = sq.glass_evolve(ctx, N, L, c["Pos"], c["Vel"], mass, nsteps=1)
    for k in ("Pos", "Vel", "Disp"):
        assert np.array_equal(full[k], c[k]), k
    # t_f, t_v, t_x of a long call, exactly as the reference advances them
    t_x = t_v = 0.0
    for st in full["steps"]:
        t_x += gr.HDT
        t_v += gr.DT
        t_f = t_x
        t_x += gr.HDT
        assert (st["t_f"], st["t_v"], st["t_x"]) == (t_f, t_v, t_x)
    assert full["steps"][-1]["force_std"] < full["steps"][0]["force_std"]
    # a permuted particle order gives the permuted result (equal masses: totmass is the same double)
    perm = np.random.default_rng(3).permutation(n)
    p = sq.glass_evolve(ctx, N, L, pos[perm], _zero_vel(n), mass, nsteps=14)
    for k in ("Pos", "Vel", "Disp"):
        assert np.array_equal(full[k][perm], p[k]), k
    assert full["phase_ms"][3] > 0 and full["phase_ms"][1] > 0


def test_two_species_in_one_call(ctx):
    """the coherent pass of genic/main.cpp:152-153: CDM and gas together, per-particle masses"""
    Ngrid, N = 16, 32
    cdm, gas = _input(Ngrid, 31), _input(Ngrid, 32, outside=False) + 0.5 * L / Ngrid
    pos = np.concatenate([cdm, gas])
    n = len(pos)
    mass = np.concatenate([np.full(len(cdm), 0.84, dtype=np.float32), np.full(len(gas), 0.16, dtype=np.float32)])
    out = sq.glass_evolve(ctx, N, L, pos, _zero_vel(n), mass, nsteps=1)
    d0, m0, _ = gr.glass_force(pos, mass, N, L)
    one = sq.glass_evolve(ctx, N, L, pos, _zero_vel(n), mass, nsteps=0)
    assert np.abs(one["Disp"].astype(np.float64) - d0).max() <= _disp_bar(m0)
    v1 = gr.kick(_zero_vel(n), d0)
    bar_v1 = _disp_bar(m0) * gr.HDT + _ulp32(v1)
    assert np.abs(out["Pos"] - gr.drift(pos, v1)).max() <= bar_v1 * gr.DT + 2 * float(np.spacing(np.abs(pos).max()))
    d1, m1, _ = gr.glass_force(out["Pos"], mass, N, L)
    assert np.abs(out["Disp"].astype(np.float64) - d1).max() <= _disp_bar(m1)
    # the masses matter: equal masses give another force
    eq, _, _ = gr.glass_force(pos, np.ones(n, dtype=np.float32), N, L)
    assert np.abs(eq.astype(np.float64) - d0).max() > 100 * _disp_bar(m0)


def test_bad_input_changes_nothing(ctx):
    n, N = 64, 16
    pos0 = _input(4, 1)
    steps = (capi.GlassStep * 2)()
    kk = np.full((2, N), 7.0); power = kk.copy(); nmodes = np.full((2, N), 7, dtype=np.int64); norm = np.full(2, 7.0)

    def call(Nmesh=N, nsteps=2, box=L, n_=n, pos=None, vel=None, mass=None, sp=(True, True, True, True)):
        p = pos0.copy() if pos is None else pos
        v = np.full((n, 3), 0.5, dtype=np.float32) if vel is None else vel
        m = np.ones(n, dtype=np.float32) if mass is None else mass
        d = np.full((n, 3), 9.0, dtype=np.float32)
        keep = (p.copy(), v.copy())
        gp = capi.GlassParams(Nmesh, nsteps, box)
        arrs = [capi.ptr(a) if on else None for a, on in zip((kk, power, nmodes, norm), sp)]
        rc = capi.hip.shq_glass_evolve(ctx.h, C.byref(gp), n_, capi.ptr(p), capi.ptr(v), capi.ptr(d), capi.ptr(m), C.cast(steps, C.c_void_p), *arrs)
        assert np.array_equal(p, keep[0], equal_nan=True) and np.array_equal(v, keep[1], equal_nan=True) and (d == 9.0).all()
        assert (kk == 7).all() and (power == 7).all() and (nmodes == 7).all() and (norm == 7).all()
        return rc

    def with_(arr, idx, val):
        arr = arr.copy()
        arr[idx] = val
        return arr

    v0, m0 = np.zeros((n, 3), dtype=np.float32), np.ones(n, dtype=np.float32)
    for kw in (dict(Nmesh=17), dict(Nmesh=2), dict(Nmesh=2050), dict(nsteps=-1), dict(box=0.0), dict(box=float("inf")), dict(box=float("nan")),
               dict(n_=0), dict(n_=2**32), dict(pos=with_(pos0, (3, 1), np.nan)), dict(pos=with_(pos0, (63, 2), np.inf)),
               dict(vel=with_(v0, (5, 0), np.nan)), dict(mass=with_(m0, 9, np.inf)), dict(mass=np.zeros(n, dtype=np.float32)),
               dict(mass=-m0), dict(sp=(True, True, True, False)), dict(sp=(False, True, False, False))):
        assert call(**kw) == ERR_INVALID, kw
    assert capi.hip.shq_glass_phase_ms(ctx.h, None) == ERR_INVALID
    # and the same arguments without the fault are accepted
    out = sq.glass_evolve(ctx, N, L, pos0, None, 1.0, nsteps=2, spectra=True)
    assert len(out["steps"]) == 2 and out["nmodes"].sum() == 2 * 2 * (N**3 - 1)


def test_no_interference_with_the_contexts_residents(ctx):
    """a resident particle set with a finished PM run, a pending spectrum and a resident Zel'dovich field: the same bits from
    shq_pm_download, the finish and shq_zeldovich_download_field with glass calls in between as without; the settings survive"""
    n = 16**3
    pos = cm.random_positions(np.random.default_rng(9).random(3 * n), n)
    pman = cm.make_partmanager(pos)
    pmp = sq.PMParams(48, 0, cm.BOX, 1.5, cm.G)
    gpos = _input(8, 4)

    def glass(N):
        sq.glass_evolve(ctx, N, L, gpos, None, 1.0, nsteps=2, spectra=True)

    def download():
        g = np.zeros((n, 3)); p = np.zeros(n)
        capi.check(capi.hip.shq_pm_download(ctx.h, capi.ptr(g), capi.ptr(p)))
        return g, p

    def run(with_glass):
        capi.check(capi.hip.shq_zeldovich_drop_field(ctx.h))
        pv = pman.view()
        capi.check(capi.hip.shq_particles_upload(ctx.h, C.byref(pv)))
        capi.check(capi.hip.shq_pm_run(ctx.h, C.byref(pmp)))
        if with_glass:
            glass(48)
            glass(18)
        first = download()
        field = sq.zeldovich_field(ctx, 16, 5)
        capi.check(capi.hip.shq_pm_forward(ctx.h, C.byref(pmp)))
        state = (capi.hip.shq_pm_get_measure_power(ctx.h), capi.hip.shq_pm_get_deposit_log2scale(ctx.h))
        if with_glass:
            glass(32)
            glass(48)
            glass(18)
        assert state == (capi.hip.shq_pm_get_measure_power(ctx.h), capi.hip.shq_pm_get_deposit_log2scale(ctx.h))
        capi.check(capi.hip.shq_pm_run(ctx.h, C.byref(pmp)))          # finishes the pending spectrum
        second = download()
        spec = np.zeros((16, 9, 16), dtype=np.complex128)
        capi.check(capi.hip.shq_zeldovich_download_field(ctx.h, 16, capi.ptr(spec)))
        return first + second + (field, spec)

    try:
        ref, got = run(False), run(True)
        for a, b in zip(ref, got):
            assert np.array_equal(a, b)
        assert np.array_equal(got[4], got[5])
    finally:
        capi.check(capi.hip.shq_zeldovich_drop_field(ctx.h))
        capi.check(capi.hip.shq_set_inputs_current(ctx.h, 0))


def test_wrapped_output_feeds_the_displacement_call(ctx):
    Ngrid, N = 8, 16
    pos = _input(Ngrid, 2)
    raw = sq.glass_evolve(ctx, N, L, pos, None, 1.0, nsteps=3)
    out = sq.glass_evolve(ctx, N, L, pos, None, 1.0, nsteps=3, wrap=True)
    assert ((raw["Pos"] < 0) | (raw["Pos"] >= L)).any()
    assert (out["Pos"] >= 0).all() and (out["Pos"] < L).all()
    assert np.abs(np.round((out["Pos"] - raw["Pos"]) / L) * L - (out["Pos"] - raw["Pos"])).max() < 1e-15
    try:
        with pytest.raises(Exception):
            sq.displacement_fields(ctx, raw["Pos"], N, L, 5, lambda k: 1e-3 / (1 + k))
        z = sq.displacement_fields(ctx, out["Pos"], N, L, 5, lambda k: 1e-3 / (1 + k))
        assert np.isfinite(z["Pos"]).all() and np.isfinite(z["Disp"]).all() and z["Disp"].any()
    finally:
        capi.check(capi.hip.shq_zeldovich_drop_field(ctx.h))
