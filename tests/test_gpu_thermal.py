"""The thermal velocities on the device (shq_thermal_speeds: add_thermal_speeds, libgenic/thermal.cpp:95-110, in the particle loops of
genic/main.cpp:176-184 and 218-226) against the Python restatement (thermal_restated.py): the engine bit for bit through the test
entry, the call end to end on the three smallest shapes at which the kernel can go wrong, the launch shape, bad input and no
interference.  Every test restores what it changes on the shared context."""
import ctypes as C
import functools

import numpy as np
import pytest

import shenqi_amd as sq
from shenqi_amd import capi
import common as cm
import thermal_restated as tr

pytestmark = pytest.mark.gpu

ERR_INVALID = 1
V_AMP = 137.5
# (Ngrid, x0, nx, y0, ny): 36 columns (less than a wave; 18 draws per column cross a discard block), a rank's sub-block (the column
# arithmetic and the transposed seed lookup), 400 columns = 6.25 waves with a ragged last tile along z
SHAPES = {"whole6": (6, 0, 6, 0, 6), "block12": (12, 3, 5, 2, 7), "whole20": (20, 0, 20, 0, 20)}
# |dvel - restatement| per component in units of 2^-52 * v: the speed is bit-equal, so this is the device's sin, cos and acos against
# glibc's.  Measured on an MI355X: 2.12 (whole6), 1.98 (block12), 2.44 (whole20), the largest always in z = v cos(acos(2 u - 1)).
# The bound is 4 x the measured maximum; above 64 something other than libm rounding would be wrong.
DVEL_MEASURED = 2.44
DVEL_BOUND = 4 * DVEL_MEASURED


def _restore(ctx):
    capi.check(capi.hip.shq_set_inputs_current(ctx.h, 0))
    capi.check(capi.hip.shq_zeldovich_drop_field(ctx.h))


@pytest.fixture
def tctx(ctx):
    _restore(ctx)
    try:
        yield ctx
    finally:
        _restore(ctx)


@functools.lru_cache(maxsize=None)
def _tables():
    vel, cumprob, _ = sq.thermal_tables(50.0)
    for a in (vel, cumprob):
        a.setflags(write=False)
    return cumprob, vel


@functools.lru_cache(maxsize=None)
def _case(name):
    """inputs and the restatement's result of one shape, computed once and never written"""
    Ngrid, x0, nx, y0, ny = SHAPES[name]
    n = nx * ny * Ngrid
    rng = np.random.default_rng(Ngrid)
    vin = (rng.standard_normal((n, 3)) * V_AMP * 10.0 ** rng.uniform(-3, 0, (n, 3))).astype(np.float32)
    vin[vin == 0] = np.float32(0.25)
    table = sq.thermal_seed_table(4711 + Ngrid, Ngrid)
    cumprob, fdvel = _tables()
    ref = tr.thermal_speeds(vin, Ngrid, V_AMP, table, cumprob, fdvel, x0, nx, y0, ny)
    for a in (vin, table, *ref.values()):
        a.setflags(write=False)
    return vin, table, ref


def _draws(ctx, seeds, m):
    seeds = np.ascontiguousarray(seeds, dtype=np.uint32)
    raw = np.zeros((len(seeds), m), dtype=np.uint64)
    capi.check(capi.hip.shq_thermal_column_draws(ctx.h, len(seeds), capi.ptr(seeds), m, capi.ptr(raw)))
    return raw


def test_engine_bit_for_bit(tctx):
    """m = 40 crosses three discard blocks; 70 engines are more than one wave, the last one partly filled"""
    seeds = [0, 1, 12345, 2**32 - 1]
    raw = _draws(tctx, seeds, 40)
    for row, seed in zip(raw, seeds):
        assert [int(v) for v in row] == tr.ranlux48_stream(seed, 40), seed
    seeds = (np.arange(70, dtype=np.uint64) * 2654435761 % 2**32).astype(np.uint32)
    raw = _draws(tctx, seeds, 40)
    assert np.array_equal(raw, tr.Ranlux48(seeds).outputs(40))
    assert int(raw.max()) < 2**48


@pytest.mark.parametrize("name", list(SHAPES))
def test_end_to_end(tctx, name):
    Ngrid, x0, nx, y0, ny = SHAPES[name]
    vin, table, ref = _case(name)
    cumprob, fdvel = _tables()
    got = sq.thermal_speeds(tctx, vin, Ngrid, V_AMP, table, cumprob, fdvel, x0, nx, y0, ny, want_dvel=True, want_speed=True)
    n = len(vin)
    assert got["phase_ms"][2] >= got["phase_ms"][1] > 0 and got["phase_ms"][0] > 0

    # the bin: from the device's own first draw of every particle, and the speed inside the bin's two knots
    xs, ys = np.arange(x0, x0 + nx), np.arange(y0, y0 + ny)
    col_seeds = table[(xs[:, None] * Ngrid + ys[None, :]).ravel()]
    raw = _draws(tctx, col_seeds, 3 * Ngrid).reshape(n, 3)
    p = raw[:, 0].astype(np.float64) * 2.0 ** -48
    ibin = tr.find_bin(cumprob, p)
    assert np.array_equal(ibin, ref["bin"])
    upper = V_AMP * fdvel[ibin + 1]
    ulp = np.spacing(upper)
    assert np.all(got["speed"] >= V_AMP * fdvel[ibin] - 8 * ulp) and np.all(got["speed"] <= upper + 8 * ulp)

    # the speed: IEEE operations in the stated order on both sides; it came out bit-equal on an MI355X, so equality is asserted (the
    # looser bound would be 8 ulp of the bin's upper knot speed times v_amp: about a dozen rounded operations without cancellation)
    serr = (np.abs(got["speed"] - ref["speed"]) / ulp).max()
    print(f"{name}: speed max |diff| {serr:.2f} ulp of the bin's upper knot speed times v_amp")
    assert np.array_equal(got["speed"], ref["speed"])

    # what was added is what is reported, bit for bit
    assert np.array_equal(got["Vel"], (vin.astype(np.float64) + got["dvel"]).astype(np.float32))

    # the increments: the device's sin, cos and acos against glibc's
    derr = np.abs(got["dvel"] - ref["dvel"]) / (2.0 ** -52 * ref["speed"][:, None])
    print(f"{name}: dvel max |diff| {derr.max():.2f} (x {derr[:, 0].max():.2f}, y {derr[:, 1].max():.2f}, z {derr[:, 2].max():.2f}) "
          f"in units of 2^-52 v")
    assert DVEL_BOUND <= 64
    assert derr.max() <= DVEL_BOUND

    # the float velocities: a differing last bit of the double sum moves the rounded float about once in 10^3 shapes
    differ = got["Vel"] != ref["Vel"]
    print(f"{name}: {int(differ.sum())} of {3 * n} float components differ")
    assert np.all(np.abs(got["Vel"].astype(np.float64) - ref["Vel"].astype(np.float64)) <= np.spacing(np.abs(ref["Vel"])).astype(np.float64))
    assert differ.sum() <= 2


def test_second_call_is_bit_equal(tctx):
    """the launch is not chunked over columns: a second identical call, and a call without the optional outputs"""
    Ngrid, x0, nx, y0, ny = SHAPES["whole20"]
    vin, table, _ = _case("whole20")
    cumprob, fdvel = _tables()

    def run():
        return sq.thermal_speeds(tctx, vin, Ngrid, V_AMP, table, cumprob, fdvel, x0, nx, y0, ny, want_dvel=True, want_speed=True)

    a, b = run(), run()
    for name in ("Vel", "dvel", "speed"):
        assert np.array_equal(a[name], b[name]), name
    d = sq.thermal_speeds(tctx, vin, Ngrid, V_AMP, table, cumprob, fdvel, x0, nx, y0, ny)
    assert d["dvel"] is None and d["speed"] is None and np.array_equal(a["Vel"], d["Vel"])


def test_bad_input_is_refused_before_anything_is_written(tctx):
    Ngrid, x0, nx, y0, ny = SHAPES["block12"]
    vin, table, _ = _case("block12")
    cumprob, fdvel = _tables()
    n = len(vin)

    def call(Ngrid=Ngrid, x0=x0, nx=nx, y0=y0, ny=ny, n=n, v_amp=V_AMP, table=table, cumprob=cumprob, fdvel=fdvel, params=True, vel=True):
        tp = capi.ThermalParams(Ngrid, x0, nx, y0, ny, 0, v_amp)
        v = vin.copy()
        dv, sp = np.full((len(v), 3), 7.0), np.full(len(v), 7.0)
        rc = capi.hip.shq_thermal_speeds(tctx.h, C.byref(tp) if params else None, capi.ptr(table), capi.ptr(cumprob), capi.ptr(fdvel), n,
                                         capi.ptr(v) if vel else None, capi.ptr(dv), capi.ptr(sp))
        return rc, bool(np.array_equal(v, vin) and np.all(dv == 7.0) and np.all(sp == 7.0))

    def changed(a, i, value):
        a = a.copy()
        a[i] = value
        return a

    refused = (ERR_INVALID, True)
    assert call(Ngrid=1, x0=0, nx=1, y0=0, ny=1, n=1) == refused
    assert call(Ngrid=0, x0=0, nx=0, y0=0, ny=0, n=0) == refused
    for kw in (dict(x0=-1), dict(x0=8), dict(nx=0), dict(y0=-2), dict(y0=6), dict(ny=0), dict(x0=12, nx=1), dict(nx=2**30)):
        assert call(**kw) == refused, kw
    assert call(n=n - 1) == refused and call(n=n + Ngrid) == refused
    assert call(Ngrid=1291, x0=0, nx=1291, y0=0, ny=1291, n=1291**3, table=np.zeros(1291**2, dtype=np.uint32)) == refused    # n >= 2^31
    for kw in (dict(params=False), dict(table=None), dict(cumprob=None), dict(fdvel=None), dict(vel=False)):
        assert call(**kw) == refused, kw
    for bad in (np.nan, np.inf, -np.inf):
        assert call(v_amp=bad) == refused
        assert call(cumprob=changed(cumprob, 700, bad)) == refused
        assert call(fdvel=changed(fdvel, 1999, bad)) == refused
    assert call(cumprob=changed(cumprob, 0, 1e-300)) == refused
    assert call(cumprob=changed(cumprob, 1999, np.nextafter(1.0, 0.0))) == refused
    assert call(cumprob=changed(cumprob, 1000, cumprob[999])) == refused        # not strictly increasing
    assert call(cumprob=changed(cumprob, 1000, cumprob[1001])) == refused
    assert call(fdvel=changed(fdvel, 5, fdvel[4])) == refused
    rc, untouched = call()
    assert rc == 0 and not untouched
    # the test entry
    raw = np.full((2, 4), 7, dtype=np.uint64)
    seeds = np.zeros(2, dtype=np.uint32)
    for args in ((0, capi.ptr(seeds), 4, capi.ptr(raw)), (65537, capi.ptr(seeds), 4, capi.ptr(raw)), (2, capi.ptr(seeds), 0, capi.ptr(raw)),
                 (2, None, 4, capi.ptr(raw)), (2, capi.ptr(seeds), 4, None)):
        assert capi.hip.shq_thermal_column_draws(tctx.h, *args) == ERR_INVALID
    assert np.all(raw == 7)
    assert capi.hip.shq_thermal_phase_ms(tctx.h, None) == ERR_INVALID


def test_no_interference_with_resident_state(tctx):
    """a resident Zel'dovich field, a resident particle set and tree: a thermal call changes neither (the field's bytes before and after;
    shq_treepm_step on the resident set gives the same bits with thermal calls in between)"""
    ctx = tctx
    Nf = 16
    field = sq.zeldovich_field(ctx, Nf, 99)
    n, L, nmesh = 12**3, 1.0, 24
    pos = sq.synth_positions("cluster", n, L=L)
    pos = pos[sq.morton_order(pos, L)]
    pman = cm.make_partmanager(pos, box=L)
    tree = sq.force_tree_full(pman)
    sq.set_gravshort_treepar(ErrTolForceAcc=0.005, BHOpeningAngle=0.175, MaxBHOpeningAngle=0.9, TreeUseBH=0, Rcut=6.0)
    sq.gravshort_set_softenings(L / 12)
    gp = sq.make_grav_params(L, 1.5, nmesh, cm.G, cm.RHO0)
    pmp = sq.PMParams(nmesh, 0, L, 1.5, cm.G)
    rng = np.random.default_rng(11)
    pman.Base["FullTreeGravAccel"] = rng.standard_normal((n, 3)) * 50.0
    pman.Base["GravPM"] = rng.standard_normal((n, 3))
    cumprob, fdvel = _tables()

    def thermal(name):
        Ngrid, x0, nx, y0, ny = SHAPES[name]
        vin, table, _ = _case(name)
        sq.thermal_speeds(ctx, vin, Ngrid, V_AMP, table, cumprob, fdvel, x0, nx, y0, ny, want_dvel=True)

    def results():
        g = np.zeros((n, 3)); pp = np.zeros(n)
        capi.check(capi.hip.shq_pm_download(ctx.h, capi.ptr(g), capi.ptr(pp)))
        acc = np.zeros((n, 3)); pot = np.zeros(n); nint = np.zeros(n, dtype=np.int64)
        capi.check(capi.hip.shq_grav_short_download(ctx.h, capi.ptr(acc), capi.ptr(pot), capi.ptr(nint), C.byref(sq.WalkStats())))
        return g, pp, acc, pot, nint

    def run(with_thermal):
        pv, tv = pman.view(), tree.view()
        capi.check(capi.hip.shq_particles_upload(ctx.h, C.byref(pv)))
        capi.check(capi.hip.shq_tree_upload(ctx.h, C.byref(tv)))
        if with_thermal:
            thermal("block12")
        capi.check(capi.hip.shq_treepm_step(ctx.h, C.byref(pmp), C.byref(gp), 1, sq.WALK_EXACT))
        first = results()
        if with_thermal:
            thermal("whole6")
        return first, results()

    ref, _ = run(False)
    got, got_after = run(True)
    for a, b, c, name in zip(ref, got, got_after, ("GravPM", "PM potential", "acc", "pot", "ninteractions")):
        assert np.array_equal(a, b), name
        assert np.array_equal(a, c), name
    spec = np.zeros_like(field)
    capi.check(capi.hip.shq_zeldovich_download_field(ctx.h, Nf, capi.ptr(spec)))
    assert spec.tobytes() == field.tobytes()
