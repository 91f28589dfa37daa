"""The Zel'dovich displacements on the device (shq_zeldovich_displacements: displacement_fields, libgenic/zeldovich.cpp:150-264, with
the Gaussian fill of libgenic/pmesh.h:64-178) against the numpy restatement (zeldovich_restated.py), which does the literal
two-generator procedure: the engine bit for bit through the test entry, the field, the call end to end, agreement with shq_pm_apply,
reuse of the resident field, determinism, bad input and no interference.  Every test restores what it changes on the shared context."""
import ctypes as C

import numpy as np
import pytest

import shenqi_amd as sq
from shenqi_amd import capi
import common as cm
import zeldovich_restated as zr

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE = 1, 4
BOX = 25.0
# |device - restatement| per component of a mode: the phase double is the same on both sides (u * 2 * M_PI, plain IEEE);
# |ampl| <= sqrt(32 ln 2) = 4.71; device sin / cos <= 4 ulp, log <= 3 ulp, sqrt exact, glibc < 1 ulp: about 6e-15, times 3
FIELD_ATOL = 2e-14
# the bar of test_pm_apply_other_petapm_clients for the same transfer + c2r, relative to max|field|
BAR = 1e-11


def _restore(ctx):
    capi.check(capi.hip.shq_set_inputs_current(ctx.h, 0))
    capi.check(capi.hip.shq_zeldovich_set_fill_chunk(ctx.h, 0))
    capi.check(capi.hip.shq_zeldovich_drop_field(ctx.h))


@pytest.fixture
def zctx(ctx):
    _restore(ctx)
    try:
        yield ctx
    finally:
        _restore(ctx)


def _draws(ctx, m, seeds=None, states=None):
    n = len(seeds) if seeds is not None else len(states)
    raw = np.zeros((n, m), dtype=np.uint32)
    pairs = np.zeros((n, m // 2, 2))
    s = None if seeds is None else np.ascontiguousarray(seeds, dtype=np.uint32)
    st = None if states is None else np.ascontiguousarray(states, dtype=np.uint32)
    capi.check(capi.hip.shq_zeldovich_column_draws(ctx.h, n, capi.ptr(s), capi.ptr(st), m, capi.ptr(raw), capi.ptr(pairs)))
    return raw, pairs


def test_raw_draws_bit_for_bit(zctx):
    """the engine alone: m = 1600 is past the second twist"""
    seeds = [0, 1, 5489, 0x7FFFFFFE]
    raw, pairs = _draws(zctx, 1600, seeds=seeds)
    st = zr.init_genrand(seeds)
    assert np.array_equal(raw, zr.raw_outputs(st, 1600))
    assert np.array_equal(pairs, zr.sample_pairs(st, 1600))
    # 70 generators: more than one wave, the last one partly filled
    seeds = np.arange(70) * 2654435761 % 2**31
    raw, pairs = _draws(zctx, 700, seeds=seeds)
    assert np.array_equal(raw, zr.raw_outputs(zr.init_genrand(seeds), 700))


def test_engine_standard_value(zctx):
    """[rand.predef]: the 10000th output of mt19937(5489) is 4123659995"""
    raw, _ = _draws(zctx, 10000, seeds=[5489])
    assert int(raw[0, 9999]) == 4123659995


def test_redraw_on_a_crafted_state(zctx):
    """mt[1] = mt[2] = mt[398] = 0 before the twist: the second output is 0, the first SAMPLE redraws its ampl and the stream shifts"""
    st = zr.init_genrand([12345, 99])
    st[0, [1, 2, 398]] = 0
    raw, pairs = _draws(zctx, 40, states=st)
    assert raw[0, 1] == 0 and raw[1, 1] != 0
    assert np.array_equal(raw, zr.raw_outputs(st, 40))
    ref = zr.sample_pairs(st, 40)
    assert np.array_equal(pairs, ref)
    assert pairs[0, 0, 1] == raw[0, 2] / 4294967296.0 and pairs[0, 1, 0] == raw[0, 3] / 4294967296.0 * 2 * np.pi


@pytest.mark.parametrize("N", [16, 24, 48, 18])
def test_field_matches_restatement(zctx, N):
    """the downloaded spectrum ([y][z'][x]) against the literal fill, each flag on and off"""
    sc = np.ix_((0, N // 2), (0, N // 2), (0, N // 2))
    for unitary, invert in ((0, 0), (1, 0), (0, 1), (1, 1)):
        got = sq.zeldovich_field(zctx, N, 4242, unitary, invert)
        dense = zr.fill_gaussian(N, 4242, unitary, invert)
        ref = zr.reference_layout(dense)
        err = max(np.abs(got.real - ref.real).max(), np.abs(got.imag - ref.imag).max())
        print(f"N {N} unitary {unitary} invert {invert}: max |diff| per component {err:.3e}")
        assert err < FIELD_ATOL, (N, unitary, invert, err)
        gd = got.transpose(2, 0, 1)                     # [x][y][z']
        assert gd[0, 0, 0] == 0
        assert np.all(gd[sc].imag == 0)                 # set exactly by the reference
        # the conjugate columns' two planes are exact conjugates of each other, as in the restatement
        idx = (N - np.arange(N)) % N
        for k in (0, N // 2):
            assert np.array_equal(gd[:, :, k], np.conj(gd[np.ix_(idx, idx)][:, :, k]))


def test_field_is_independent_of_the_column_ranges(zctx):
    N = 24
    ref = sq.zeldovich_field(zctx, N, 7)
    for chunk in (64, 200, 320):
        capi.check(capi.hip.shq_zeldovich_drop_field(zctx.h))
        capi.check(capi.hip.shq_zeldovich_set_fill_chunk(zctx.h, chunk))
        assert np.array_equal(sq.zeldovich_field(zctx, N, 7), ref)


def _delta(k):
    return 3.0 * k / (1.0 + (k / 2.0) ** 3)             # a stand-in for curpower->DeltaSpec


def _growth(k):
    return 1.0 + 0.2 * np.tanh(k)                       # ... and dlogGrowth


def _tables(N, other=False):
    d = zr.tabulate_k2(_delta, N, BOX)
    g = zr.tabulate_k2(_growth, N, BOX)
    return (d * zr.tabulate_k2(lambda k: 1.0 / (1.0 + k), N, BOX), g) if other else (d, g)


def _pdist(a, b, box=BOX):
    d = np.abs(a - b)
    return np.minimum(d, box - d)


def _compare(got, ref, tag, box=BOX):
    for name in ("Density", "Disp", "Vel"):
        scale = np.abs(ref[name]).max()
        err = np.abs(got[name] - ref[name]).max()
        print(f"{tag} {name}: max |diff| {err:.3e}, max |field| {scale:.3e}")
        assert err < BAR * scale, (tag, name, err, scale)
    dmax = np.abs(ref["Disp"]).max()
    perr = _pdist(got["Pos"], ref["Pos"], box).max()
    print(f"{tag} Pos: periodic distance {perr:.3e}, max |Disp| {dmax:.3e}")
    assert perr < BAR * dmax, (tag, perr)
    assert np.all((got["Pos"] >= 0) & (got["Pos"] < box))
    assert abs(got["maxdisp"] - ref["maxdisp"]) < BAR * dmax
    assert abs(got["maxvel"] - ref["maxvel"]) < BAR * ref["maxvel"]


@pytest.mark.parametrize("N", [16, 24, 48, 18])
@pytest.mark.parametrize("scaledep", [0, 1])
def test_end_to_end(zctx, N, scaledep):
    """an Ngrid^3 lattice, Ngrid = Nmesh / 2, unshifted and shifted by half a cell"""
    Ngrid = N // 2
    delta, growth = _tables(N)
    for shift in (0.0, 0.5 * BOX / Ngrid):
        pos, _ = sq.setup_grid(sq.IDGenerator(Ngrid, BOX), shift, 1.0)
        got = sq.displacement_fields(zctx, pos, N, BOX, 181170, delta, growth if scaledep else None, vel_prefac=37.5, ScaleDepVelocity=scaledep)
        ref = zr.displacement_fields(N, BOX, 181170, 0, 0, 37.5, scaledep, delta, growth, pos)
        _compare(got, ref, f"N {N} scaledep {scaledep} shift {shift:.3f}")
        assert got["maxdisp"] == max(0.0, got["Disp"].max())
        assert got["maxvel"] == (got["Vel"] ** 2).sum(axis=1).max() or abs(got["maxvel"] / (got["Vel"] ** 2).sum(axis=1).max() - 1) < 4e-16
        if not scaledep:
            assert np.array_equal(got["Vel"], got["Disp"] * 37.5)


@pytest.mark.parametrize("N", [18, 24])
def test_last_position_below_the_box_edge(zctx, N):
    """BoxSize 1 and coordinates at nextafter(1, 0): Pos / CellSize rounds up to exactly Nmesh (at 18 and 24, not at 16), which the readout
    must take as cell 0 with residual 0.  Eight particles, every choice of the axes at the edge, one mesh size per transform route."""
    edge = np.nextafter(1.0, 0.0)
    assert edge / (1.0 / N) == N
    inner = np.array([[0.3, 0.55, 0.71], [0.12, 0.91, 0.47], [0.66, 0.05, 0.38], [0.83, 0.29, 0.14],
                      [0.41, 0.77, 0.95], [0.58, 0.18, 0.62], [0.07, 0.49, 0.86], [0.24, 0.64, 0.02]])
    at_edge = np.array([(0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1), (1, 1, 0)], dtype=bool)
    pos = np.ascontiguousarray(np.where(at_edge, edge, inner))
    delta, growth = zr.tabulate_k2(_delta, N, 1.0), zr.tabulate_k2(_growth, N, 1.0)
    got = sq.displacement_fields(zctx, pos, N, 1.0, 181170, delta, growth, vel_prefac=37.5, ScaleDepVelocity=1)
    ref = zr.displacement_fields(N, 1.0, 181170, 0, 0, 37.5, 1, delta, growth, pos)
    _compare(got, ref, f"N {N} box edge", box=1.0)


def test_agrees_with_pm_apply(zctx):
    """the downloaded spectrum through shq_pm_apply with the library's own factor tables, and a numpy CIC readout of those meshes"""
    N = 24
    delta, growth = _tables(N)
    pos = np.random.default_rng(2).uniform(0, BOX, (3000, 3))
    got = sq.displacement_fields(zctx, pos, N, BOX, 5, delta, growth, vel_prefac=1.0, ScaleDepVelocity=True)
    spec = sq.zeldovich_field(zctx, N, 5)
    n = len(delta)
    dens, disp, vel = np.zeros(n), np.zeros(n), np.zeros(n)
    capi.check(capi.hip.shq_zeldovich_factor_tables(N, BOX, capi.ptr(delta), capi.ptr(growth), capi.ptr(dens), capi.ptr(disp), capi.ptr(vel)))

    def field(kind, axis, tab):
        tf = capi.PMTransfer(kind, axis, 0, 0, tab.ctypes.data)
        mesh = np.zeros((N, N, N))
        capi.check(capi.hip.shq_pm_apply(zctx.h, N, capi.ptr(spec), C.byref(tf), capi.ptr(mesh)))
        return zr.cic_readout(mesh, pos, N, BOX)

    ref = dict(Density=field(0, 0, dens), Disp=np.stack([field(1, a, disp) for a in range(3)], axis=1),
               Vel=np.stack([field(1, a, vel) for a in range(3)], axis=1))
    for name in ref:
        scale = np.abs(ref[name]).max()
        assert np.abs(got[name] - ref[name]).max() < BAR * scale, name


def test_resident_field_is_reused(zctx, ctx):
    N = 24
    pos, _ = sq.setup_grid(sq.IDGenerator(12, BOX), 0.0, 1.0)
    d0, g0 = _tables(N)
    d1, g1 = _tables(N, other=True)
    a = sq.displacement_fields(zctx, pos, N, BOX, 11, d0)
    assert a["phase_ms"][0] > 0 and a["phase_ms"][3] >= a["phase_ms"][1] > 0
    b = sq.displacement_fields(zctx, pos, N, BOX, 11, d1)           # another species, the same seed
    assert b["phase_ms"][0] == 0
    assert not np.array_equal(a["Disp"], b["Disp"])
    with sq.Context(0) as fresh:
        c = sq.displacement_fields(fresh, pos, N, BOX, 11, d1)
        assert c["phase_ms"][0] > 0
    for name in ("Pos", "Vel", "Density", "Disp"):
        assert np.array_equal(b[name], c[name]), name
    # refilled after the drop call and after a changed seed, flag or mesh
    capi.check(capi.hip.shq_zeldovich_drop_field(zctx.h))
    assert sq.displacement_fields(zctx, pos, N, BOX, 11, d1)["phase_ms"][0] > 0
    assert sq.displacement_fields(zctx, pos, N, BOX, 11, d1)["phase_ms"][0] == 0
    e = sq.displacement_fields(zctx, pos, N, BOX, 12, d1)
    assert e["phase_ms"][0] > 0 and not np.array_equal(e["Disp"], b["Disp"])
    assert sq.displacement_fields(zctx, pos, N, BOX, 12, d1, InvertPhase=True)["phase_ms"][0] > 0
    assert sq.displacement_fields(zctx, pos, 16, BOX, 12, _tables(16)[0], InvertPhase=True)["phase_ms"][0] > 0


def test_deterministic(zctx):
    N = 48
    delta, growth = _tables(N)
    pos = np.random.default_rng(8).uniform(0, BOX, (20000, 3))
    a = sq.displacement_fields(zctx, pos, N, BOX, 3, delta, growth, ScaleDepVelocity=True)
    capi.check(capi.hip.shq_zeldovich_drop_field(zctx.h))
    b = sq.displacement_fields(zctx, pos, N, BOX, 3, delta, growth, ScaleDepVelocity=True)
    for name in ("Pos", "Vel", "Density", "Disp", "maxdisp", "maxvel"):
        assert np.array_equal(a[name], b[name]), name


def test_bad_input_is_refused_before_anything_is_written(zctx):
    N = 16
    delta, growth = _tables(N)
    pos = np.random.default_rng(1).uniform(0, BOX, (100, 3))

    def call(N=N, pos=pos, delta=delta, growth=None, scaledep=0, box=BOX):
        zp = capi.ZeldovichParams(N, 1, 0, 0, scaledep, 0, box, 1.0)
        out = [np.full((len(pos), 3), 7.0), np.full((len(pos), 3), 7.0), np.full(len(pos), 7.0), np.full((len(pos), 3), 7.0)]
        md, mv = C.c_double(7.0), C.c_double(7.0)
        rc = capi.hip.shq_zeldovich_displacements(zctx.h, C.byref(zp), capi.ptr(delta), capi.ptr(growth), len(pos), capi.ptr(pos),
                                                  capi.ptr(out[0]), capi.ptr(out[1]), capi.ptr(out[2]), capi.ptr(out[3]), C.byref(md), C.byref(mv))
        untouched = all(np.all(o == 7.0) for o in out) and md.value == 7.0 and mv.value == 7.0
        return rc, untouched

    for bad in (BOX, -1e-9, np.nextafter(0.0, -1.0), np.nan, 2 * BOX):
        p = pos.copy()
        p[37, 1] = bad
        assert call(pos=p) == (ERR_INVALID, True), bad
    assert call(N=17, delta=np.ones(3 * 8 * 8 + 1)) == (ERR_INVALID, True)
    assert call(scaledep=1, growth=None) == (ERR_INVALID, True)
    assert call(box=0.0) == (ERR_INVALID, True)
    d = delta.copy()
    d[5] = np.inf
    assert call(delta=d) == (ERR_INVALID, True)
    rc, untouched = call(scaledep=1, growth=growth)
    assert rc == 0 and not untouched
    # positions just inside the box are fine, on both faces
    p = pos.copy()
    p[0] = (0.0, np.nextafter(BOX, 0.0), 0.0)
    assert call(pos=p)[0] == 0


def test_download_needs_a_resident_field(zctx):
    """what the header says is discarded: the resident field, by the drop call - and by nothing a displacement call with its key does"""
    N = 16
    spec = np.zeros((N, N // 2 + 1, N), dtype=np.complex128)
    assert capi.hip.shq_zeldovich_download_field(zctx.h, N, capi.ptr(spec)) == ERR_STATE
    sq.displacement_fields(zctx, np.zeros((1, 3)), N, BOX, 1, _tables(N)[0])
    capi.check(capi.hip.shq_zeldovich_download_field(zctx.h, N, capi.ptr(spec)))
    assert capi.hip.shq_zeldovich_download_field(zctx.h, 24, capi.ptr(spec)) == ERR_INVALID
    capi.check(capi.hip.shq_zeldovich_drop_field(zctx.h))
    assert capi.hip.shq_zeldovich_download_field(zctx.h, N, capi.ptr(spec)) == ERR_STATE


def test_no_interference_with_the_resident_step(zctx):
    """a resident particle set and tree, then shq_treepm_step: the same bits with a displacement call (another mesh size, then the PM's
    own) in between; and a finished PM result stays downloadable across the call"""
    ctx = zctx
    n, L, nmesh = 20**3, 1.0, 48
    pos = sq.synth_positions("cluster", n, L=L)
    pos = pos[sq.morton_order(pos, L)]
    pman = cm.make_partmanager(pos, box=L)
    tree = sq.force_tree_full(pman)
    sq.set_gravshort_treepar(ErrTolForceAcc=0.005, BHOpeningAngle=0.175, MaxBHOpeningAngle=0.9, TreeUseBH=0, Rcut=6.0)
    sq.gravshort_set_softenings(L / 20)
    gp = sq.make_grav_params(L, 1.5, nmesh, cm.G, cm.RHO0)
    pmp = sq.PMParams(nmesh, 0, L, 1.5, cm.G)
    rng = np.random.default_rng(11)
    pman.Base["FullTreeGravAccel"] = rng.standard_normal((n, 3)) * 50.0
    pman.Base["GravPM"] = rng.standard_normal((n, 3))
    lattice, _ = sq.setup_grid(sq.IDGenerator(12, BOX), 0.0, 1.0)

    def zel(N):
        sq.displacement_fields(ctx, lattice, N, BOX, 5, _tables(N)[0])

    def results():
        g = np.zeros((n, 3)); pp = np.zeros(n)
        capi.check(capi.hip.shq_pm_download(ctx.h, capi.ptr(g), capi.ptr(pp)))
        acc = np.zeros((n, 3)); pot = np.zeros(n); nint = np.zeros(n, dtype=np.int64)
        capi.check(capi.hip.shq_grav_short_download(ctx.h, capi.ptr(acc), capi.ptr(pot), capi.ptr(nint), C.byref(sq.WalkStats())))
        return g, pp, acc, pot, nint

    def run(with_zel):
        pv, tv = pman.view(), tree.view()
        capi.check(capi.hip.shq_particles_upload(ctx.h, C.byref(pv)))
        capi.check(capi.hip.shq_tree_upload(ctx.h, C.byref(tv)))
        if with_zel:
            zel(24)
            zel(48)
        capi.check(capi.hip.shq_treepm_step(ctx.h, C.byref(pmp), C.byref(gp), 1, sq.WALK_EXACT))
        first = results()
        if with_zel:
            zel(24)
            zel(18)
        return first, results()

    ref, ref_again = run(False)
    got, got_after = run(True)
    for a, b, c, name in zip(ref, got, got_after, ("GravPM", "PM potential", "acc", "pot", "ninteractions")):
        assert np.array_equal(a, b), name
        assert np.array_equal(a, c), name
