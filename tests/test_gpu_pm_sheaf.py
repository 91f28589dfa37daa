"""Every compiled size of the bespoke PM FFT (csrc/fft3d.hip) against an independent reference, through the C-ABI.

The particle load (tests/pm_sheaf.py) lies on lines along an integer direction d, which makes the PM problem two-dimensional:
the reference is one N x N numpy fft2 / ifft2 pair with the Green's function of tests/cpu_ops.py, whatever the mesh size.  2^17
probes of MASS ZERO at random positions deposit nothing (the library accepts them) and are read out like every particle, so the
potential mesh is sampled densely; the lines' own particles are compared too.  tests/test_pm_sheaf_cpu.py checks the reduction
against a dense numpy PM and the row coverage of every load used here.

Bounds, from test_pm_parity_16 and test_pm_power_spectrum, the same at every size: GravPM and the PM potential 1e-10 of the
reference's maximum, power[] 1e-9.  Measured on an MI355X (the table in DESIGN 3.2, "Every compiled size against the sheaf
reference"): the PM potential is within 2.0e-15 of its maximum at every size; GravPM's error grows in proportion to Nmesh (a difference
of potentials one cell apart) from 7.6e-16 at 16 to 8.5e-14 at 1536; power[] within 9.1e-15 of the largest bin.  The nearest any
case comes to its bound is a factor 1200 (GravPM at 1536).  Every case prints its figures (pytest -s)."""
import ctypes as C
import functools

import numpy as np
import pytest

import shenqi_amd as sq
from shenqi_amd import capi
import common as cm
import orc
import pm_sheaf as ps

pytestmark = pytest.mark.gpu

ASMTH, G = 1.5, cm.G
TOL_FORCE = 1e-10        # test_pm_parity_16: GravPM and the PM potential, of the reference's maximum
TOL_POWER = 1e-9         # test_pm_power_spectrum
ASMTH_SHORT = 0.25       # cells: exp(-k^2 Asmth^2) is 0.54 at the Nyquist frequency, where Asmth = 1.5 leaves 2e-10
SIZES = ps.compiled_sizes()
INPLACE_SIZES = [32, 64, 80, 128, 256, 768, 960, 1152, 1200, 1536]     # the ones the older bit test leaves out
SPLIT_SIZES = [48, 768, 960, 1024, 1200, 1536]
SLAB_SIZES = [48, 768, 960, 1024, 1200]
SHIFT_SIZES = [960, 1024, 1200]


@functools.lru_cache(maxsize=3)
def _case(N, d, shift=None, modefac=False, asmth=ASMTH):
    """the sheaf, its GravPM and PM potential by the reduction: computed once per case, shared, never written to"""
    sh = ps.gpu_case(N, d)
    if shift is not None:
        sh = sh.shifted(shift)
    g, pot = ps.reduced_reference(sh, asmth, G, modefac=ps.mode_factor(N) if modefac else None)
    for a in (sh.pos, sh.mass, g, pot):
        a.flags.writeable = False
    return sh, g, pot


def _upload(ctx, sh):
    pman = cm.make_partmanager(sh.pos, box=float(sh.N), mass=sh.mass)
    pv = pman.view()
    capi.check(capi.hip.shq_particles_upload(ctx.h, C.byref(pv)))
    return pman


def _download(ctx, n):
    g = np.zeros((n, 3)); pot = np.zeros(n)
    capi.check(capi.hip.shq_pm_download(ctx.h, capi.ptr(g), capi.ptr(pot)))
    return g, pot


def _check(tag, N, d, got, ref):
    """both arrays of all particles, lines and probes, against the reduction"""
    (g, pot), (rg, rpot) = got, ref
    eg = float(np.abs(g - rg).max() / np.abs(rg).max())
    ep = float(np.abs(pot - rpot).max() / np.abs(rpot).max())
    print(f"sheaf {tag} N={N} d={d}: GravPM err {eg:.2e} PM potential err {ep:.2e} of the maximum")
    assert np.all(np.isfinite(g)) and np.all(np.isfinite(pot))
    assert eg < TOL_FORCE, (tag, N, d, eg)
    assert ep < TOL_FORCE, (tag, N, d, ep)


@pytest.mark.parametrize("N,d", [pytest.param(N, d, id=f"{N}-{d[0]}_{d[1]}_{d[2]}")
                                 for N, d in ps.gpu_cases() + [(36, d) for d in ps.DIAGONALS] + [(100, d) for d in ps.DIAGONALS]])
def test_pm_run_at_every_compiled_size(ctx, N, d):
    """shq_pm_run on the transposing pipeline at every size shq_fft3d_supported lists (the list is asked of the library: a new
    size is tested, or fails, without an edit here), d = (1, 1, 1) and (1, -1, 1): 92 % of the excited modes have all of kx, ky, kz
    non-zero and every line of the spectrum along every axis holds exactly one.  The axis directions at 48, 768, 960 and 1024 put the
    spectrum on the kz = 0 (resp. kx = 0) plane: the z' = 0 column and the DC lines of the two-for-one passes.  36 and 100 have no
    bespoke transform: the hipFFT route through the same check."""
    assert (capi.hip.shq_pm_slab_pitch(N) != 0) == (N not in (36, 100))
    sh, rg, rpot = _case(N, d)
    pman = _upload(ctx, sh)
    pmp = sq.PMParams(N, 0, float(N), ASMTH, G)
    capi.check(capi.hip.shq_pm_run(ctx.h, C.byref(pmp)))
    _check("run", N, d, _download(ctx, len(sh.pos)), (rg, rpot))
    del pman


def test_every_compiled_size_is_listed():
    """the sizes the issue of this test counted; one more in shq_fft3d_supported extends the run above by itself"""
    assert set(SIZES) >= {16, 24, 32, 40, 48, 64, 80, 96, 128, 192, 256, 384, 512, 768, 960, 1024, 1152, 1200, 1536}
    assert set(INPLACE_SIZES + SPLIT_SIZES + SLAB_SIZES + SHIFT_SIZES) <= set(SIZES)


@pytest.mark.parametrize("N", INPLACE_SIZES)
def test_in_place_pipeline_gives_the_transposing_pipelines_bits(ctx, N):
    """the same call on the in-place pipeline (shq_pm_set_fft_transposed(0)): bit-equal to the transposing one, at the sizes
    test_pm_transposing_fft_pipeline_gives_the_in_place_pipelines_bits does not run - and both against the reduction.  A run with
    -G after each download replaces the result on the device, so the second download cannot be the first run's arrays."""
    d = (1, 1, 1)
    sh, rg, rpot = _case(N, d)
    pman = _upload(ctx, sh)
    pmp = sq.PMParams(N, 0, float(N), ASMTH, G)
    flipped = sq.PMParams(N, 0, float(N), ASMTH, -G)
    got = {}
    try:
        for mode in (1, 0):
            capi.check(capi.hip.shq_pm_set_fft_transposed(ctx.h, mode))
            capi.check(capi.hip.shq_pm_run(ctx.h, C.byref(pmp)))
            got[mode] = _download(ctx, len(sh.pos))
            # the device's arrays now hold the other sign: an in-place run that wrote nothing cannot pass on what this one left
            capi.check(capi.hip.shq_pm_run(ctx.h, C.byref(flipped)))
    finally:
        capi.check(capi.hip.shq_pm_set_fft_transposed(ctx.h, 1))
    _check("in-place", N, d, got[0], (rg, rpot))
    for a, b, name in zip(got[0], got[1], ("GravPM", "PM potential")):
        assert np.array_equal(a, b), (name, N, float(np.abs(a - b).max()))
    del pman


@pytest.mark.parametrize("N", SPLIT_SIZES)
def test_split_x_pass_with_a_mode_factor(ctx, N):
    """shq_pm_forward, shq_pm_set_mode_factor with T = 1 + 0.3 tanh(log k), the finish by shq_pm_run (fft_t_tile MODES 3 and 4):
    forces against the reduction with the same T; power[] of the forward against the sums restated for the excited modes, norm
    against (sum of the masses)^2.  nmodes and kk do not depend on the input: compared, against the dense count, at 48 only."""
    d = (1, -1, 1)
    sh, rg, rpot = _case(N, d, None, True)
    pman = _upload(ctx, sh)
    pmp = sq.PMParams(N, 0, float(N), ASMTH, G)
    T = ps.mode_factor(N)
    capi.check(capi.hip.shq_pm_forward(ctx.h, C.byref(pmp)))
    kk = np.zeros(N); power = np.zeros(N); nmodes = np.zeros(N, dtype=np.int64); norm = C.c_double()
    capi.check(capi.hip.shq_pm_download_power(ctx.h, N, capi.ptr(kk), capi.ptr(power), capi.ptr(nmodes), C.byref(norm)))
    capi.check(capi.hip.shq_pm_set_mode_factor(ctx.h, N, capi.ptr(T)))
    capi.check(capi.hip.shq_pm_run(ctx.h, C.byref(pmp)))
    got = _download(ctx, len(sh.pos))
    rpower, rnorm = ps.power_sums(sh)
    epw = float(np.abs(power - rpower).max() / rpower.max())
    msum2 = float(sh.mass.sum()) ** 2
    print(f"sheaf split N={N}: power err {epw:.2e} of the maximum, norm err {abs(norm.value - msum2) / msum2:.2e}")
    _check("split", N, d, got, (rg, rpot))
    assert epw < TOL_POWER, (N, epw)
    assert abs(norm.value - msum2) < 1e-10 * msum2 and abs(rnorm - msum2) < 1e-10 * msum2
    if N <= 96:
        okk, _, onmodes, _ = orc.power_spectrum(np.zeros((N, N, N)), N)
        assert np.array_equal(nmodes, onmodes) and np.abs(kk - okk).max() < 1e-10 * okk.max()
    del pman


@pytest.mark.parametrize("N", SLAB_SIZES)
def test_unsharded_slab_pipeline(ctx, N):
    """the slab passes on one rank (run_n stages YZ_FORWARD, X_SOLVE, YZ_INVERSE): one torch buffer [N][N][zp], xoff = 0, nalloc = N, through deposit,
    (y, z) forward, the X pass with the Green's function, (y, z) inverse and the readout - against the reduction and bit-equal to the undivided PM, which
    runs after it, at every size"""
    import torch
    d = (1, 1, 1)
    sh, rg, rpot = _case(N, d)
    pman = _upload(ctx, sh)
    pmp = sq.PMParams(N, 0, float(N), ASMTH, G)
    zp = int(capi.hip.shq_pm_slab_pitch(N))
    assert zp >= N + 2
    # whatever an earlier run left in the device's GravPM / PM potential is replaced by the other sign first: a slab chain or a
    # slab readout that wrote nothing cannot pass on it; the undivided PM runs after the slab result is down
    capi.check(capi.hip.shq_pm_run(ctx.h, C.byref(sq.PMParams(N, 0, float(N), ASMTH, -G))))
    buf = torch.empty((N, N, zp), dtype=torch.int64, device="cuda:0")
    p = C.c_void_p(buf.data_ptr())
    torch.cuda.synchronize()
    try:
        capi.check(capi.hip.shq_pm_slab2_deposit(ctx.h, C.byref(pmp), 0, N, 0, N, p))
        capi.check(capi.hip.shq_pm_slab2_fft_yz(ctx.h, N, p, N, 0))
        capi.check(capi.hip.shq_pm_slab2_xgreen(ctx.h, C.byref(pmp), p, 0, N))
        capi.check(capi.hip.shq_pm_slab2_fft_yz(ctx.h, N, p, N, 1))
        capi.check(capi.hip.shq_pm_slab2_readout(ctx.h, C.byref(pmp), 0, N, 0, N, p))
        got = _download(ctx, len(sh.pos))
    finally:
        ctx.synchronize()
        del buf
    _check("slab", N, d, got, (rg, rpot))
    capi.check(capi.hip.shq_pm_run(ctx.h, C.byref(pmp)))
    whole = _download(ctx, len(sh.pos))
    same = all(np.array_equal(a, b) for a, b in zip(got, whole))
    print(f"sheaf slab N={N}: bit-equal to the undivided PM: {same}, "
          f"GravPM differs by {float(np.abs(got[0] - whole[0]).max() / np.abs(whole[0]).max()):.2e}")
    assert same, N
    del pman


@pytest.mark.parametrize("N", SHIFT_SIZES)
def test_translated_load_crosses_the_last_tiles(ctx, N):
    """every particle moved by one seeded integer vector with all components within the last 2 FFT_C = 8 cells of their axis:
    line 0, which starts in cell (0, 0) at r-cell 0, and the lines after it then start inside the last tile of each axis - ragged
    at 960 and 1200 - and run across the box boundary; against the reduction of the moved set.  Run twice: with Asmth = 1.5 cells
    the Green's function damps a mode at the Nyquist frequency by exp(-pi^2 1.5^2) = 2e-10, and a last tile of the half spectrum
    (z' = N / 2) read from the wrong place passed every force check here (tried on a scratch build at 960); with Asmth = 0.25 cells
    0.54 of such a mode is left and it counts."""
    d = (1, -1, 1)
    shift = tuple(int(N - 1 - x) for x in np.random.default_rng(N).integers(0, 8, 3))
    sh, rg, rpot = _case(N, d, shift)
    pman = _upload(ctx, sh)
    pmp = sq.PMParams(N, 0, float(N), ASMTH, G)
    capi.check(capi.hip.shq_pm_run(ctx.h, C.byref(pmp)))
    _check(f"shift {shift}", N, d, _download(ctx, len(sh.pos)), (rg, rpot))
    _, rg, rpot = _case(N, d, shift, False, ASMTH_SHORT)
    capi.check(capi.hip.shq_pm_run(ctx.h, C.byref(sq.PMParams(N, 0, float(N), ASMTH_SHORT, G))))
    _check(f"shift {shift} Asmth {ASMTH_SHORT}", N, d, _download(ctx, len(sh.pos)), (rg, rpot))
    del pman


# ---- the launch plans a context keeps per mesh size (shq_context::fft_plans)

PLAN_D = (1, 1, 1)


def _plan_run(c, N, transposed):
    """shq_pm_run of the sheaf (N, PLAN_D) on context c, checked against the reduction: what it downloads"""
    sh, rg, rpot = _case(N, PLAN_D)
    pman = _upload(c, sh)
    capi.check(capi.hip.shq_pm_set_fft_transposed(c.h, transposed))
    capi.check(capi.hip.shq_pm_run(c.h, C.byref(sq.PMParams(N, 0, float(N), ASMTH, G))))
    got = _download(c, len(sh.pos))
    _check(f"plans transposed={transposed}", N, PLAN_D, got, (rg, rpot))
    del pman
    return got


def _same_bits(a, b, what):
    for x, y, name in zip(a, b, ("GravPM", "PM potential")):
        assert np.array_equal(x, y), (what, name, float(np.abs(x - y).max()))


def _two_contexts(dev_b, transposed):
    """context A on device 0 and B on dev_b, alive together: A at 16, B at 24, A at 24, B at 16, each bit-equal to a fresh
    context of its device that has run nothing else"""
    fresh = {}
    for dev in {0, dev_b}:
        for N in (16, 24):
            with sq.Context(dev) as c:
                fresh[dev, N] = _plan_run(c, N, transposed)
    with sq.Context(0) as a, sq.Context(dev_b) as b:
        for c, dev, N in ((a, 0, 16), (b, dev_b, 24), (a, 0, 24), (b, dev_b, 16)):
            _same_bits(_plan_run(c, N, transposed), fresh[dev, N], (dev, N, transposed))


@pytest.mark.parametrize("transposed", [1, 0], ids=["transposing", "in_place"])
def test_two_contexts_keep_their_own_launch_plans(transposed):
    """two contexts alive at once, each at mesh 16 and 24 in turn, on either pipeline.  Both sit on device 0 here, where the
    plans of one context would serve the other as well: this also passed while the resident-workgroup counts were statics of
    fft3d.hip, and guards the per-context table from now on."""
    _two_contexts(0, transposed)


def test_one_context_keeps_a_plan_per_mesh_size():
    """meshes 16, 40, 16 on one context: the third result has the first one's bits.  40 has a radix-5 stage and another LDS size, so
    a plan reused across sizes would launch with the wrong dynamic LDS at least.  The statics this table replaces were per mesh
    size too: this passed before it."""
    with sq.Context(0) as c:
        first = _plan_run(c, 16, 1)
        _plan_run(c, 40, 1)
        _same_bits(_plan_run(c, 16, 1), first, "16 after 40")


@pytest.mark.parametrize("transposed", [1, 0], ids=["transposing", "in_place"])
def test_two_contexts_on_two_devices_keep_their_own_launch_plans(transposed):
    """the two-context test with the second context on device 1, which got the first device's CU count and no
    hipFuncSetAttribute call of its own while the counts were statics: the one case here that could fail before the table"""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs torch.cuda.device_count() > 1: the second context sits on device 1")
    _two_contexts(1, transposed)
