"""The numpy restatement of the lensing potential planes (lens_restated.py) pinned by hand: bins on their edges and the rounding that
decides them, the layout per normal, the potential of a single mode, empty planes, the defaults, and the neutrino correction's
overlap, transpose and bilinear add.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from shenqi_amd import capi
import lens_restated as lr

nb = np.nextafter
COSMO = dict(atime=0.5, comoving_distance=1.2e6, HubbleParam=0.7, omega_source=0.3, num_particles_tot=1000)


def _count(pos, normal, center, th, R=4, L=4.0, flags=None, types=None, excl=0, off=(0.0, 0.0, 0.0)):
    pos = np.asarray(pos, dtype=np.float64)
    flags = np.zeros(len(pos), np.uint8) if flags is None else np.asarray(flags, np.uint8)
    types = np.ones(len(pos), np.uint8) if types is None else np.asarray(types, np.uint8)
    return lr.count_plane(pos, flags, types, excl, L, off, normal, center, th, R)


def test_hand_counted_4x4():
    """L = 4, R = 4, normal 2, slab [1.5, 2.5]: positions at 0 and L (both wrap to bin 0), on bin edges and their neighbours"""
    pos = [(0.0, 0.0, 2.0),                      # x = 0 wraps to L, find_bin wraps L to 0: [0][0]
           (4.0, 4.0, 2.0),                      # [0][0]
           (1.0, nb(3.0, 0), 1.5),               # x on the edge of bin 1, y just below bin 3; z = centre - th/2 is inside: [1][2]
           (3.0, 3.0, 2.5),                      # z = centre + th/2: rel == width, dropped
           (3.0, 3.0, nb(2.5, 0)),               # just inside the upper edge: [3][3]
           (2.0, 1.0, nb(1.5, 0)),               # just below the slab: rel = -2^-52, + L rounds to L, wraps to 0: inside, [2][1]
           (2.0, 1.0, nb(1.5, 2)),               # [2][1]
           (0.5, 0.5, 3.0),                      # outside the slab
           (nb(4.0, 0), 0.5, 2.0),               # [3][0]
           (0.5, 0.5, 2.0),                      # swallowed: skipped
           (0.5, 0.5, 2.0),                      # garbage: counted [0][0]
           (0.5, 0.5, 2.0)]                      # Type 2: counted unless exclude_type2, [0][0]
    flags = [0] * 9 + [2, 1, 0]
    types = [1] * 11 + [2]
    want = np.zeros((4, 4), np.uint32)
    want[0, 0], want[1, 2], want[3, 3], want[2, 1], want[3, 0] = 4, 1, 1, 2, 1
    got = _count(pos, 2, 2.0, 1.0, flags=flags, types=types)
    assert np.array_equal(got, want)
    want[0, 0] = 3
    assert np.array_equal(_count(pos, 2, 2.0, 1.0, flags=flags, types=types, excl=1), want)


def test_slab_wrapping_through_the_box_edge():
    """centre 0.25, thickness 1: bins [-0.25, 0.75]; z = 3.75 gives rel = L exactly, which wraps to 0"""
    zs = [3.9, 3.7, 0.7, 0.75, 3.75, 0.0, nb(0.75, 0)]
    pos = [(2.5, 1.5, z) for z in zs]
    got = _count(pos, 2, 0.25, 1.0)
    assert got[2, 1] == 5 and got.sum() == 5      # 3.9, 0.7, 3.75, 0 (-> L -> rel 4.25 - 4), nextafter(0.75, 0)


def test_offset_is_removed_before_binning():
    got = _count([(4.5, 0.5, 2.0)], 2, 2.0, 1.0, off=(1.0, 0.0, 0.0))   # x - 1 = 3.5: bin 3
    assert got[3, 0] == 1 and got.sum() == 1
    got = _count([(0.5, 0.5, 2.0)], 2, 2.0, 1.0, off=(1.0, 0.0, 0.0))   # x - 1 = -0.5 -> 3.5
    assert got[3, 0] == 1


def test_layout_per_normal():
    pos = [(0.5, 1.5, 2.5)]
    for normal, ij in ((0, (1, 2)), (1, (0, 2)), (2, (0, 1))):     # [y][z], [x][z], [x][y]
        got = _count(pos, normal, 2.0, 4.0)
        assert got[ij] == 1 and got.sum() == 1, normal


def test_single_cosine_mode_gives_the_filter_factor():
    R, b, chi = 16, 0.25, 3.0
    i, j = np.meshgrid(np.arange(R), np.arange(R), indexing="ij")
    dens = np.cos(2 * np.pi * (3 * i + 2 * j) / R)
    l2 = (3.0 / R) ** 2 + (2.0 / R) ** 2
    f = -2.0 * (b * b / (chi * chi)) / (l2 * 4 * np.pi ** 2) * np.exp(-0.5 * (2 * np.pi) ** 2 * l2)
    pot = lr.lensing_potential(dens, b, b, chi)
    assert np.allclose(pot, f * dens, rtol=0, atol=1e-13 * abs(f))


def test_nyquist_row_for_even_R():
    R = 8
    l2 = lr.l_squared(R)
    assert l2[R // 2, 0] == 0.25 and l2[0, R // 2] == 0.25 and l2[0, 0] == 1.0
    dens = np.cos(np.pi * np.arange(R))[:, None] * np.ones((1, R))       # (-1)^i: the Nyquist row alone
    f = -2.0 * 1.0 / (0.25 * 4 * np.pi ** 2) * np.exp(-0.5 * (2 * np.pi) ** 2 * 0.25)
    assert np.allclose(lr.lensing_potential(dens, 1.0, 1.0, 1.0), f * dens, rtol=0, atol=1e-13 * abs(f))


def test_dc_is_dropped_and_an_empty_plane_is_zero():
    assert np.abs(lr.lensing_potential(np.full((6, 6), 7.0), 1.0, 1.0, 1.0)).max() < 1e-13
    pot, n = lr.particle_plane(np.zeros((5, 5), np.uint32), dict(BoxSize=4.0, Thickness=1.0), COSMO, 2)
    assert n == 0 and not pot.any()
    p = dict(BoxSize=4.0, Resolution=4, Normals=[2], CutPoints=[2.0], Thickness=1.0)
    planes, npl, counts = lr.lens_planes(np.array([[1.0, 1.0, 0.5]]), [0], [1], p, COSMO)
    assert npl[0, 0] == 0 and not planes.any() and not counts.any()


def test_normalisation_of_one_plane():
    """density = counts / N_tot * L^3 / (b0 b1 b2); the potential scales with 1.5 H0^2 Omega / c^2 * th * chi * (kpc/h)^2 / a"""
    assert lr.norm_factor(1000, 4.0, 4, 0.5, 1) == 1. / 1000 * (64.0 / (1.0 * 0.5 * 1.0))
    H0 = 100 * 0.7 * 3.2407793e-20
    assert lr.cosmo_normalization(0.7, 0.3) == 1.5 * H0 ** 2 * 0.3 / 2.99792458e10 ** 2
    assert lr.density_normalization(0.5, 2.0, 0.7, 0.25) == 0.5 * 2.0 * (3.085678e21 / 0.7) ** 2 / 0.25


def test_default_cut_list_and_thickness():
    assert lr.default_cuts(100.0, 30.0) == (30.0, [15.0, 45.0, 75.0])
    assert lr.default_cuts(100.0, 0.0) == (100.0, [50.0])
    assert lr.default_cuts(100.0, -5.0) == (100.0, [50.0])
    assert lr.default_cuts(100.0, 150.0) == (150.0, [])
    # Thickness <= 0: one slab of the whole box takes every active particle
    rng = np.random.default_rng(1)
    pos = rng.uniform(0, 4.0, (200, 3))
    p = dict(BoxSize=4.0, Resolution=4, Normals=[2, 0], CutPoints=None, Thickness=0.0)
    planes, npl, counts = lr.lens_planes(pos, np.zeros(200, np.uint8), np.ones(200, np.uint8), p, COSMO)
    assert counts.shape == (1, 2, 4, 4) and np.all(npl == 200)
    h = np.histogram2d(pos[:, 0], pos[:, 1], bins=4, range=[[0, 4], [0, 4]])[0]
    assert np.array_equal(counts[0, 0], h.astype(np.uint32))


@pytest.mark.parametrize("box,th,ncuts", [(100.0, 30.0, 3), (100.0, 0.0, 1), (100.0, -1.0, 1), (100.0, 150.0, 0), (64.0, 16.0, 4)])
def test_library_default_cut_count(box, th, ncuts):
    """shq_lens_num_cuts (host only) agrees with write_plane's default list"""
    lp = capi.LensParams()
    lp.Resolution, lp.ncuts, lp.nnormals, lp.Thickness, lp.BoxSize = 8, 0, 1, th, box
    n = C.c_int32(-1)
    capi.check(capi.hip.shq_lens_num_cuts(C.byref(lp), C.byref(n)))
    assert n.value == ncuts == len(lr.default_cuts(box, th)[1])
    lp.ncuts = 5
    capi.check(capi.hip.shq_lens_num_cuts(C.byref(lp), C.byref(n)))
    assert n.value == 5


def test_slab_overlap_by_hand():
    L = 10.0
    assert lr.slab_overlap(4.0, 1.0, 5.0, 2.0, L) == 1.0          # slab [4, 6]
    assert lr.slab_overlap(3.0, 1.0, 5.0, 2.0, L) == 0.0
    assert lr.slab_overlap(0.0, 1.0, 0.5, 2.0, L) == 1.0          # slab [-0.5, 1.5]
    assert lr.slab_overlap(1.0, 1.0, 0.5, 2.0, L) == 0.5
    assert lr.slab_overlap(9.0, 1.0, 0.5, 2.0, L) == 0.5          # the periodic image [9.5, 11.5]
    assert lr.slab_overlap(9.0, 1.0, -9.5, 2.0, L) == 0.5         # the centre wraps to 0.5 first
    assert lr.slab_overlap(5.0, 1.0, 5.25, 0.5, L) == 0.5         # slab [5, 5.5] inside one cell
    assert lr.slab_overlap(3.0, 1.0, 5.0, 10.0, L) == 1.0         # thickness >= L: the cell size
    assert lr.slab_overlap(3.0, 0.25, 5.0, 12.0, L) == 0.25
    assert list(lr.overlap_table(10, L, 5.0, 2.0)) == [0, 0, 0, 0, 1, 1, 0, 0, 0, 0]


def test_correction_projection_of_normal_1_is_transposed():
    """a mesh that varies along x only: the normal-1 projection is [z][x], so it varies along its SECOND index"""
    N, L = 6, 6.0
    real = np.broadcast_to(np.arange(N, dtype=np.float64)[:, None, None], (N, N, N)).copy()
    proj = lr.project_correction(real, 0, N, 0.5, 2.0, L, 1, 3.0, L)         # thickness = L: weight = cellsize = 1
    want = N * np.arange(N) * 0.5 / 2.0 * 1.0 / L                            # sum over y of delta * cellsize / th
    assert np.allclose(proj, np.broadcast_to(want[None, :], (N, N)), rtol=1e-15, atol=0)
    p0 = lr.project_correction(real, 0, N, 0.5, 2.0, L, 0, 3.0, L)          # normal 0 sums over x: constant
    assert np.allclose(p0, N * (N - 1) / 2 * 0.25 / L)
    p2 = lr.project_correction(real, 0, N, 0.5, 2.0, L, 2, 3.0, L)          # normal 2: [x][y], varies along the FIRST index
    assert np.allclose(p2, np.broadcast_to(want[:, None], (N, N)))
    # an x-slab only fills its own columns (normal 1) / rows (normal 2)
    s1 = lr.project_correction(real[2:4], 2, N, 0.5, 2.0, L, 1, 3.0, L)
    assert np.array_equal(s1[:, 2:4], proj[:, 2:4]) and not s1[:, :2].any() and not s1[:, 4:].any()


def test_bilinear_add_of_a_constant():
    for R, N in ((7, 3), (8, 8), (45, 32), (2, 48)):
        dst = np.full((R, R), 1.5)
        lr.bilinear_add(dst, np.full((N, N), 2.5))
        assert np.allclose(dst, 4.0, rtol=1e-15, atol=0), (R, N)
    # an identity resampling at equal sizes
    src = np.random.default_rng(0).random((8, 8))
    assert np.allclose(lr.bilinear_add(np.zeros((8, 8)), src), src, rtol=0, atol=1e-15)


def test_activity():
    assert list(lr.is_active([0, 1, 2, 3, 0], [1, 1, 1, 1, 2], 0)) == [True, True, False, False, True]
    assert list(lr.is_active([0, 1, 2, 3, 0], [1, 1, 1, 1, 2], 1)) == [True, True, False, False, False]
