"""Host side of the excursion-set reionisation: shq_uvbg_filter_table against glibc (the table the device multiplies by must hold the
reference's filter_pm values bit for bit) and the restatement's radius schedule against hand-worked cases."""
import math

import numpy as np
import pytest

from shenqi_amd import capi
import uvbg_restated as ur


def _lib_table(ftype, N, L, R):
    t = np.full(3 * (N // 2) ** 2 + 1, np.nan)
    capi.check(capi.hip.shq_uvbg_filter_table(ftype, N, L, R, capi.ptr(t)), "shq_uvbg_filter_table")
    return t


@pytest.mark.parametrize("ftype", [0, 1, 2])
@pytest.mark.parametrize("N", [32, 64])
def test_filter_table_is_glibc_bit_for_bit(ftype, N):
    L = 20000.0
    for R in (L, 20000.0 / 1.1 ** 7, 1234.5, 1.7 * L / N, L / N):
        got, want = _lib_table(ftype, N, L, R), ur.filter_table(ftype, N, L, R)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (ftype, N, R, int(np.sum(got != want)))
    if ftype == 0:
        assert got[0] == 1.0 and np.any(got < 0)          # kR <= 1e-4 keeps the mode; the top-hat's side lobes are negative
    if ftype == 1:
        assert set(np.unique(got)) <= {0.0, 1.0} and got[-1] == 0.0


def test_filter_table_rejects_bad_arguments():
    t = np.zeros(3 * 16 ** 2 + 1)
    assert capi.hip.shq_uvbg_filter_table(3, 32, 1.0, 1.0, capi.ptr(t)) == 1
    assert capi.hip.shq_uvbg_filter_table(0, 32, 0.0, 1.0, capi.ptr(t)) == 1
    assert capi.hip.shq_uvbg_filter_table(0, 32, 1.0, 1.0, None) == 1


def test_radius_schedule_box_cap():
    # ReionRBubbleMax above the box: the first radius is BoxSize; 100 / 2^k down to the cell (12.5): 100, 50, 25, then the cell
    assert ur.radius_schedule(1e6, 0.0, 2.0, 100.0, 12.5) == [100.0, 50.0, 25.0, 12.5]


def test_radius_schedule_rmin_stop():
    # R / Rdelta < Rmin ends it before the cell size does: 64, 32, and at 16 (16 / 2 = 8 < 10) the test fires before 16 is used:
    # the last step is the unfiltered cell instead
    assert ur.radius_schedule(64.0, 10.0, 2.0, 1000.0, 1.0) == [64.0, 32.0, 1.0]


def test_radius_schedule_cellsize_stop():
    # Rmin below the cell: the cell stops it; 30, 20, 13.33.. (13.33 / 1.5 = 8.88 >= 8), then at 8.88 (8.88 / 1.5 < 8) R = CellSize
    r = ur.radius_schedule(30.0, 1.0, 1.5, 1000.0, 8.0)
    assert r == [30.0, 30.0 / 1.5, 30.0 / 1.5 / 1.5, 8.0]
    # one step only: the first radius already sits below Rmin * Rdelta: the loop runs the unfiltered step alone
    assert ur.radius_schedule(5.0, 4.0, 2.0, 1000.0, 1.0) == [1.0]


def test_radius_schedule_default_parameters():
    # the defaults (params.cpp:326-328) at 64^3 in a 100 Mpc/h box: 27 radii, 42 at 256^3 and 512^3 (petapm.cpp:536-606)
    for N, L, want in ((64, 100000.0, 27), (256, 100000.0, 42), (512, 100000.0, 42)):
        assert len(ur.radius_schedule(20340.0, 406.8, 1.1, L, L / N)) == want
    assert math.isclose(ur.radius_schedule(20340.0, 406.8, 1.1, 100000.0, 100000.0 / 64)[-1], 100000.0 / 64)
