"""The host half of the light cone (shq_lightcone_horizon / _init / _set_time, sq.lightcone_table) against the restatement of
libgadget/lightcone.cpp in lightcone_restated.py, bit for bit, and the conditions the shared cases must meet for the GPU test to mean
something.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import shenqi_amd as sq
from shenqi_amd import capi
import lightcone_restated as lr

DH = 2997.92458
TIMEBEGIN = 0.005


@pytest.fixture(scope="module")
def eds():
    return lr.eds_table(TIMEBEGIN, DH)


def table_struct(tab_loga, tab_Dc, dloga):
    return capi.LightconeTable(tab_loga.ctypes.data, tab_Dc.ctypes.data, len(tab_loga), 0, dloga)


def bits(x):
    return np.float64(x).view(np.uint64)


# ---- horizon ----------------------------------------------------------------------------------------------------------------------------

def test_horizon_equals_the_restatement_bit_for_bit(eds):
    la, dc, dl = eds
    rng = np.random.default_rng(lr.SEED)
    points = [1e-4, TIMEBEGIN * 0.999, TIMEBEGIN, 1.0, 1.0 + 1e-12, 1.5, 40.0]          # below the table, its ends, above 1
    points += [math.exp(la[i]) for i in (0, 1, 2, 17, 2048, 4094, 4095)]                # at nodes (to rounding: either side of one)
    points += list(np.exp(rng.uniform(math.log(TIMEBEGIN), 0.0, size=200)))
    t = table_struct(la, dc, dl)
    out = C.c_double()
    for a in points:
        assert capi.hip.shq_lightcone_horizon(C.byref(t), float(a), C.byref(out)) == 0
        assert bits(out.value) == bits(lr.horizon(la, dc, dl, float(a))), a
        assert sq.lightcone_horizon(la, dc, float(a), dloga=dl) == out.value
    assert lr.horizon(la, dc, dl, 1e-4) == dc[0] and lr.horizon(la, dc, dl, 1.5) == dc[-1] == 0.0
    assert capi.hip.shq_lightcone_horizon(C.byref(t), 0.0, C.byref(out)) == capi.ERR_INVALID
    assert capi.hip.shq_lightcone_horizon(None, 0.5, C.byref(out)) == capi.ERR_INVALID


# ---- state ------------------------------------------------------------------------------------------------------------------------------

# crosses zmax = 80 (a = 1 / 81), ReferenceRedshift = 2 (a = 1 / 3) and zmin = 0.1 (a = 1 / 1.1); 0.3 is repeated
SEQUENCE = (0.008, 0.012, 0.0125, 0.05, 0.2, 0.3, 0.3, 0.34, 0.6, 0.9, 0.95, 1.0)
BOX = 400.0


def test_set_time_equals_the_restatement_over_a_run(eds):
    la, dc, dl = eds
    lc = sq.Lightcone(la, dc, BOX, dloga=dl)
    want = lr.init_state(la, dc, dl)
    assert bytes(lc._state) == want.bytes() and want.HorizonDistanceRef > 0
    first = True
    kinds = set()
    for a in SEQUENCE:
        before = bytes(lc._state)
        lc.set_time(a)
        lr.set_time(want, la, dc, dl, a, BOX)
        now = bytes(lc._state)
        assert now == want.bytes(), a
        z = 1 / a - 1
        if 0.1 < z < 80.0:
            if first:
                assert lc.state.HorizonDistancePrev == 0 and lc.state.HorizonDistance2Prev == 0   # nothing can cross yet
                first = False
            assert 0 < lc.state.Nreplica <= lr.MAXREPLICA and lc.state.SampleFraction > 0
            kinds.add("full" if z < 2.0 else "sampled")
            assert (lc.state.SampleFraction == 1.0) == (z < 2.0)
        else:                                           # only SampleFraction moves
            off = capi.LightconeState.SampleFraction.offset
            assert lc.state.SampleFraction == 0.0
            assert now[:off] == before[:off] and now[off + 8:] == before[off + 8:]
            kinds.add("outside")
    assert kinds == {"full", "sampled", "outside"}
    v = lc.state
    assert v.Reps.shape == (v.Nreplica, 3) and not v.Reps.flags.writeable


def test_the_1001st_replica_is_refused():
    """BoxBoost and H are chosen by counting: 23 boxes a side and H = 27.094 have exactly 1000 straddling boxes, 24 and 29.156 have 1003
    (no pair in reach has 1001 exactly: the count moves in steps).  The horizon comes out of the table by its lower clamp, so H is exact."""
    for boost, H, ok in ((23, 27.094, True), (24, 29.156, False)):
        count = lr.count_straddling(H, 1.0, boost)
        assert count == 1000 if ok else count >= 1001
        la = np.array([math.log(0.5), 0.0])
        dc = np.array([H, 0.0])
        dl = -la[0]
        t = table_struct(la, dc, dl)
        p = capi.LightconeParams(0.1, 80.0, 2.0, boost, 0)
        s = capi.LightconeState()
        assert capi.hip.shq_lightcone_init(C.byref(t), C.byref(p), C.byref(s)) == 0
        rc = capi.hip.shq_lightcone_set_time(C.byref(t), C.byref(p), 0.1, 1.0, C.byref(s))
        want = lr.State(s.HorizonDistanceRef)
        if ok:
            lr.set_time(want, la, dc, dl, 0.1, 1.0, BoxBoost=boost)
            assert rc == 0 and s.Nreplica == 1000 and s.HorizonDistance == H and bytes(s) == want.bytes()
        else:
            with pytest.raises(lr.TooManyReplica):
                lr.set_time(want, la, dc, dl, 0.1, 1.0, BoxBoost=boost)
            assert rc == capi.ERR_INVALID and b"too many replica" in capi.hip.shq_last_error()


# ---- table helper -------------------------------------------------------------------------------------------------------------------------

def test_lightcone_table_matches_the_closed_form():
    """Einstein-de Sitter: E = a^-3/2, Dc = 2 DH (1 - sqrt(a)).  The integrand is entire in log a, so the 64-point rule leaves rounding only;
    the last entry is the empty interval."""
    la, dc, dl = sq.lightcone_table(lambda a: a ** -1.5, TIMEBEGIN, DH, nentry=512)
    wla, wdc, wdl = lr.eds_table(TIMEBEGIN, DH, nentry=512)
    assert dl == wdl and np.array_equal(la, wla) and dc[-1] == 0.0
    exact = 2.0 * DH * (-np.expm1(0.5 * la))          # 1 - sqrt(a) without the cancellation near a = 1
    assert np.all(np.abs(dc[:-1] - exact[:-1]) <= 1e-12 * exact[:-1])


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------

def test_the_cases_reach_every_branch():
    for (H, Hprev), nrep in lr.NREPLICA.items():
        assert lr.hand_state(H, Hprev, 1.0).Nreplica == nrep
    half = {"consistent": 0, "as_written": 0}
    plain = dict(half)
    wrapped = 0
    for mode, H, Hprev, f, offset in lr.combos():
        e = lr.expected(1000, mode, H, Hprev, f, offset)
        assert len(e.rows) >= 1, (mode, H, Hprev, f)
        assert e.rows.shape == (len(e.index), 4) and np.all(e.rows[:, 3] == f)
        order = e.index.astype(np.int64) * 1000 + e.replica
        assert np.all(np.diff(order) > 0)                 # (particle, replica) ascending, no pair twice
        half[mode] += e.half
        plain[mode] += len(e.rows) - e.half
        wrapped += e.wrapped
        if f < 1.0:
            assert e.drawn_out >= 1 and len(e.rows) >= 1 and e.geometric == e.drawn_out + len(e.rows)
        else:
            assert e.drawn_out == 0
    assert min(half.values()) >= 1 and min(plain.values()) >= 1 and wrapped >= 1


def test_as_written_is_silent_beyond_the_box_diagonal():
    """pnew[k] = Pos[k] + Base[i].Vel[k] * ddrift - off[k] carries no replica shift: with Pos - off inside [0, BoxSize) and a drift of at
    most VMAX * DDRIFT per coordinate, |pnew| < sqrt(3) (BoxSize + VMAX * DDRIFT) = 1.82 BoxSize, below H = 2.30.  dnew >= H^2 cannot hold."""
    bound = math.sqrt(3.0) * (lr.BOXSIZE + lr.VMAX * lr.DDRIFT)
    assert bound < 2.30
    c = lr.case(1000)
    st = lr.hand_state(2.30, 2.40, 1.0)
    e = lr.cross(c.P, st, "as_written", lr.DDRIFT, c.offset, c.rnd)
    assert len(e.rows) == 0 and e.geometric == 0
    assert len(lr.expected(1000, "consistent", 2.30, 2.40, 1.0, lr.OFFSET).rows) > 100


def test_layout_and_refusals_without_a_device():
    L = sq.lightcone_layout()
    f = capi.PARTICLE_DTYPE.fields
    assert (L.part_elsize, L.off_type, L.off_pos, L.off_vel, L.off_id) == (160, f["Type"][1], f["Pos"][1], f["Vel"][1], f["ID"][1])
    Q, dt = lr.embed(lr.case(65).P)
    L2 = sq.lightcone_layout(dt)
    assert L2.part_elsize == 192 and np.array_equal(Q["Pos"], lr.case(65).P["Pos"])
    with pytest.raises(ValueError):
        sq.Lightcone(np.zeros(3), np.zeros(4), 1.0)
