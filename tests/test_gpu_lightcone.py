"""Light-cone crossings on the device (csrc/lightcone.hip: shq_lightcone_compute) against the restatement of lightcone_cross in
lightcone_restated.py, on its shared cases (seed 20261019; 0, 1, 63, 65, 257, 1000 and 5000 particles: a wave is 64 lanes, a workgroup 256).

Everything is compared as bytes, in order: the kernel evaluates the reference's double expressions without contraction, with IEEE sqrt and
division, and emits rows by (particle, replica).  test_lightcone_cpu.py shows that the cases reach every branch."""
import ctypes as C

import numpy as np
import pytest
import torch

import shenqi_amd as sq
from shenqi_amd import capi
import lightcone_restated as lr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODE = {"consistent": capi.LIGHTCONE_CONSISTENT, "as_written": capi.LIGHTCONE_AS_WRITTEN}
PATTERN = -7.25          # what the outputs hold before a call
IPATTERN = -77


def dev(a):
    """the records as device bytes (16 spare bytes behind them, so that nothing is empty)"""
    raw = np.concatenate([a.view(np.uint8).reshape(-1), np.zeros(16, dtype=np.uint8)])
    return torch.from_numpy(raw).to(DEV)


def outputs(cap, index=True, replica=True):
    rows = torch.full((max(cap, 1), 4), PATTERN, dtype=torch.float64, device=DEV)
    idx = torch.full((max(cap, 1),), IPATTERN, dtype=torch.int32, device=DEV) if index else None
    rep = torch.full((max(cap, 1),), IPATTERN, dtype=torch.int32, device=DEV) if replica else None
    return rows, idx, rep


def untouched(rows, idx, rep):
    return bool((rows == PATTERN).all()) and (idx is None or bool((idx == IPATTERN).all())) and (rep is None or bool((rep == IPATTERN).all()))


def run(ctx, d_parts, n, st, mode, c, cap, index=True, replica=True, layout=None, ddrift=lr.DDRIFT, rnd=None):
    rows, idx, rep = outputs(cap, index, replica)
    rc, nrows = sq.lightcone_compute_raw(ctx, sq.lightcone_layout() if layout is None else layout, d_parts, n, st.struct() if isinstance(st, lr.State) else st,
                                         MODE[mode], ddrift, c.offset, c.rnd if rnd is None else rnd, rows, idx, rep, cap)
    return rc, nrows, rows, idx, rep


def same(e, nrows, rows, idx, rep):
    m = len(e.rows)
    if nrows != m or rows[:m].cpu().numpy().tobytes() != e.rows.tobytes():
        return False
    if idx is not None and not np.array_equal(idx[:m].cpu().numpy(), e.index):
        return False
    if rep is not None and not np.array_equal(rep[:m].cpu().numpy(), e.replica):
        return False
    tail_ok = bool((rows[m:] == PATTERN).all()) and (idx is None or bool((idx[m:] == IPATTERN).all())) and (rep is None or bool((rep[m:] == IPATTERN).all()))
    return tail_ok


# ---- (1) every case ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", lr.COUNTS)
def test_rows_equal_the_restatement(ctx, n):
    parts = {}
    for mode, H, Hprev, f, offset in lr.combos():
        c = lr.case(n, offset)
        if offset not in parts:
            parts[offset] = dev(c.P)
        st = lr.hand_state(H, Hprev, f)
        if mode == "as_written" and n < st.Nreplica:    # record i must exist
            rc, nrows, rows, idx, rep = run(ctx, parts[offset], n, st, mode, c, 64)
            assert rc == capi.ERR_INVALID and untouched(rows, idx, rep)
            continue
        e = lr.expected(n, mode, H, Hprev, f, offset)
        cap = len(e.rows) + 3
        rc, nrows, rows, idx, rep = run(ctx, parts[offset], n, st, mode, c, cap)
        assert rc == 0 and same(e, nrows, rows, idx, rep), (mode, H, Hprev, f, nrows, len(e.rows))
        rc, nrows, rows, idx, rep = run(ctx, parts[offset], n, st, mode, c, cap, index=False, replica=False)
        assert rc == 0 and same(e, nrows, rows, None, None), (mode, H, Hprev, f, "no index, no replica")


# ---- (2) capacity -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode, H, Hprev, offset", [("consistent", 2.30, 2.40, lr.OFFSET), ("as_written", 1.20, 1.30, lr.ZERO)])
def test_capacity(ctx, mode, H, Hprev, offset):
    n = 1000
    c = lr.case(n, offset)
    d = dev(c.P)
    st = lr.hand_state(H, Hprev, 1.0)
    e = lr.expected(n, mode, H, Hprev, 1.0, offset)
    want = len(e.rows)
    assert want > 1
    rc, nrows, rows, idx, rep = run(ctx, d, n, st, mode, c, want - 1)
    assert rc == capi.ERR_NOMEM and nrows == want and untouched(rows, idx, rep)
    rc, nrows, rows, idx, rep = run(ctx, d, n, st, mode, c, want)
    assert rc == 0 and same(e, nrows, rows, idx, rep)
    # the wrapper: a first guess that is too small grows once
    lc = sq.Lightcone(np.array([-1.0, 0.0]), np.array([1.0, 0.0]), lr.BOXSIZE, BoxBoost=lr.BOXBOOST)
    lc._state = st.struct()
    grown = lc.compute(ctx, d, n, lr.DDRIFT, offset, c.rnd, mode=mode)
    assert grown[0].shape == (want, 4) and same(e, want, *grown)
    with pytest.raises(capi.ShqError):
        lc.compute(ctx, d, n, lr.DDRIFT, offset, c.rnd, mode=mode, capacity=want - 1)
    import shenqi_amd.lightcone as lcm
    caps = []
    raw = lcm.lightcone_compute_raw
    try:                                                 # a first guess of 15 rows (n // 64): the wrapper must come back with room
        def counting(*a):
            caps.append(a[-1])
            return raw(*a)
        lcm.lightcone_compute_raw = counting
        lc.first_capacity = 2
        grown = lc.compute(ctx, d, n, lr.DDRIFT, offset, c.rnd, mode=mode)
    finally:
        lcm.lightcone_compute_raw = raw
    assert caps == [n // 64, want] and same(e, want, *grown)


# ---- (3) reproducible, and free of the record size ------------------------------------------------------------------------------------------

def test_two_calls_and_another_record_size_give_the_same_bytes(ctx):
    n = 1000
    for mode, H, Hprev, offset in (("consistent", 2.30, 2.40, lr.OFFSET), ("as_written", 1.20, 1.30, lr.ZERO)):
        c = lr.case(n, offset)
        st = lr.hand_state(H, Hprev, 0.3)
        e = lr.expected(n, mode, H, Hprev, 0.3, offset)
        d = dev(c.P)
        a = run(ctx, d, n, st, mode, c, len(e.rows))
        b = run(ctx, d, n, st, mode, c, len(e.rows))
        assert a[0] == 0 and b[0] == 0 and a[1] == b[1] == len(e.rows)
        for x, y in zip(a[2:], b[2:]):
            assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
        Q, dt = lr.embed(c.P)
        w = run(ctx, dev(Q), n, st, mode, c, len(e.rows), layout=sq.lightcone_layout(dt))
        assert w[0] == 0 and same(e, *w[1:])


# ---- (4) refusals -----------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_outputs_alone(ctx):
    c = lr.case(65, lr.ZERO)
    d = dev(c.P)
    st = lr.hand_state(1.20, 1.30, 1.0)
    assert st.Nreplica == 4
    rc, _, *out = run(ctx, d, 1, st, "as_written", c, 64)                      # record 1 .. 3 do not exist
    assert rc == capi.ERR_INVALID and untouched(*out)
    rows, idx, rep = outputs(64)
    rnd = np.ascontiguousarray(c.rnd)
    off = (C.c_double * 3)(*c.offset)
    nrows = C.c_int64(-5)
    s = st.struct()
    L = sq.lightcone_layout()

    def call(state=s, mode=0, ddrift=lr.DDRIFT, rnd_size=len(rnd), layout=L, numpart=65):
        return capi.hip.shq_lightcone_compute(ctx.h, C.byref(layout), d.data_ptr(), numpart, C.byref(state), mode, ddrift, off, capi.ptr(rnd), rnd_size, rows.data_ptr(),
                                              idx.data_ptr(), rep.data_ptr(), 64, C.byref(nrows))

    assert call(rnd_size=0) == capi.ERR_INVALID and untouched(rows, idx, rep)
    many = st.struct()
    many.Nreplica = 1001
    assert call(state=many) == capi.ERR_INVALID and untouched(rows, idx, rep)
    assert call(ddrift=float("nan")) == capi.ERR_INVALID and untouched(rows, idx, rep)
    assert call(ddrift=float("inf")) == capi.ERR_INVALID and untouched(rows, idx, rep)
    assert call(mode=2) == capi.ERR_INVALID and untouched(rows, idx, rep)
    assert call(numpart=-1) == capi.ERR_INVALID and untouched(rows, idx, rep)
    odd = sq.lightcone_layout()
    odd.part_elsize = 164
    assert call(layout=odd) == capi.ERR_INVALID and untouched(rows, idx, rep)
    big = sq.lightcone_layout()
    big.part_elsize = 488
    assert call(layout=big) == capi.ERR_INVALID and untouched(rows, idx, rep)
    nan_h = st.struct()
    nan_h.HorizonDistance2 = float("nan")
    assert call(state=nan_h) == capi.ERR_INVALID and untouched(rows, idx, rep)
    assert nrows.value == -5
    zero = st.struct()
    zero.SampleFraction = 0.0
    assert call(state=zero) == 0 and nrows.value == 0 and untouched(rows, idx, rep)
    nrows.value = -5
    none = st.struct()
    none.Nreplica = 0
    assert call(state=none) == 0 and nrows.value == 0 and untouched(rows, idx, rep)
    assert call() == 0 and nrows.value == len(lr.expected(65, "consistent", 1.20, 1.30, 1.0, lr.ZERO).rows)


# ---- (5) garbage, and draws that reject everything --------------------------------------------------------------------------------------------

def test_garbage_is_not_tested_and_a_rejecting_draw_silences_a_particle(ctx):
    n = 257
    c = lr.case(n)
    st = lr.hand_state(2.30, 2.40, 0.3)
    e1 = lr.cross(c.P, lr.hand_state(2.30, 2.40, 1.0), "consistent", lr.DDRIFT, c.offset, c.rnd)
    hits = np.unique(e1.index)
    assert len(hits) >= 4
    P = c.P.copy()
    g, quiet = int(hits[0]), int(hits[-1])
    P["Flags"] = 0
    P["Flags"][g] = 1                                    # IsGarbage
    # a table in which exactly the draws of `quiet` reject: its ID becomes one whose entries nobody else reads
    rnd = np.full(lr.RNDSIZE, 0.1)
    P["ID"] = np.uint64(lr.RNDSIZE) * np.arange(n, dtype=np.uint64) + np.arange(n, dtype=np.uint64) % np.uint64(900)   # ID + i reads entries 0 .. 914
    P["ID"][quiet] = np.uint64(lr.RNDSIZE * 1000 + lr.RNDSIZE - 20)                                                      # ... 977 .. 992
    rnd[lr.RNDSIZE - 20:] = 0.9
    assert all(int(P["ID"][p]) % lr.RNDSIZE + 15 < lr.RNDSIZE - 20 for p in range(n) if p != quiet)
    e = lr.cross(P, st, "consistent", lr.DDRIFT, c.offset, rnd)
    assert g in e.index and quiet not in e.index and e.drawn_out == int((e1.index == quiet).sum())
    rc, nrows, rows, idx, rep = run(ctx, dev(P), n, st, "consistent", c, len(e.rows) + 1, rnd=rnd)
    assert rc == 0 and same(e, nrows, rows, idx, rep)


# ---- (6) end to end -----------------------------------------------------------------------------------------------------------------------

def test_lightcone_class_end_to_end(ctx):
    DH, box, boost = 3.0, 1.0, 6
    la, dc, dl = lr.eds_table(0.05, DH, nentry=256)
    n = 1000
    c = lr.case(n)
    d = dev(c.P)
    lc = sq.Lightcone(la, dc, box, BoxBoost=boost, dloga=dl)
    want = lr.init_state(la, dc, dl)
    total = 0
    for a, mode in ((0.30, "consistent"), (0.31, "consistent"), (0.3125, "consistent")):
        lc.set_time(a)
        lr.set_time(want, la, dc, dl, a, box, BoxBoost=boost)
        assert bytes(lc._state) == want.bytes() and lc.state.Nreplica >= 8
        e = lr.cross(c.P, want, mode, lr.DDRIFT, c.offset, c.rnd)
        rows, idx, rep = lc.compute(ctx, d, n, lr.DDRIFT, c.offset, c.rnd, mode=mode)
        assert rows.shape == (len(e.rows), 4) and rows.is_cuda and idx.dtype == torch.int32 and rep.dtype == torch.int32
        assert same(e, len(e.rows), rows, idx, rep)
        total += len(e.rows)
    assert total > 0
    ms = sq.lightcone_phase_ms(ctx)
    assert len(ms) == 3 and ms[0] > 0 and ms[1] > 0
