"""Snapshot blocks on the device (csrc/snapshot.hip: shq_io_select, shq_io_gather, shq_io_scatter; shq_io_ion_fractions) against the
restatement of petaio.cpp's loops in snapshot_restated.py, on its shared cases (seed 20261019; 0, 1, 63, 65, 257 and 1000 particles: a
tile of the gather is 128 rows, a wave 64).

Columns are compared as bytes.  InternalEnergy is the one exception, because the device's pow may differ from glibc's in the last bits of
the double: rows whose double lies within 2^-40 (relative) of a float32 rounding boundary are left out of the bit comparison and must be
within one float32 ulp; test_snapshot_cpu.py bounds their share.  In the readout, Entropy = GAMMA_MINUS1 * u / pow(...) is a double: one
multiplication and one division, each correctly rounded, around a pow that may be one ulp off on either side, so 4 x 2^-52 relative; every
other member must be equal."""
import itertools

import numpy as np
import pytest
import torch

import shenqi_amd as sq
from shenqi_amd import capi
import snapshot_restated as sr
import sfr_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_INVALID = 1
PRED = {"all": capi.IO_SELECT_ALL, "fof": capi.IO_SELECT_FOF}
ORDER = {"index": capi.IO_ORDER_INDEX, "grnr": capi.IO_ORDER_GRNR}
TABLE = sq.io_blocks(1, 1, 1, debug=True, OutputHeliumFractions=True)


def dev(a, spare=0):
    """the records as device bytes, with `spare` more records of zeros behind them"""
    raw = a.view(np.uint8).reshape(-1)
    raw = np.concatenate([raw, np.zeros(spare * a.dtype.itemsize + 16, dtype=np.uint8)])
    return torch.from_numpy(raw).to(DEV)


def back(d, like):
    return d.cpu().numpy()[:like.nbytes].view(like.dtype).copy()


def upload(P, slots, spare=0):
    return dev(P, spare), [dev(slots[t], spare) if t in slots else None for t in range(6)]


def conv_of(c, setter=False):
    return sq.io_conv(c.atime, c.BoxSize, c.offset, c.pecvel, setter=setter)


def same_records(a, b, skip=()):
    return [f for f in a.dtype.names if f not in skip and not np.array_equal(a[f], b[f])]


def status_of(call):
    try:
        call()
    except capi.ShqError as e:
        return int(str(e).split("status ")[1].split(":")[0])
    return 0


# ---- (1) selection ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", sr.COUNTS)
def test_selection_equals_the_restatement(ctx, n):
    c = sr.case(n)
    d_parts = dev(c.P)
    L = sq.io_layout()
    for pred, order in itertools.product(PRED, ORDER):
        want, wcount, woffset = sr.select(c.P, pred, order)
        sel, count, offset = sq.io_select(ctx, L, d_parts, n, PRED[pred], ORDER[order])
        assert np.array_equal(count, wcount) and np.array_equal(offset, woffset), (pred, order)
        assert np.array_equal(sel.cpu().numpy()[:len(want)], want), (pred, order)


def test_selection_refuses_a_type_above_five(ctx):
    c = sr.case(65)
    P = c.P.copy()
    live = np.flatnonzero(((P["Flags"] & sr.GARBAGE) == 0) & (P["GrNr"] >= 0) & ((P["Flags"] & sr.SWALLOWED) == 0))
    P["Type"][live[3]] = 7
    for pred, order in itertools.product(PRED, ORDER):
        assert status_of(lambda: sq.io_select(ctx, sq.io_layout(), dev(P), len(P), PRED[pred], ORDER[order])) == ERR_INVALID
    # a garbage particle is not selected, whatever its type
    P = c.P.copy()
    P["Type"][np.flatnonzero(P["Flags"] & sr.GARBAGE)[0]] = 7
    _, count, _ = sq.io_select(ctx, sq.io_layout(), dev(P), len(P))
    assert np.array_equal(count, sr.select(P, "all", "index")[1])


# ---- (2) gather -------------------------------------------------------------------------------------------------------------------------

def check_column(b, got, want, c, P, slots, s):
    assert got.dtype == want.dtype and got.shape == want.shape, b
    if b.name != "InternalEnergy":
        assert got.tobytes() == want.tobytes(), b
        return
    S = slots[0][P["PI"][s]]
    v = sr.internal_energy_f64(S["Entropy"], S["Density"], c.conv.atime)
    near = sr.near_f32_boundary(v)
    print(f"InternalEnergy: {near.sum()} of {len(v)} rows near a float32 boundary; {np.sum(got != want)} rows differ")
    assert np.array_equal(got[~near], want[~near])
    up, down = np.nextafter(want[near], np.float32(np.inf)), np.nextafter(want[near], np.float32(-np.inf))
    assert np.all((got[near] == want[near]) | (got[near] == up) | (got[near] == down))


@pytest.mark.parametrize("n", sr.COUNTS)
def test_gather_every_block_equals_the_restatement(ctx, n):
    c = sr.case(n)
    d_parts, d_slots = upload(c.P, c.slots)
    L, cv = sq.io_layout(), conv_of(c.conv)
    sel, count, offset = sr.select(c.P, "all", "index")
    want = sr.columns(TABLE, c.P, c.slots, sel, count, offset, c.conv)
    got, hsel, gcount, goffset = sq.snapshot_columns(ctx, TABLE, d_parts, n, d_slots, c.slot_size, cv)
    assert np.array_equal(hsel, sel) and np.array_equal(gcount, count)
    assert set(got) == set(want) and len(want) > 80
    d_sel = torch.from_numpy(np.concatenate([sel, np.zeros(1, np.int32)])).to(DEV)
    for t in range(6):
        s = sel[offset[t]:offset[t] + count[t]]
        blocks = [b for b in TABLE if b.ptype == t and b.ion is None]
        for b in blocks:
            check_column(b, got[(t, b.name)], want[(t, b.name)], c, c.P, c.slots, s)
            # one block per call gives the same bytes as all blocks of the type in one call
            one, = sq.io_gather(ctx, L, d_parts, n, d_slots, c.slot_size, t, d_sel, offset[t], count[t], [b.getter], cv)
            assert one.tobytes() == got[(t, b.name)].tobytes(), b
        if n == 257:   # more blocks than one launch takes: the same columns again, several times over
            many = blocks * (capi_maxblocks() // len(blocks) + 2)
            cols = sq.io_gather(ctx, L, d_parts, n, d_slots, c.slot_size, t, d_sel, offset[t], count[t], [b.getter for b in many], cv)
            assert len(many) > capi_maxblocks() and all(x.tobytes() == got[(t, b.name)].tobytes() for b, x in zip(many, cols))


def capi_maxblocks():
    return 48   # SHQ_IO_MAXBLOCKS


# ---- (3) error paths --------------------------------------------------------------------------------------------------------------------

def test_gather_error_paths(ctx):
    """each returns SHQ_ERR_INVALID; the buffers hold spare records, so a missing check would read valid memory and fail here"""
    c = sr.case(257)
    n = c.n
    L, cv = sq.io_layout(), conv_of(c.conv)
    sel, count, offset = sr.select(c.P, "all", "index")
    gas = [b.getter for b in TABLE if b.ptype == 0 and b.ion is None]
    bh = [b.getter for b in TABLE if b.ptype == 5 and b.ion is None]

    def run(P, slots, s, t, blocks, slot_size=c.slot_size):
        d_parts, d_slots = upload(P, slots, spare=8)
        d_sel = torch.from_numpy(np.ascontiguousarray(s, dtype=np.int32)).to(DEV)
        return status_of(lambda: sq.io_gather(ctx, L, d_parts, n, d_slots, slot_size, t, d_sel, 0, len(s), blocks, cv))

    s0 = sel[offset[0]:offset[0] + count[0]].copy()
    s5 = sel[offset[5]:offset[5] + count[5]].copy()
    assert run(c.P, c.slots, s0, 0, gas) == 0 and run(c.P, c.slots, s5, 5, bh) == 0
    wrong = s0.copy()
    wrong[len(wrong) - 3] = sel[offset[1]]                         # a dark-matter particle among the gas
    assert run(c.P, c.slots, wrong, 0, gas) == ERR_INVALID
    past = s0.copy()
    past[1] = n                                        # an index equal to numpart
    assert run(c.P, c.slots, past, 0, gas) == ERR_INVALID
    past[1] = -1
    assert run(c.P, c.slots, past, 0, gas) == ERR_INVALID
    P = c.P.copy()
    P["PI"][s5[2]] = c.slot_size[5]                    # a PI equal to slot_size
    assert run(P, c.slots, s5, 5, bh) == ERR_INVALID
    base_only = [b.getter for b in TABLE if b.ptype == 5 and b.ion is None and b.getter.source == capi.IO_SRC_BASE]
    assert run(P, c.slots, s5, 5, base_only) == 0      # no block reads the slot: PI is not looked at
    P = c.P.copy()
    P["Pos"][s0[-2], 1] = np.nan                       # a NaN position
    assert run(P, c.slots, s0, 0, gas) == ERR_INVALID
    P["Pos"][s0[-2], 1] = np.inf
    assert run(P, c.slots, s0, 0, gas) == ERR_INVALID
    P["Pos"][s0[-2], 1] = 70 * sr.BOXSIZE              # a loop that does not end within 64 rounds
    assert run(P, c.slots, s0, 0, gas) == ERR_INVALID
    slots = {t: v.copy() for t, v in c.slots.items()}
    slots[5]["MinPotPos"][c.P["PI"][s5[1]], 2] = np.nan
    assert run(c.P, slots, s5, 5, bh) == ERR_INVALID


# ---- (4) readout ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", sr.COUNTS)
def test_readout_equals_the_restatement(ctx, n):
    c = sr.case(n)
    table = sq.io_blocks(1, 1, 1)
    cols = {}
    for b in table:    # the file's columns: every particle of the type in index order, garbage included
        idx = np.flatnonzero(c.P["Type"] == b.ptype)
        if b.ion is None and len(idx):
            cols[(b.ptype, b.name)] = sr.get_column(b.name, b.ptype, b.dtype, b.items, c.P, c.slots, idx, c.conv)
    P0 = np.zeros_like(c.P)
    P0["Type"], P0["PI"] = c.P["Type"], c.P["PI"]
    S0 = {t: np.zeros_like(s) for t, s in c.slots.items()}
    wantP, wantS = P0.copy(), {t: s.copy() for t, s in S0.items()}
    sr.readout(table, cols, wantP, wantS, c.conv)
    d_parts, d_slots = upload(P0, S0)
    cv = conv_of(c.conv, setter=True)
    sq.snapshot_readout(ctx, table, cols, d_parts, n, d_slots, c.slot_size, cv)
    gotP, gotS = back(d_parts, P0), {t: back(d_slots[t], S0[t]) for t in S0}
    assert same_records(gotP, wantP) == []
    for t in S0:
        assert same_records(gotS[t], wantS[t], skip=("Entropy",) if t == 0 else ()) == [], t
    e, w = gotS[0]["Entropy"], wantS[0]["Entropy"]
    print(f"readout, {n} particles: {np.sum(e != w)} of {len(w)} Entropy values differ from glibc's")
    assert np.all(np.abs(e - w) <= 4 * 2.0 ** -52 * np.abs(w))
    if n:
        assert np.any(w != 0) and np.array_equal(gotS[0]["Density"], wantS[0]["Density"]) and np.any(wantS[0]["Density"] != 0)
    # gather back what a float column holds exactly
    live = sr.select(wantP, "all", "index")
    got, hsel, count, offset = sq.snapshot_columns(ctx, table, d_parts, n, d_slots, c.slot_size, sq.io_conv(c.conv.atime, c.conv.BoxSize, (0.0, 0.0, 0.0), False))
    assert np.array_equal(hsel, live[0])
    for b in table:
        if b.setter is None or b.name in ("Velocity", "InternalEnergy") or (b.ptype, b.name) not in cols:
            continue
        keep = np.flatnonzero(np.isin(np.flatnonzero(c.P["Type"] == b.ptype), hsel))    # rows of the live particles
        assert got[(b.ptype, b.name)].tobytes() == cols[(b.ptype, b.name)][keep].tobytes(), b


def test_readout_refuses_a_wrong_row_count(ctx):
    c = sr.case(257)
    table = [b for b in sq.io_blocks(1, 1, 1) if b.ptype == 0 and b.setter is not None]
    idx = np.flatnonzero(c.P["Type"] == 0)
    cols = [sr.get_column(b.name, 0, b.dtype, b.items, c.P, c.slots, idx, c.conv) for b in table]
    P0 = np.zeros_like(c.P)
    P0["Type"], P0["PI"] = c.P["Type"], c.P["PI"]
    S0 = {t: np.zeros_like(s) for t, s in c.slots.items()}
    L, cv = sq.io_layout(), conv_of(c.conv, setter=True)
    for cut in (slice(0, -1), slice(1, None)):
        d_parts, d_slots = upload(P0, S0, spare=4)
        short = [x[cut] for x in cols]
        assert status_of(lambda: sq.io_scatter(ctx, L, d_parts, c.n, d_slots, c.slot_size, 0, [b.setter for b in table], short, cv)) == ERR_INVALID
        assert same_records(back(d_parts, P0), P0) == [] and same_records(back(d_slots[0], S0[0]), S0[0]) == []
    # one row more than there are particles of the type
    d_parts, d_slots = upload(P0, S0, spare=4)
    longer = [np.concatenate([x, x[:1]]) for x in cols]
    assert status_of(lambda: sq.io_scatter(ctx, L, d_parts, c.n, d_slots, c.slot_size, 0, [b.setter for b in table], longer, cv)) == ERR_INVALID
    assert same_records(back(d_parts, P0), P0) == [] and same_records(back(d_slots[0], S0[0]), S0[0]) == []
    # a PI outside the slot array: refused before any write
    P1 = P0.copy()
    P1["PI"][idx[5]] = c.slot_size[0]
    d_parts, d_slots = upload(P1, S0, spare=4)
    assert status_of(lambda: sq.io_scatter(ctx, L, d_parts, c.n, d_slots, c.slot_size, 0, [b.setter for b in table], cols, cv)) == ERR_INVALID
    assert same_records(back(d_parts, P1), P1) == [] and same_records(back(d_slots[0], S0[0]), S0[0]) == []


# ---- (5) ion fractions ------------------------------------------------------------------------------------------------------------------

HARD = 2.5e-6   # test_gpu_sfr.py's figures and derivation: a fraction query is within (2 T + R) relative of the host engine's
T = 10 * HARD
R = 1e-9


def _ion_records():
    """sfr_cases' first 300 particles and its edge rows as gas records, dark matter interleaved, one row without mass"""
    p = sc.particles()
    n = len(p["Density"])
    p = sc.subset(p, np.r_[0:300, n - len(sc.EDGE_ROWS):n])
    ng = len(p["Density"])
    rng = np.random.default_rng(sr.SEED)
    types = rng.permutation(np.concatenate([np.zeros(ng, np.uint8), np.ones(60, np.uint8)]))
    P = np.zeros(len(types), dtype=capi.PARTICLE_DTYPE)
    P["Type"] = types
    gi = np.flatnonzero(types == 0)
    pi = rng.permutation(ng)
    P["PI"][gi] = pi
    P["Mass"] = 1.0
    P["Mass"][gi], P["Hsml"][gi], P["TimeBinHydro"][gi], P["Flags"][gi], P["ID"][gi] = p["Mass"], p["Hsml"], p["timebin"], p["flags"], p["ID"]
    P["Mass"][gi[17]] = 0.0
    S = np.zeros(ng, dtype=capi.SPH_DTYPE)
    for member, key in (("Density", "Density"), ("Entropy", "Entropy"), ("Ne", "Ne"), ("Metallicity", "Metallicity"), ("DivVel", "DivVel"), ("CurlVel", "CurlVel"),
                        ("DelayTime", "DelayTime")):
        S[member][pi] = p[key]
    st = capi.CoolingStep()
    st.redshift, st.a3inv, st.hubble = sc.REDSHIFT, sc.A3INV, sc.HUBBLE
    for b in range(capi.TIMEBINS + 1):
        st.kf.dloga_for_bin[b] = sc.DLOGA_FOR_BIN.get(b, 2e-3)
        st.lastred_for_bin[b] = sc.REDSHIFT
    for k, v in sc.case().uv.items():
        setattr(st.GlobalUVBG, k, v)
    st.uvbg_mode, st.StarformationOn = capi.COOL_UVBG_GLOBAL, 1
    par = sc.params()
    st.temp_to_u, st.HIReionTemp, st.MinGasTemp, st.lmfp_heat = par["temp_to_u"], 0.0, 100.0, sc.case().lmfp_heat
    st.PhysDensThresh, st.OverDensThresh = par["PhysDensThresh"], par["OverDensThresh"]
    # what the engine sees of a listed gas particle, for the host engine
    arrays = dict(Density=S["Density"][pi], Entropy=S["Entropy"][pi], Ne=S["Ne"][pi], Metallicity=S["Metallicity"][pi], Mass=P["Mass"][gi].astype(np.float64),
                  Hsml=P["Hsml"][gi].astype(np.float64), DivVel=S["DivVel"][pi], CurlVel=S["CurlVel"][pi], GradRho=np.zeros(ng),
                  dloga=np.array([st.kf.dloga_for_bin[int(b)] for b in P["TimeBinHydro"][gi]]), DelayTime=S["DelayTime"][pi],
                  timebin=P["TimeBinHydro"][gi].astype(np.uint8), flags=P["Flags"][gi].astype(np.uint8), ID=P["ID"][gi])
    return P, S, st, gi, arrays


@pytest.mark.parametrize("quicklya", [0.0, 0.25])
def test_ion_fraction_columns(ctx, quicklya):
    """under the GLOBAL mode the per-particle local UVBG is the global one, which is what shq_sfr_eval_host takes"""
    P, S, st, gi, arrays = _ion_records()
    par = sc.params(QuickLymanAlphaProbability=quicklya)
    capi.check(capi.hip.shq_set_inputs_current(ctx.h, 0))
    sq.cooling_set_tables(ctx, sc.case().tables())
    pman = sq.PartManager(len(P), 20000.0)
    pman.Base[:] = P
    S1 = S.copy()
    cols, status, listed, res = sq.io_ion_fractions(ctx, pman, S1, sc.lib_params(par), st, list_=gi.astype(np.int32))
    assert same_records(pman.Base, P) == [] and same_records(S1, S) == []       # a query writes no record
    hosts = [sc.host(w, par, arrays) for w in ("NH0", "HE0", "HEP", "HEPP")]
    want_status = np.zeros(len(gi), dtype=np.int32)
    for h in hosts:
        want_status = np.where(want_status == capi.COOL_OK, h.status, want_status)
    assert np.array_equal(status, want_status)
    bad = want_status != capi.COOL_OK
    assert bad[17] and bad.sum() < 10 and np.array_equal(listed, np.flatnonzero(bad)) and res.n_listed == bad.sum()
    assert [res.n_status[s] for s in range(4)] == [int(np.sum(want_status == s)) for s in range(4)]
    for q, h in enumerate(hosts):
        got = cols[q]
        assert got.dtype == np.float32 and np.all(np.isnan(got[bad])) and np.all(np.isfinite(got[~bad]))
        w = h.query[~bad]
        err = np.abs(got[~bad].astype(np.float64) - w)
        print(f"ion fraction {q}, QuickLymanAlphaProbability {quicklya}: largest deviation {np.max(err / np.maximum(np.abs(w), 1e-300)):.3g} relative")
        assert np.all(err <= (2 * T + R + 2.0 ** -24) * np.abs(w))
    # one column alone gives the same rows; without tables the call is refused
    one, st1, _, _ = sq.io_ion_fractions(ctx, pman, S1, sc.lib_params(par), st, list_=gi.astype(np.int32), which=(2,))
    ok1 = st1 == capi.COOL_OK
    assert np.array_equal(one[2][ok1 & ~bad], cols[2][ok1 & ~bad]) and np.array_equal(st1, hosts[2].status)
    with sq.Context(0) as fresh:
        assert status_of(lambda: sq.io_ion_fractions(fresh, pman, S1, sc.lib_params(par), st, list_=gi.astype(np.int32))) == 4    # SHQ_ERR_STATE


# ---- (6) the order of the FOF particle blocks -----------------------------------------------------------------------------------------

def test_fof_order_groups_each_type_by_group_number(ctx):
    c = sr.case(1000)
    d_parts, d_slots = upload(c.P, c.slots)
    table = sq.io_blocks(1, 1, 1)
    got, hsel, count, offset = sq.snapshot_columns(ctx, table, d_parts, c.n, d_slots, c.slot_size, conv_of(c.conv), predicate=capi.IO_SELECT_FOF,
                                                   order=capi.IO_ORDER_GRNR)
    sel, wcount, woffset = sr.select(c.P, "fof", "grnr")
    assert np.array_equal(hsel, sel) and np.array_equal(count, wcount) and np.array_equal(offset, woffset)
    want = sr.columns(table, c.P, c.slots, sel, wcount, woffset, c.conv)
    for t in range(6):
        g = got[(t, "GroupID")]
        assert g.dtype == np.uint32 and np.all(np.diff(g.astype(np.int64)) >= 0) and (t == 3 or len(np.unique(g)) > 5)
        for b in table:
            if b.ptype == t and b.ion is None and b.name != "InternalEnergy":
                assert got[(t, b.name)].tobytes() == want[(t, b.name)].tobytes(), b


def test_gather_reads_records_past_two_gibibytes(ctx):
    """byte offsets into the record array pass 2^31 at 13.4 million records of 160 bytes: the 257-particle case sits at the end of an array of
    14 million zeroed records, and its dark matter is gathered from there"""
    c = sr.case(257)
    N = 14_000_000
    esz = capi.PARTICLE_DTYPE.itemsize
    d_parts = torch.zeros(N * esz + 16, dtype=torch.uint8, device=DEV)
    first = N - c.n
    assert first * esz > 2 ** 31
    d_parts[first * esz:N * esz] = torch.from_numpy(c.P.view(np.uint8).reshape(-1).copy()).to(DEV)
    sel, count, offset = sr.select(c.P, "all", "index")
    s = sel[offset[1]:offset[1] + count[1]]
    d_sel = torch.from_numpy((s.astype(np.int64) + first).astype(np.int32)).to(DEV)
    blocks = [b for b in TABLE if b.ptype == 1 and b.ion is None]
    got = sq.io_gather(ctx, sq.io_layout(), d_parts, N, None, None, 1, d_sel, 0, len(s), [b.getter for b in blocks], conv_of(c.conv))
    for b, col in zip(blocks, got):
        assert col.tobytes() == sr.get_column(b.name, 1, b.dtype, b.items, c.P, c.slots, s, c.conv).tobytes(), b
