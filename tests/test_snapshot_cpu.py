"""Snapshot blocks without a GPU: shenqi_amd.io_blocks against the reference's registrations (tests/golden/ref_io_blocks.json, read off
petaio.cpp:908-1047), its descriptors against the record dtypes, and the properties of the restatement (tests/snapshot_restated.py) that the
GPU tests in test_gpu_snapshot.py lean on."""
import itertools
import json
import os

import numpy as np
import pytest

import shenqi_amd as sq
from shenqi_amd import capi
import snapshot_restated as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_io_blocks.json")))


def expected(regs, **switch):
    out = []
    for r in regs:
        if all((not switch.get(w[1:], False)) if w.startswith("!") else switch.get(w, False) for w in r["when"]):
            out.append({k: r[k] for k in ("name", "ptype", "dtype", "items", "required")})
    return out


@pytest.mark.parametrize("WriteGroupID,MetalReturnOn", list(itertools.product([0, 1], [0, 1])))
@pytest.mark.parametrize("dis", [0, 1])
def test_io_blocks_equal_the_reference_registrations(WriteGroupID, MetalReturnOn, dis):
    for potential, timebins, helium in itertools.product([False, True], repeat=3):
        sw = dict(WriteGroupID=WriteGroupID, MetalReturnOn=MetalReturnOn, DensityIndependentSph=dis, OutputPotential=potential, OutputTimebins=timebins,
                  OutputHeliumFractions=helium)
        table = sq.io_blocks(WriteGroupID, MetalReturnOn, dis, OutputPotential=potential, OutputTimebins=timebins, OutputHeliumFractions=helium)
        want = expected(GOLDEN["register_io_blocks"], **sw)
        assert [b.key() for b in sorted(table, key=lambda b: b.zorder)] == want
        # sorted as order_by_type sorts: by type, ties in registration order
        assert [b.key() for b in table] == [w for _, w in sorted(enumerate(want), key=lambda e: (e[1]["ptype"], e[0]))]
        dbg = sq.io_blocks(WriteGroupID, MetalReturnOn, dis, debug=True, OutputPotential=potential, OutputTimebins=timebins, OutputHeliumFractions=helium)
        assert [b.key() for b in sorted(dbg, key=lambda b: b.zorder)] == want + expected(GOLDEN["register_debug_io_blocks"], **sw)


def test_defaults_are_the_reference_parameter_defaults():
    """OutputPotential 1, OutputTimebins 0, OutputHeliumFractions 0 (gadget/params.cpp:72-74)"""
    names = {(b.ptype, b.name) for b in sq.io_blocks(1, 1, 1)}
    assert (1, "Potential") in names and (1, "TimeBinHydro") not in names and (0, "HeliumIFraction") not in names and (0, "NeutralHydrogenFraction") in names


def test_excursion_set_blocks_follow_the_sph_dtype():
    ext = np.dtype({"names": list(capi.SPH_DTYPE.names) + ["local_J21", "zreion"],
                    "formats": [capi.SPH_DTYPE.fields[k][0] for k in capi.SPH_DTYPE.names] + ["<f8", "<f8"],
                    "offsets": [capi.SPH_DTYPE.fields[k][1] for k in capi.SPH_DTYPE.names] + [176, 184], "itemsize": 192})
    assert not any(b.name in ("J21", "ZReionized") for b in sq.io_blocks(1, 1, 1))
    t = sq.io_blocks(1, 1, 1, sph_dtype=ext)
    j = [b for b in t if b.name in ("J21", "ZReionized")]
    assert [b.name for b in j] == ["J21", "ZReionized"] and [b.getter.offset for b in j] == [176, 184]
    assert [b.key() for b in sorted(t, key=lambda b: b.zorder)] == expected(GOLDEN["register_io_blocks"], WriteGroupID=1, MetalReturnOn=1, DensityIndependentSph=1,
                                                                          OutputPotential=True, EXCUR_REION=True)


def test_descriptors_name_members_of_the_records():
    """every descriptor lies inside its record, reads the member the restatement reads for that name, and WRONLY blocks have no setter"""
    slot = sr.SLOT_DTYPES
    ions = 0
    for b in sq.io_blocks(1, 1, 1, debug=True, OutputHeliumFractions=True):
        if b.ion is not None:
            ions += 1
            assert b.getter is None and b.setter is None and b.name == sq.snapshot.ION_BLOCKS[b.ion]
            continue
        g = b.getter
        rec = capi.PARTICLE_DTYPE if g.source == capi.IO_SRC_BASE else slot[b.ptype]
        size = {capi.IO_F64: 8, capi.IO_I64: 8, capi.IO_U64: 8, capi.IO_F32: 4, capi.IO_I32: 4, capi.IO_U32: 4}.get(g.field_type, 1)
        assert g.offset + size * g.items <= rec.itemsize and g.items == b.items and g.col_type == capi.IO_TYPE_OF_DTYPE[b.dtype]
        if b.name in sr.SIMPLE:
            r, member = sr.SIMPLE[b.name]
            assert (r == "P") == (g.source == capi.IO_SRC_BASE) and g.offset == rec.fields[member][1] and g.kind == capi.IO_COPY
        elif b.name in sr.BITFIELD:
            assert g.field_type == capi.IO_BITS and (g.bit_shift, g.bit_width) == sr.BITFIELD[b.name] and g.offset == capi.PARTICLE_DTYPE.fields["Flags"][1]
        else:
            assert b.name in ("Position", "Velocity", "BlackholeMinPotPos", "InternalEnergy")
        if b.setter is not None:
            assert bytes(b.setter) == bytes(g)
    assert ions == 4
    ie = [b for b in sq.io_blocks(0, 0, 0) if b.name == "InternalEnergy"][0].getter
    assert (ie.kind, ie.offset, ie.offset2) == (capi.IO_INTERNAL_ENERGY, capi.SPH_DTYPE.fields["Entropy"][1], capi.SPH_DTYPE.fields["Density"][1])
    wronly = {"Potential", "GroupID", "StarFormationRate", "NeutralHydrogenFraction"}
    assert all((b.setter is None) == (b.name in wronly) for b in sq.io_blocks(1, 1, 1))
    order = [b.name for b in sq.io_blocks(1, 1, 1) if b.ptype == 0]
    assert order.index("Density") < order.index("EgyWtDensity") < order.index("InternalEnergy")   # "ensure density is read before this"


def test_struct_sizes_match_the_header():
    assert C_sizeof(capi.IoBlock) == 48 and C_sizeof(capi.IoConv) == 48 and C_sizeof(capi.IoLayout) == 8 * 11 and C_sizeof(capi.IoIonResult) == 56


def C_sizeof(t):
    import ctypes
    return ctypes.sizeof(t)


@pytest.mark.parametrize("n", sr.COUNTS)
def test_case_generator_covers_what_the_gpu_tests_need(n):
    c = sr.case(n)
    P = c.P
    assert len(P) == n and not (P["Type"] == 3).any()
    if n >= 63:
        assert set(np.unique(P["Type"])) == {0, 1, 2, 4, 5}
        assert (P["Flags"] & sr.GARBAGE).any() and (P["Flags"] & sr.SWALLOWED).any() and (P["Flags"] & sr.HEIII).any() and (P["Flags"] >> 4).max() == 15
        assert P["GrNr"].min() == -1 and P["GrNr"].max() <= 40 and len(np.unique(P["GrNr"])) < n
    for t, S in c.slots.items():
        idx = np.flatnonzero(P["Type"] == t)
        assert sorted(P["PI"][idx]) == list(range(len(idx))) and len(S) == len(idx) + 3
        if len(idx) > 8:
            assert not np.array_equal(P["PI"][idx], np.arange(len(idx)))   # shuffled
    for pred, order in itertools.product(("all", "fof"), ("index", "grnr")):
        sel, count, offset = sr.select(P, pred, order)
        assert count[3] == 0 and count.sum() == len(sel) and np.array_equal(offset, np.concatenate([[0], np.cumsum(count)[:-1]]))
        for t in range(6):
            s = sel[offset[t]:offset[t] + count[t]]
            assert np.all(P["Type"][s] == t) and not (P["Flags"][s] & sr.GARBAGE).any()
            if order == "index":
                assert np.all(np.diff(s) > 0)
            else:
                g = P["GrNr"][s]
                assert np.all(np.diff(g) >= 0) and np.all(np.diff(s)[np.diff(g) == 0] > 0)   # ties in index order
            if pred == "fof":
                assert np.all(P["GrNr"][s] >= 0) and not (P["Flags"][s] & sr.SWALLOWED).any()


def test_position_edges():
    c = sr.case(1000)
    sel, count, offset = sr.select(c.P, "all", "index")
    for t in (0, 1, 2, 4, 5):
        idx = np.flatnonzero(c.P["Type"] == t)[:5]
        pos = sr.get_column("Position", t, "f8", 3, c.P, c.slots, idx, c.conv)
        B = sr.BOXSIZE
        assert np.all(pos[0] == B)                              # Pos - offset exactly 0 (also with offset 0) becomes BoxSize
        assert np.all(pos[1] == B)                              # exactly BoxSize stays
        assert np.all((pos[2] > 0) & (pos[2] < 1e-3))           # just above: one box down
        assert np.all((pos[3] > 0) & (pos[3] <= B))
        assert np.all((pos[4] > 0) & (pos[4] <= B))
    allpos = sr.get_column("Position", 1, "f8", 3, c.P, c.slots, sel[offset[1]:offset[1] + count[1]], c.conv)
    assert np.all((allpos > 0) & (allpos <= sr.BOXSIZE))


def test_setters_invert_getters_on_representable_blocks():
    """gather, zero the records (Type and PI kept), read out: what a float column can hold comes back; ID, the bit fields, the positions
    inside the box and the integer members exactly"""
    c = sr.case(257)
    table = sq.io_blocks(1, 1, 1)
    P0, S0 = c.records()
    sel, count, offset = sr.select(P0, "all", "index")
    live = np.zeros(len(P0), dtype=bool)
    live[sel] = True
    P0 = P0[live]                       # the readout has no garbage test: drop garbage first, as a written snapshot does
    sel, count, offset = sr.select(P0, "all", "index")
    cols = sr.columns(table, P0, S0, sel, count, offset, c.conv)
    P1 = np.zeros_like(P0)
    P1["Type"], P1["PI"] = P0["Type"], P0["PI"]
    S1 = {t: np.zeros_like(s) for t, s in S0.items()}
    sr.readout(table, cols, P1, S1, c.conv)
    again = sr.columns(table, P1, S1, sel, count, offset, sr.Conv(offset=(0.0, 0.0, 0.0)))
    for key, col in cols.items():
        if key[1] in ("Potential", "GroupID", "StarFormationRate", "Velocity", "InternalEnergy"):
            continue      # write-only, or through an inexact product
        assert np.array_equal(again[key], col), key
    assert np.array_equal(P1["ID"], P0["ID"])
    kept = np.array([0xf4, 0, 0, 0, 0xf0, 0xf2], dtype=np.uint8)[P0["Type"]]   # Generation of gas, stars, black holes; HeIIIionized of gas; Swallowed of black holes
    assert np.array_equal(P1["Flags"], P0["Flags"] & kept)
    with np.errstate(all="ignore"):
        assert np.allclose(again[(0, "InternalEnergy")], cols[(0, "InternalEnergy")], rtol=3e-7)


@pytest.mark.parametrize("n", sr.COUNTS + (4096,))
def test_internal_energy_rows_near_a_float_boundary_are_rare(n):
    """the device's pow may differ from glibc's in the last bits of the double; rows within 2^-40 (relative) of a float32 rounding boundary are
    left out of the GPU tests' bit comparison: at most 1 % of the rows at every size"""
    if n == 4096:
        rng = np.random.default_rng(sr.SEED)
        ent, dens = np.exp(rng.normal(0, 3, n)), np.exp(rng.normal(0, 4, n))
    else:
        S = sr.case(n).slots[0]
        ent, dens = S["Entropy"], S["Density"]
    v = sr.internal_energy_f64(ent, dens, sr.ATIME)
    near = sr.near_f32_boundary(v)
    print(f"InternalEnergy, {len(v)} rows: {near.sum()} within 2^-40 of a float32 boundary")
    assert np.all(np.isfinite(v)) and np.all(v > 0)
    assert near.sum() <= 0.01 * max(len(v), 1)
    # the mask finds a planted boundary row and not its neighbourhood
    f = np.float32(1.5)
    mid = 0.5 * (float(f) + float(np.nextafter(f, np.float32(2))))
    assert sr.near_f32_boundary(np.array([mid, mid * (1 + 2.0 ** -41), mid * (1 + 2.0 ** -38), float(f)])).tolist() == [True, True, False, False]
