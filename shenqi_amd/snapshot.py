"""Snapshot blocks: the table of register_io_blocks / register_debug_io_blocks (libgadget/petaio.cpp:908-1047) as block descriptors over
the record dtypes, and the three device calls that turn device-resident records into typed columns and back (csrc/snapshot.hip):
shq_io_select, shq_io_gather, shq_io_scatter; the four ion-fraction columns come from shq_io_ion_fractions.

Records live in device memory behind objects with a data_ptr() (torch uint8 tensors); columns come back as numpy arrays."""
import ctypes as C

import numpy as np

from . import capi

_PLAIN = {"f8": np.dtype("<f8"), "f4": np.dtype("<f4"), "u8": np.dtype("<u8"), "u4": np.dtype("<u4"), "i4": np.dtype("<i4"), "u1": np.dtype("u1")}
# the bit fields of particle_data's flag byte (partmanager.h:19-23): (shift, width)
_BITS = {"IsGarbage": (0, 1), "Swallowed": (1, 1), "HeIIIionized": (2, 1), "BHHeated": (3, 1), "Generation": (4, 4)}
ION_BLOCKS = ("NeutralHydrogenFraction", "HeliumIFraction", "HeliumIIFraction", "HeliumIIIFraction")


class IOBlock:
    """One registration: name, ptype, dtype ("f4" ...), items, required, zorder (its place in the registration sequence), getter (a
    capi.IoBlock; None for the ion-fraction blocks, whose `ion` is 0..3), setter (a capi.IoBlock, or None for IO_REG_WRONLY)."""

    def __init__(self, name, ptype, dtype, items, required, zorder, getter, setter, ion=None):
        self.name, self.ptype, self.dtype, self.items, self.required, self.zorder = name, ptype, dtype, items, required, zorder
        self.getter, self.setter, self.ion = getter, setter, ion

    def key(self):
        return dict(name=self.name, ptype=self.ptype, dtype=self.dtype, items=self.items, required=self.required)

    def __repr__(self):
        return f"IOBlock({self.ptype}/{self.name} {self.dtype}x{self.items})"


def _field_type(dt):
    return capi.IO_TYPE_OF_DTYPE[f"{dt.kind}{dt.itemsize}"]


def _desc(source, rec_dtype, field, dtype, items, kind=capi.IO_COPY):
    dt, off = rec_dtype.fields[field][0], rec_dtype.fields[field][1]
    n = int(np.prod(dt.shape)) if dt.shape else 1
    if items > n:
        raise ValueError(f"{field}: {items} items asked of {n}")
    return capi.IoBlock(source, kind, _field_type(dt.base), capi.IO_TYPE_OF_DTYPE[dtype], items, 0, 0, 0, off, 0)


def io_blocks(WriteGroupID, MetalReturnOn, DensityIndependentSph, debug=False, OutputPotential=True, OutputTimebins=False, OutputHeliumFractions=False,
              part_dtype=None, sph_dtype=None, star_dtype=None, bh_dtype=None):
    """The IOTable of register_io_blocks(IOTable, WriteGroupID, MetalReturnOn) - with register_debug_io_blocks appended under `debug` -
    sorted as the reference sorts it: by particle type, then by registration order.  The Output* switches are the reference's parameters of
    those names, at their defaults.  The J21 / ZReionized blocks of EXCUR_REION builds are present when sph_dtype has local_J21 / zreion."""
    P = capi.PARTICLE_DTYPE if part_dtype is None else part_dtype
    slot = {0: capi.SPH_DTYPE if sph_dtype is None else sph_dtype, 4: capi.STAR_DTYPE if star_dtype is None else star_dtype,
            5: capi.BH_DTYPE if bh_dtype is None else bh_dtype}
    table = []
    BASE, SLOT = capi.IO_SRC_BASE, capi.IO_SRC_SLOT

    def reg(name, dtype, items, ptype, required, getter, rw, ion=None):
        setter = None
        if rw:
            setter = capi.IoBlock.from_buffer_copy(getter)
        table.append(IOBlock(name, ptype, dtype, items, required, len(table), getter, setter, ion))

    def base(name, dtype, items, ptype, field, required=1, rw=True, kind=capi.IO_COPY):
        reg(name, dtype, items, ptype, required, _desc(BASE, P, field, dtype, items, kind), rw)

    def pi(name, dtype, items, ptype, field, required=1, rw=True, kind=capi.IO_COPY):
        reg(name, dtype, items, ptype, required, _desc(SLOT, slot[ptype], field, dtype, items, kind), rw)

    def bits(name, ptype, field, required):
        shift, width = _BITS[field]
        reg(name, "u1", 1, ptype, required, capi.IoBlock(BASE, capi.IO_COPY, capi.IO_BITS, capi.IO_U8, 1, shift, width, 0, P.fields["Flags"][1], 0), True)

    # ---- register_io_blocks, petaio.cpp:908-1007 ----
    for i in range(6):
        base("Mass", "f4", 1, i, "Mass")
        base("Position", "f8", 3, i, "Pos", kind=capi.IO_POSITION)
        base("Velocity", "f4", 3, i, "Vel", kind=capi.IO_SCALE)
        base("ID", "u8", 1, i, "ID")
        if OutputPotential:
            base("Potential", "f4", 1, i, "Potential", rw=False)
        if WriteGroupID:
            base("GroupID", "u4", 1, i, "GrNr", rw=False)
        if OutputTimebins:
            base("TimeBinHydro", "u4", 1, i, "TimeBinHydro", rw=False)
            base("TimeBinGravity", "u4", 1, i, "TimeBinGravity", rw=False)
    for t in (0, 4, 5):
        bits("Generation", t, "Generation", 1)
    base("SmoothingLength", "f4", 1, 0, "Hsml")
    pi("Density", "f4", 1, 0, "Density")
    if DensityIndependentSph:
        pi("EgyWtDensity", "f4", 1, 0, "EgyWtDensity")
    ie = _desc(SLOT, slot[0], "Entropy", "f4", 1, capi.IO_INTERNAL_ENERGY)
    ie.offset2 = slot[0].fields["Density"][1]
    reg("InternalEnergy", "f4", 1, 0, 1, ie, True)
    pi("ElectronAbundance", "f4", 1, 0, "Ne")
    reg("NeutralHydrogenFraction", "f4", 1, 0, 1, None, False, ion=0)
    if OutputHeliumFractions:
        for q in (1, 2, 3):
            reg(ION_BLOCKS[q], "f4", 1, 0, 1, None, False, ion=q)
    bits("HeIIIIonized", 0, "HeIIIionized", 0)
    pi("StarFormationRate", "f4", 1, 0, "Sfr", rw=False)
    pi("DelayTime", "f4", 1, 0, "DelayTime", required=0)
    pi("BirthDensity", "f4", 1, 4, "BirthDensity", required=0)
    pi("StarFormationTime", "f4", 1, 4, "FormationTime", required=0)
    pi("Metallicity", "f4", 1, 0, "Metallicity", required=0)
    pi("Metallicity", "f4", 1, 4, "Metallicity", required=0)
    if MetalReturnOn:
        pi("Metals", "f4", int(np.prod(slot[0].fields["Metals"][0].shape)), 0, "Metals", required=0)
        pi("Metals", "f4", int(np.prod(slot[4].fields["Metals"][0].shape)), 4, "Metals", required=0)
        pi("LastEnrichmentMyr", "f4", 1, 4, "LastEnrichmentMyr", required=0)
        pi("TotalMassReturned", "f4", 1, 4, "TotalMassReturned", required=0)
        base("SmoothingLength", "f4", 1, 4, "Hsml", required=0)
    pi("StarFormationTime", "f4", 1, 5, "FormationTime", required=0)
    pi("BlackholeMass", "f4", 1, 5, "Mass")
    pi("BlackholeDensity", "f4", 1, 5, "Density")
    pi("BlackholeAccretionRate", "f4", 1, 5, "Mdot")
    pi("BlackholeProgenitors", "i4", 1, 5, "CountProgs")
    pi("BlackholeMinPotPos", "f8", 3, 5, "MinPotPos", kind=capi.IO_POSITION)
    pi("BlackholeJumpToMinPot", "i4", 1, 5, "JumpToMinPot")
    pi("BlackholeMtrack", "f4", 1, 5, "Mtrack")
    pi("BlackholeMseed", "f4", 1, 5, "Mseed", required=0)
    pi("BlackholeKineticFdbkEnergy", "f4", 1, 5, "KineticFdbkEnergy", required=0)
    base("SmoothingLength", "f4", 1, 5, "Hsml", required=0)
    bits("Swallowed", 5, "Swallowed", 0)
    pi("BlackholeSwallowID", "u8", 1, 5, "SwallowID", required=0)
    pi("BlackholeSwallowTime", "f4", 1, 5, "SwallowTime", required=0)
    if "local_J21" in slot[0].fields and "zreion" in slot[0].fields:
        pi("J21", "f4", 1, 0, "local_J21", required=0)
        pi("ZReionized", "f4", 1, 0, "zreion", required=0)
    # ---- register_debug_io_blocks, :1025-1049 ----
    if debug:
        for t in range(6):
            base("GravAccel", "f4", 3, t, "FullTreeGravAccel", rw=False)
            base("GravPM", "f4", 3, t, "GravPM", rw=False)
            if not OutputTimebins:
                base("TimeBinHydro", "u4", 1, t, "TimeBinHydro", rw=False)
                base("TimeBinGravity", "u4", 1, t, "TimeBinGravity", rw=False)
        pi("HydroAccel", "f4", 3, 0, "HydroAccel", rw=False)
        for name, field in (("MaxSignalVel", "MaxSignalVel"), ("Entropy", "Entropy"), ("DtEntropy", "DtEntropy"), ("DhsmlEgyDensityFactor", "DhsmlEgyDensityFactor"),
                            ("DivVel", "DivVel"), ("CurlVel", "CurlVel"), ("VelDisp", "VDisp")):
            pi(name, "f4", 1, 0, field, rw=False)
        pi("BHVelDisp", "f4", 1, 5, "VDisp", rw=False)
        pi("StarVelDisp", "f4", 1, 4, "VDisp", rw=False)
    table.sort(key=lambda b: (b.ptype, b.zorder))  # order_by_type
    return table


def io_layout(part_dtype=None, slot_dtypes=None):
    """shq_io_layout of the record dtypes (slot_dtypes: {ptype: dtype}; default gas, star and black-hole slots)"""
    P = capi.PARTICLE_DTYPE if part_dtype is None else part_dtype
    slots = {0: capi.SPH_DTYPE, 4: capi.STAR_DTYPE, 5: capi.BH_DTYPE} if slot_dtypes is None else slot_dtypes
    L = capi.IoLayout()
    f = P.fields
    L.part_elsize, L.off_flags, L.off_type, L.off_pi, L.off_grnr = P.itemsize, f["Flags"][1], f["Type"][1], f["PI"][1], f["GrNr"][1]
    for t in range(6):
        L.slot_elsize[t] = slots[t].itemsize if slots.get(t) is not None else 0
    return L


def io_conv(atime=1.0, BoxSize=1.0, CurrentParticleOffset=(0.0, 0.0, 0.0), UsePeculiarVelocity=False, setter=False):
    """shq_io_conv: fac is GTVelocity's 1 / atime (STVelocity's atime under `setter`) with UsePeculiarVelocity, else 1"""
    fac = (float(atime) if setter else 1.0 / float(atime)) if UsePeculiarVelocity else 1.0
    return capi.IoConv(fac, float(atime), float(BoxSize), (C.c_double * 3)(*[float(x) for x in CurrentParticleOffset]))


def _slot_args(d_slots, slot_size):
    sp = (C.c_void_p * 6)(*[None if d_slots is None or d_slots[t] is None else d_slots[t].data_ptr() for t in range(6)])
    sz = (C.c_int64 * 6)(*[0 if slot_size is None else int(slot_size[t]) for t in range(6)])
    return sp, sz


def io_select(ctx, layout, d_parts, numpart, predicate=capi.IO_SELECT_ALL, order=capi.IO_ORDER_INDEX):
    """shq_io_select: (d_selection, count[6], offset[6]); d_selection is an int32 torch tensor of numpart entries on the records' device"""
    import torch
    sel = torch.empty(max(int(numpart), 1), dtype=torch.int32, device=d_parts.device)
    count, offset = (C.c_int64 * 6)(), (C.c_int64 * 6)()
    capi.check(capi.hip.shq_io_select(ctx.h, C.byref(layout), d_parts.data_ptr(), int(numpart), int(predicate), int(order), sel.data_ptr(), count, offset), "io_select")
    return sel, np.array(count[:], dtype=np.int64), np.array(offset[:], dtype=np.int64)


def io_gather(ctx, layout, d_parts, numpart, d_slots, slot_size, ptype, d_selection, first, n, blocks, conv):
    """shq_io_gather for rows first .. first + n of d_selection: one numpy array [n, items] (or [n]) per block (capi.IoBlock getters)"""
    import torch
    arr = (capi.IoBlock * max(len(blocks), 1))(*blocks)
    tdt = {capi.IO_F64: torch.float64, capi.IO_F32: torch.float32, capi.IO_U64: torch.int64, capi.IO_I64: torch.int64, capi.IO_U32: torch.int32, capi.IO_I32: torch.int32,
           capi.IO_U8: torch.uint8, capi.IO_I8: torch.int8}
    ndt = {capi.IO_F64: "<f8", capi.IO_F32: "<f4", capi.IO_U64: "<u8", capi.IO_I64: "<i8", capi.IO_U32: "<u4", capi.IO_I32: "<i4", capi.IO_U8: "u1", capi.IO_I8: "i1"}
    cols = [torch.zeros((max(int(n), 1), b.items), dtype=tdt[b.col_type], device=d_parts.device) for b in blocks]
    outp = (C.c_void_p * max(len(blocks), 1))(*[c.data_ptr() for c in cols])
    sp, sz = _slot_args(d_slots, slot_size)
    selp = d_selection.data_ptr() + 4 * int(first)
    capi.check(capi.hip.shq_io_gather(ctx.h, C.byref(layout), d_parts.data_ptr(), int(numpart), sp, sz, int(ptype), selp, int(n), arr, len(blocks), C.byref(conv), outp),
               "io_gather")
    res = []
    for b, c in zip(blocks, cols):
        a = c.cpu().numpy()[:int(n)].view(ndt[b.col_type])
        res.append(a[:, 0].copy() if b.items == 1 else a.copy())
    return res


def io_scatter(ctx, layout, d_parts, numpart, d_slots, slot_size, ptype, blocks, columns, conv):
    """shq_io_scatter: columns[b] (numpy, [n] or [n, items] of the block's file type) into the records of the particles of `ptype`, block by
    block in list order per particle (capi.IoBlock setters)"""
    import torch
    arr = (capi.IoBlock * max(len(blocks), 1))(*blocks)
    n = len(columns[0]) if columns else 0
    ndt = {capi.IO_F64: "<f8", capi.IO_F32: "<f4", capi.IO_U64: "<u8", capi.IO_I64: "<i8", capi.IO_U32: "<u4", capi.IO_I32: "<i4", capi.IO_U8: "u1", capi.IO_I8: "i1"}
    dev = []
    for b, c in zip(blocks, columns):
        c = np.ascontiguousarray(c, dtype=ndt[b.col_type]).reshape(-1)
        if len(c) != n * b.items:
            raise ValueError("io_scatter: every column has one row per particle of the type")
        pad = c if len(c) else np.zeros(1, dtype=c.dtype)
        dev.append(torch.from_numpy(pad.view(np.uint8).copy()).to(d_parts.device))
    inp = (C.c_void_p * max(len(blocks), 1))(*[d.data_ptr() for d in dev])
    sp, sz = _slot_args(d_slots, slot_size)
    capi.check(capi.hip.shq_io_scatter(ctx.h, C.byref(layout), d_parts.data_ptr(), int(numpart), sp, sz, int(ptype), int(n), arr, len(blocks), C.byref(conv), inp),
               "io_scatter")
    ctx.synchronize()   # the staged columns must outlive the kernels


def io_ion_fractions(ctx, pman, SphP, par, step, list_=None, which=(0, 1, 2, 3)):
    """shq_io_ion_fractions on host views (as starformation()): ({q: float32[n]}, status[n], listed, capi.IoIonResult); rows of the
    particles in `listed` (positions in the list) hold NaN and are the caller's to fill with the reference's own function"""
    pv, sv = pman.view(), capi.sph_view(SphP)
    f = SphP.dtype.fields
    sf = capi.SfrFields(f["Ne"][1], f["Metallicity"][1], f["Sfr"][1], f["DelayTime"][1])
    lst = None if list_ is None else np.ascontiguousarray(list_, dtype=np.int32)
    n = pman.NumPart if lst is None else len(lst)
    cols = {q: np.zeros(max(n, 1), dtype=np.float32) for q in which}
    outp = (C.c_void_p * 4)(*[cols[q].ctypes.data if q in cols else None for q in range(4)])
    status, listed = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.int32)
    res = capi.IoIonResult()
    mask = sum(1 << q for q in which)
    capi.check(capi.hip.shq_io_ion_fractions(ctx.h, C.byref(pv), C.byref(sv), C.byref(sf), C.byref(par), C.byref(step), capi.ptr(lst), n, mask, outp, capi.ptr(status),
                                             capi.ptr(listed), n, C.byref(res)), "io_ion_fractions")
    return {q: c[:n] for q, c in cols.items()}, status[:n], listed[:res.n_listed].copy(), res


def snapshot_columns(ctx, table, d_parts, numpart, d_slots, slot_size, conv, predicate=capi.IO_SELECT_ALL, order=capi.IO_ORDER_INDEX, layout=None, ion=None):
    """petaio_save_snapshot's loop (petaio.cpp:156-172) on device records: one selection, then per particle type one gather of all its
    blocks.  Returns ({(ptype, name): numpy array}, selection as numpy, count, offset).  The ion-fraction blocks of the table are filled by
    `ion`, a callable (gas_indices) -> {q: float32 array} (e.g. around io_ion_fractions, which works on host views), and left out without
    one.  Types without selected particles give empty columns."""
    L = io_layout() if layout is None else layout
    sel, count, offset = io_select(ctx, L, d_parts, numpart, predicate, order)
    out = {}
    for t in range(6):
        blocks = [b for b in table if b.ptype == t and b.getter is not None]
        cols = io_gather(ctx, L, d_parts, numpart, d_slots, slot_size, t, sel, offset[t], count[t], [b.getter for b in blocks], conv)
        for b, c in zip(blocks, cols):
            out[(t, b.name)] = c
    hsel = sel.cpu().numpy()[:int(count.sum())]
    ions = [b for b in table if b.ion is not None]
    if ion is not None and ions:
        got = ion(hsel[offset[0]:offset[0] + count[0]])
        for b in ions:
            out[(0, b.name)] = got[b.ion]
    return out, hsel, count, offset


def snapshot_readout(ctx, table, columns, d_parts, numpart, d_slots, slot_size, conv, layout=None):
    """The inverse: petaio_readout_buffer for every block of `table` that has a setter and a column in `columns` ({(ptype, name): array}),
    per type in table order (so Density lands before InternalEnergy, as the registration order arranges)."""
    L = io_layout() if layout is None else layout
    for t in range(6):
        blocks = [b for b in table if b.ptype == t and b.setter is not None and (t, b.name) in columns]
        if blocks:
            io_scatter(ctx, L, d_parts, numpart, d_slots, slot_size, t, [b.setter for b in blocks], [columns[(t, b.name)] for b in blocks], conv)
