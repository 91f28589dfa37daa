"""Device time of the snapshot path (shenqi_amd/csrc/snapshot.hip) on one rank, for two sets of particle_data records:

  gas_dm    2 x 128^3: gas and dark matter interleaved at random, the gas with 176-byte SPH slots in shuffled PI order
  dm        256^3 dark matter only

per set: shq_io_select, shq_io_gather per particle type over all blocks sq.io_blocks(1, 1, 1) registers for the type, and (gas_dm) the
NeutralHydrogenFraction column of shq_io_ion_fractions (its kernel's HIP-event time; the gas state drawn as tools/time_sfr.py draws it).
Event times on the context's stream, medians of --rounds after one warm-up.  Two yardsticks from the same run:

  *_over_copy     pass time / (the bytes the pass must move / the rate of a plain contiguous device copy): records once (base record, and
                  the slot record where a block reads it), the selection once, every column once.  tools/domain_timing.py's ratio.
  parent_route    what a caller had before these calls: a device-to-host copy of the record arrays (wall clock, pageable memory) and the
                  getters as numpy expressions on the host (one pass per block over the selected records), once.

Writes one JSON object to --out (profiles/snapshot_timing.json)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import shenqi_amd as sq  # noqa: E402
from shenqi_amd import capi  # noqa: E402
from domain_timing import timed, copy_rate  # noqa: E402

DEV = "cuda:0"
BOXSIZE = 20000.0
OFFSET = (0.25 * BOXSIZE, -0.125 * BOXSIZE, 0.0)
ATIME = 0.25
COLSIZE = {"f8": 8, "f4": 4, "u8": 8, "u4": 4, "i4": 4, "u1": 1}
TORCH_DT = {"f8": torch.float64, "f4": torch.float32, "u8": torch.int64, "u4": torch.int32, "i4": torch.int32, "u1": torch.uint8}


def dev(a):
    return torch.from_numpy(a.view(np.uint8).reshape(-1)).to(DEV)


def host_getters(table, P, S, sel, count, offset):
    """the getters as numpy expressions over the selected records: one pass per block"""
    out = {}
    for t in range(6):
        s = sel[offset[t]:offset[t] + count[t]]
        if len(s) == 0:
            continue
        rows = P[s]
        srows = S[rows["PI"]] if t == 0 and S is not None else None
        for b in table:
            if b.ptype != t or b.getter is None:
                continue
            g = b.getter
            rec, dt = (rows, capi.PARTICLE_DTYPE) if g.source == capi.IO_SRC_BASE else (srows, capi.SPH_DTYPE)
            if rec is None:
                continue
            member = [k for k in dt.names if dt.fields[k][1] == g.offset][0]
            if g.kind == capi.IO_POSITION:
                x = rec[member] - np.array(OFFSET)
                x -= BOXSIZE * np.ceil(x / BOXSIZE - 1)
                out[(t, b.name)] = x
            elif g.kind == capi.IO_SCALE:
                out[(t, b.name)] = (rec[member] / ATIME).astype(np.float32)
            elif g.kind == capi.IO_INTERNAL_ENERGY:
                out[(t, b.name)] = (rec["Entropy"] / (2.0 / 3.0) * np.power(rec["Density"] / ATIME ** 3, 2.0 / 3.0)).astype(np.float32)
            elif g.field_type == capi.IO_BITS:
                out[(t, b.name)] = (rec["Flags"] >> g.bit_shift) & ((1 << g.bit_width) - 1)
            else:
                out[(t, b.name)] = rec[member].astype({"f8": "<f8", "f4": "<f4", "u8": "<u8", "u4": "<u4", "i4": "<i4", "u1": "u1"}[b.dtype])
    return out


def run_set(ctx, name, P, S, table, rate, rounds, res):
    n = len(P)
    L = sq.io_layout()
    cv = sq.io_conv(ATIME, BOXSIZE, OFFSET, True)
    d_parts = dev(P)
    d_slots = [dev(S) if S is not None else None] + [None] * 5
    slot_size = [len(S) if S is not None else 0] + [0] * 5
    sel = torch.empty(n, dtype=torch.int32, device=DEV)
    count, offset = (C.c_int64 * 6)(), (C.c_int64 * 6)()

    def select():
        capi.check(capi.hip.shq_io_select(ctx.h, C.byref(L), d_parts.data_ptr(), n, capi.IO_SELECT_ALL, capi.IO_ORDER_INDEX, sel.data_ptr(), count, offset))

    r = res[name] = dict(n=n)
    r["select_ms"] = timed(ctx, select, rounds)
    r["select_bytes"] = n * (160 + 4)     # every record's flag byte and Type cost its cache lines; the selection once
    r["select_over_copy"] = r["select_ms"] * 1e-3 / (r["select_bytes"] / rate)
    sp = (C.c_void_p * 6)(*[None if d is None else d.data_ptr() for d in d_slots])
    sz = (C.c_int64 * 6)(*slot_size)
    for t in range(6):
        m = int(count[t])
        if m == 0:
            continue
        blocks = [b for b in table if b.ptype == t and b.getter is not None]
        arr = (capi.IoBlock * len(blocks))(*[b.getter for b in blocks])
        cols = [torch.empty((m, b.items), dtype=TORCH_DT[b.dtype], device=DEV) for b in blocks]
        outp = (C.c_void_p * len(blocks))(*[c.data_ptr() for c in cols])
        selp = sel.data_ptr() + 4 * int(offset[t])

        def gather(k=len(blocks)):
            capi.check(capi.hip.shq_io_gather(ctx.h, C.byref(L), d_parts.data_ptr(), n, sp, sz, t, selp, m, arr, k, C.byref(cv), outp))

        slot = any(b.getter.source == capi.IO_SRC_SLOT for b in blocks)
        colbytes = sum(COLSIZE[b.dtype] * b.items for b in blocks)
        nbytes = m * (160 + (capi.SPH_DTYPE.itemsize if slot else 0) + 4 + colbytes)
        g = r[f"gather_type{t}"] = dict(rows=m, blocks=len(blocks), column_bytes_per_row=colbytes, bytes=nbytes)
        g["ms"] = timed(ctx, gather, rounds)
        g["over_copy"] = g["ms"] * 1e-3 / (nbytes / rate)
        # the same columns one block per call: what per-block kernels would cost
        one = 0.0
        for k in range(len(blocks)):
            a1 = (capi.IoBlock * 1)(blocks[k].getter)
            o1 = (C.c_void_p * 1)(cols[k].data_ptr())
            one += timed(ctx, lambda: capi.check(capi.hip.shq_io_gather(ctx.h, C.byref(L), d_parts.data_ptr(), n, sp, sz, t, selp, m, a1, 1, C.byref(cv), o1)), 1)
        g["one_block_per_call_ms"] = one
        del cols
    # the parent route, once
    t0 = time.perf_counter()
    hP = d_parts.cpu().numpy()[:P.nbytes].view(P.dtype)
    hS = d_slots[0].cpu().numpy()[:S.nbytes].view(S.dtype) if S is not None else None
    r["parent_d2h_ms"] = (time.perf_counter() - t0) * 1e3
    hsel = sel.cpu().numpy()
    t0 = time.perf_counter()
    host_getters(table, hP, hS, hsel, list(count), list(offset))
    r["parent_numpy_getters_ms"] = (time.perf_counter() - t0) * 1e3
    dev_ms = r["select_ms"] + sum(v["ms"] for k, v in r.items() if k.startswith("gather_type"))
    r["device_select_and_gather_ms"] = dev_ms
    r["parent_route_over_device"] = (r["parent_d2h_ms"] + r["parent_numpy_getters_ms"]) / dev_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ngas", type=int, default=128)
    ap.add_argument("--ndm", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snapshot_timing.json"))
    args = ap.parse_args()
    import sfr_cases as sc
    import time_sfr
    table = sq.io_blocks(1, 1, 1)
    res = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, blocks="sq.io_blocks(WriteGroupID=1, MetalReturnOn=1, DensityIndependentSph=1)")
    rate = copy_rate(1 << 29)
    res["copy_TBps"] = rate / 1e12
    rng = np.random.default_rng(20261019)
    with sq.Context(0) as ctx:
        # ---- gas + dark matter ----
        ng = args.ngas ** 3
        par = sc.params(avg_baryon_mass=1.0)
        G, S, ids, _ = time_sfr.particles(ng, par)
        n = 2 * ng
        P = np.zeros(n, dtype=capi.PARTICLE_DTYPE)
        order = rng.permutation(n)
        gi, di = np.sort(order[:ng]), np.sort(order[ng:])
        P[gi] = G
        P["Type"][di] = 1
        P["Pos"][di] = rng.random((ng, 3)) * BOXSIZE
        P["Mass"][di] = 1.0
        P["PI"][gi] = rng.permutation(ng)
        Ssh = np.zeros_like(S)
        Ssh[P["PI"][gi]] = S
        P["ID"] = rng.permutation(n).astype(np.uint64)
        P["GrNr"] = rng.integers(-1, 1000, n)
        P["Vel"] = rng.normal(0, 100, (n, 3))
        run_set(ctx, "gas_dm", P, Ssh, table, rate, args.rounds, res)
        # the ion-fraction column: host views, as shq_starformation takes them
        sq.cooling_set_tables(ctx, sc.case().tables())
        pman = sq.PartManager(n, BOXSIZE)
        pman.Base[:] = P
        st = time_sfr.step(par)
        ms = []
        for it in range(3):
            _, status, listed, ir = sq.io_ion_fractions(ctx, pman, Ssh, sc.lib_params(par), st, list_=gi.astype(np.int32), which=(0,))
            ms.append(ir.kernel_ms)
        res["gas_dm"]["ion_nh0_kernel_ms"] = float(np.median(ms[1:]))
        res["gas_dm"]["ion_nh0_rows"] = int(len(gi))
        res["gas_dm"]["ion_nh0_refused"] = int(ir.n_listed)
        res["gas_dm"]["ion_nh0_steps_per_row"] = ir.steps / len(gi)
        del pman, P, G, S, Ssh
        # ---- dark matter only ----
        n = args.ndm ** 3
        P = np.zeros(n, dtype=capi.PARTICLE_DTYPE)
        P["Type"] = 1
        P["Pos"] = rng.random((n, 3)) * BOXSIZE
        P["Vel"] = rng.normal(0, 100, (n, 3))
        P["Mass"] = 1.0
        P["ID"] = np.arange(n, dtype=np.uint64)
        P["Potential"] = rng.normal(0, 1e4, n)
        run_set(ctx, "dm", P, None, table, rate, args.rounds, res)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
