"""Device time of the domain decomposition's stages (shenqi_amd/csrc/domain.hip) on one rank: 256^3 particles from the bench's S-cluster
generator (--kind cluster, or uniform) as particle_data records, event times on the context's stream per stage, medians of --rounds.

  keys_packed      shq_peano_keys on packed positions (24 bytes in, 8 out per particle)
  keys_records     the same from inside the 160-byte records (what shq_slots_gc_sorted's keys cost)
  samples_presort  shq_domain_samples, PreSort = 1, distance 256: all keys, the 64-bit radix sort, the subsample
  samples_plain    PreSort = 0: one key per 256 slots
  local_toptree    shq_domain_local_toptree of the PreSort samples (limits of 4 top leaves)
  leaf_counts      shq_domain_leaf_counts on the finished tree
  topleaves        shq_domain_particle_topleaves (leaf and target per particle)
  decompose        DistDomain.decompose() with GpuDomainOps on one rank, wall clock: policy loop, balance, slots_gc_sorted included
The yardstick for the key and leaf-count passes is their traffic at the rate of a plain contiguous device copy measured in the same
run (read + written bytes per second; tools/copy_probe.hip measures the same on tiles): ratio = pass time / (bytes / copy rate).
Writes one JSON object to --out (profiles/domain_timing.json)."""
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
import shenqi_amd as sq  # noqa: E402
from shenqi_amd import capi, dist as sd  # noqa: E402

DEV = "cuda:0"
BOX = 1.0


def tables():
    """the key automaton: from the reference's function where oracle/_ref is built, else the stored derivation"""
    import domain_restated as dr
    return dr.tables()[0]


def timed(ctx, fn, rounds, warmup=1):
    ms = []
    for it in range(warmup + rounds):
        ctx.synchronize()
        capi.check(capi.hip.shq_timer_begin(ctx.h, 1))
        fn()
        capi.check(capi.hip.shq_timer_end(ctx.h, 1))
        ctx.synchronize()
        v = C.c_double()
        capi.check(capi.hip.shq_timer_elapsed_ms(ctx.h, 1, C.byref(v)))
        if it >= warmup:
            ms.append(v.value)
    return float(np.median(ms))


def copy_rate(nbytes):
    x = torch.empty(nbytes // 8, dtype=torch.float64, device=DEV).normal_()
    y = torch.empty_like(x)
    for _ in range(3):
        y.copy_(x)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(10):
        y.copy_(x)
    b.record()
    torch.cuda.synchronize()
    return 2 * nbytes * 10 / (a.elapsed_time(b) * 1e-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ngrid", type=int, default=256)
    ap.add_argument("--kind", default="cluster", choices=["cluster", "uniform"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "domain_timing.json"))
    args = ap.parse_args()
    n = args.ngrid ** 3
    t = tables()
    pos = sq.synth_positions(args.kind, n, L=BOX)
    f = capi.PARTICLE_DTYPE.fields
    esz = capi.PARTICLE_DTYPE.itemsize
    maxpart = n + n // 8
    P = np.zeros(maxpart, dtype=capi.PARTICLE_DTYPE)
    P["Pos"][:n] = pos
    P["ID"][:n] = np.arange(n)
    P["Type"] = 1
    d_parts = torch.from_numpy(P.view(np.uint8).reshape(-1)).to(DEV)
    d_pos = torch.from_numpy(np.ascontiguousarray(pos)).to(DEV)
    del P, pos
    d_keys = torch.empty(n, dtype=torch.int64, device=DEV)
    d_samples = torch.empty(n // 256 + 1, dtype=torch.int64, device=DEV)
    d_leaf = torch.empty(n, dtype=torch.int32, device=DEV)
    d_tgt = torch.empty(n, dtype=torch.int32, device=DEV)
    L = capi.ExchangeLayout()
    L.part_elsize, L.off_flags, L.off_type, L.off_pi = esz, f["Flags"][1], f["Type"][1], f["PI"][1]
    res = dict(ngrid=args.ngrid, kind=args.kind, n=n, device=torch.cuda.get_device_name(0))
    rate = copy_rate(1 << 29)
    res["copy_TBps"] = rate / 1e12
    with sq.Context(0) as ctx:
        pv = capi.DomainParts(d_parts.data_ptr(), esz, f["Flags"][1], f["Pos"][1], n, BOX)
        ns = C.c_int64()
        hip = capi.hip
        res["keys_packed_ms"] = timed(ctx, lambda: capi.check(hip.shq_peano_keys(ctx.h, C.byref(t), d_pos.data_ptr(), 24, n, BOX, d_keys.data_ptr())), args.rounds)
        res["keys_records_ms"] = timed(ctx, lambda: capi.check(hip.shq_peano_keys(ctx.h, C.byref(t), d_parts.data_ptr() + f["Pos"][1], esz, n, BOX, d_keys.data_ptr())),
                                       args.rounds)
        res["samples_plain_ms"] = timed(ctx, lambda: capi.check(hip.shq_domain_samples(ctx.h, C.byref(t), C.byref(pv), 256, 0, d_samples.data_ptr(), C.byref(ns))),
                                        args.rounds)
        res["samples_presort_ms"] = timed(ctx, lambda: capi.check(hip.shq_domain_samples(ctx.h, C.byref(t), C.byref(pv), 256, 1, d_samples.data_ptr(), C.byref(ns))),
                                          args.rounds)
        nsample = int(ns.value)
        maxtop = n // 4
        tree = np.zeros(maxtop, dtype=capi.LOCAL_TOPNODE_DTYPE)
        size = C.c_int()
        limit = nsample // 4
        res["local_toptree_ms"] = timed(ctx, lambda: capi.check(hip.shq_domain_local_toptree(ctx.h, d_samples.data_ptr(), nsample, limit, limit, maxtop,
                                                                                          tree.ctypes.data, C.byref(size))), args.rounds)
        res["nsample"], res["local_toptree_nodes"] = nsample, int(size.value)
        N, Lv = sd.GpuDomainOps.finish(tree[:size.value], maxtop, limit, limit)
        capi.check(hip.shq_domain_install(ctx.h, C.byref(t), N.ctypes.data, len(N), Lv.ctypes.data, len(Lv) - 1, None))
        count = np.zeros(len(Lv) - 1, dtype=np.int64)
        res["ntopleaves"] = len(Lv) - 1
        res["leaf_counts_ms"] = timed(ctx, lambda: capi.check(hip.shq_domain_leaf_counts(ctx.h, C.byref(pv), count.ctypes.data)), args.rounds)
        assert int(count.sum()) == n
        res["topleaves_ms"] = timed(ctx, lambda: capi.check(hip.shq_domain_particle_topleaves(ctx.h, C.byref(pv), d_leaf.data_ptr(), d_tgt.data_ptr())), args.rounds)
        ops = sd.GpuDomainOps(ctx, t, L, f["Pos"][1], f["TopLeaf"][1], BOX, d_parts, n, [None] * 6, [0] * 6)
        dd = sd.DistDomain(sd.Comm(), ops, dict(DomainOverDecompositionFactor=4, TopNodeAllocFactor=0.1))
        t0 = time.perf_counter()
        dd.decompose()
        ctx.synchronize()
        res["decompose_wall_ms"] = (time.perf_counter() - t0) * 1e3
        res["decompose_policy"], res["decompose_ntopleaves"], res["decompose_factor"] = dd.policy, len(dd.TopLeaves) - 1, dd.factor
    for name, nbytes in (("keys_packed", n * 32), ("keys_records", n * 32), ("leaf_counts", n * 25), ("topleaves", n * 33)):
        res[name + "_bytes"] = nbytes
        res[name + "_over_copy"] = res[name + "_ms"] * 1e-3 / (nbytes / rate)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
