"""Device time of the light-cone pass (shenqi_amd/csrc/lightcone.hip) on one rank: --ngrid^3 (256^3) Type-1 particles in 160-byte
particle_data records, an Einstein-de Sitter horizon table and two set_time calls that leave a few hundred replicas and a thin shell.

  pass_a_ms, scan_ms, pass_b_ms   shq_lightcone_phase_ms (HIP events around the kernels), medians of --rounds after one warm-up
  call_ms                         the whole synchronous call (host clock around it)
  rows                            crossings found
Three yardsticks from the same run:
  records_copy_ms    the record bytes once at the rate of a plain contiguous device copy (read + written bytes per second, the
                     method of tools/copy_rate.py): what reading the records costs at least
  arithmetic_ms      pairs x 24 f64 vector instructions (12 additions, 6 multiplications and 4 additions of the two squared distances,
                     2 compares) at the f64 rate tools/isa_rate_probe.hip measures on the same card (--probe: its output as a file; v_add_f64 with 8 waves per
                     SIMD; the compares issue at the same cost).  Without --probe the entry is left out.
  route_before       what a caller had without the device pass: a device-to-host copy of the records (host clock, pageable memory) plus
                     the loop as numpy expressions over all particles of one replica at a time.  The numpy part is timed on the first
                     --slice particles and SCALED by numpart / slice; its rows are compared with the device's rows of those particles.

Writes one JSON object to --out (profiles/lightcone_timing.json)."""
import argparse
import json
import os
import re
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
from domain_timing import copy_rate  # noqa: E402
import lightcone_restated as lr  # noqa: E402

DEV = "cuda:0"
DH = 2997.92458
OPS_PER_PAIR = 24


def records_on_device(n, box, rng_seed):
    """n Type-1 records made on the device: uniform positions, normal velocities, IDs 0 .. n-1"""
    f = capi.PARTICLE_DTYPE.fields
    g = torch.Generator(device=DEV)
    g.manual_seed(rng_seed)
    rec = torch.zeros((n, capi.PARTICLE_DTYPE.itemsize // 8), dtype=torch.float64, device=DEV)
    rec[:, f["Pos"][1] // 8:f["Pos"][1] // 8 + 3] = torch.rand((n, 3), dtype=torch.float64, device=DEV, generator=g) * box
    rec[:, f["Vel"][1] // 8:f["Vel"][1] // 8 + 3] = torch.randn((n, 3), dtype=torch.float64, device=DEV, generator=g) * 100.0
    rec.view(torch.int64)[:, f["ID"][1] // 8] = torch.arange(n, dtype=torch.int64, device=DEV)
    raw = rec.view(torch.uint8).view(n, capi.PARTICLE_DTYPE.itemsize)
    raw[:, f["Type"][1]] = 1
    return raw.view(-1)


def host_cross(P, st, ddrift, offset, rnd):
    """lightcone_cross, consistent form, as numpy expressions over all particles per replica: (rows, index, replica) unsorted"""
    who = np.flatnonzero(P["Type"] == 1)
    X, V, ids = P["Pos"][who], P["Vel"][who] * ddrift, P["ID"][who]
    size = np.uint64(len(rnd))
    out = []
    for i in range(st.Nreplica):
        pold = X + st.Reps[i] - offset
        pnew = X + st.Reps[i] + V - offset
        dold = (pold * pold).sum(axis=1)
        dnew = (pnew * pnew).sum(axis=1)
        hit = np.flatnonzero((dold <= st.HorizonDistance2Prev) & (dnew >= st.HorizonDistance2))
        hit = hit[~(rnd[((ids[hit] + np.uint64(i)) % size).astype(np.int64)] > st.SampleFraction)]
        if len(hit):
            cn, co = np.sqrt(dnew[hit]) - st.HorizonDistance, np.sqrt(dold[hit]) - st.HorizonDistancePrev
            same = dold[hit] == dnew[hit]
            with np.errstate(invalid="ignore", divide="ignore"):
                u1 = np.where(same, 0.5, -co / (cn - co))
                u2 = np.where(same, 0.5, cn / (cn - co))
            out.append((who[hit], np.full(len(hit), i), pold[hit] * u2[:, None] + pnew[hit] * u1[:, None]))
    if not out:
        return np.zeros((0, 3)), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    return np.concatenate([o[2] for o in out]), np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])


def probe_rate(path):
    """f64 vector lane operations per second of the whole chip, from the v_add_f64 line (8 waves per SIMD) of the text
    tools/isa_rate_probe.hip printed: (rate, line)"""
    text = open(path).read()
    ncu = int(re.search(r"(\d+) CUs", text).group(1))
    line = [x for x in text.splitlines() if x.startswith("add_f64")][0]
    ms = float(re.search(r"w=8: ([0-9.]+) ms", line).group(1))
    iters = int(re.search(r"16 instr x (\d+) iterations", text).group(1))
    return ncu * 8 * 4 * 16 * iters * 64 / (ms * 1e-3), line.strip()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ngrid", type=int, default=256)
    ap.add_argument("--box", type=float, default=300.0)
    ap.add_argument("--a0", type=float, default=0.2)
    ap.add_argument("--a1", type=float, default=0.2002)
    ap.add_argument("--ddrift", type=float, default=1e-3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--slice", type=int, default=1 << 18)
    ap.add_argument("--probe", default=None, help="what tools/isa_rate_probe.hip printed on this card, as a file")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lightcone_timing.json"))
    args = ap.parse_args()
    n = args.ngrid ** 3
    res = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, numpart=n, record_bytes=capi.PARTICLE_DTYPE.itemsize, BoxSize=args.box,
               a=[args.a0, args.a1], ddrift=args.ddrift, mode="consistent")
    if args.probe:
        rate64, line = probe_rate(args.probe)
        res["f64_vector_lane_ops_per_s"] = rate64
        res["isa_rate_probe_add_f64"] = line
    la, dc, dl = lr.eds_table(0.005, DH)
    lc = sq.Lightcone(la, dc, args.box, dloga=dl)
    want = lr.init_state(la, dc, dl)
    for a in (args.a0, args.a1):
        lc.set_time(a)
        lr.set_time(want, la, dc, dl, a, args.box)
    st = lc.state
    res.update(Nreplica=st.Nreplica, HorizonDistance=st.HorizonDistance, HorizonDistancePrev=st.HorizonDistancePrev, SampleFraction=st.SampleFraction)
    offset = (0.25 * args.box, -0.125 * args.box, 0.0)
    rnd = np.random.default_rng(20261019).random(100003)
    rate = copy_rate(1 << 29)
    res["copy_TBps"] = rate / 1e12
    d_parts = records_on_device(n, args.box, 20261019)
    L = sq.lightcone_layout()
    with sq.Context(0) as ctx:
        rc, nrows = sq.lightcone_compute_raw(ctx, L, d_parts, n, lc._state, capi.LIGHTCONE_CONSISTENT, args.ddrift, offset, rnd, None, None, None, 0)
        assert rc in (0, capi.ERR_NOMEM), rc
        rows = torch.empty((max(nrows, 1), 4), dtype=torch.float64, device=DEV)
        idx = torch.empty(max(nrows, 1), dtype=torch.int32, device=DEV)
        rep = torch.empty(max(nrows, 1), dtype=torch.int32, device=DEV)
        phases, wall = [], []
        for it in range(1 + args.rounds):
            ctx.synchronize()
            t0 = time.perf_counter()
            rc, m = sq.lightcone_compute_raw(ctx, L, d_parts, n, lc._state, capi.LIGHTCONE_CONSISTENT, args.ddrift, offset, rnd, rows, idx, rep, nrows)
            dt = (time.perf_counter() - t0) * 1e3
            assert rc == 0 and m == nrows
            if it:
                phases.append(sq.lightcone_phase_ms(ctx))
                wall.append(dt)
        pa, sc, pb = [float(x) for x in np.median(np.array(phases), axis=0)]
        pairs = n * st.Nreplica
        res.update(rows=int(nrows), pairs=int(pairs), pass_a_ms=pa, scan_ms=sc, pass_b_ms=pb, call_ms=float(np.median(wall)),
                   pass_a_spread_ms=[float(np.min(np.array(phases)[:, 0])), float(np.max(np.array(phases)[:, 0]))])
        res["records_copy_ms"] = n * capi.PARTICLE_DTYPE.itemsize / rate * 1e3
        res["pass_a_over_records_copy"] = pa / res["records_copy_ms"]
        if args.probe:
            res["f64_instructions_per_pair"] = OPS_PER_PAIR
            res["arithmetic_ms"] = pairs * OPS_PER_PAIR / res["f64_vector_lane_ops_per_s"] * 1e3
            res["pass_a_over_arithmetic"] = pa / res["arithmetic_ms"]
        # the route before
        t0 = time.perf_counter()
        hP = d_parts.cpu().numpy().view(capi.PARTICLE_DTYPE)
        d2h = (time.perf_counter() - t0) * 1e3
        k = min(args.slice, n)
        t0 = time.perf_counter()
        hrows, hidx, hrep = host_cross(hP[:k], want, args.ddrift, np.array(offset), rnd)
        sl = (time.perf_counter() - t0) * 1e3
        order = np.lexsort((hrep, hidx))
        didx = idx[:nrows].cpu().numpy()
        cut = int(np.searchsorted(didx, k))
        drows = rows[:cut].cpu().numpy()
        agree = cut == len(order) and np.array_equal(didx[:cut], hidx[order]) and np.array_equal(rep[:cut].cpu().numpy(), hrep[order])
        res["route_before"] = dict(d2h_records_ms=d2h, numpy_slice_particles=k, numpy_slice_ms=sl, numpy_scaled_ms=sl * n / k,
                                   scaled="numpy_scaled_ms = numpy_slice_ms x numpart / slice", total_ms=d2h + sl * n / k,
                                   slice_rows=int(len(order)), slice_rows_agree_with_device=bool(agree),
                                   slice_max_abs_diff=float(np.abs(drows[:, :3] - hrows[order]).max()) if agree and cut else None)
        res["route_before_over_device_call"] = res["route_before"]["total_ms"] / res["call_ms"]
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
