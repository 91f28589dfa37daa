"""Times the linear-response neutrino step on the device (csrc/nulra.hip) inside the PM, and the gap the host route leaves.

    python tools/time_nulra.py [--probe <output of tools/isa_rate_probe.hip on the same card>]   ->  profiles/nulra_timing.json

Per (Nmesh, Na) with three massive species, 128^3 particles:
  device_ms           node-table upload, delta_nu kernels (get_delta_nu of every bin and species, and their sum), mode table: HIP events
  callback_s          host time of the step's node table, the ~10^4 callbacks in it (Python callables here: a C caller's cost less)
  gap_new_ms          wall time from the end of the forward to the moment the finish can start when the step is only called then:
                      shq_nulra_step (the host's node table first), then the device idle
  gap_new_queued_ms   the same when the step is called right behind the forward (it does not wait): (forward + step, then wait) - (forward,
                      then wait); the host builds the node table while the forward runs (forward_ms)
  gap_host_T1_ms      the same for the route before with none of its physics: shq_pm_download_power, a table of ones, shq_pm_set_mode_factor
                      (a lower bound of the old route: delta_nu_from_power and the spline loop over 3 (Nmesh/2)^2 modes come on top)
  f64_floor_ms        nodes x bins x species x NU_F64_PER_NODE vector f64 instructions at the rate tools/isa_rate_probe.hip measured
The reference's own delta_nu_from_power is not timed: it does not build without boost."""
import argparse
import ctypes as C
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import shenqi_amd as sq  # noqa: E402
from shenqi_amd import capi  # noqa: E402
import nulra_restated as nr  # noqa: E402
import nulra_cases as nc  # noqa: E402

# vector f64 instructions per node of nulra_delta_nu_kernel's loop on the specialJ_fit path, counted in the gfx950 code object
# (hipcc --offload-device-only -S of nulra.hip: the v_*_f64 of the loop's head and its specialJ_fit block, 119 - most of them the log and
# the exp of x^4.1811 and two divisions - and of its tail, 10: the row's four products, W J delta; the Jfrac_high block left out)
NU_F64_PER_NODE = 129


def probe_rate(path):
    text = open(path).read()
    ncu = int(re.search(r"(\d+) CUs", text).group(1))
    line = [x for x in text.splitlines() if x.startswith("add_f64")][0]
    ms = float(re.search(r"w=8: ([0-9.]+) ms", line).group(1))
    iters = int(re.search(r"16 instr x (\d+) iterations", text).group(1))
    return ncu * 8 * 4 * 16 * iters * 64 / (ms * 1e-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nmesh", type=int, nargs="*", default=[512, 1024])
    ap.add_argument("--na", type=int, nargs="*", default=[32, 128])
    ap.add_argument("--ngrid", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--probe", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nulra_timing.json"))
    args = ap.parse_args()
    import torch
    if args.probe:
        rate64 = probe_rate(args.probe)
    else:   # the rate recorded with the light-cone timing on the same kind of card
        rate64 = json.load(open(os.path.join(ROOT, "profiles", "lightcone_timing.json")))["f64_vector_lane_ops_per_s"]
    res = dict(device=torch.cuda.get_device_name(0), numpart=args.ngrid**3, rounds=args.rounds, species=3, f64_vector_lane_ops_per_s=rate64,
               f64_per_node=NU_F64_PER_NODE, cases=[])
    import common as cm
    import orc
    n = args.ngrid**3
    pos = cm.random_positions(orc.boost_mt19937_uniform(1, 3 * n), n)
    c = nr.Cosmo([0.1, 0.06, 0.05], [1, 1, 1], H0=100.0)
    with sq.Context(0) as ctx:
        h = ctx.h
        pman = cm.make_partmanager(pos)
        pv = pman.view()
        capi.check(capi.hip.shq_particles_upload(h, C.byref(pv)))
        for N in args.nmesh:
            pmp = sq.PMParams(N, 0, cm.BOX, 1.5, cm.G)
            ones = np.ones(3 * (N // 2) ** 2 + 1)
            kk, pw, nm, norm = np.zeros(N), np.zeros(N), np.zeros(N, dtype=np.int64), C.c_double()
            for Na in args.na:
                with nc.make(ctx, c, nk_allocated=N, TimeMax=1.2) as nu:
                    # first init on this mesh's bins, then a history of Na spectra a = 0.01 .. 0.5 grown linearly from it
                    capi.check(capi.hip.shq_pm_forward(h, C.byref(pmp)))
                    nu.step(0.01, 0.01)
                    capi.check(capi.hip.shq_pm_run(h, C.byref(pmp)))
                    st = nu.get_state()
                    a = 0.01 * 50 ** (np.arange(Na) / (Na - 1.0))
                    st.update(ia=Na, scalefact=np.log(a), delta_tot=np.ascontiguousarray(st["delta_tot"][:, :1] * (a[None, :] / 0.01)))
                    nu.set_state(st)
                    gaps, steps, infos = [], [], []
                    for r in range(args.rounds + 1):
                        t = 0.5 + 0.02 * (r + 1)
                        capi.check(capi.hip.shq_pm_forward(h, C.byref(pmp)))
                        ctx.synchronize()
                        t0 = time.perf_counter()
                        nu.step(t, 0.01)
                        t1 = time.perf_counter()
                        ctx.synchronize()
                        t2 = time.perf_counter()
                        capi.check(capi.hip.shq_pm_run(h, C.byref(pmp)))
                        if r > 0:   # the first round sizes buffers
                            gaps.append((t2 - t0) * 1e3)
                            steps.append((t1 - t0) * 1e3)
                            infos.append(nu.info())
                    # the same with the step queued right behind the forward, as a run calls it: the host builds the node table while the
                    # forward runs; what the step adds to forward + wait is the gap a run sees
                    fwd, both = [], []
                    for r in range(2 * (args.rounds + 1)):
                        with_step = r % 2 == 1
                        t = 0.7 + 0.01 * (r + 1)
                        ctx.synchronize()
                        t0 = time.perf_counter()
                        capi.check(capi.hip.shq_pm_forward(h, C.byref(pmp)))
                        if with_step:
                            nu.step(t, 0.01)
                        ctx.synchronize()
                        t1 = time.perf_counter()
                        capi.check(capi.hip.shq_pm_run(h, C.byref(pmp)))
                        if r > 1:
                            (both if with_step else fwd).append((t1 - t0) * 1e3)
                    old = []
                    for r in range(args.rounds + 1):
                        capi.check(capi.hip.shq_pm_forward(h, C.byref(pmp)))
                        ctx.synchronize()
                        t0 = time.perf_counter()
                        capi.check(capi.hip.shq_pm_download_power(h, N, capi.ptr(kk), capi.ptr(pw), capi.ptr(nm), C.byref(norm)))
                        capi.check(capi.hip.shq_pm_set_mode_factor(h, N, capi.ptr(ones)))
                        t1 = time.perf_counter()
                        capi.check(capi.hip.shq_pm_run(h, C.byref(pmp)))
                        if r > 0:
                            old.append((t1 - t0) * 1e3)
                    i = infos[-1]
                    ms = np.median([[x.ms[0], x.ms[1], x.ms[2]] for x in infos], axis=0)
                    floor = i.nnodes * i.nk * 3 * NU_F64_PER_NODE / rate64 * 1e3
                    case = dict(Nmesh=N, Na=Na, nk=i.nk, nodes=i.nnodes, device_ms=dict(node_table=ms[0], delta_nu=ms[1], mode_table=ms[2]),
                                callback_s=float(np.median([x.callback_s for x in infos])), step_call_ms=float(np.median(steps)),
                                gap_new_ms=float(np.median(gaps)), forward_ms=float(np.median(fwd)),
                                gap_new_queued_ms=float(np.median(both) - np.median(fwd)), gap_host_T1_ms=float(np.median(old)), f64_floor_ms=floor)
                    print(json.dumps(case), flush=True)
                    res["cases"].append(case)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
