"""Device time of the sharded slab PM with the massive-neutrino hook at the bench configuration (256^3 S-cluster, Nmesh 768) as a ONE-rank
RCCL group with SHQ_COMM_FORCE=1 (the transposes and the all-reduces are real collectives), three routes alternated in one process:
  plain    SlabPM.force()                        (the fused X pass, fft_pass_strided MODE 2)
  measure  SlabPM.force(measure_power=True)      (the split X pass with T = 1 and the finish's sums)
  neutrino SlabPM.force(analysis=<T = 1 table>)   (the split X pass: X forward + sums, all-reduce, table, (v T) green + X inverse)
Device times are stream events: for the split routes the spans between the P(k) downloads and the device work that follows them, so the
host's downloads, all-reduce staging and analysis are excluded (the table's upload is inside the finish's span).  Wall times are host
clocks around each route with a device synchronise at the end.  One JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("SHQ_COMM_FORCE", "1")
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402
import shenqi_amd as sq  # noqa: E402
from shenqi_amd import dist as sd  # noqa: E402

G = 43.0071


class TimedOps(sd.GpuOps):
    """GpuOps that marks the stream where the host takes over (a P(k) download) and where the device work resumes (the finish)"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.marks = []
        self.finished = False

    def mark(self, tag):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.marks.append((tag, e))

    def power(self):
        self.mark("pause")
        return super().power()

    def _finish(self, fn, args, table, measure):
        self.mark("resume")
        try:
            return super()._finish(fn, args, table, measure)
        finally:
            self.finished = True

    def device_ms(self):
        """the sum of the spans in which the device works without waiting for the host"""
        ms, open_ = 0.0, None
        for tag, e in self.marks:
            if tag in ("start", "resume"):
                open_ = e
            elif open_ is not None:
                ms += open_.elapsed_time(e)
                open_ = None
        return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n1", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kind", default="cluster")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    tmp = tempfile.mkdtemp()
    dist.init_process_group("nccl", init_method="file://" + os.path.join(tmp, "init"), rank=0, world_size=1, device_id=dev)
    try:
        n1 = args.n1
        n, L, nmesh = n1**3, 1.0, 3 * n1
        pos = sq.synth_positions(args.kind, n, seed=20240601, L=L)
        posm = torch.from_numpy(np.concatenate([pos, np.ones((n, 1))], axis=1)).to(dev)
        del pos
        work_stream = torch.cuda.Stream(device=dev)
        work_stream.wait_stream(torch.cuda.current_stream(dev))
        torch.cuda.set_stream(work_stream)
        ctx = sq.Context(0, stream=work_stream.cuda_stream)
        comm = sd.Comm()
        assert comm.multi, "needs the collectives: SHQ_COMM_FORCE=1"
        ops = TimedOps(ctx, nmesh, L, 1.5, G, dev)
        pm = sd.SlabPM(comm, nmesh, L, 1.5, G, ops)
        reduce_power = comm.allreduce_power

        def timed_reduce(sums):     # the finish's sums: the device resumes (return transpose, ...) once they are reduced
            r = reduce_power(sums)
            if ops.finished:
                ops.mark("resume")
            return r
        comm.allreduce_power = timed_reduce
        local = sd.exchange_to_owner(comm, pm.d, posm)
        ops.set_deposit_scale(float(n))
        ops.set_particles(local, n)
        ones = np.ones(3 * (nmesh // 2) ** 2 + 1)
        routes = {"plain": lambda: pm.force(), "measure": lambda: pm.force(measure_power=True),
                  "neutrino": lambda: pm.force(analysis=lambda *s: ones)}
        devms = {k: [] for k in routes}
        wall = {k: [] for k in routes}
        for r in range(args.warmup + args.rounds):
            for name, fn in routes.items():
                torch.cuda.synchronize(dev)
                ops.marks, ops.finished = [], False
                t0 = time.perf_counter()
                ops.mark("start")
                fn()
                ops.mark("end")
                torch.cuda.synchronize(dev)
                t = (time.perf_counter() - t0) * 1e3
                if r >= args.warmup:
                    devms[name].append(ops.device_ms())
                    wall[name].append(t)
        routes["plain"]()
        g0, _ = ops.results(n)
        routes["neutrino"]()
        g1, _ = ops.results(n)
        med = {k: float(np.median(v)) for k, v in devms.items()}
        out = {
            "tool": "time_slab_neutrino", "n": n, "nmesh": nmesh, "ranks": 1, "collectives": "rccl (SHQ_COMM_FORCE=1)", "rounds": args.rounds,
            "device_ms_median": med,
            "device_ms_min": {k: float(np.min(v)) for k, v in devms.items()},
            "wall_ms_median": {k: float(np.median(v)) for k, v in wall.items()},
            "neutrino_minus_plain_ms": med["neutrino"] - med["plain"],
            "measure_minus_plain_ms": med["measure"] - med["plain"],
            "unit_table_same_bits_as_plain": bool(np.array_equal(g0, g1)),
            "unit_table_gravpm_max_rel_diff": float(np.abs(g1 - g0).max() / np.abs(g0).max()),
        }
        print(json.dumps(out), flush=True)
        ctx.close()
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
