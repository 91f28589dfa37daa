"""Multi-GPU TreePM: one process per GPU, x-slab domain decomposition, RCCL over xGMI.

How the path shards:
  * particles and the PM mesh are cut into equal x-slabs, one per rank (the reference cuts its
    real-space PM pencils over a 2-D rank grid np0 x np1, petapm.cpp:217-257; here np1 = 1);
  * PM: local CIC deposit (HIP kernel, 64-bit fixed point) -> one ghost plane to the right
    neighbour (integer add: bit-identical for any rank count) -> 2-D r2c over (y, z) per local
    plane -> all-to-all transpose (x-slabs -> y-slabs; the reference's heffte reshape /
    petapm.cpp:1036 alltoallv) -> 1-D FFT along x -> Green's function on the transposed spectrum
    [y][z'][x] (the reference's own Fourier layout) -> inverse 1-D -> all-to-all back -> 2-D c2r
    -> 2+3 potential ghost planes from the neighbours -> CIC readout with the 4-point stencil;
  * tree: instead of exporting queries to remote trees and importing results
    (treewalk2.h:618-812, two alltoallv per walk and a second remote walk), every rank imports
    the neighbours' particles within `halo` of its slab (one alltoallv of 32-byte records),
    the host builds the local tree over local + ghost particles with the global root cell, and
    the walk runs for the local targets only.  Nodes beyond TreeRcut are discarded by the walk,
    so nothing farther than the halo can contribute.
The FFT stages use rocFFT through torch.fft; torch.distributed (backend "nccl" = RCCL, or
"gloo" with host staging for tests) carries every exchange.  The local compute is abstracted as
`ops` so that the orchestration can be exercised on CPU (tests/cpu_ops.py) with gloo.
"""
import ctypes as C
import math
import os

import numpy as np
import torch
import torch.distributed as dist

from . import capi


class _Done:
    def __init__(self, recv):
        self.recv = recv

    def wait(self):
        return self.recv


class _Pending:
    """A started all-to-all: keeps the buffers alive until the communicator's stream is done with them."""

    def __init__(self, works, send, recv, cplx):
        self.works, self.send, self.recv, self.cplx = works, send, recv, cplx

    def wait(self):
        for w in self.works:
            w.wait()           # the current stream waits for the communicator's; the host does not block
        self.send = None
        return torch.view_as_complex(self.recv) if self.cplx else self.recv


class Comm:
    """Thin wrapper over torch.distributed for the exchanges the path needs."""

    def __init__(self, group=None):
        self.group = group
        self.on = dist.is_available() and dist.is_initialized()
        self.rank = dist.get_rank(group) if self.on else 0
        self.size = dist.get_world_size(group) if self.on else 1
        self.backend = dist.get_backend(group) if self.on else "none"
        # SHQ_COMM_FORCE=1: a one-rank group still goes through the collectives (particle / ghost exchange, the two
        # mesh transposes, the scalar all-reduce): rehearses the RCCL calls of an N-GPU run on a one-GPU box.
        self.multi = self.size > 1 or (self.on and os.environ.get("SHQ_COMM_FORCE", "0") == "1")

    def _stage(self, t):
        """gloo cannot move device tensors: stage through the host (tests only)."""
        if self.backend == "gloo" and t.is_cuda:
            return t.cpu(), t.device
        return t, None

    # RCCL moved a single 3.6 GB peer message wrongly (768^3 spectrum of a one-rank rehearsal: PM force off by 10^2 while
    # the same code is exact at 48^3); messages are therefore kept below 1 GiB: larger ones go as K row-chunked rounds.
    MAX_MSG_BYTES = int(os.environ.get("SHQ_COMM_MAX_MSG", str(1 << 30)))   # the tests lower it to reach the chunked rounds

    def all_to_all_rows(self, send, send_counts):
        """Variable all-to-all of the rows of a 2-D+ tensor: rows [sum(c[:d]), sum(c[:d+1])) go to rank d.
        Returns (recv, recv_counts)."""
        if not self.multi:
            return send, list(send_counts)
        cplx = send.is_complex()
        s, dev = self._stage(torch.view_as_real(send.contiguous()) if cplx else send.contiguous())
        row_bytes = (s[0].numel() if s.shape[0] else int(np.prod(s.shape[1:]))) * s.element_size()
        # counts and the largest message any rank sends travel together, so that every rank derives the same K
        cnt = torch.tensor([[c, max(send_counts) * row_bytes] for c in send_counts], dtype=torch.int64)
        rcnt = torch.empty_like(cnt)
        cdev = send.device if self.backend == "nccl" else torch.device("cpu")
        cnt_d, rcnt_d = cnt.to(cdev), rcnt.to(cdev)
        dist.all_to_all_single(rcnt_d, cnt_d, group=self.group)
        rc = rcnt_d.cpu()
        recv_counts = [int(x) for x in rc[:, 0]]
        K = max(1, -(-int(rc[:, 1].max()) // self.MAX_MSG_BYTES)) if self.backend == "nccl" else 1
        r = torch.empty((sum(recv_counts),) + tuple(s.shape[1:]), dtype=s.dtype, device=s.device)
        if K == 1:
            dist.all_to_all_single(r, s, output_split_sizes=recv_counts, input_split_sizes=list(send_counts), group=self.group)
        else:
            soff = np.concatenate([[0], np.cumsum(send_counts)])
            roff = np.concatenate([[0], np.cumsum(recv_counts)])
            for k in range(K):   # chunk k of every peer segment: rows [c k / K, c (k + 1) / K) of its c rows, views, no copies
                ins = [s[soff[d] + send_counts[d] * k // K:soff[d] + send_counts[d] * (k + 1) // K] for d in range(self.size)]
                outs = [r[roff[d] + recv_counts[d] * k // K:roff[d] + recv_counts[d] * (k + 1) // K] for d in range(self.size)]
                dist.all_to_all(outs, ins, group=self.group)
        r = r.to(dev) if dev is not None else r
        return (torch.view_as_complex(r) if cplx else r), recv_counts

    def all_to_all_rows_start(self, send, send_counts, recv_counts):
        """all_to_all_rows with the receive counts known to the caller (the mesh transposes), started without waiting:
        returns a handle whose wait() gives the received rows.  Over RCCL the rounds run on the communicator's stream and
        the caller may queue independent kernels in the meantime; the other backends complete here."""
        if not self.multi or self.backend != "nccl":
            recv, _ = self.all_to_all_rows(send, send_counts)
            return _Done(recv)
        cplx = send.is_complex()
        s = torch.view_as_real(send.contiguous()) if cplx else send.contiguous()
        row_bytes = int(np.prod(s.shape[1:])) * s.element_size()
        # every rank sees the same counts matrix through (send_counts, recv_counts) only if the caller's counts are global
        # knowledge (slab widths): K follows from the largest width, which all ranks know
        K = max(1, -(-max(max(send_counts), max(recv_counts)) * row_bytes // self.MAX_MSG_BYTES))
        r = torch.empty((sum(recv_counts),) + tuple(s.shape[1:]), dtype=s.dtype, device=s.device)
        works = []
        if K == 1:
            works.append(dist.all_to_all_single(r, s, output_split_sizes=list(recv_counts), input_split_sizes=list(send_counts),
                                                group=self.group, async_op=True))
        else:
            soff = np.concatenate([[0], np.cumsum(send_counts)])
            roff = np.concatenate([[0], np.cumsum(recv_counts)])
            for k in range(K):
                ins = [s[soff[d] + send_counts[d] * k // K:soff[d] + send_counts[d] * (k + 1) // K] for d in range(self.size)]
                outs = [r[roff[d] + recv_counts[d] * k // K:roff[d] + recv_counts[d] * (k + 1) // K] for d in range(self.size)]
                works.append(dist.all_to_all(outs, ins, group=self.group, async_op=True))
        return _Pending(works, s, r, cplx)

    def all_to_all_equal(self, send):
        """Equal-split all-to-all along dim 0 (dim 0 must be a multiple of size)."""
        if not self.multi:
            return send
        cplx = send.is_complex()
        s, dev = self._stage(torch.view_as_real(send.contiguous()) if cplx else send.contiguous())
        r = torch.empty_like(s)
        dist.all_to_all_single(r, s, group=self.group)
        r = r.to(dev) if dev is not None else r
        return torch.view_as_complex(r) if cplx else r

    def shift(self, t, direction):
        """Send `t` to rank + direction (periodic), receive the same-shaped tensor from rank - direction."""
        if not self.multi:
            return t.clone()
        dst = (self.rank + direction) % self.size
        counts = [0] * self.size
        counts[dst] = t.shape[0]
        recv, _ = self.all_to_all_rows(t, counts)
        return recv

    # ---- collectives on small host values: RCCL moves device memory only, so they are staged on the device for it
    def _cdev(self):
        return torch.device("cuda") if self.backend == "nccl" else torch.device("cpu")

    def allreduce_sum(self, x):
        if not self.multi:
            return x
        t = torch.tensor([x], dtype=torch.float64).to(self._cdev())
        dist.all_reduce(t, group=self.group)
        return float(t.item())

    def allreduce_sum_vec(self, a):
        """Element-wise sum over the ranks of a numpy array (or a CPU torch tensor) of any shape, in its own dtype (float64 or
        int64); every rank gets the same new array, of the kind it gave."""
        if torch.is_tensor(a):
            return torch.from_numpy(self.allreduce_sum_vec(a.numpy()))
        a = np.array(a, order="C")             # a copy: the reduction runs in place
        if not self.multi or a.size == 0:      # the shape is the same on every rank
            return a
        t = torch.from_numpy(a).to(self._cdev())
        dist.all_reduce(t, group=self.group)
        return t.cpu().numpy()

    def allreduce_max_vec(self, a):
        """Element-wise maximum over the ranks of a numpy array of any shape, in its own dtype (float64 or int64); every rank gets
        the same new array."""
        a = np.array(a, order="C")             # a copy: the reduction runs in place
        if not self.multi or a.size == 0:
            return a
        t = torch.from_numpy(a).to(self._cdev())
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=self.group)
        return t.cpu().numpy()

    def gather_scalar(self, v, dtype=np.float64):
        """every rank's v as an array indexed by rank: float64, or int64 for counts (exact beyond 2^53)"""
        a = np.zeros(self.size, dtype=dtype)
        a[self.rank] = v
        return self.allreduce_sum_vec(a)

    def allgather_u64(self, a):
        """every rank's uint64 array, concatenated in rank order"""
        if not self.multi:
            return np.asarray(a, dtype=np.uint64).copy()
        n = self.gather_scalar(len(a), np.int64)
        m = int(n.max())
        mine = torch.zeros(max(m, 1), dtype=torch.int64)
        mine[:len(a)] = torch.from_numpy(np.asarray(a, dtype=np.uint64).view(np.int64).copy())
        mine = mine.to(self._cdev())
        outs = [torch.empty_like(mine) for _ in range(self.size)]
        dist.all_gather(outs, mine, group=self.group)
        return np.concatenate([o.cpu().numpy()[:int(c)] for o, c in zip(outs, n)]).view(np.uint64)

    def send_array(self, arr, dst):
        """a (structured) numpy array to rank dst, as its length and its bytes; recv_array(src, dtype) takes it there"""
        b = torch.from_numpy(np.frombuffer(arr.tobytes(), dtype=np.uint8).copy())
        dist.send(torch.tensor([len(arr)], dtype=torch.int64).to(self._cdev()), dst, group=self.group)
        if len(arr):
            dist.send(b.to(self._cdev()), dst, group=self.group)

    def recv_array(self, src, dtype):
        n = torch.zeros(1, dtype=torch.int64).to(self._cdev())
        dist.recv(n, src, group=self.group)
        b = torch.zeros(int(n.item()) * dtype.itemsize, dtype=torch.uint8).to(self._cdev())
        if int(n.item()):
            dist.recv(b, src, group=self.group)
        return np.frombuffer(b.cpu().numpy().tobytes(), dtype=dtype).copy()

    def bcast_array(self, arr, dtype):
        """rank 0's structured array on every rank"""
        if not self.multi:
            return arr
        n = torch.tensor([len(arr) if self.rank == 0 else 0], dtype=torch.int64).to(self._cdev())
        dist.broadcast(n, 0, group=self.group)
        b = torch.zeros(int(n.item()) * dtype.itemsize, dtype=torch.uint8)
        if self.rank == 0:
            b = torch.from_numpy(np.frombuffer(arr.tobytes(), dtype=np.uint8).copy())
        b = b.to(self._cdev())
        dist.broadcast(b, 0, group=self.group)
        return np.frombuffer(b.cpu().numpy().tobytes(), dtype=dtype).copy()

    def allreduce_power(self, sums):
        """powerspectrum_sum (powerspectrum.cpp:53-88): the raw P(k) sums (kk, power, nmodes, Norm) of every rank added up - kk, power
        and Norm as float64, nmodes as int64."""
        kk, power, nmodes, norm = sums
        nb = len(kk)
        f = self.allreduce_sum_vec(np.concatenate([np.asarray(kk, np.float64), np.asarray(power, np.float64), [float(norm)]]))
        m = self.allreduce_sum_vec(np.asarray(nmodes, np.int64))
        return f[:nb], f[nb:2 * nb], m, float(f[2 * nb])

    def barrier(self):
        if self.size > 1:
            dist.barrier(group=self.group)


class SlabDecomp:
    """x-slabs of the box = runs of mesh planes, one per rank.  `bounds` (P+1 plane indices, 0 ... Nmesh)
    may be unequal: balanced_bounds() picks them so that every rank owns about the same number of
    particles (the reference balances work through its Peano top-leaf assignment, domain.cpp:620).
    `ycuts` (P+1 lengths, the first and last 0) refine a boundary below the plane: the particles of plane bounds[r] with
    y < ycuts[r] belong to rank r - 1 (its walk targets, its deposit and readout) while the MESH plane stays rank r's —
    a plane through the core of a cluster carries several per cent of all the work, more than the share of a rank at 64
    ranks.  The left rank then deposits into two planes of its right neighbour instead of one and reads four of its
    potential planes instead of three (dep_ghosts, pot_right)."""

    MIN_PLANES = 3   # the readout needs 3 planes from the right neighbour and 2 from the left

    def __init__(self, comm, Nmesh, BoxSize, bounds=None, ycuts=None):
        P = comm.size
        if bounds is None:
            if Nmesh % P != 0:
                raise ValueError("Nmesh %d must be divisible by the number of ranks %d (or pass bounds)" % (Nmesh, P))
            bounds = [r * (Nmesh // P) for r in range(P + 1)]
        bounds = [int(b) for b in bounds]
        if len(bounds) != P + 1 or bounds[0] != 0 or bounds[-1] != Nmesh:
            raise ValueError("bounds must run from 0 to Nmesh with one entry per rank + 1")
        ycuts = [0.0] * (P + 1) if ycuts is None else [float(c) for c in ycuts]
        if len(ycuts) != P + 1 or ycuts[0] != 0.0 or ycuts[-1] != 0.0 or min(ycuts) < 0.0 or max(ycuts) > BoxSize:
            raise ValueError("ycuts must hold one length in [0, BoxSize] per boundary, none at the box's own edge")
        self.split = max(ycuts) > 0.0
        self.dep_ghosts, self.pot_right = (2, 4) if self.split else (1, 3)
        self.min_planes = self.MIN_PLANES + (1 if self.split else 0)
        widths = [bounds[r + 1] - bounds[r] for r in range(P)]
        if P > 1 and min(widths) < self.min_planes:
            raise ValueError("every slab needs at least %d mesh planes (got %s)" % (self.min_planes, widths))
        if Nmesh % P != 0:
            raise ValueError("Nmesh %d must be divisible by the number of ranks %d (equal y-slabs of the spectrum)" % (Nmesh, P))
        self.comm, self.N, self.L, self.bounds, self.widths, self.ycuts = comm, Nmesh, BoxSize, bounds, widths, ycuts
        self.cell = BoxSize / Nmesh
        self.nxl = widths[comm.rank]
        self.plane0 = bounds[comm.rank]
        self.x0, self.x1 = self.slab_range(comm.rank)

    def owner_of(self, x, y=None):
        """rank owning positions x (tensor), by the mesh plane of the CIC base cell (floor(x / cell)); with sub-plane cuts
        the y coordinates decide inside a boundary plane."""
        plane = torch.floor(x / self.cell).to(torch.int64) % self.N
        inner = torch.tensor(self.bounds[1:-1], dtype=torch.int64, device=x.device)
        owner = torch.searchsorted(inner, plane, right=True)
        if self.split:
            if y is None:
                raise ValueError("this decomposition cuts planes by y: owner_of needs the y coordinates")
            first = torch.tensor(self.bounds[:-1], dtype=torch.int64, device=x.device)[owner]
            cut = torch.tensor(self.ycuts[:-1], dtype=y.dtype, device=x.device)[owner]
            owner = owner - ((plane == first) & (y < cut)).to(owner.dtype)
        return owner

    def slab_range(self, r):
        """x extent of what rank r owns: its planes, and the boundary plane behind them when part of that is its own too"""
        return self.bounds[r] * self.cell, (self.bounds[r + 1] + (1 if self.ycuts[r + 1] > 0.0 else 0)) * self.cell

    def reach_mask(self, d, x, halo):
        """which of the positions x lie within `halo` (one length, or one per position) of what rank d owns, periodically:
        a - halo <= x < b + halo for its x extent [a, b), or everything once that span covers the box.  x and a per-position
        halo are both torch tensors or both numpy arrays; the mask is of the same kind."""
        xp = torch if torch.is_tensor(x) else np
        a, b = self.slab_range(d)
        span = (b - a) + 2 * halo
        near = xp.remainder(x - (a - halo), self.L) < span
        wide = span >= self.L          # one answer for a plain length (the common one, False, costs no operation on x), else one per position
        return near if wide is False else near | wide


class SlabMesh:
    """What the drivers of a slab-decomposed mesh share (SlabPM, DistUVBG, DistZeldovich, DistGlass derive from it): the communicator,
    the SlabDecomp `d`, the counted exchanges, the particles' route to their owners and back, the ghost planes, and the two routes
    of the mesh transposes between the x-slabs [nxl, N, z] and the y-slab of the spectrum [N, nyl, z'] (x slowest) - torch.fft,
    or the library's own FFT passes (csrc/fft3d.hip) through the callables of the driver's ops.
    Counters: nalltoall (all-to-alls and shifts started through a2a / shift) and rows_sent (the rows that left this rank in the last
    to_owners); a driver zeroes them when a call begins."""

    def __init__(self, comm, Nmesh, BoxSize, ops, bounds=None, ycuts=None):
        self.comm, self.ops, self.N, self.L = comm, ops, Nmesh, BoxSize
        self.d = SlabDecomp(comm, Nmesh, BoxSize, bounds, ycuts)
        self.rows_sent = self.nalltoall = 0

    def _equal_widths(self):
        if len(set(self.d.widths)) != 1:
            raise ValueError("%s needs slabs of equal width (got %s)" % (type(self).__name__, self.d.widths))

    def a2a(self, send, send_counts, recv_counts=None):
        """Comm.all_to_all_rows, or with recv_counts all_to_all_rows_start (a handle to wait() for), counted"""
        self.nalltoall += 1
        if recv_counts is None:
            return self.comm.all_to_all_rows(send, send_counts)
        return self.comm.all_to_all_rows_start(send, send_counts, recv_counts)

    def shift(self, t, direction):
        self.nalltoall += 1
        return self.comm.shift(t, direction)

    def bespoke(self, pitch):
        """the route of the transposes: the library's own FFT passes where it has the mesh size (pitch: doubles per z row, 0
        without them), unless SHQ_SLAB_TORCH_FFT=1 asks for torch.fft"""
        return pitch > 0 and os.environ.get("SHQ_SLAB_TORCH_FFT", "0") != "1"

    # ---- particles: to the owner of their plane and back
    def _send_sorted(self, rows, owner):
        """the rows (a device tensor) to the ranks `owner` names, in one all-to-all; rows already at home stay in the self block.
        Returns (the rows received, the stable sort by owner they left in, the counts sent, the counts received)."""
        order = torch.argsort(owner, stable=True)
        counts = torch.bincount(owner, minlength=self.comm.size).tolist()
        got, rcounts = self.a2a(rows[order].contiguous(), counts)
        return got, order, counts, rcounts

    def to_owners(self, rows, owner):
        """Returns (the rows this rank owns now, the route for back()) and records rows_sent."""
        mine, order, counts, rcounts = self._send_sorted(rows, owner)
        self.rows_sent = rows.shape[0] - counts[self.comm.rank]
        return mine, (order, rcounts)

    def back(self, route, cols):
        """cols [rows owned, k]: results of the rows to_owners delivered, in that order.  They return along the same counts - the
        order within a (source, destination) pair is kept, so no key travels - as a numpy array [n, k] in the caller's order."""
        order, rcounts = route
        got, _ = self.a2a(cols, rcounts)
        out = np.empty((order.shape[0], cols.shape[1]))
        out[order.cpu().numpy()] = got.cpu().numpy()
        return out

    # ---- ghost planes (nothing to do on one rank: the mesh is periodic in place)
    def add_ghosts(self, bufs, nxl):
        """the deposit ghost plane bufs[f][nxl] of every int64 field into the right-hand neighbour's plane 0: all fields in ONE
        message; an integer add, exact"""
        if self.comm.size > 1:
            ghost = self.shift(torch.stack([b[nxl] for b in bufs]), +1)
            for b, g in zip(bufs, ghost):
                b[0] += g

    def neighbour_plane(self, ext, nxl):
        """the right-hand neighbour's first plane behind the own ones: one shift to the left"""
        if self.comm.size > 1:
            ext[nxl] = self.shift(ext[0:1].contiguous(), -1)[0]

    # ---- the transposes' row order: x planes [nxl, N, z] <-> rows [rank q][x_l] of [nyl, z] blocks
    def pack_rows(self, planes):
        P, nxl, nyl = self.comm.size, self.d.nxl, self.N // self.comm.size
        return planes.reshape(nxl, P, nyl, -1).permute(1, 0, 2, 3).reshape(P * nxl, nyl, -1)          # rows [dest q][x_l]

    def unpack_rows(self, rows):
        P, nxl, nyl = self.comm.size, self.d.nxl, self.N // self.comm.size
        return rows.reshape(P, nxl, nyl, -1).permute(1, 0, 2, 3).reshape(nxl, self.N, -1)             # from rows [src q][x_l]

    # ---- the torch.fft route: mesh sizes without a bespoke transform, and the CPU stand-ins
    def forward_torch(self, real):
        """real f64 [nxl, N, N] -> its unscaled spectrum on this rank's y-slab, complex [N, nyl, N / 2 + 1]"""
        N, P, nxl = self.N, self.comm.size, self.d.nxl
        spec = torch.fft.rfft2(real, dim=(1, 2))                                                     # [nxl, N, Nc], unscaled
        recv, _ = self.a2a(self.pack_rows(spec).contiguous(), [nxl] * P)                             # rows [src p][x_l] = all x
        return torch.fft.fft(recv.reshape(N, N // P, N // 2 + 1), dim=0).contiguous()

    def back_torch(self, spec):
        """the y-slab spectrum [N, nyl, N / 2 + 1] -> the real mesh of this rank's planes f64 [nxl, N, N], unscaled"""
        N = self.N
        out = torch.fft.ifft(spec, dim=0, norm="forward").contiguous()                               # rows = x planes, in order
        recv, _ = self.a2a(out, self.d.widths)                                                       # rows [src q][x_l]
        return torch.fft.irfft2(self.unpack_rows(recv), s=(N, N), dim=(1, 2), norm="forward")

    # ---- the bespoke route: planes [nxl, N, zp] doubles, the y-slab [N, nyl, zp / 2] complex
    def forward_bespoke(self, own, yz_forward):
        """The Y/Z forward of the planes `own` and the exchange, started: yz_forward(packed) runs the passes, storing into the
        all-to-all buffer `packed`, rows [dest q][x_l] - or in place for None, on a lone process, whose planes are the y-slab
        already.  Returns the pending spectrum: wait() for it."""
        P, nxl = self.comm.size, self.d.nxl
        if not self.comm.multi:
            yz_forward(None)
            return _Done(own.view(torch.float64).view(torch.complex128))
        send = torch.empty((P * nxl, self.N // P, own.shape[2] // 2), dtype=torch.complex128, device=own.device)
        yz_forward(send)
        return self.a2a(send, [nxl] * P, self.d.widths)                                              # [x (all)][y_l][z']

    def back_bespoke(self, planes, like, xpass, yz_inverse, inflight=1):
        """The way back of len(planes) fields, one after another; yields f once field f's real mesh stands in planes[f] (the same
        buffer for all, or one each).  xpass(f, out) queues the field's out-of-place X pass (inverse) from the kept y-slab into
        `out`, shaped as `like`; yz_inverse(f, packed) the Y/Z inverse into planes[f] from the received rows.  `inflight`
        exchanges are kept started ahead of the one waited for: field f + inflight's pass is queued before field f's exchange is
        waited for.  On a lone process the X pass lands where the Y/Z inverse (packed None) takes it."""
        nf, P, nxl = len(planes), self.comm.size, self.d.nxl

        def start(f):
            out = torch.empty_like(like)
            xpass(f, out)
            return self.a2a(out, self.d.widths, [nxl] * P)                                           # rows [src q][x_l]

        pend = [start(f) for f in range(min(inflight, nf))] if self.comm.multi else None
        for f in range(nf):
            if pend is None:
                xpass(f, planes[f].view(torch.float64).view(torch.complex128))
                yz_inverse(f, None)
            else:
                packed = pend.pop(0).wait().contiguous()
                if f + inflight < nf:
                    pend.append(start(f + inflight))
                yz_inverse(f, packed)
            yield f


def balanced_bounds(comm, Nmesh, BoxSize, x, weights=None, plane_cost=0.0, y=None):
    """Plane boundaries giving every rank about the same share of the work (x: positions held by this rank, any
    distribution).  Work of a plane = the sum of `weights` over its particles (1 each when None: equal counts) +
    `plane_cost` (what a mesh plane costs whoever owns it, in the units of the weights).  One all-reduce of an
    Nmesh-long histogram.
    With y (the same particles' y coordinates) the cut is refined below the plane and (bounds, ycuts) come back for
    SlabDecomp: the plane in which a rank's share ends goes to the right-hand rank as a mesh plane, and its particles
    with y < ycut — a whole number of mesh cells — to the left-hand one, so that the shares meet to within one row of
    cells instead of one plane.  A second all-reduce, of the cut planes' y histograms."""
    P = comm.size
    cell = BoxSize / Nmesh
    plane = (torch.floor(x / cell).to(torch.int64) % Nmesh).cpu()
    w = None if weights is None else torch.as_tensor(weights).to(torch.float64).cpu()
    hist = comm.allreduce_sum_vec(torch.bincount(plane, weights=w, minlength=Nmesh).to(torch.float64))
    cum = torch.cumsum(hist + float(plane_cost), 0).numpy()
    total = cum[-1]
    minp = SlabDecomp.MIN_PLANES + (0 if y is None else 1)
    bounds, want = [0], [0.0]
    for r in range(1, P):
        target = total * r / P
        i = int(np.searchsorted(cum, target, side="left"))          # first plane whose cumulated work reaches the target
        if y is None:
            # cut before or after that plane, whichever leaves the left ranks closer to their share (a plane through the
            # cluster's core carries several per cent of the work)
            b = i if (i > 0 and target - cum[i - 1] < cum[min(i, Nmesh - 1)] - target) else i + 1
        else:
            b = min(i, Nmesh - 1)                                     # the share ends inside plane i: cut that plane
        lo, hi = bounds[-1] + minp, Nmesh - minp * (P - r)
        want.append(target - (cum[b - 1] if b > 0 else 0.0) if lo <= b <= hi and y is not None else 0.0)
        bounds.append(min(max(b, lo), hi))
    bounds.append(Nmesh)
    if y is None:
        return bounds
    # the particles of the cut planes by their row of cells in y
    row = (torch.floor(y / cell).to(torch.int64) % Nmesh).cpu()
    yh = torch.zeros((P - 1, Nmesh), dtype=torch.float64)
    for r in range(1, P):
        sel = plane == bounds[r]
        yh[r - 1] = torch.bincount(row[sel], weights=None if w is None else w[sel], minlength=Nmesh).to(torch.float64)
    yh = comm.allreduce_sum_vec(yh).numpy()
    ycuts = [0.0]
    for r in range(1, P):
        cy = np.cumsum(yh[r - 1])
        k = int(np.searchsorted(cy, want[r], side="left"))            # rows 0 .. k reach the share
        if want[r] <= 0.0:
            k = 0
        elif k < Nmesh and want[r] - (cy[k - 1] if k > 0 else 0.0) >= cy[k] - want[r]:
            k = k + 1                                                 # with row k the left rank comes closer to its share
        ycuts.append(min(k * cell, float(BoxSize)))
    ycuts.append(0.0)
    return bounds, ycuts


# Cost model of one force step on an MI355X, from the one-GPU bench: the walk takes 39.5 ms for 8.5e9 interactions,
# deposit + readout 4.2 ms for 1.7e7 particles, the four (y, z) FFT passes 7.9 ms for 768^3 cells.
COST_MS_PER_INTERACTION = 39.5 / 8.5e9
COST_MS_PER_PARTICLE = 4.2 / 16777216
COST_MS_PER_CELL = 7.9 / 768.0**3


def cost_balanced_bounds(comm, drv, subplane=False):
    """Slab boundaries that even out the measured work instead of the particle count: every local particle weighs its
    interaction count of the last walk (plus its deposit / readout), every mesh plane its share of the (y, z) passes.
    The reference balances its domains the same way, by the work counted in the previous step (domain.cpp:620-700,
    GravCost).  Call after a drv.step(); all ranks get the same list — with subplane the pair (bounds, ycuts)."""
    n = int(drv.allp.shape[0])
    nint = np.zeros(n, dtype=np.int64)
    capi.check(capi.hip.shq_grav_short_download(drv.ctx.h, None, None, capi.ptr(nint), None))
    w = COST_MS_PER_INTERACTION * nint[: drv.nloc].astype(np.float64) + COST_MS_PER_PARTICLE
    return balanced_bounds(comm, drv.N, drv.L, drv.local[:, 0], weights=torch.from_numpy(w),
                           plane_cost=COST_MS_PER_CELL * float(drv.N) ** 2, y=drv.local[:, 1] if subplane else None)


def exchange_to_owner(comm, decomp, posm, types=None):
    """Domain exchange: send every particle (rows x, y, z, m) to the rank owning its slab.  With types (one integer per row) the
    rows' types travel with them and (posm, types) comes back."""
    owner = decomp.owner_of(posm[:, 0], posm[:, 1])
    order = torch.argsort(owner, stable=True)
    counts = torch.bincount(owner, minlength=comm.size).tolist()
    if types is None:
        recv, _ = comm.all_to_all_rows(posm[order], counts)
        return recv
    recv, _ = comm.all_to_all_rows(_with_types(posm, types)[order], counts)
    return _split_types(recv, types.dtype)


def _with_types(posm, types):
    """rows (x, y, z, m, type): the type as a fifth column (exact in float64) so that it travels with its row"""
    return torch.cat([posm, types.to(device=posm.device, dtype=posm.dtype)[:, None]], dim=1)


def _split_types(rows, dtype):
    return rows[:, :4].contiguous(), rows[:, 4].to(dtype)


def ghost_records(comm, decomp, x, reach, recs, reach_of_rank=None):
    """Import the records (rows of a tensor) of other ranks' particles: a particle at x with own reach `reach` (a tensor) goes to
    rank d if it lies within max(reach, reach_of_rank[d]) of d's slab (SlabDecomp.reach_mask); without reach_of_rank `reach` is one
    length for all.  Returns the received rows in source-rank order; a particle goes at most once to a rank."""
    if not comm.multi:
        return recs[:0]
    parts, counts = [], [0] * comm.size
    for d in range(comm.size):
        if d == comm.rank:
            continue
        halo = reach if reach_of_rank is None else torch.clamp(reach, min=float(reach_of_rank[d]))
        parts.append(recs[decomp.reach_mask(d, x, halo)])
        counts[d] = int(parts[-1].shape[0])
    send = torch.cat(parts, dim=0) if parts else recs[:0]
    recv, _ = comm.all_to_all_rows(send, counts)
    return recv


def ghost_exchange(comm, decomp, posm, halo):
    """Import every other rank's particles (rows x, y, z, m) within `halo` (periodic) of this rank's slab"""
    return ghost_records(comm, decomp, posm[:, 0], halo, posm)


def append_records(local, got):
    """the records `local` followed by those in the rows of `got` (uint8, one record each), e.g. what ghost_records returned.  Not
    np.concatenate: it repacks structured dtypes (sph_particle_data's padding would go, 176 -> 168 bytes)."""
    n, ng = len(local), len(got)
    out = np.empty(n + ng, dtype=local.dtype)
    out[:n] = local
    out[n:] = np.ascontiguousarray(got).view(local.dtype).reshape(ng)
    return out


def import_ghost_gas(comm, decomp, P, SphP, reach, reach_of_rank):
    """P (everything this rank owns) followed by the other ranks' live gas within reach of this rank's slab, by ghost_records' rule
    (reach: one length per live gas particle of P, or None for 0).  A ghost's record carries its owner and its row there in fields
    the walks do not read (TopLeaf, GrNr).  With SphP the ghosts' gas slots travel too, into slots after SphP's (PI rewritten).
    Returns (Pall, Sall or None, number of ghosts)."""
    nloc = len(P)
    gas = np.flatnonzero((P["Type"] == 0) & ((P["Flags"] & 1) == 0))
    G = P[gas].copy()
    G["TopLeaf"] = comm.rank
    G["GrNr"] = gas
    rec = G.view(np.uint8).reshape(len(G), -1)
    if SphP is not None:
        rec = np.concatenate([rec, SphP[P["PI"][gas]].view(np.uint8).reshape(len(G), -1)], axis=1)
    reach = torch.zeros(len(G), dtype=torch.float64) if reach is None else torch.from_numpy(reach)
    got = ghost_records(comm, decomp, torch.from_numpy(np.ascontiguousarray(G["Pos"][:, 0])), reach,
                        torch.from_numpy(np.ascontiguousarray(rec)), reach_of_rank).numpy()
    ng, psz = len(got), P.dtype.itemsize
    Pall = append_records(P, got[:, :psz])
    if SphP is None:
        return Pall, None, ng
    Sall = append_records(SphP, got[:, psz:])
    Pall["PI"][nloc:] = len(SphP) + np.arange(ng)
    return Pall, Sall, ng


def import_ghost_gas_bh(comm, decomp, P, SphP, BhP, reach_of_rank):
    """import_ghost_gas for the black-hole walks, whose neighbour search is symmetric (r2 <= max(Hsml_i, Hsml_j)^2) over gas and holes:
    P followed by the other ranks' live gas and their live, unswallowed holes within max(own Hsml, reach_of_rank[d]) of this rank's
    slab (reach_of_rank[d]: the largest Hsml of rank d's queued holes).  The ghosts' gas and black-hole slot rows come after SphP's and
    BhP's (PI rewritten); owner in TopLeaf, row at the owner in GrNr.  Returns (Pall, Sall, Ball, number of ghosts)."""
    nloc, psz, ssz, bsz = len(P), P.dtype.itemsize, SphP.dtype.itemsize, BhP.dtype.itemsize
    gas, hole = P["Type"] == 0, (P["Type"] == 5) & ((P["Flags"] & 2) == 0)
    sel = np.flatnonzero(((P["Flags"] & 1) == 0) & (gas | hole))
    G = P[sel].copy()
    G["TopLeaf"] = comm.rank
    G["GrNr"] = sel
    g = G["Type"] == 0
    rec = np.zeros((len(G), psz + max(ssz, bsz)), dtype=np.uint8)                 # a particle's record, then its slot's
    rec[:, :psz] = G.view(np.uint8).reshape(len(G), psz)
    rec[g, psz:psz + ssz] = SphP[G["PI"][g]].view(np.uint8).reshape(-1, ssz)
    rec[~g, psz:psz + bsz] = BhP[G["PI"][~g]].view(np.uint8).reshape(-1, bsz)
    got = ghost_records(comm, decomp, torch.from_numpy(np.ascontiguousarray(G["Pos"][:, 0])), torch.from_numpy(np.ascontiguousarray(G["Hsml"])),
                        torch.from_numpy(rec), reach_of_rank).numpy()
    Pall = append_records(P, got[:, :psz])
    gg = Pall["Type"][nloc:] == 0
    Sall = append_records(SphP, got[gg, psz:psz + ssz])
    Ball = append_records(BhP, got[~gg, psz:psz + bsz])
    Pall["PI"][nloc:][gg] = len(SphP) + np.arange(int(gg.sum()))
    Pall["PI"][nloc:][~gg] = len(BhP) + np.arange(int((~gg).sum()))
    return Pall, Sall, Ball, len(got)


def fetch_from_owners(comm, owner, index, rows):
    """For each (owner[k], index[k]) asked for, row index[k] of the owner's `rows` as it is now: a 2-D numpy array (uint8, or any type
    all_to_all_rows moves), or a function of the asked indices that returns their rows.  Two all_to_all_rows: the indices out, the rows
    back along the same counts - the order within a pair of ranks is kept, so no key travels back."""
    owner, index = np.asarray(owner, dtype=np.int64), np.asarray(index, dtype=np.int64)
    take = rows if callable(rows) else (lambda ask: rows[ask])
    order = np.argsort(owner, kind="stable")
    counts = np.bincount(owner, minlength=comm.size).tolist()
    ask, acounts = comm.all_to_all_rows(torch.from_numpy(index[order].reshape(-1, 1)), counts)
    ans = np.ascontiguousarray(take(np.ascontiguousarray(ask.numpy()).reshape(-1)))
    back, _ = comm.all_to_all_rows(torch.from_numpy(ans), acounts)
    out = np.empty_like(ans, shape=(len(owner),) + ans.shape[1:])
    out[order] = back.numpy()
    return out


def widen_until_covered(comm, hfac, start_radius, attempt):
    """The repeat-on-a-wider-halo protocol of the operators that iterate a search radius (the Hsml loops of density and
    stellar_density).  Every rank starts with the halo hfac x start_radius (the largest radius of its targets) and calls
    attempt(halos), halos being every rank's halo by rank: it restores the targets' saved radii, imports the ghosts within the
    halos, runs the operator and returns the largest radius the loop TRIED on this rank (0.0 with no targets) - not the one it ended
    with: a guess that reaches past the imported ghosts undercounts the neighbours, which steers the guesses after it, so a loop
    whose guesses left the halo is run again even if it came back inside (the reference runs every guess against all ranks,
    treewalk2.h:480-557).  An operator that does not report the radii tried (the CPU stand-ins of the tests) gives the final one:
    with hfac = 1.3 the first guess, at most 1.26 x the start value (densitytree2.hpp:233-246), cannot leave the halo.
    The exit rule, the same on every rank: no rank tried a radius beyond its own halo.  Otherwise every rank repeats with
    hfac x max(tried, halo).  One rank alone has nothing to import and ends after the first round.  Returns the rounds it took."""
    halo, rounds = hfac * start_radius, 0
    while True:
        rounds += 1
        halos = comm.gather_scalar(halo)
        tried = attempt(halos)
        if not comm.multi or max(t / max(h, 1e-300) for t, h in zip(comm.gather_scalar(tried), halos)) <= 1.0:
            return rounds
        halo = hfac * max(tried, halo)


class SlabPM(SlabMesh):
    """Distributed PM force for the particles this rank owns.  Of SlabMesh it takes the route decision and the transposes' row
    order; its two pipelines are its own: the torch.fft one keeps the spectrum as [y_l][z'][x] for shq_pm_slab_green, the bespoke
    one has the walk hooks and the split X step, and with slabs cut below the plane two deposit ghost planes travel and potential
    planes come from both neighbours."""

    def __init__(self, comm, Nmesh, BoxSize, Asmth, G, ops, bounds=None, ycuts=None):
        super().__init__(comm, Nmesh, BoxSize, ops, bounds, ycuts)
        self.Asmth, self.G = Asmth, G
        self.power = self.power_finish = None

    def force(self, hooks=(), analysis=None, measure_power=False):
        """Runs one PM step for the particles loaded in `ops`; results stay in ops (gravpm, potential).
        hooks: up to two callables that queue work independent of the PM (pieces of the tree walk); the bespoke pipeline
        calls them right after starting its first and its second mesh transpose, so that work runs while the spectrum
        travels.
        analysis: gravpm_force's global_analysis hook (MassiveNuLinRespOn, gravpm.cpp:76-85, 308-321) - the X step splits in two:
        X forward with this rank's raw P(k) sums, their sum over the ranks (powerspectrum_sum), then on every rank
        analysis(kk, power, nmodes, norm) -> T (3 (Nmesh/2)^2 + 1 factors by integer k2, or None for 1), and (v T) green + X inverse.
        measure_power: the finish also takes the sums of v T (potential_transfer's); without analysis the split runs with T = 1.
        The reduced sums stay on the object, the same on every rank: self.power (the density's) and self.power_finish (v T's, when
        measuring); each is (kk, power, nmodes, norm), scaling Norm is the caller's.  With analysis the first hook is queued
        right after the return transpose has started, beside the second: the P(k) round trip waits for the stream, and would wait for
        a walk piece queued before it."""
        split = analysis is not None or measure_power
        self.power = self.power_finish = None
        xstep = (lambda spec_t, y0, nyl, xfwd, xfin: self._xsplit(spec_t, y0, nyl, xfwd, xfin, analysis, measure_power)) if split else None
        if getattr(self.ops, "pitch", None) is not None and self.bespoke(self.ops.pitch()):
            return self._force_bespoke(list(hooks), xstep)
        self._force_torch(xstep)
        for h in hooks:
            h()

    def _xsplit(self, spec_t, y0, nyl, xforward, xfinish, analysis, measure_power):
        """the split X step: this rank's sums, their all-reduce, the caller's table, the finish (and its sums, all-reduced)"""
        self.power = self.comm.allreduce_power(xforward(spec_t, y0, nyl))
        T = analysis(*self.power) if analysis is not None else None
        if T is not None:
            T = np.ascontiguousarray(T, dtype=np.float64)
            if T.shape != (3 * (self.N // 2) ** 2 + 1,):
                raise ValueError("analysis must return 3 (Nmesh/2)^2 + 1 factors (got shape %s)" % (T.shape,))
        fin = xfinish(spec_t, y0, nyl, T, measure_power)
        if measure_power:
            self.power_finish = self.comm.allreduce_power(fin)

    def _force_bespoke(self, hooks=(), xstep=None):
        """The slab pipeline on the library's own FFT passes (csrc/fft3d.hip): ONE buffer [nalloc][N][zp] is the
        int64 deposit mesh, the (y, z) half spectrum and the potential, ghost planes in place; the blocks the
        all-to-all delivers are transformed along x as they are (x slowest), fused with the Green's function.
        Passes over the slab: zero, deposit, Z, Y, pack | x+Green+x | unpack, Y, Z, readout."""
        c, N, nxl, P = self.comm, self.N, self.d.nxl, self.comm.size
        ops = self.ops
        zp = ops.pitch()
        zpc = zp // 2
        multi = c.multi   # SHQ_COMM_FORCE: one rank keeps its periodic geometry but still runs the transposes as collectives
        dg, pr = self.d.dep_ghosts, self.d.pot_right     # deposit ghost planes behind the slab, potential planes read from there
        xoff, nalloc = (0, N) if P == 1 else (2, nxl + 2 + pr)
        buf = ops.mesh_buffer(nalloc, N, zp)                               # int64 [nalloc, N, zp]
        ops.deposit2(buf, self.d.plane0, nxl, xoff, nalloc, dg)
        if P > 1:
            ghost = c.shift(buf[xoff + nxl:xoff + nxl + dg].contiguous(), +1)
            buf[xoff:xoff + dg] += ghost
        own = buf[xoff:xoff + nxl]
        nyl = N // P
        if multi:      # the pack / unpack around the transposes is fused into the Y pass of the FFT
            send = torch.empty((P * nxl, nyl, zpc), dtype=torch.complex128, device=buf.device)      # rows [dest q][x_l]
            ops.fft_yz_packed(own, nxl, 0, send, P)
        else:          # a lone process: nothing to pack, the planes are the y-slab
            ops.fft_yz(own, nxl, 0)
        spec = own.view(torch.float64).view(torch.complex128)               # [nxl, N, zpc]
        hooks = list(hooks) + [None, None]
        first = hooks[0]
        if xstep is not None:
            hooks[0] = None          # queued beside hooks[1] instead, behind the return transpose (force())
        if multi:
            pend = c.all_to_all_rows_start(send, [nxl] * P, self.d.widths)                         # [x (all)][y_l][z']
            del send
            if hooks[0]:
                hooks[0]()
            spec_t = pend.wait().contiguous()
        else:
            if hooks[0]:
                hooks[0]()
            spec_t = spec
        if xstep is None:
            ops.xgreen(spec_t, c.rank * nyl, nyl)
        else:
            xstep(spec_t, c.rank * nyl, nyl, ops.xforward, ops.xfinish)
        deferred = first if xstep is not None else None   # behind the return transpose's start, beside the second piece
        if multi:
            pend = c.all_to_all_rows_start(spec_t, self.d.widths, [nxl] * P)                       # rows [src q][x_l]
            if deferred:
                deferred()
            if hooks[1]:
                hooks[1]()
            recv = pend.wait()                                                                     # rows [src q][x_l]
            ops.fft_yz_packed(own, nxl, 1, recv.contiguous(), P)
            del recv, pend
        else:
            if deferred:
                deferred()
            if hooks[1]:
                hooks[1]()
            ops.fft_yz(own, nxl, 1)
        phi = buf.view(torch.float64)
        if P > 1:
            phi[0:2] = c.shift(phi[xoff + nxl - 2:xoff + nxl].contiguous(), +1)    # my last 2 -> right rank's left ghosts
            phi[xoff + nxl:xoff + nxl + pr] = c.shift(phi[xoff:xoff + pr].contiguous(), -1)  # my first 3 (4) -> left rank's right ghosts
        ops.readout2(phi, self.d.plane0, nxl, xoff, nalloc)

    def _force_torch(self, xstep=None):
        """The same pipeline with torch.fft (rocFFT) for mesh sizes without a bespoke transform, and on the
        CPU stand-ins of the gloo tests."""
        c, N, nxl, P = self.comm, self.N, self.d.nxl, self.comm.size
        Nc = N // 2 + 1
        widths = self.d.widths
        # 1. deposit + ghost plane to the right neighbour (integer add)
        dg, pr = self.d.dep_ghosts, self.d.pot_right
        mesh_i = self.ops.deposit(self.d.plane0, nxl, dg)             # int64 [nxl(+dg), N, N+2]
        if P > 1:
            ghost = c.shift(mesh_i[nxl:nxl + dg].contiguous(), +1)
            mesh_i[0:dg] += ghost
        real = self.ops.to_real(mesh_i[:nxl])                          # f64 [nxl, N, N+2]
        # 2. forward: 2-D r2c over (y, z), transpose (x-slabs -> equal y-slabs), 1-D along x
        spec = torch.fft.rfft2(real[..., :N], dim=(1, 2))              # [nxl, N, Nc], unscaled
        nyl = N // P
        recv, _ = c.all_to_all_rows(self.pack_rows(spec), [nxl] * P)                         # rows [src p][x_l] = all x
        spec_t = recv.reshape(N, nyl, Nc).permute(1, 2, 0).contiguous()                      # [y_l][z][x]
        spec_t = torch.fft.fft(spec_t, dim=2)
        # 3. Green's function / CIC deconvolution on the transposed spectrum (split around the P(k) all-reduce for an analysis hook)
        if xstep is None:
            self.ops.green(spec_t, c.rank * nyl, nyl)
        else:
            xstep(spec_t, c.rank * nyl, nyl, self.ops.green_forward, self.ops.green_finish)
        # 4. inverse: 1-D along x, transpose back, 2-D c2r
        spec_t = torch.fft.ifft(spec_t, dim=2, norm="forward")
        send = spec_t.permute(2, 0, 1).contiguous()                                          # rows = x planes, in order
        recv, _ = c.all_to_all_rows(send, widths)                                            # rows [src q][x_l]
        phi = torch.fft.irfft2(self.unpack_rows(recv), s=(N, N), dim=(1, 2), norm="forward")  # [nxl, N, N], unscaled
        # 5. potential ghost planes (2 from the left neighbour, 3 from the right) and readout
        if P > 1:
            ext = self.ops.empty((nxl + 2 + pr, N, N + 2), torch.float64)
            ext[2:2 + nxl, :, :N] = phi
            ext[0:2, :, :N] = c.shift(phi[nxl - 2:nxl].contiguous(), +1)          # my last 2 -> right rank's left ghosts
            ext[2 + nxl:, :, :N] = c.shift(phi[0:pr].contiguous(), -1)            # my first 3 (4) -> left rank's right ghosts
        else:
            ext = self.ops.empty((N, N, N + 2), torch.float64)
            ext[:, :, :N] = phi
        self.ops.readout(ext, self.d.plane0, nxl, pr)


class _StreamHandover:
    """The hand-over between torch's current stream and the library context's, around a library call on tensors: before() once
    torch has produced the call's inputs, after() once the library has written its outputs."""

    def __init__(self, ctx, device):
        self.ctx, self.device = ctx, device

    def _shared(self):
        """The context was created on torch's current stream: library kernels and torch operators are ordered by the stream
        itself (and the RCCL rounds join it through their work handles), so no host synchronisation is needed anywhere in a
        step.  With a stream of its own (the tests) every hand-over is a full synchronisation of the producing stream."""
        if os.environ.get("SHQ_DIST_SYNC", "0") == "1":      # diagnostic: synchronise around every phase anyway
            return False
        s = getattr(self.ctx, "stream", None)      # 0 is the null stream: shq_init then made a stream of its own
        return bool(s) and int(s) == int(torch.cuda.current_stream(self.device).cuda_stream)

    def before(self):
        if not self._shared():
            torch.cuda.current_stream(self.device).synchronize()

    def after(self):
        if not self._shared():
            self.ctx.synchronize()


def records_pman(sq, L, Pall):
    """the host mirror's particle manager holding a copy of the records Pall (what its tree builder and views take)"""
    pman = sq.PartManager(len(Pall), L)
    pman.Base[:] = Pall
    return pman


def sized_call(call, count, dtype):
    """The library's "how many, then fill" convention: call(buffer, capacity) runs once without a buffer, which leaves the number of
    records in `count` (the c_int64 the call writes), and again with room for them.  Returns the records."""
    capi.check(call(None, 0))
    out = np.zeros(max(count.value, 1), dtype=dtype)
    capi.check(call(capi.ptr(out), len(out)))
    return out[:count.value]


class GpuOps:
    """Local compute phases on the device through the C-ABI (libshenqi_hip.so)."""

    def __init__(self, ctx, Nmesh, BoxSize, Asmth, G, device):
        self.ctx, self.device = ctx, device
        self.pm = capi.PMParams(Nmesh, 0, BoxSize, Asmth, G)
        self.N = Nmesh
        self._hand = _StreamHandover(ctx, device)

    def empty(self, shape, dtype):
        return torch.zeros(shape, dtype=dtype, device=self.device)

    def set_particles(self, posm_all, nlocal, keep_tree=False, types=None, carry=False):
        """posm_all: device tensor [n, 4] (x, y, z, m), the first nlocal rows are this rank's own.  keep_tree: these are the
        positions the resident tree was built from (nothing moved since).  types: the rows' Types (n integers; without them every
        row is Type 1 and the deposit type mask must stay SHQ_ALL_TYPES).  carry: the first nlocal rows are the previous set's
        own particles in the same order (a re-import): their previous-step accelerations stay whatever the ghost count does
        (SHQ_SET_CARRY_LOCAL)."""
        t = posm_all.contiguous()
        ty = None if types is None else types.to(device=t.device, dtype=torch.uint8).contiguous()
        flags = (capi.SET_KEEP_TREE if keep_tree else 0) | (capi.SET_CARRY_LOCAL if carry else 0)
        self._hand.before()                  # torch produced t on its stream; the library copies on its own
        capi.check(capi.hip.shq_particles_set_device(self.ctx.h, C.c_void_p(t.data_ptr()), t.shape[0], nlocal, flags))
        if ty is not None:
            capi.check(capi.hip.shq_particles_set_device_types(self.ctx.h, C.c_void_p(ty.data_ptr()), ty.shape[0]))
        self._hand.after()
        self._keep, self._keep_types = t, ty

    def set_deposit_types(self, mask):
        """shq_pm_set_deposit_types: bit t set = Type t is deposited (capi.ALL_TYPES: all)"""
        capi.check(capi.hip.shq_pm_set_deposit_types(self.ctx.h, int(mask)))

    # ---- phases on the bespoke FFT passes (shq_pm_slab2_*) ----
    def pitch(self):
        return int(capi.hip.shq_pm_slab_pitch(self.N))

    def mesh_buffer(self, nalloc, N, zp):
        key = (nalloc, N, zp)
        if getattr(self, "_mesh_key", None) != key:
            self._mesh = torch.empty((nalloc, N, zp), dtype=torch.int64, device=self.device)
            self._mesh_key = key
        return self._mesh

    def _call(self, fn, *args):
        self._hand.before()
        capi.check(fn(self.ctx.h, *args))
        self._hand.after()

    def deposit2(self, buf, plane0, nxl, xoff, nalloc, ghosts=1):
        self._call(capi.hip.shq_pm_slab2_deposit_ghosts, C.byref(self.pm), plane0, nxl, xoff, nalloc, ghosts, C.c_void_p(buf.data_ptr()))

    def fft_yz(self, planes, nplanes, direction):
        assert planes.is_contiguous()
        self._call(capi.hip.shq_pm_slab2_fft_yz, self.N, C.c_void_p(planes.data_ptr()), nplanes, direction)

    def fft_yz_packed(self, planes, nplanes, direction, packed, nranks):
        """fft_yz with the pack (direction 0) / unpack (direction 1) of the transposes fused into the Y pass: `packed` is the
        all-to-all buffer [nranks * nplanes, N / nranks, zpc] complex"""
        assert planes.is_contiguous() and packed.is_contiguous() and packed.dtype == torch.complex128
        self._call(capi.hip.shq_pm_slab2_fft_yz_packed, self.N, C.c_void_p(planes.data_ptr()), nplanes, direction, C.c_void_p(packed.data_ptr()), nranks)

    def xgreen(self, spec_t, y0, nyl):
        assert spec_t.is_contiguous() and spec_t.dtype == torch.complex128
        self._call(capi.hip.shq_pm_slab2_xgreen, C.byref(self.pm), C.c_void_p(spec_t.data_ptr()), y0, nyl)

    def power(self):
        """this rank's raw P(k) sums of the last X forward / measuring finish: (kk, power, nmodes, norm)"""
        N = self.N
        kk, pw, nm, norm = np.zeros(N), np.zeros(N), np.zeros(N, dtype=np.int64), C.c_double()
        capi.check(capi.hip.shq_pm_download_power(self.ctx.h, N, capi.ptr(kk), capi.ptr(pw), capi.ptr(nm), C.byref(norm)))
        return kk, pw, nm, norm.value

    def _finish(self, fn, args, table, measure):
        """the finish with the context's shq_pm_measure_power set to `measure` for the call; the caller's setting is restored after"""
        tab = None if table is None else np.ascontiguousarray(table, dtype=np.float64)
        h = self.ctx.h
        before = int(capi.hip.shq_pm_get_measure_power(h))
        if before != int(measure):
            capi.check(capi.hip.shq_pm_measure_power(h, int(measure)))
        try:
            self._call(fn, *args, None if tab is None else capi.ptr(tab))
            return self.power() if measure else None
        finally:
            if before != int(measure):
                capi.check(capi.hip.shq_pm_measure_power(h, before))

    def xforward(self, spec_t, y0, nyl):
        """X forward of the y-slab in place and this rank's raw P(k) sums of the density (shq_pm_slab2_xforward)"""
        assert spec_t.is_contiguous() and spec_t.dtype == torch.complex128
        self._call(capi.hip.shq_pm_slab2_xforward, C.byref(self.pm), C.c_void_p(spec_t.data_ptr()), y0, nyl)
        return self.power()

    def xfinish(self, spec_t, y0, nyl, table=None, measure=False):
        """(v T) green and X inverse (shq_pm_slab2_xfinish); with measure the raw sums of v T"""
        assert spec_t.is_contiguous() and spec_t.dtype == torch.complex128
        return self._finish(capi.hip.shq_pm_slab2_xfinish, (C.byref(self.pm), C.c_void_p(spec_t.data_ptr()), y0, nyl), table, measure)

    def readout2(self, phi, plane0, nxl, xoff, nalloc):
        assert phi.is_contiguous()
        self._call(capi.hip.shq_pm_slab2_readout, C.byref(self.pm), plane0, nxl, xoff, nalloc, C.c_void_p(phi.data_ptr()))

    def hilbert_order(self, posm, L):
        """the permutation that orders the rows of posm (x, y, z, m) along the Peano-Hilbert curve, on the device (shq_hilbert_order)"""
        posm = posm.contiguous()
        n = int(posm.shape[0])
        order = torch.empty(n, dtype=torch.int64, device=posm.device)
        if n > 0:
            self._call(capi.hip.shq_hilbert_order, posm.data_ptr(), n, float(L), order.data_ptr())
        return order

    def hilbert_sorted(self, posm, L):
        """rows of posm (x, y, z, m) along the Peano-Hilbert curve, ordered on the device (shq_hilbert_order)"""
        posm = posm.contiguous()
        if int(posm.shape[0]) == 0:
            return posm
        return posm[self.hilbert_order(posm, L)].contiguous()

    def set_deposit_scale(self, total_mass):
        e = 61 - math.frexp(total_mass if total_mass > 0 else 1.0)[1]
        capi.check(capi.hip.shq_pm_set_deposit_log2scale(self.ctx.h, e))
        self.log2scale = e

    def deposit(self, plane0, nxl, ghosts=1):
        if ghosts != 1:
            raise NotImplementedError("slabs cut below the plane need a mesh size with a bespoke transform (shq_pm_slab2_*)")
        nalloc = nxl if nxl == self.N else nxl + 1
        mesh = torch.empty((nalloc, self.N, self.N + 2), dtype=torch.int64, device=self.device)
        self._call(capi.hip.shq_pm_slab_deposit, C.byref(self.pm), plane0, nxl, C.c_void_p(mesh.data_ptr()))
        return mesh

    def to_real(self, mesh_i):
        return mesh_i.to(torch.float64) * (1.0 / 2.0 ** self.log2scale)

    def green(self, spec_t, y0, nyl):
        assert spec_t.is_contiguous() and spec_t.dtype == torch.complex128
        self._call(capi.hip.shq_pm_slab_green, C.byref(self.pm), y0, nyl, C.c_void_p(spec_t.data_ptr()))

    def green_forward(self, spec_t, y0, nyl):
        """this rank's raw P(k) sums of the transposed density spectrum [y_l][z'][x] (shq_pm_slab_xforward)"""
        assert spec_t.is_contiguous() and spec_t.dtype == torch.complex128
        self._call(capi.hip.shq_pm_slab_xforward, C.byref(self.pm), y0, nyl, C.c_void_p(spec_t.data_ptr()))
        return self.power()

    def green_finish(self, spec_t, y0, nyl, table=None, measure=False):
        """(v T) green on that layout (shq_pm_slab_xfinish); with measure the raw sums of v T"""
        assert spec_t.is_contiguous() and spec_t.dtype == torch.complex128
        return self._finish(capi.hip.shq_pm_slab_xfinish, (C.byref(self.pm), y0, nyl, C.c_void_p(spec_t.data_ptr())), table, measure)

    def readout(self, ext, plane0, nxl, pot_right=3):
        assert ext.is_contiguous() and pot_right == 3
        self._call(capi.hip.shq_pm_slab_readout, C.byref(self.pm), plane0, nxl, C.c_void_p(ext.data_ptr()))

    def results(self, nlocal):
        g = np.zeros((self._keep.shape[0], 3))
        p = np.zeros(self._keep.shape[0])
        capi.check(capi.hip.shq_pm_download(self.ctx.h, capi.ptr(g), capi.ptr(p)))
        return g[:nlocal], p[:nlocal]


class DistTreePM:
    """One rank of the sharded TreePM force: PM over x-slabs + tree walk over local + ghost particles."""

    def __init__(self, comm, ctx, Nmesh, BoxSize, Asmth, G, device, halo_factor=1.5, bounds=None, ycuts=None):
        import shenqi_amd as sq
        self.sq = sq
        self.comm, self.ctx, self.device = comm, ctx, device
        self.N, self.L, self.Asmth, self.G = Nmesh, BoxSize, Asmth, G
        self.ops = GpuOps(ctx, Nmesh, BoxSize, Asmth, G, device)
        self.pm = SlabPM(comm, Nmesh, BoxSize, Asmth, G, self.ops, bounds, ycuts)
        self.decomp = self.pm.d
        self.halo_factor = halo_factor
        self.tree = None
        self.local_types = self.types = None
        self._moved = False

    def setup(self, posm_local, Rcut, types=None):
        """posm_local: device tensor [nloc, 4] of the particles this rank owns (already exchanged to
        their owner).  Orders them along a space-filling curve, imports ghosts, builds the tree on the device.
        types: the particles' Types (nloc integers), which then travel with their rows through the ordering and every ghost import
        (for the deposit type mask, ops.set_deposit_types)."""
        order = self.ops.hilbert_order(posm_local, self.L)
        self.local = posm_local.contiguous()[order].contiguous()
        self.local_types = None if types is None else types.to(posm_local.device)[order].contiguous()
        self.nloc = int(self.local.shape[0])
        self.halo = self.halo_factor * Rcut
        self.ops.set_deposit_scale(self.comm.allreduce_sum(float(self.local[:, 3].sum().item())))
        self._load_particles()
        self._build_tree()
        self._moved = False

    def move(self, posm_local):
        """New positions (a drift) of the particles this rank owns: device tensor [nloc, 4], the rows of self.local in the same
        order.  The next step() imports the ghosts for them and rebuilds the tree, and the rows keep their previous-step
        accelerations.  Every particle must still lie in this rank's slab (with ycuts: on its side of a shared plane): the slab
        deposit has ghost planes for the CIC cloud only, not for particles of another slab.  That is checked here on the host,
        before anything is launched; a particle that left goes through exchange_to_owner + setup instead."""
        if tuple(posm_local.shape) != (self.nloc, 4):
            raise ValueError("move: expected the %d rows (x, y, z, m) of self.local, got shape %s" % (self.nloc, tuple(posm_local.shape)))
        host = posm_local.detach().contiguous().cpu()
        owner = self.decomp.owner_of(host[:, 0], host[:, 1])
        out = int((owner != self.comm.rank).sum())
        if out:
            i = int(torch.nonzero(owner != self.comm.rank)[0])
            raise ValueError("move: %d of the %d particles left the slab of rank %d (the first: row %d at x = %.17g, y = %.17g, now rank "
                             "%d's): migration between ranks goes through exchange_to_owner + setup, not through move"
                             % (out, self.nloc, self.comm.rank, i, float(host[i, 0]), float(host[i, 1]), int(owner[i])))
        self.local = posm_local.detach().to(self.device).contiguous()
        self._moved = True

    def _build_tree(self):
        """local + ghost particles are resident: build their tree (global root cell) on the device"""
        sq = self.sq
        try:
            self.tree = sq.tree_build_device(self.ctx, self.L)
        except sq.ShqError as e:
            if "deeper" not in str(e) and "levels" not in str(e):
                raise       # out of memory, invalid state ...: not something a host build would cure
            # deeper than the device build's 21 levels (more than 8 particles within L / 2^21): host build + upload
            allh = self.allp.cpu().numpy()
            pman = sq.PartManager(allh.shape[0], self.L)
            pman.Base["Pos"] = allh[:, :3]
            pman.Base["Mass"] = allh[:, 3]
            pman.Base["Type"] = 1
            self.pman = pman
            self.tree = sq.force_tree_full(pman)
            tv = self.tree.view()
            capi.check(capi.hip.shq_tree_upload(self.ctx.h, C.byref(tv)))

    def _load_particles(self, keep_tree=False, carry=False):
        if self.local_types is None:
            ghosts = ghost_exchange(self.comm, self.decomp, self.local, self.halo)
            self.types = None
        else:
            ghosts, gtypes = _split_types(ghost_exchange(self.comm, self.decomp, _with_types(self.local, self.local_types), self.halo),
                                          self.local_types.dtype)
            self.types = torch.cat([self.local_types, gtypes], dim=0).contiguous()
        self.allp = torch.cat([self.local, ghosts], dim=0).contiguous()
        self.nghost = int(ghosts.shape[0])
        self.ops.set_particles(self.allp, self.nloc, keep_tree, types=self.types, carry=carry)

    def step(self, gp, update_potential=1, walk_mode=0, overlap=None, moved=False, analysis=None, measure_power=False):
        """One force evaluation: ghost import, PM, OldAcc, walk for the local targets.
        moved: self.local changed since the tree was built (a drift; implied after move()): the ghosts are imported for the new
        positions and the tree is rebuilt.  Without it the step repeats the evaluation on the positions of setup(): the ghost
        exchange still runs (it is part of a step), the tree is kept.  Either way the local rows keep the accelerations of the
        previous step, however many ghosts come and go (SHQ_SET_CARRY_LOCAL).
        Without overlap the order is the reference's (run.cpp:518-523, gravshort2.hpp:111-121): PM, then OldAcc =
        |FullTreeGravAccel(k-1) + GravPM(k)| / G from the NEW GravPM, then the walk - what shq_treepm_step does on one card.
        overlap (default: whenever the transposes are collectives; SHQ_DIST_OVERLAP=0 turns it off): the walk is cut in two
        pieces that are queued behind the start of the two mesh transposes, so that it computes while the spectrum travels over
        xGMI.  It therefore runs before its own step's PM exists and opens nodes by |FullTreeGravAccel(k-1) + GravPM(k-1)| / G,
        the OldAcc formed at the end of the previous step: this departs from run.cpp:518-523, which uses the new GravPM.
        analysis, measure_power: as SlabPM.force (massive neutrinos); the reduced sums are in self.pm.power / power_finish."""
        moved = bool(moved) or self._moved
        self._load_particles(keep_tree=not moved, carry=True)
        if moved:
            self._build_tree()
            self._moved = False
        if overlap is None:
            overlap = self.comm.multi and os.environ.get("SHQ_DIST_OVERLAP", "1") != "0"
        if overlap and self.nloc >= 512:
            half = (self.nloc // 2) // 256 * 256

            def piece(first, count):
                return lambda: capi.check(capi.hip.shq_grav_short_run_range(self.ctx.h, C.byref(gp), first, count,
                                                                           int(update_potential), walk_mode))
            self.pm.force([piece(0, half), piece(half, self.nloc - half)], analysis=analysis, measure_power=measure_power)
        else:
            self.pm.force(analysis=analysis, measure_power=measure_power)
            if not overlap:      # a rank too small to cut its walk still computes what the overlap mode computes
                capi.check(capi.hip.shq_grav_refresh_oldacc(self.ctx.h, self.G))
            capi.check(capi.hip.shq_grav_short_run(self.ctx.h, C.byref(gp), None, 0, int(update_potential), walk_mode))
        # |FullTreeGravAccel(k) + GravPM(k)| / G: what the next step's walk opens by when that step overlaps
        capi.check(capi.hip.shq_grav_refresh_oldacc(self.ctx.h, self.G))

    def download(self, ninteractions=False):
        """(FullTreeGravAccel, tree potential, GravPM, PM potential) of the local rows; with ninteractions also the last walk's
        interaction count of every local target, as a fifth entry"""
        n = int(self.allp.shape[0])
        acc = np.zeros((n, 3))
        pot = np.zeros(n)
        nint = np.zeros(n, dtype=np.int64) if ninteractions else None
        capi.check(capi.hip.shq_grav_short_download(self.ctx.h, capi.ptr(acc), capi.ptr(pot), capi.ptr(nint), None))
        gpm, ppot = self.ops.results(self.nloc)
        if ninteractions:
            return acc[: self.nloc], pot[: self.nloc], gpm, ppot, nint[: self.nloc]
        return acc[: self.nloc], pot[: self.nloc], gpm, ppot


# ---------------------------------------------------------------------------------------------------------------------
# Sharded SPH (density with the Hsml loop, hydro force): the same ghost-import design as the tree.
# The reference exports queries to the ranks whose top-leaves a target's search sphere touches, walks them there and
# imports the partial results (treewalk2.h:480-557 do_hsml_loop with exports, DensityQuery / HydroQuery wire formats,
# densitytree2.hpp:260-344, hydratree2.hpp:151-228), once per Hsml iteration.  Here every rank imports, once per operator,
# the records of the other ranks' gas within reach of its slab and runs the whole operator locally for its own targets:
#   density: a neighbour j matters to target i if r_ij < Hsml_i           -> import within halo = hfac * max local Hsml;
#            the Hsml loop may grow a target's Hsml past the halo: then the import is repeated with a larger one
#            (widen_until_covered above);
#   hydro:   symmetric, r_ij < max(Hsml_i, Hsml_j) (hydratree2.hpp:258-259; the reference propagates hmax for this,
#            run.cpp:493)                                                 -> a particle goes to rank d if it lies within
#            max(its own Hsml, max Hsml of d's targets) of d's slab; its record carries the density results of its owner.
# Records travel whole (particle_data 160 B + sph_particle_data 176 B), so predicted velocities and entropies of ghosts are
# evaluated from the same fields as on their owner.  The operators on sets that hold more than gas (winds, metal return) import
# through import_ghost_gas above, which stamps the ghosts with their owner and row.
class DistSPH:
    """One rank of the sharded SPH operators.  `P` / `SphP`: numpy arrays (capi.PARTICLE_DTYPE / capi.SPH_DTYPE) of the gas this
    rank owns (PI = slot index).  `ops` runs an operator on local + ghost particles for the first `nloc` of them:
    ops.density(P, SphP, nloc, **kw) updates Hsml / DtHsml / the density fields of the targets in place;
    ops.hydro(P, SphP, nloc, **kw) likewise HydroAccel / DtEntropy / MaxSignalVel (GpuSphOps below; the tests use the oracle)."""

    def __init__(self, comm, decomp, ops, hfac=1.3):
        self.comm, self.d, self.ops, self.hfac = comm, decomp, ops, hfac
        self.nghost = 0

    def _import(self, P, SphP, reach, reach_of_rank):
        """local + ghost records, everything gas: the slots in the order of the particles, PI = 0 .. n"""
        nloc, S = len(P), SphP[P["PI"]]
        rec = np.concatenate([P.view(np.uint8).reshape(nloc, -1), S.view(np.uint8).reshape(nloc, -1)], axis=1)
        got = ghost_records(self.comm, self.d, torch.from_numpy(np.ascontiguousarray(P["Pos"][:, 0])), torch.from_numpy(reach),
                            torch.from_numpy(rec), reach_of_rank).numpy()
        self.nghost = len(got)
        psz = P.dtype.itemsize
        Pall, Sall = append_records(P, got[:, :psz]), append_records(S, got[:, psz:])
        Pall["PI"] = np.arange(len(Pall))
        return Pall, Sall

    def density(self, P, SphP, **kw):
        """density() for the local gas (Hsml loop included), by widen_until_covered.  Returns the number of import rounds it took.
        ops.density returns the largest Hsml the loop tried where it can (shq_sph_stats.hsml_max_tried), else None."""
        nloc = len(P)
        h0 = P["Hsml"].copy()
        Pall = Sall = None

        def attempt(halos):
            nonlocal Pall, Sall
            Pall, Sall = self._import(P, SphP, np.zeros(nloc), halos)
            Pall["Hsml"][:nloc] = h0
            tried = self.ops.density(Pall, Sall, nloc, **kw)
            return max(float(Pall["Hsml"][:nloc].max()), float(tried or 0.0)) if nloc else 0.0
        rounds = widen_until_covered(self.comm, self.hfac, float(h0.max()) if nloc else 0.0, attempt)
        for k in ("Hsml", "DtHsml"):
            P[k] = Pall[k][:nloc]
        for k in ("Density", "EgyWtDensity", "DhsmlEgyDensityFactor", "DivVel", "CurlVel"):
            SphP[k][P["PI"]] = Sall[k][:nloc]
        return rounds

    def hydro(self, P, SphP, **kw):
        """hydro_force() for the local gas; needs the density fields of density() above on every rank"""
        nloc = len(P)
        hmax = self.comm.gather_scalar(float(P["Hsml"].max()) if nloc else 0.0)
        Pall, Sall = self._import(P, SphP, P["Hsml"].astype(np.float64), hmax)
        self.ops.hydro(Pall, Sall, nloc, **kw)
        for k in ("HydroAccel", "DtEntropy", "MaxSignalVel"):
            SphP[k][P["PI"]] = Sall[k][:nloc]


def gas_rows_from_records(P, SphP):
    """[n, capi.GAS_NCOL] float64 rows (the layout of shq_gas_set_device, include/shenqi_hip.h) of gas records
    (capi.PARTICLE_DTYPE / capi.SPH_DTYPE, slot = PI)"""
    n = len(P)
    S = SphP[P["PI"]]
    r = np.zeros((n, capi.GAS_NCOL))
    r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = P["Pos"], P["Mass"], P["Vel"], P["Hsml"]
    r[:, 8:11], r[:, 11:14], r[:, 14:17] = P["FullTreeGravAccel"], P["GravPM"], S["HydroAccel"]
    r[:, 17], r[:, 18], r[:, 19] = S["Entropy"], S["DtEntropy"], S["DelayTime"]
    r[:, 20], r[:, 21], r[:, 22], r[:, 23], r[:, 24] = S["Density"], S["EgyWtDensity"], S["DhsmlEgyDensityFactor"], S["DivVel"], S["CurlVel"]
    r[:, 25], r[:, 26] = S["MaxSignalVel"], P["DtHsml"]
    r[:, 27] = P["TimeBinGravity"].astype(np.float64) + 256.0 * P["TimeBinHydro"].astype(np.float64)
    return r


def gas_rows_to_records(rows, P, SphP):
    """the result columns of rows (density and hydro) back into the records"""
    pi = P["PI"]
    P["Hsml"], P["DtHsml"] = rows[:, 7], rows[:, 26]
    for c, k in ((20, "Density"), (21, "EgyWtDensity"), (22, "DhsmlEgyDensityFactor"), (23, "DivVel"), (24, "CurlVel"), (18, "DtEntropy"),
                 (25, "MaxSignalVel")):
        SphP[k][pi] = rows[:, c]
    SphP["HydroAccel"][pi] = rows[:, 14:17]


class DistSPHDevice:
    """One rank of the sharded SPH operators with the gas RESIDENT on the device: `rows` is a float64 device tensor
    [nloc, capi.GAS_NCOL] of the gas this rank owns (layout: shq_gas_set_device).  Ghost rows travel as device tensors through the
    all-to-all (RCCL; gloo stages them through the host inside Comm), local + ghost rows become the context's particle set by one
    scatter kernel, the tree of that set is built on the device (shq_tree_build over the gas), density / hydro run on the first
    nloc rows (shq_density_resident / shq_hydro_resident) and one gather kernel writes the results back into the rows: no host
    numpy and no PCIe copy of particle data inside an operator (the import rule is DistSPH's, see above)."""

    def __init__(self, comm, decomp, ctx, BoxSize, hfac=1.3):
        import shenqi_amd as sq
        self.sq, self.comm, self.d, self.ctx, self.L, self.hfac = sq, comm, decomp, ctx, BoxSize, hfac
        self.nghost = 0
        self.stats = {}

    def _load(self, rows, reach, reach_of_rank):
        """import the ghosts, make local + ghost rows the resident set, build their tree"""
        ghosts = ghost_records(self.comm, self.d, rows[:, 0], reach, rows, reach_of_rank)
        allrows = torch.cat([rows, ghosts.to(rows.device)], dim=0).contiguous()
        self.nghost = int(ghosts.shape[0])
        self._hand = _StreamHandover(self.ctx, rows.device)
        self._hand.before()        # torch produced allrows on its stream
        capi.check(capi.hip.shq_gas_set_device(self.ctx.h, allrows.data_ptr(), int(allrows.shape[0]), int(rows.shape[0])), "shq_gas_set_device")
        self.sq.tree_build_device(self.ctx, self.L, mask=self.sq.GASMASK)
        return allrows

    def _results(self, allrows, nloc, which):
        capi.check(capi.hip.shq_gas_get_device(self.ctx.h, allrows.data_ptr(), nloc, which), "shq_gas_get_device")
        self._hand.after()         # the library wrote allrows on its stream

    def density(self, rows, dp):
        """density() for the local gas (Hsml loop included), by widen_until_covered; rows are updated in place.  Returns the number
        of import rounds."""
        nloc = int(rows.shape[0])
        h0 = rows[:, 7].clone()
        st = capi.SphStats()
        allrows = None

        def attempt(halos):
            nonlocal allrows
            rows[:, 7] = h0
            allrows = self._load(rows, torch.zeros(nloc, dtype=torch.float64, device=rows.device), halos)
            capi.check(capi.hip.shq_density_resident(self.ctx.h, C.byref(dp), C.byref(st)), "shq_density_resident")
            self._results(allrows, nloc, 1)
            return max(float(st.hsml_max_tried), float(allrows[:nloc, 7].max().item())) if nloc else 0.0
        rounds = widen_until_covered(self.comm, self.hfac, float(h0.max().item()) if nloc else 0.0, attempt)
        rows.copy_(allrows[:nloc])
        self.stats["density"] = dict(kernel_ms=float(st.kernel_ms), iterations=int(st.niterations), ninteractions=int(st.ninteractions), nghost=self.nghost)
        return rounds

    def hydro(self, rows, hp):
        """hydro_force() for the local gas; needs the density fields of density() above on every rank"""
        nloc = int(rows.shape[0])
        hmax = self.comm.gather_scalar(float(rows[:, 7].max().item()) if nloc else 0.0)
        allrows = self._load(rows, rows[:, 7].contiguous(), hmax)
        st = capi.SphStats()
        capi.check(capi.hip.shq_hydro_resident(self.ctx.h, C.byref(hp), C.byref(st)), "shq_hydro_resident")
        self._results(allrows, nloc, 2)
        rows.copy_(allrows[:nloc])
        self.stats["hydro"] = dict(kernel_ms=float(st.kernel_ms), ninteractions=int(st.ninteractions), nghost=self.nghost)


class GpuSphOps:
    """DistSPH's operators on the device library, through the host mirror of the reference API (one-shot calls: the records
    cross PCIe once per operator)."""

    def __init__(self, ctx, BoxSize):
        import shenqi_amd as sq
        self.sq, self.ctx, self.L = sq, ctx, BoxSize

    def density(self, Pall, Sall, nloc, DoEgyDensity=1, kick=None, **_):
        sq = self.sq
        pman = records_pman(sq, self.L, Pall)
        tree = sq.force_tree_rebuild_mask(pman, sq.GASMASK)
        BhP = np.zeros(2, dtype=sq.BH_SLOT_DTYPE)
        _, st = sq.density(self.ctx, np.arange(nloc, dtype=np.int32), 1, DoEgyDensity, 0, kick, tree, pman, Sall, BhP)
        Pall[:] = pman.Base
        return float(st.hsml_max_tried)     # the largest Hsml any walk of the loop searched with

    def hydro(self, Pall, Sall, nloc, atime=0.1, hubble=0.1, kick=None, **_):
        sq = self.sq
        pman = records_pman(sq, self.L, Pall)
        tree = sq.force_tree_rebuild_mask(pman, sq.GASMASK)
        sq.force_tree_update_hmax(tree, pman)
        sq.hydro_force(self.ctx, np.arange(nloc, dtype=np.int32), atime, hubble, None, kick, tree, pman, Sall)


class DistFOF:
    """One rank of the friends-of-friends finder over x-slabs (fof.cpp's multi-task part, re-cut for ghost imports).

    The reference links across tasks by exporting primary particles to the tasks whose top leaves they touch and lowering MinID
    on both sides until nothing changes (fof_label_primary's do-while with the ghost branch of fof_primary_ngbiter, fof.cpp:404-470,
    565-580), then reduces the groups that span tasks onto the task of their MinID particle (fof_reduce_groups).  Here every rank
    imports the particles within `halo` of its slab once, labels local + ghost particles (ops.labels: shq_fof on the device, the
    oracle in the CPU tests), and the ranks then lower labels through the particles they share — the owner's label goes to its
    ghost copies, each rank takes the minimum over its local components — until no label changes anywhere.  The secondary types are
    attached by a second labelling call that carries the final labels of the primaries as their "IDs".  Groups are summed per rank
    over the particles it owns and reduced by MinID; FirstPos is the position of the group's MinID particle on every rank (the
    reference uses whichever member its unstable sort put first on the prime task).

    `P`: numpy records (capi.PARTICLE_DTYPE) of the particles this rank owns, all inside its slab.
    ops.labels(Pall, ids, linkl, primary_mask, secondary_mask) -> MinID per particle of Pall (np.uint64)."""

    def __init__(self, comm, decomp, ops):
        self.comm, self.d, self.ops = comm, decomp, ops
        self.rounds = 0
        self.nghost = 0

    def _selections(self, x, halo):
        """per destination rank: which of my particles it holds as ghosts (the same masks give the order of every later label
        message, so labels travel as bare uint64 rows)"""
        return [None if dd == self.comm.rank or not self.comm.multi else self.d.reach_mask(dd, x, halo) for dd in range(self.comm.size)]

    def _send(self, rows, sels):
        parts, counts = [], [0] * self.comm.size
        for dd, s in enumerate(sels):
            if s is None:
                continue
            parts.append(rows[s])
            counts[dd] = int(s.sum())
        send = np.concatenate(parts, axis=0) if parts else rows[:0]
        recv, _ = self.comm.all_to_all_rows(torch.from_numpy(np.ascontiguousarray(send)), counts)
        return recv.numpy()

    def fof(self, P, linkl, minlength, primary_mask=2, secondary_mask=1 + 16 + 32):
        """Returns (MinID per local particle, groups hosted by this rank as a list of dicts ordered by MinID, GrNr per local
        particle).  A group is hosted by the rank that owns its MinID particle; GrNr is global (by decreasing length, then MinID)."""
        comm, L = self.comm, self.d.L
        nloc = len(P)
        ids = P["ID"].astype(np.uint64)
        # the largest radius the secondary search can reach: the first of 0.4 L 2^k (or 0.5 Hsml 2^k) that is >= 4 linking lengths
        hs = float(P["Hsml"].max()) if nloc else 0.0
        halo = float(comm.gather_scalar(max(8.0 * linkl, hs if comm.multi else 0.0)).max())
        sels = self._selections(np.ascontiguousarray(P["Pos"][:, 0]), halo)
        got = self._send(P.view(np.uint8).reshape(nloc, -1), sels)      # nothing on one rank
        self.nghost = len(got)
        Pall = append_records(P, got)
        idall = Pall["ID"].astype(np.uint64)
        prim = (((1 << Pall["Type"].astype(np.int64)) & primary_mask) != 0) & ((Pall["Flags"] & 3) == 0)
        # 1. local components of the primaries (label = smallest ID inside local + ghost)
        lab = self.ops.labels(Pall, idall, linkl, primary_mask, 0)
        comp_key, comp = np.unique(lab, return_inverse=True)
        # 2. lower the labels through the shared particles until nothing changes anywhere
        self.rounds = 0
        while comm.multi:
            self.rounds += 1
            # my owners' labels -> their ghost copies elsewhere (as int64 bit patterns: gloo / NCCL carry no uint64)
            recv = np.ascontiguousarray(self._send(lab[:nloc].view(np.int64).reshape(-1, 1), sels).reshape(-1)).view(np.uint64)
            new = lab.copy()
            new[nloc:] = np.minimum(new[nloc:], recv)
            low = np.full(len(comp_key), np.iinfo(np.uint64).max, dtype=np.uint64)
            np.minimum.at(low, comp, new)
            new = np.where(prim, low[comp], new)
            changed = int((new != lab).sum())
            lab = new
            if comm.allreduce_sum(float(changed)) == 0.0:      # a count, exact as a float
                break
        # 3. secondary types: nearest primary; the primaries carry their final labels as IDs, everybody else its own ID
        ids2 = np.where(prim, lab, idall)
        lab2 = self.ops.labels(Pall, ids2, linkl, primary_mask, secondary_mask)
        minid = lab2[:nloc].copy()
        # 4. catalogue: lengths first (groups below minlength go), then the sums of the owned members, reduced by MinID
        key, inv = np.unique(minid, return_inverse=True)
        cnt = np.bincount(inv, minlength=len(key)).astype(np.int64)
        allk, allc = self._gather_pairs(key, cnt)
        tot_key, tinv = np.unique(allk, return_inverse=True)
        tot_len = np.bincount(tinv, weights=allc, minlength=len(tot_key)).astype(np.int64)
        keep = tot_len >= minlength
        kept_key, kept_len = tot_key[keep], tot_len[keep]
        order = np.lexsort((kept_key, -kept_len))
        grnr_of = np.empty(len(kept_key), dtype=np.int64)
        grnr_of[order] = np.arange(1, len(kept_key) + 1)
        pos_in_kept = np.searchsorted(kept_key, minid)
        pos_in_kept = np.minimum(pos_in_kept, max(len(kept_key) - 1, 0))
        ingroup = (kept_key[pos_in_kept] == minid) if len(kept_key) else np.zeros(nloc, dtype=bool)
        part_grnr = np.where(ingroup, grnr_of[pos_in_kept] if len(kept_key) else -1, -1)
        groups = self._catalogue(P, minid, ingroup, pos_in_kept, kept_key, kept_len, grnr_of, ids)
        return minid, groups, part_grnr

    def _gather_pairs(self, key, val):
        """all ranks' (key, value) rows"""
        if not self.comm.multi:
            return key, val
        rows = np.stack([key.astype(np.uint64).view(np.int64), val.astype(np.int64)], axis=1)
        counts = [len(rows)] * self.comm.size
        send = np.concatenate([rows] * self.comm.size, axis=0) if len(rows) else rows
        recv, _ = self.comm.all_to_all_rows(torch.from_numpy(np.ascontiguousarray(send)), counts)
        r = recv.numpy()
        return r[:, 0].copy().view(np.uint64), r[:, 1].copy()

    def _catalogue(self, P, minid, ingroup, gidx, kept_key, kept_len, grnr_of, ids):
        """add_particle_to_group over the owned members of every kept group, fof_reduce_groups by allgather, then
        fof_finish_group_properties on the host rank of each group (fof.cpp:583-705, 903-1040)"""
        comm, L = self.comm, self.d.L
        ngk = len(kept_key)
        # FirstPos: the position (as float, BaseGroup.FirstPos) of the MinID particle, known to its owner, gathered
        fp = np.zeros((ngk, 4))
        mine = np.flatnonzero(ingroup & (ids == minid))
        fp[gidx[mine], :3] = P["Pos"][mine].astype(np.float32).astype(np.float64)
        fp[gidx[mine], 3] = 1.0
        fp = comm.allreduce_sum_vec(fp)
        host = fp[:, 3] > 0                    # exactly one owner per kept group holds the MinID particle
        first = fp[:, :3]
        hosted = np.zeros(ngk, dtype=bool)
        hosted[gidx[mine]] = True
        nf = 1 + 6 + 6 + 3 + 3 + 9 + 3          # Mass, LenType, MassType, CM, Vel, Imom, Jmom
        S = np.zeros((ngk, nf))
        m = np.flatnonzero(ingroup)
        if len(m):
            g = gidx[m]
            mass = P["Mass"][m].astype(np.float64)
            ty = P["Type"][m].astype(np.int64)
            d = P["Pos"][m] - first[g]
            rel = np.where(d > 0.5 * L, d - L, np.where(d < -0.5 * L, d + L, d))
            xyz = rel + first[g]
            vel = P["Vel"][m]
            jm = np.stack([rel[:, 1] * vel[:, 2] - vel[:, 1] * rel[:, 2], rel[:, 2] * vel[:, 0] - vel[:, 2] * rel[:, 0],
                           rel[:, 0] * vel[:, 1] - vel[:, 0] * rel[:, 1]], axis=1)
            np.add.at(S[:, 0], g, mass)
            np.add.at(S, (g, 1 + ty), 1.0)
            np.add.at(S, (g, 7 + ty), mass)
            for k in range(3):
                np.add.at(S[:, 13 + k], g, mass * xyz[:, k])
                np.add.at(S[:, 16 + k], g, mass * vel[:, k])
                np.add.at(S[:, 28 + k], g, mass * jm[:, k])
                for k2 in range(3):
                    np.add.at(S[:, 19 + 3 * k + k2], g, mass * rel[:, k] * rel[:, k2])
        S = comm.allreduce_sum_vec(S)
        groups = []
        for gi in np.flatnonzero(hosted):
            s = S[gi]
            M = s[0]
            G = dict(MinID=int(kept_key[gi]), Length=int(kept_len[gi]), GrNr=int(grnr_of[gi]), LenType=[int(round(v)) for v in s[1:7]],
                     MassType=[float(v) for v in s[7:13]], Mass=float(M), FirstPos=first[gi].astype(np.float32))
            vcm = s[16:19] / M
            cm = s[13:16] / M
            dcm = cm - first[gi]
            rel = np.where(dcm > 0.5 * L, dcm - L, np.where(dcm < -0.5 * L, dcm + L, dcm))
            G["CM"] = np.mod(cm, L)
            G["Vel"] = vcm
            jcm = np.array([rel[1] * vcm[2] - vcm[1] * rel[2], rel[2] * vcm[0] - vcm[2] * rel[0], rel[0] * vcm[1] - vcm[0] * rel[1]])
            G["Jmom"] = s[28:31] - jcm * M
            G["Imom"] = s[19:28].reshape(3, 3) - M * np.outer(rel, rel)
            groups.append(G)
        groups.sort(key=lambda G: G["MinID"])
        return groups

class GpuFofOps:
    """DistFOF's labelling on the device library (shq_fof: tree of the primary types, linking, secondary attachment)."""

    def __init__(self, ctx, BoxSize):
        import shenqi_amd as sq
        self.sq, self.ctx, self.L = sq, ctx, BoxSize

    def labels(self, Pall, ids, linkl, primary_mask, secondary_mask):
        sq = self.sq
        n = len(Pall)
        pman = records_pman(sq, self.L, Pall)
        pv = pman.view()
        capi.check(capi.hip.shq_particles_upload(self.ctx.h, C.byref(pv)))
        sq.dynamics_upload(self.ctx, pman)
        fp = capi.FofParams(self.L, linkl, primary_mask, secondary_mask, 1 << 30, 0)     # no catalogue wanted here
        out = np.zeros(n, dtype=np.uint64)
        idarr = np.ascontiguousarray(ids, dtype=np.uint64)
        ng = C.c_int64()
        capi.check(capi.hip.shq_fof(self.ctx.h, C.byref(fp), capi.ptr(idarr), capi.ptr(out), None, C.byref(ng)))
        return out


# ---------------------------------------------------------------------------------------------------------------------
# Particle exchange between ranks on full records: ExchangePlan::domain_exchange
# (libgadget/exchange.hpp:242-333) with the loops on the device (shq_exchange_plan / _pack / _unpack, shq_slots_gc) and the
# collectives through Comm — RCCL when the group is nccl, so the payloads cross xGMI from device buffer to device buffer.
class DistExchange:
    """One rank of a domain exchange.  parts: device uint8 tensor of MaxPart records (layout.part_elsize bytes each), slots: per type a
    device uint8 tensor of slot records or None; layoutfn(parts, numpart) -> device int32 tensor with one target task per particle
    (ExchangePlan::layoutfunc; under shenqi's decomposition what shq_domain_maintain_topleaf writes), evaluated every round as the
    reference does.  maxlast caps the list entries sent per round (find_iter_space's role); a capped or memory-short round runs the
    garbage collection between pack and receive (exchange_once, exchange.hpp:398-406, with shall_we_compact_slots)."""

    def __init__(self, comm, ctx, layout):
        self.comm, self.ctx, self.L = comm, ctx, layout
        self.rounds = 0

    @staticmethod
    def _entries(arr):
        e = (capi.ExchangeEntry * len(arr))()
        for k, row in enumerate(arr):
            e[k].base = int(row[0])
            for t in range(6):
                e[k].slots[t] = int(row[1 + t])
        return e

    @staticmethod
    def _offsets(c):
        o = np.zeros_like(c)
        o[1:] = np.cumsum(c[:-1], axis=0)
        return o

    def _allsum(self, v):
        """element-wise sum of a small int64 vector over the ranks"""
        return self.comm.allreduce_sum_vec(np.asarray(v, dtype=np.int64))

    def exchange(self, parts, numpart, slots, slot_size, layoutfn, maxlast=0, maxrounds=10000):
        comm, L, h = self.comm, self.L, self.ctx.h
        esz = int(L.part_elsize)
        maxpart = parts.numel() // esz
        ssz = [int(L.slot_elsize[t]) for t in range(6)]
        cap = [0 if slots[t] is None else slots[t].numel() // ssz[t] for t in range(6)]
        slot_size = [int(x) for x in slot_size]
        dev = parts.device
        ntask = comm.size
        self.rounds = 0
        sp = (C.c_void_p * 6)(*[None if s is None else s.data_ptr() for s in slots])
        while True:
            if self.rounds >= maxrounds:
                raise RuntimeError("DistExchange: no end after %d rounds" % maxrounds)
            target = layoutfn(parts, numpart).to(torch.int32).contiguous()
            tg = (capi.ExchangeEntry * ntask)()
            nex, last = C.c_int64(), C.c_int64()
            torch.cuda.current_stream(dev).synchronize()
            capi.check(capi.hip.shq_exchange_plan(h, C.byref(L), parts.data_ptr(), numpart, target.data_ptr(), comm.rank, ntask, int(maxlast), C.byref(nex),
                                                  C.byref(last), tg))
            togo = np.array([[tg[t].base] + list(tg[t].slots) for t in range(ntask)], dtype=np.int64)
            if int(self._allsum([nex.value])[0]) == 0:          # nobody has anything to send
                break
            self.rounds += 1
            # MPI_Alltoall of the plan (exchange.hpp:217-219)
            if comm.multi:
                toget = comm.all_to_all_equal(torch.from_numpy(togo.copy()).to(dev if comm.backend == "nccl" else "cpu")).cpu().numpy()
            else:
                toget = togo.copy()
            soff, goff = self._offsets(togo), self._offsets(toget)
            nsend, nrecv = togo.sum(axis=0), toget.sum(axis=0)
            # Capacity first, before anything is packed or marked (the pack turns the leavers into garbage, and a rank that raised
            # alone would leave the others blocked in the next collective): what cannot fit even once every leaver's record has been
            # collected fails here, on every rank together, as the reference's endrun ends the whole job (exchange.hpp:286-296).
            short = [int(numpart - int(nsend[0]) + int(nrecv[0]) > maxpart)]
            short += [int(slots[t] is not None and slot_size[t] - int(nsend[1 + t]) + int(nrecv[1 + t]) > cap[t]) for t in range(6)]
            gshort = self._allsum(short)
            if gshort.sum() > 0:
                what = "MaxPart %d" % maxpart if gshort[0] else "the slot array of type %d" % int(np.flatnonzero(gshort[1:])[0])
                raise MemoryError("DistExchange: the arrivals of this round do not fit %s on %d rank(s); nothing was packed" % (what, int(gshort.max())))
            partbuf = torch.empty(max(int(nsend[0]), 1) * esz, dtype=torch.uint8, device=dev)
            slotbuf = [None if slots[t] is None else torch.empty(max(int(nsend[1 + t]), 1) * ssz[t], dtype=torch.uint8, device=dev) for t in range(6)]
            bp = (C.c_void_p * 6)(*[None if b is None else b.data_ptr() for b in slotbuf])
            capi.check(capi.hip.shq_exchange_pack(h, C.byref(L), parts.data_ptr(), sp, maxpart, self._entries(soff), ntask, partbuf.data_ptr(), bp))
            # shall_we_gc on any task (:398-402), the slot types to compact on any task (shall_we_compact_slots, :300-317)
            mine = [int(last.value < nex.value or numpart + int(nrecv[0]) > maxpart)]
            for t in range(6):
                c = 0
                if slots[t] is not None and (slot_size[t] + int(nrecv[1 + t]) > 0.95 * cap[t] or int(nsend[1 + t]) > 0.1 * slot_size[t]):
                    c = 1
                mine.append(c)
            glob = self._allsum(mine)
            if glob[0] > 0:
                n = C.c_int64(numpart)
                sz = (C.c_int64 * 6)(*slot_size)
                compact = (C.c_int * 6)(*[int(glob[1 + t] > 0) for t in range(6)])
                capi.check(capi.hip.shq_slots_gc(h, C.byref(L), parts.data_ptr(), C.byref(n), maxpart, sp, sz, compact))
                numpart, slot_size = int(n.value), [int(x) for x in sz]
            self.ctx.synchronize()
            # second line (garbage that was there before this round may or may not have been collected): still collective
            if int(self._allsum([int(numpart + int(nrecv[0]) > maxpart)])[0]) > 0:
                raise MemoryError("DistExchange: %d + %d particles do not fit MaxPart %d on some rank" % (numpart, int(nrecv[0]), maxpart))
            # the alltoallv of the base records and of every slot type (:409-480): device buffers, over RCCL when the group is nccl
            rows, _ = comm.all_to_all_rows(partbuf[:int(nsend[0]) * esz].view(-1, esz), [int(x) for x in togo[:, 0]])
            parts[numpart * esz:(numpart + int(nrecv[0])) * esz] = rows.reshape(-1)
            for t in range(6):
                if slots[t] is None:
                    continue
                if int(self._allsum([int(slot_size[t] + int(nrecv[1 + t]) > cap[t])])[0]) > 0:
                    raise MemoryError("DistExchange: slot array of type %d is full on some rank" % t)
                rows, _ = comm.all_to_all_rows(slotbuf[t][:int(nsend[1 + t]) * ssz[t]].view(-1, ssz[t]), [int(x) for x in togo[:, 1 + t]])
                slots[t][slot_size[t] * ssz[t]:(slot_size[t] + int(nrecv[1 + t])) * ssz[t]] = rows.reshape(-1)
            torch.cuda.current_stream(dev).synchronize()
            so = (C.c_int64 * 6)(*slot_size)
            capi.check(capi.hip.shq_exchange_unpack(h, C.byref(L), parts.data_ptr(), numpart, so, self._entries(toget), self._entries(goff), ntask))
            numpart += int(nrecv[0])
            for t in range(6):
                if slots[t] is not None:
                    slot_size[t] += int(nrecv[1 + t])
            self.ctx.synchronize()
            if int(self._allsum([int(last.value < nex.value)])[0]) == 0:
                break
        return numpart, slot_size


# ---------------------------------------------------------------------------------------------------------------------
# Winds from new stars across ranks (libgadget/winds.cpp:295-369).  The reference exports every new star's query to the ranks whose
# top leaves its Hsml touches and merges the StarKick queues afterwards; here, as for the SPH operators, every rank imports the gas
# records within reach of its slab, runs the two walks for its own new stars on local + ghost gas, and sends the kick candidates
# that fell on ghosts to the ghosts' owners, who resolve all candidates of their own particles (nearest star, then smaller star
# ID: the same outcome whatever the decomposition) and kick.
class DistWinds:
    """P: numpy PARTICLE_DTYPE array of everything this rank owns (gas PI -> SphP, star PI -> StarP), IDs in P["ID"].
    ops.candidates(Pall, Sall, StarP, newstars, prm, rnd) -> (TotalWeight by star slot, kicks: numpy array of capi.WIND_KICK_DTYPE),
    ops.apply(P, SphP, kicks, prm, rnd) -> number kicked (GpuWindOps below; the CPU tests use the restatement)."""

    def __init__(self, comm, decomp, ops):
        self.comm, self.d, self.ops = comm, decomp, ops
        self.nghost = self.nkicks = 0

    def run(self, P, SphP, StarP, newstars, prm, rnd):
        comm = self.comm
        nloc = len(P)
        newstars = np.asarray(newstars, dtype=np.int32)
        reach = float(comm.gather_scalar(float(P["Hsml"][newstars].max()) if len(newstars) else 0.0).max())
        Pall, Sall, self.nghost = import_ghost_gas(comm, self.d, P, SphP, None, [reach] * comm.size)
        tw, kicks = self.ops.candidates(Pall, Sall, StarP, newstars, prm, rnd)
        # a candidate goes to the owner of its particle, with the particle's index there
        part = kicks["part_index"].astype(np.int64)
        ghost = part >= nloc
        owner = np.full(len(kicks), comm.rank, dtype=np.int64)
        owner[ghost] = Pall["TopLeaf"][part[ghost]]
        kicks = kicks.copy()
        kicks["part_index"][ghost] = Pall["GrNr"][part[ghost]]
        if comm.multi:
            order = np.argsort(owner, kind="stable")
            counts = np.bincount(owner, minlength=comm.size).tolist()
            rows = np.ascontiguousarray(kicks[order]).view(np.int64).reshape(len(kicks), -1)      # 40-byte records as five int64 words
            recv, _ = comm.all_to_all_rows(torch.from_numpy(rows), counts)
            kicks = np.ascontiguousarray(recv.numpy()).view(kicks.dtype).reshape(-1)
        self.nkicks = len(kicks)
        applied = self.ops.apply(P, SphP, kicks, prm, rnd)
        return tw, applied


class GpuWindOps:
    """DistWinds' two steps on the device library (shq_winds_candidates / shq_winds_apply) through the host mirror's tree builder."""

    def __init__(self, ctx, BoxSize):
        import shenqi_amd as sq
        self.sq, self.ctx, self.L = sq, ctx, BoxSize

    def _params(self, prm):
        p = capi.WindParams()
        for k, _ in capi.WindParams._fields_:
            if k != "pad_":
                setattr(p, k, getattr(prm, k))
        return p

    def candidates(self, Pall, Sall, StarP, newstars, prm, rnd):
        sq = self.sq
        pman = records_pman(sq, self.L, Pall)
        tree = sq.force_tree_rebuild_mask(pman, sq.GASMASK)
        ids = np.ascontiguousarray(Pall["ID"])
        new = np.ascontiguousarray(newstars, dtype=np.int32)
        rnd = np.ascontiguousarray(rnd, dtype=np.float64)
        tw = np.zeros(len(StarP))
        pv, tv, sv = pman.view(), tree.view(), capi.sph_view(Sall)
        stv = capi.StarView(StarP.ctypes.data, StarP.dtype.itemsize, len(StarP), StarP.dtype.fields["VDisp"][1])
        cp = self._params(prm)
        nk = C.c_int64()

        def call(kicks, cap):
            return capi.hip.shq_winds_candidates(self.ctx.h, C.byref(tv), C.byref(pv), C.byref(sv), C.byref(stv), capi.ptr(ids), capi.ptr(new), len(new), C.byref(cp),
                                                 capi.ptr(rnd), len(rnd), capi.ptr(tw), kicks, cap, C.byref(nk))
        return tw, sized_call(call, nk, capi.WIND_KICK_DTYPE)

    def apply(self, P, SphP, kicks, prm, rnd):
        pman = records_pman(self.sq, self.L, P)
        ids = np.ascontiguousarray(P["ID"])
        rnd = np.ascontiguousarray(rnd, dtype=np.float64)
        kicks = np.ascontiguousarray(kicks, dtype=capi.WIND_KICK_DTYPE)
        pv, sv = pman.view(), capi.sph_view(SphP)
        cp = self._params(prm)
        na = C.c_int64()
        capi.check(capi.hip.shq_winds_apply(self.ctx.h, C.byref(pv), C.byref(sv), capi.ptr(ids), capi.ptr(kicks), len(kicks), C.byref(cp), capi.ptr(rnd), len(rnd),
                                            C.byref(na)))
        P["Vel"] = pman.Base["Vel"]
        return na.value


# Metal return across ranks (libgadget/metal_return.cpp:464-530, stellar_density2.cpp:306-341).  The reference exports every dying
# star's query to the ranks its kernel touches and updates the gas there under a spin lock, in thread-arrival order.  Here every rank
# imports the gas records within reach of its slab (as DistWinds does), walks its own stars over local + ghost gas, and the walk only
# emits (gas particle, star, kernel weight) triples: those that fell on ghosts travel to the ghosts' owners, every owner applies the
# triples of a particle in the order of the GLOBAL queue (the ranks' queues one after the other), and the mass each triple moved
# travels back to the star's rank.  The gas ends as in the undivided run with that queue, whatever the decomposition.
class DistMetalReturn:
    """P: numpy PARTICLE_DTYPE array of everything this rank owns (gas PI -> SphP, star PI -> the star slots), queue: rows of P, the
    dying stars of the step in the order shq_metal_yields returned them.

    A step's metal return is, per rank: shq_metal_yields (per star, local: ages, yields, the queue) -> stellar_density() below ->
    run() below -> shq_metal_return_postprocess (per star, local: Mass -= MassReturn, TotalMassReturned, LastEnrichmentMyr).  The two
    per-star calls need nothing from other ranks and stay outside this class.

    ops.stellar_density(Pall, Sall, queue, params) -> (StarVolumeSPH by queue position, largest radius tried or None), Hsml of the
        queue's stars updated in Pall;
    ops.triples(Pall, nlocal, queue, ghost_owner, ghost_index, nranks, rank, queue_offset, SPHWeighting, kt) -> (triples: numpy array
        of capi.METAL_TRIPLE_DTYPE sorted by (owner, part_index, star), counts per owner);
    ops.apply(P, SphP, triples, star_table, MaxGasMass) -> thismass per triple, the gas of P / SphP updated;
    ops.sums(qpos, owner, part_index, thismass, nqueue) -> MassReturn by queue position
    (GpuMetalOps below; the CPU tests use restatements).  Nothing here has run on more than one GPU."""

    def __init__(self, comm, decomp, ops, hfac=1.3):
        self.comm, self.d, self.ops, self.hfac = comm, decomp, ops, hfac
        self.nghost = self.ntriples_sent = self.nrounds = 0

    def stellar_density(self, P, SphP, queue, params):
        """stellar_density() for the stars of `queue`: the Hsml loop for star targets over local + ghost gas, by widen_until_covered
        from the largest Hsml of the rank's queue.  Writes P["Hsml"] of the stars; returns (StarVolumeSPH by queue position, number of
        import rounds)."""
        queue = np.ascontiguousarray(queue, dtype=np.int32)
        nq = len(queue)
        h0 = P["Hsml"][queue].copy()
        Pall = vol = None

        def attempt(halos):
            nonlocal Pall, vol
            Pall, Sall, self.nghost = import_ghost_gas(self.comm, self.d, P, SphP, None, halos)
            Pall["Hsml"][queue] = h0
            vol, tried = self.ops.stellar_density(Pall, Sall, queue, params)
            return max(float(Pall["Hsml"][queue].max()), float(tried or 0.0)) if nq else 0.0
        self.nrounds = widen_until_covered(self.comm, self.hfac, float(h0.max()) if nq else 0.0, attempt)
        P["Hsml"][queue] = Pall["Hsml"][queue]
        return np.asarray(vol, dtype=np.float64), self.nrounds

    def run(self, P, SphP, queue, StarVolumeSPH, MassGenerated, MetalGenerated, MetalSpeciesGenerated, MaxGasMass, SPHWeighting, kt):
        """metal_return()'s treewalk for the stars of `queue` (per-star arrays by queue position).  Updates Mass of P and Density,
        Metallicity, Metals of SphP for the gas this rank owns; returns MassReturn by local queue position."""
        comm = self.comm
        nloc, size = len(P), comm.size
        queue = np.ascontiguousarray(queue, dtype=np.int32)
        nq = len(queue)
        nqs = [int(x) for x in comm.gather_scalar(nq, np.int64)]
        off, total = sum(nqs[:comm.rank]), sum(nqs)
        self.nghost = self.ntriples_sent = 0
        if total == 0:          # "if(nqueue_total == 0) return", metal_return.cpp:500-503
            return np.zeros(0)
        # The star table of the global queue on every rank: dying stars per step are few next to the gas.  Should that ever not hold,
        # this is the place to send a star's row only to the ranks its triples go to.
        rows = np.zeros((nq, capi.METAL_STAR_NCOL))
        if nq:
            rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3:] = StarVolumeSPH, MassGenerated, MetalGenerated, np.reshape(MetalSpeciesGenerated, (nq, -1))
        table, _ = comm.all_to_all_rows(torch.from_numpy(np.tile(rows, (size, 1))), [nq] * size)
        table = np.ascontiguousarray(table.numpy())
        reach = float(comm.gather_scalar(float(P["Hsml"][queue].max()) if nq else 0.0).max())
        Pall, _, self.nghost = import_ghost_gas(comm, self.d, P, None, None, [reach] * size)
        trip, counts = self.ops.triples(Pall, nloc, queue, np.ascontiguousarray(Pall["TopLeaf"][nloc:], dtype=np.int32),
                                        np.ascontiguousarray(Pall["GrNr"][nloc:], dtype=np.int32), size, comm.rank, off, SPHWeighting, kt)
        self.ntriples_sent = len(trip) - int(counts[comm.rank])
        # 24-byte records as three int64 words, to the owners; thismass comes back along the same counts: the order within a
        # (source, destination) pair is kept, so no key travels back
        words = torch.from_numpy(np.ascontiguousarray(trip).view(np.int64).reshape(len(trip), 3))
        recv, rcounts = comm.all_to_all_rows(words, [int(c) for c in counts])
        mine = np.ascontiguousarray(recv.numpy()).view(capi.METAL_TRIPLE_DTYPE).reshape(-1)
        tm = np.ascontiguousarray(self.ops.apply(P, SphP, mine, table, MaxGasMass), dtype=np.float64)
        back, _ = comm.all_to_all_rows(torch.from_numpy(tm.reshape(-1, 1)), rcounts)
        back = np.ascontiguousarray(back.numpy()).reshape(-1)
        return self.ops.sums((trip["star"].astype(np.int64) - off).astype(np.int32), trip["owner"], trip["part_index"], back, nq)


class GpuMetalOps:
    """DistMetalReturn's steps on the device library (shq_stellar_density, shq_metal_return_triples / _apply / _sums) through the host
    mirror's tree builder."""

    def __init__(self, ctx, BoxSize):
        import shenqi_amd as sq
        self.sq, self.ctx, self.L = sq, ctx, BoxSize

    def stellar_density(self, Pall, Sall, queue, params):
        sq = self.sq
        pman = records_pman(sq, self.L, Pall)
        tree = sq.force_tree_rebuild_mask(pman, sq.GASMASK)
        queue = np.ascontiguousarray(queue, dtype=np.int32)
        sp = capi.StellarParams(self.L, params.DesNumNgb, params.MaxNgbDeviation, params.SPHWeighting, params.DensityKernelType)
        slots = Pall["PI"][queue]
        vol = np.zeros(int(slots.max()) + 1 if len(queue) else 1)
        st = capi.SphStats()
        pv, tv, sv = pman.view(), tree.view(), capi.sph_view(Sall)
        capi.check(capi.hip.shq_stellar_density(self.ctx.h, C.byref(tv), C.byref(pv), C.byref(sv), capi.ptr(queue), len(queue), C.byref(sp), capi.ptr(vol), C.byref(st)))
        Pall["Hsml"] = pman.Base["Hsml"]
        return vol[slots], float(st.hsml_max_tried)

    def triples(self, Pall, nlocal, queue, ghost_owner, ghost_index, nranks, rank, queue_offset, SPHWeighting, kt):
        sq = self.sq
        pman = records_pman(sq, self.L, Pall)
        tree = sq.force_tree_rebuild_mask(pman, sq.GASMASK)
        queue = np.ascontiguousarray(queue, dtype=np.int32)
        pv, tv = pman.view(), tree.view()
        counts = np.zeros(nranks, dtype=np.int64)
        nt = C.c_int64()

        def call(trip, cap):
            return capi.hip.shq_metal_return_triples(self.ctx.h, C.byref(tv), C.byref(pv), capi.ptr(queue), len(queue), SPHWeighting, kt, nlocal, capi.ptr(ghost_owner),
                                                     capi.ptr(ghost_index), nranks, rank, queue_offset, trip, cap, capi.ptr(counts), C.byref(nt))
        return sized_call(call, nt, capi.METAL_TRIPLE_DTYPE), counts

    def apply(self, P, SphP, triples, star_table, MaxGasMass):
        pman = records_pman(self.sq, self.L, P)
        triples = np.ascontiguousarray(triples, dtype=capi.METAL_TRIPLE_DTYPE)
        star_table = np.ascontiguousarray(star_table, dtype=np.float64)
        f = SphP.dtype.fields
        gv = capi.GasMetalView(SphP.ctypes.data, SphP.dtype.itemsize, len(SphP), f["Density"][1], f["Metallicity"][1], f["Metals"][1], 9, 0)
        pv = pman.view()
        tm = np.zeros(max(len(triples), 1))
        capi.check(capi.hip.shq_metal_return_apply(self.ctx.h, C.byref(pv), C.byref(gv), capi.ptr(triples), len(triples), capi.ptr(star_table), len(star_table),
                                                   MaxGasMass, capi.ptr(tm)))
        P["Mass"] = pman.Base["Mass"]
        return tm[:len(triples)]

    def sums(self, qpos, owner, part_index, thismass, nqueue):
        a = [np.ascontiguousarray(x, dtype=np.int32) for x in (qpos, owner, part_index)]
        thismass = np.ascontiguousarray(thismass, dtype=np.float64)
        out = np.zeros(max(nqueue, 1))
        capi.check(capi.hip.shq_metal_return_sums(self.ctx.h, capi.ptr(a[0]), capi.ptr(a[1]), capi.ptr(a[2]), capi.ptr(thismass), len(thismass), nqueue, capi.ptr(out)))
        return out[:nqueue]


# Black-hole accretion and feedback across ranks (libgadget/blackhole.cpp:217-370).  Both walks write on the neighbours' side: merger
# and swallow marks, flags, the entropy with its cap, kicks.  The reference exports a hole's query to the ranks its kernel touches
# and does those writes there with atomics, in thread-arrival order.  Here, as for the metal return, every rank imports the gas and the
# holes within reach of its slab, walks its own queued holes over local + ghost particles, and a walk only emits records of what it
# would have written: they travel to the particle's owner, who applies a particle's records in the order of the GLOBAL queue (the ranks'
# queues one after the other).  Between the two walks the ghosts are refreshed from their owners: the resolved marks, and the holes'
# slots, whose Mass grew in the owner's accretion postprocess.
BH_WORK = (("SPH_SwallowID", np.uint64, 0, ()), ("BH_SwallowID", np.uint64, 1, ()), ("BH_FeedbackWeightSum", np.float64, 1, ()), ("BH_Entropy", np.float64, 1, ()),
           ("BH_SurroundingGasVel", np.float64, 1, (3,)), ("MgasEnc", np.float64, 1, ()), ("KEflag", np.int32, 1, ()), ("BH_accreted_Mass", np.float64, 1, ()),
           ("BH_accreted_BHMass", np.float64, 1, ()), ("BH_accreted_momentum", np.float64, 1, (3,)))


def bh_work_arrays(nsph, nbh):
    """struct BHPriv's arrays (shq_bh_work) by slot index, zeroed: SPH_SwallowID over the gas slots, the rest over the hole slots"""
    return {k: np.zeros((max(nbh if by_bh else nsph, 1),) + shape, dtype=t) for k, t, by_bh, shape in BH_WORK}


class DistBlackHole:
    """P: numpy PARTICLE_DTYPE array of everything this rank owns (gas PI -> SphP, hole PI -> BhP), IDs in P["ID"]; queue: rows of P, the
    active live holes.  kf: the kick factors, prm: the shq_bh_params fields as attributes, eeqos: one byte per row of P or None.

    ops.accretion_marks(Pall, Sall, Ball, nlocal, queue, ghost_owner, ghost_index, nranks, rank, queue_offset, kf, prm, Ti_Current, rnd,
        work) -> (marks: capi.BH_MARK_DTYPE sorted by (owner, part_index, hole), counts per owner); the slots of Ball and the hole-side
        arrays of work updated for the queue's holes;
    ops.marks_resolve(P, marks, Ti_Current, nsph, nbh, work): SPH_SwallowID[:nsph] and BH_SwallowID[:nbh] of work zeroed and set;
    ops.feedback_effects(Pall, Sall, Ball, nlocal, queue, ghost_owner, ghost_index, nranks, rank, queue_offset, kf, prm, rnd, work)
        -> (effects: capi.BH_EFFECT_DTYPE, counts per owner); Vel and Mass of Pall, Ball and work updated for the queue's holes;
    ops.effects_apply(P, SphP, BhP, effects, prm, MaxPart, rnd, eeqos, work) -> (gas swallowed, holes swallowed)
    (GpuBhOps below; the CPU tests use the restatement).  After run(): nghost, marks_sent[kind], effects_sent[kind] (records that left
    this rank), n_sph_swallowed, n_bh_swallowed, and work: the BHPriv arrays of the rank's own slots.
    Nothing here has run on more than one GPU."""

    def __init__(self, comm, decomp, ops):
        self.comm, self.d, self.ops = comm, decomp, ops
        self._reset(0, 0)

    def _reset(self, nsph, nbh):
        self.nghost = self.n_sph_swallowed = self.n_bh_swallowed = 0
        self.marks_sent, self.effects_sent = [0, 0], [0, 0, 0, 0]
        self.work = bh_work_arrays(nsph, nbh)

    def _to_owners(self, rec, counts, sent):
        """24-byte records as three int64 words to their owners; counts those that leave, by kind, into `sent`"""
        away = rec["kind"][rec["owner"] != self.comm.rank]
        sent[:] = np.bincount(away, minlength=len(sent)).tolist()
        words = torch.from_numpy(np.ascontiguousarray(rec).view(np.int64).reshape(len(rec), 3))
        recv, _ = self.comm.all_to_all_rows(words, [int(c) for c in counts])
        return np.ascontiguousarray(recv.numpy()).view(rec.dtype).reshape(-1)

    def run(self, P, SphP, BhP, queue, kf, prm, Ti_Current, MaxPart, rnd, eeqos):
        """blackhole()'s two treewalks for the holes of `queue`.  Updates P, SphP and BhP for what this rank owns; returns
        (gas swallowed, holes swallowed) among its own particles."""
        comm, ops = self.comm, self.ops
        nloc, ns, nb, size = len(P), len(SphP), len(BhP), comm.size
        queue = np.ascontiguousarray(queue, dtype=np.int32)
        nq = len(queue)
        nqs = [int(x) for x in comm.gather_scalar(nq, np.int64)]
        off, total = sum(nqs[:comm.rank]), sum(nqs)
        self._reset(ns, nb)
        if total == 0:
            return 0, 0
        reach = comm.gather_scalar(float(P["Hsml"][queue].max()) if nq else 0.0)
        Pall, Sall, Ball, self.nghost = import_ghost_gas_bh(comm, self.d, P, SphP, BhP, reach)
        work = bh_work_arrays(len(Sall), len(Ball))
        own = {k: v[:(nb if by_bh else ns)] for (k, _, by_bh, _), v in zip(BH_WORK, work.values())}     # views of the rank's own slots
        gown = np.ascontiguousarray(Pall["TopLeaf"][nloc:], dtype=np.int32)
        gidx = np.ascontiguousarray(Pall["GrNr"][nloc:], dtype=np.int32)
        marks, counts = ops.accretion_marks(Pall, Sall, Ball, nloc, queue, gown, gidx, size, comm.rank, off, kf, prm, Ti_Current, rnd, work)
        BhP[:] = Ball[:nb]
        ops.marks_resolve(P, self._to_owners(marks, counts, self.marks_sent), Ti_Current, ns, nb, work)
        # The ghosts as their owners have them now: the resolved marks, and the holes' slots - an active hole's Mass grew by Mdot dtime
        # in its owner's postprocess, and the feedback walk adds that Mass to its swallower
        ggas = Pall["Type"][nloc:] == 0
        pi = P["PI"].astype(np.int64)
        u8 = lambda a: np.ascontiguousarray(a).view(np.uint8).reshape(len(a), a.dtype.itemsize)      # noqa: E731
        work["SPH_SwallowID"][ns:ns + int(ggas.sum())] = fetch_from_owners(
            comm, gown[ggas], gidx[ggas], lambda ask: u8(own["SPH_SwallowID"][pi[ask]])).view(np.uint64).reshape(-1)
        got = fetch_from_owners(comm, gown[~ggas], gidx[~ggas], lambda ask: np.concatenate([u8(BhP[pi[ask]]), u8(own["BH_SwallowID"][pi[ask]])], axis=1))
        nbg, bsz = int((~ggas).sum()), BhP.dtype.itemsize
        Ball[nb:] = np.ascontiguousarray(got[:, :bsz]).view(BhP.dtype).reshape(nbg)
        work["BH_SwallowID"][nb:nb + nbg] = np.ascontiguousarray(got[:, bsz:]).view(np.uint64).reshape(-1)
        effects, counts = ops.feedback_effects(Pall, Sall, Ball, nloc, queue, gown, gidx, size, comm.rank, off, kf, prm, rnd, work)
        BhP[:] = Ball[:nb]
        P["Vel"][queue], P["Mass"][queue] = Pall["Vel"][queue], Pall["Mass"][queue]
        res = ops.effects_apply(P, SphP, BhP, self._to_owners(effects, counts, self.effects_sent), prm, MaxPart, rnd, eeqos, own)
        self.n_sph_swallowed, self.n_bh_swallowed = int(res[0]), int(res[1])
        self.work = {k: v.copy() for k, v in own.items()}
        return self.n_sph_swallowed, self.n_bh_swallowed


class GpuBhOps:
    """DistBlackHole's four steps on the device library (shq_bh_accretion_marks / _marks_resolve / _feedback_effects / _effects_apply)
    through the host mirror's tree builder (gas + holes, moments with hmax)."""

    def __init__(self, ctx, BoxSize):
        import shenqi_amd as sq
        self.sq, self.ctx, self.L = sq, ctx, BoxSize
        self._walkset, self._room = None, {}

    @staticmethod
    def _params(prm):
        p = capi.BhParams()
        for k, _ in capi.BhParams._fields_:
            setattr(p, k, getattr(prm, k))
        return p

    @staticmethod
    def _work(work):
        return capi.BhWork(*[work[k].ctypes.data for k, _ in capi.BhWork._fields_])

    def _tree(self, Pall):
        """the particle manager and tree of the walks; the feedback walk takes the accretion walk's (same records, nothing moved)"""
        sq = self.sq
        if self._walkset is not None and self._walkset[0] is Pall:
            pman, tree = self._walkset[1:]
            pman.Base[:] = Pall
            return pman, tree
        pman = records_pman(sq, self.L, Pall)
        tree = sq.force_tree_rebuild_mask(pman, sq.GASMASK + sq.BHMASK)
        sq.force_tree_update_hmax(tree, pman)
        self._walkset = (Pall, pman, tree)
        return pman, tree

    def _walk(self, fn, Pall, Sall, Ball, nlocal, queue, gown, gidx, nranks, rank, off, kf, prm, rnd, work, dtype, Ti=None):
        pman, tree = self._tree(Pall)
        ids = np.ascontiguousarray(Pall["ID"])
        queue = np.ascontiguousarray(queue, dtype=np.int32)
        rnd = np.ascontiguousarray(rnd, dtype=np.float64)
        pv, tv, sv, bv = pman.view(), tree.view(), capi.sph_view(Sall), capi.bh_slot_view(Ball)
        cp, cw = self._params(prm), self._work(work)
        counts = np.zeros(nranks, dtype=np.int64)
        nr = C.c_int64()
        mid = (C.byref(cp),) + (() if Ti is None else (Ti,))

        def call(rec, cap):
            return fn(self.ctx.h, C.byref(tv), C.byref(pv), C.byref(sv), C.byref(bv), capi.ptr(ids), capi.ptr(queue), len(queue), C.byref(kf), *mid,
                      capi.ptr(rnd), len(rnd), C.byref(cw), nlocal, capi.ptr(gown), capi.ptr(gidx), nranks, rank, off, rec, cap, capi.ptr(counts), C.byref(nr))
        # The count pass walks as long as the emit pass, and a sized call runs it twice (without a buffer, then before it emits).  From
        # the second step on the last step's count, with a margin, is offered as the capacity: one count pass where it suffices.
        room, rec = self._room.get(dtype, 0), None
        if room:
            buf = np.zeros(room, dtype=dtype)
            rc = call(capi.ptr(buf), room)
            if rc == 0:
                rec = buf[:nr.value]
            elif not (rc == capi.ERR_INVALID and nr.value > room):      # anything but "room for fewer records than found"
                capi.check(rc)
        if rec is None:
            rec = sized_call(call, nr, dtype)
        self._room[dtype] = len(rec) + len(rec) // 4 + 64
        return pman, rec, counts

    def accretion_marks(self, Pall, Sall, Ball, nlocal, queue, gown, gidx, nranks, rank, off, kf, prm, Ti_Current, rnd, work):
        self._walkset = None
        _, marks, counts = self._walk(capi.hip.shq_bh_accretion_marks, Pall, Sall, Ball, nlocal, queue, gown, gidx, nranks, rank, off, kf, prm, rnd, work,
                                      capi.BH_MARK_DTYPE, Ti_Current)
        return marks, counts

    def marks_resolve(self, P, marks, Ti_Current, nsph, nbh, work):
        pman = records_pman(self.sq, self.L, P)
        ids = np.ascontiguousarray(P["ID"])
        marks = np.ascontiguousarray(marks, dtype=capi.BH_MARK_DTYPE)
        pv, cw = pman.view(), self._work(work)
        capi.check(capi.hip.shq_bh_marks_resolve(self.ctx.h, C.byref(pv), capi.ptr(ids), capi.ptr(marks), len(marks), Ti_Current, nsph, nbh, C.byref(cw)))

    def feedback_effects(self, Pall, Sall, Ball, nlocal, queue, gown, gidx, nranks, rank, off, kf, prm, rnd, work):
        pman, effects, counts = self._walk(capi.hip.shq_bh_feedback_effects, Pall, Sall, Ball, nlocal, queue, gown, gidx, nranks, rank, off, kf, prm, rnd, work,
                                           capi.BH_EFFECT_DTYPE)
        Pall["Vel"], Pall["Mass"] = pman.Base["Vel"], pman.Base["Mass"]
        self._walkset = None
        return effects, counts

    def effects_apply(self, P, SphP, BhP, effects, prm, MaxPart, rnd, eeqos, work):
        pman = records_pman(self.sq, self.L, P)
        ids = np.ascontiguousarray(P["ID"])
        rnd = np.ascontiguousarray(rnd, dtype=np.float64)
        effects = np.ascontiguousarray(effects, dtype=capi.BH_EFFECT_DTYPE)
        eeqos = None if eeqos is None else np.ascontiguousarray(eeqos, dtype=np.uint8)
        pv, sv, bv, cp, cw = pman.view(), capi.sph_view(SphP), capi.bh_slot_view(BhP), self._params(prm), self._work(work)
        ns, nb = C.c_int64(), C.c_int64()
        capi.check(capi.hip.shq_bh_effects_apply(self.ctx.h, C.byref(pv), C.byref(sv), C.byref(bv), capi.ptr(ids), capi.ptr(effects), len(effects), C.byref(cp), MaxPart,
                                                 capi.ptr(rnd), len(rnd), None if eeqos is None else capi.ptr(eeqos), C.byref(cw), C.byref(ns), C.byref(nb)))
        P["Vel"], P["Flags"] = pman.Base["Vel"], pman.Base["Flags"]
        return ns.value, nb.value


class _DeviceOps:
    """What the device ops of the slab mesh drivers share (GpuUvbgOps, GpuZeldovichOps, GpuGlassOps): the library context, torch's
    device, and a library call on torch tensors between the two stream hand-overs."""

    def __init__(self, ctx, device=None):
        self.ctx = ctx
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
        self._hand = _StreamHandover(ctx, self.device)

    def _call(self, fn, *args):
        self._hand.before()
        capi.check(fn(self.ctx.h, *args), fn.__name__)
        self._hand.after()

    @staticmethod
    def _p(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    def full(self, shape, value, dtype):
        return torch.full(shape, value, dtype=dtype, device=self.device)

    def to_real(self, mesh_i, exp):
        """the fixed-point deposit of scale 2^(61 - exp) as doubles (the torch.fft route; the bespoke Y/Z forward converts itself)"""
        return mesh_i.to(torch.float64) * math.ldexp(1.0, exp - 61)


def uvbg_radii(p):
    """petapm_reion_c2r's radius schedule (petapm.cpp:536-606) from the parameters alone: the same list on every rank, the last
    entry the unfiltered cell-size step"""
    cell = p.BoxSize / p.UVBGdim
    R = min(p.ReionRBubbleMax, p.BoxSize)
    radii, last, count = [], False, 0
    while not last:
        count += 1
        if R / p.ReionDeltaRFactor < p.ReionRBubbleMin or R / p.ReionDeltaRFactor < cell or count > 10000:
            last, R = True, cell
        radii.append(R)
        R = R / p.ReionDeltaRFactor
    return radii


class DistUVBG(SlabMesh):
    """calculate_uvbg + petapm_reion (uvbg.cpp:474-597, petapm.cpp:495-685) on x-slabs of the UVBGdim mesh, one per rank: whole
    planes, equal widths unless `bounds` says otherwise (the PM's slabs live on another mesh and may be cut below a plane: they are
    not reused).  UVBGdim must be divisible by the rank count (equal y-slabs of the spectrum): otherwise the constructor raises
    ValueError on every rank, before any collective.

    The grids come from a fixed-point deposit whose three scales every rank derives from the global sums, the filter tables are made
    on every host alike and the cell loop is local, so the J21 / xHI grids and the particles' results do not depend on the rank
    count or on who held which particle.  ops (GpuUvbgOps below; the CPU tests use a numpy stand-in) works on torch tensors:
      ops.fesc(p, cosmo, posm, types, fesc, sfr) -> ([|Mass|, |Mass f_esc|, |Sfr f_esc|] of the rows, negative flag), fesc in place;
      ops.deposit(p, posm, types, fesc, sfr, exps, plane0, nxl, nalloc) -> the 2 (3) int64 meshes [nalloc, N, pitch];
      ops.tables(p, radii); ops.cells(p, cosmo, R, last, meshes, zp, nxl, J21, xHI) -> the three partial sums on the last radius;
      ops.readout(p, cosmo, posm, types, J21ext, plane0, nxl, local_J21, zreion);
      bespoke route (ops.pitch() > 0): ops.fft_yz(planes, nxl, direction, exp, packed, P), ops.xforward(spec, y0, nyl),
      ops.xfilter(spec, out, y0, nyl, r);   torch.fft route: ops.to_real(mesh_i, exp), ops.filter(spec, y0, nyl, r) in place.
    Counters of the last call: rows_sent (particle rows that left this rank), nradii, nalltoall (all-to-alls and shifts started).
    J21 / xHI hold the rank's planes of the grids afterwards (save_uvbg_grids' data).  Nothing here has run on more than one GPU."""

    COLS = 9     # x, y, z, Mass, Type, f_esc, Sfr, local_J21, zreion: one float64 row per particle (Type and float Mass are exact)

    def __init__(self, comm, UVBGdim, BoxSize, ops, bounds=None):
        super().__init__(comm, int(UVBGdim), float(BoxSize), ops, bounds)
        self.nradii = 0
        self.J21 = self.xHI = None

    def calculate(self, p, cosmo, pos, mass, types, fesc, sfr, local_J21, zreion):
        """p: capi.UvbgParams, cosmo: capi.UvbgCosmo; pos [n, 3], mass, types, fesc (in / out), sfr (may be None without
        ReionUseParticleSFR), local_J21 (out, gas) and zreion (in / out, gas): numpy arrays of the particles this rank holds, in any
        distribution over the ranks.  They are written only at the very end, in the caller's order.  Returns (volume-weighted xHI,
        mass-weighted xHI, number of radii), the same on every rank.  A negative escape fraction on any rank raises ValueError on
        every rank, the arrays untouched."""
        c, d, ops, N = self.comm, self.d, self.ops, self.N
        if p.UVBGdim != N or p.BoxSize != self.L:
            raise ValueError("the parameters' UVBGdim / BoxSize are not this decomposition's")
        use_sfr = bool(p.ReionUseParticleSFR)
        self.rows_sent = self.nalltoall = 0
        n = len(pos)
        rows = np.empty((n, self.COLS))
        rows[:, 0:3], rows[:, 3], rows[:, 4], rows[:, 5] = pos, mass, types, fesc
        rows[:, 6] = sfr if sfr is not None else 0.0
        rows[:, 7], rows[:, 8] = local_J21, zreion
        rows = torch.from_numpy(rows).to(ops.device)
        # ---- to the owner of the particle's UVBG plane; rows already at home stay in the self block
        mine, route = self.to_owners(rows, d.owner_of(rows[:, 0]))
        posm = mine[:, 0:4].contiguous()
        ty = mine[:, 4].to(torch.uint8).contiguous()
        col = [mine[:, k].contiguous() for k in range(5, 9)]
        f_esc, s_fr, lj, zr = col
        # ---- init_particle_uvbg; the three sums and the negative flag agreed on in ONE vector before anything else: a rank that
        # raised alone would leave the others inside an all-to-all
        sums, neg = ops.fesc(p, cosmo, posm, ty, f_esc, s_fr)
        tot = c.allreduce_sum_vec(np.array([sums[0], sums[1], sums[2], 1.0 if neg else 0.0]))
        if tot[3] > 0:
            raise ValueError("negative escape fraction?")
        if not np.isfinite(tot[:3]).all():
            raise ValueError("uvbg: non-finite mass, f_esc or Sfr")
        exps = [math.frexp(s if s > 0 else 1.0)[1] for s in tot[:3]]
        radii = uvbg_radii(p)
        self.nradii = len(radii)
        ops.tables(p, radii)
        P, nxl = c.size, d.nxl
        nalloc = N if P == 1 else nxl + 1
        bufs = ops.deposit(p, posm, ty, f_esc, s_fr, exps, d.plane0, nxl, nalloc)     # int64 [nalloc, N, pitch] per field
        nf = 3 if use_sfr else 2
        assert len(bufs) == nf
        self.add_ghosts(bufs, nxl)
        self._J21ext = ops.full((nalloc, N, N), 0.0, torch.float32)     # the own planes, then room for the right neighbour's first
        self.J21 = self._J21ext[:nxl]
        self.xHI = ops.full((nxl, N, N), 1.0, torch.float32)
        part = (self._loop_bespoke if self.bespoke(ops.pitch()) else self._loop_torch)(p, cosmo, bufs, exps, radii)
        # ---- UVBGgrids' globals (uvbg.cpp:446-451) and readout_J21 with the right neighbour's first plane behind the own ones
        tot = c.allreduce_sum_vec(np.asarray(part, dtype=np.float64))
        vol, mw = tot[0] / float(N ** 3), tot[1] / tot[2]
        self.neighbour_plane(self._J21ext, nxl)
        ops.readout(p, cosmo, posm, ty, self._J21ext, d.plane0, nxl, lj, zr)
        res = self.back(route, torch.stack([f_esc, lj, zr], dim=1))
        fesc[:], local_J21[:], zreion[:] = res[:, 0], res[:, 1], res[:, 2]
        return float(vol), float(mw), len(radii)

    def _loop_bespoke(self, p, cosmo, bufs, exps, radii):
        """The library's own FFT passes (csrc/fft3d.hip): a field's buffer [nalloc][N][zp] is in turn its int64 deposit, its (y, z)
        half spectrum and its real mesh of a radius.  Per field: Y/Z forward packed, all-to-all, X forward - the spectrum stays on
        the y-slab.  Per radius and field: the filter pass out of place, ONE all-to-all back, Y/Z inverse; then the cell loop."""
        c, ops, N, P, nxl = self.comm, self.ops, self.N, self.comm.size, self.d.nxl
        zp = ops.pitch()
        nyl, y0 = N // P, c.rank * (N // P)
        own = [b[:nxl] for b in bufs]
        pend = [self.forward_bespoke(o, lambda packed, f=f, o=o: ops.fft_yz(o, nxl, 0, exps[f], packed, P)) for f, o in enumerate(own)]
        kept = []
        for pe in pend:
            spec_t = pe.wait().contiguous()
            if not c.multi:       # a lone process: the planes are the y-slab, and every radius writes them again
                spec_t = spec_t.clone()
            ops.xforward(spec_t, y0, nyl)
            kept.append(spec_t)
        real = [b.view(torch.float64) for b in bufs]
        part = None
        for r, R in enumerate(radii):
            # every field's exchange in flight at once, each from a buffer of its own: the cell loop needs them all
            for _ in self.back_bespoke(own, kept[0], lambda f, out: ops.xfilter(kept[f], out, y0, nyl, r),
                                       lambda f, packed: ops.fft_yz(own[f], nxl, 1, 0, packed, P), inflight=len(own)):
                pass
            part = ops.cells(p, cosmo, R, r == len(radii) - 1, real, zp, nxl, self.J21, self.xHI)
        return part

    def _loop_torch(self, p, cosmo, bufs, exps, radii):
        """The same loop with torch.fft for mesh sizes without a bespoke transform, and on the CPU stand-ins: the spectrum is kept as
        [x][y_l][z'], x slowest, as the all-to-all delivers it."""
        c, ops, N, P, nxl = self.comm, self.ops, self.N, self.comm.size, self.d.nxl
        nyl, y0 = N // P, c.rank * (N // P)
        kept = [self.forward_torch(ops.to_real(b[:nxl, :, :N], exps[f])) for f, b in enumerate(bufs)]
        part = None
        for r, R in enumerate(radii):
            real = [self.back_torch(ops.filter(spec_t.clone(), y0, nyl, r)).contiguous() for spec_t in kept]     # [nxl, N, N] each
            part = ops.cells(p, cosmo, R, r == len(radii) - 1, real, N, nxl, self.J21, self.xHI)
        return part


class GpuUvbgOps(_DeviceOps):
    """DistUVBG's phases on the device library (shq_uvbg_slab_*), on torch tensors of the context's device."""

    def __init__(self, ctx, device=None):
        super().__init__(ctx, device)
        self.N = None

    def pitch(self):
        return int(capi.hip.shq_uvbg_slab_pitch(self.N))

    def fesc(self, p, cosmo, posm, types, fesc, sfr):
        self.N = int(p.UVBGdim)
        sums, neg = (C.c_double * 3)(), C.c_int(0)
        self._call(capi.hip.shq_uvbg_slab_fesc, C.byref(p), C.byref(cosmo), self._p(posm), self._p(types), posm.shape[0], self._p(fesc), self._p(sfr),
                   C.byref(sums), C.byref(neg))
        return list(sums), bool(neg.value)

    def tables(self, p, radii):
        r = np.ascontiguousarray(radii, dtype=np.float64)
        self.N = int(p.UVBGdim)
        self._call(capi.hip.shq_uvbg_slab_tables, int(p.ReionFilterType), int(p.UVBGdim), float(p.BoxSize), capi.ptr(r), len(r))

    def deposit(self, p, posm, types, fesc, sfr, exps, plane0, nxl, nalloc):
        N = int(p.UVBGdim)
        zp = self.pitch() or N + 2
        nf = 3 if p.ReionUseParticleSFR else 2
        bufs = [torch.empty((nalloc, N, zp), dtype=torch.int64, device=self.device) for _ in range(nf)]
        self._call(capi.hip.shq_uvbg_slab_deposit, C.byref(p), self._p(posm), self._p(types), posm.shape[0], self._p(fesc), self._p(sfr),
                   C.byref((C.c_int * 3)(*exps)), plane0, nxl, 0, nalloc, 1, *[self._p(b) for b in bufs], *([None] * (3 - nf)))
        return bufs

    def fft_yz(self, planes, nplanes, direction, exp, packed, nranks):
        assert planes.is_contiguous() and (packed is None or (packed.is_contiguous() and packed.dtype == torch.complex128))
        self._call(capi.hip.shq_uvbg_slab_fft_yz, self.N, self._p(planes), nplanes, direction, exp, self._p(packed), nranks)

    def xforward(self, spec_t, y0, nyl):
        assert spec_t.is_contiguous() and spec_t.dtype == torch.complex128
        self._call(capi.hip.shq_uvbg_slab_xforward, self.N, self._p(spec_t), y0, nyl)

    def xfilter(self, spec_t, out, y0, nyl, r):
        assert spec_t.is_contiguous() and out.is_contiguous() and out.dtype == torch.complex128 and out.shape == spec_t.shape
        self._call(capi.hip.shq_uvbg_slab_xfilter, self.N, self._p(spec_t), self._p(out), y0, nyl, r)

    def filter(self, spec_t, y0, nyl, r):
        assert spec_t.is_contiguous() and spec_t.dtype == torch.complex128
        self._call(capi.hip.shq_uvbg_slab_filter, self.N, self._p(spec_t), self._p(spec_t), y0, nyl, r)
        return spec_t

    def cells(self, p, cosmo, R, last, meshes, zp, nxl, J21, xHI):
        assert all(m.is_contiguous() and m.dtype == torch.float64 for m in meshes) and J21.is_contiguous() and xHI.is_contiguous()
        sums = (C.c_double * 3)()
        m = [self._p(x) for x in meshes] + [None] * (3 - len(meshes))
        self._call(capi.hip.shq_uvbg_slab_cells, C.byref(p), C.byref(cosmo), float(R), int(last), m[0], m[1], m[2], zp, 0, nxl, self._p(J21), self._p(xHI),
                   C.byref(sums))
        return list(sums) if last else None

    def readout(self, p, cosmo, posm, types, J21ext, plane0, nxl, local_J21, zreion):
        assert J21ext.is_contiguous() and J21ext.dtype == torch.float32
        self._call(capi.hip.shq_uvbg_slab_readout, C.byref(p), C.byref(cosmo), self._p(posm), self._p(types), posm.shape[0], self._p(J21ext), plane0, nxl,
                   J21ext.shape[0], self._p(local_J21), self._p(zreion))


class DistZeldovich(SlabMesh):
    """displacement_fields (libgenic/zeldovich.cpp:150-264) on x-slabs of the Nmesh mesh, one per rank: whole planes of equal width.
    Nmesh must be divisible by the rank count (equal y-slabs of the spectrum): otherwise the constructor raises ValueError on every
    rank, before any collective.

    Every rank fills the Gaussian field of its own y-slab (one mt19937 per mesh column: no communication, the bits of the one-rank
    field) and keeps it on this object across calls, keyed on (Nmesh, Seed, UnitaryAmplitude, InvertPhase): a second species does
    not refill.  Per field the transfer function is fused into the X inverse on the y-slab, ONE all-to-all takes the result to the
    x-slabs, the Y/Z inverse runs there, one shift brings the right-hand neighbour's first plane, and the particles routed to the
    owner of their CIC base cell gather with pm_iterate_one's weights.  A mesh line sees the same kernel arithmetic on any rank, so
    on the bespoke route the results do not depend on the rank count or on who held which particle.  ops (GpuZeldovichOps below; the
    CPU tests use a numpy stand-in) works on torch tensors:
      ops.pitch(N) -> doubles per z row of the bespoke passes, 0 without them;
      ops.fill(N, Seed, unitary, invert, y0, nyl) -> complex [N, nyl, pitch / 2 or N / 2 + 1];  ops.tables(N, L, delta, growth);
      ops.gather(N, L, pos, window, plane0, nxl, out);  ops.finalize(pos, fld, scaledep, vel_prefac, L) -> (Pos, Vel, Disp, [mx, mv]);
      bespoke route: ops.xtransfer(N, L, spec, out, y0, nyl, field), ops.fft_yz(N, planes, nxl, packed, P);
      torch.fft route: ops.transfer(N, L, spec, y0, nyl, field) -> a new tensor.
    Counters of the last call: rows_sent (particle rows that left this rank), nalltoall (all-to-alls and shifts started), filled
    (whether the field was filled rather than reused).  Nothing here has run on more than one GPU."""

    def __init__(self, comm, Nmesh, BoxSize, ops, bounds=None):
        super().__init__(comm, int(Nmesh), float(BoxSize), ops, bounds)
        self._equal_widths()
        self.filled = False
        self._key = self._spec = None

    def _refusal(self, params, delta, growth, pos):
        """what is wrong with this rank's input, or None"""
        nk2 = 3 * (self.N // 2) ** 2 + 1
        if params.Nmesh != self.N or params.BoxSize != self.L:
            return "the parameters' Nmesh / BoxSize are not this decomposition's"
        if not (math.isfinite(self.L) and self.L > 0 and math.isfinite(params.vel_prefac)):
            return "zeldovich: BoxSize must be finite and > 0, vel_prefac finite"
        if params.ScaleDepVelocity and growth is None:
            return "zeldovich: ScaleDepVelocity without a dlogGrowth table"
        if len(delta) != nk2 or (growth is not None and len(growth) != nk2):
            return "the tables by k2 need %d entries" % nk2
        if not np.isfinite(delta[1:]).all() or (params.ScaleDepVelocity and not np.isfinite(growth[1:]).all()):
            return "zeldovich: non-finite table entry"
        if pos.ndim != 2 or pos.shape[1] != 3:
            return "zeldovich: positions must be [n, 3]"
        if not ((pos >= 0) & (pos < self.L)).all():           # a NaN fails both
            return "zeldovich: a particle is outside [0, BoxSize)"
        return None

    def displacements(self, params, delta, growth, pos):
        """params: capi.ZeldovichParams; delta, growth: the tables by k2 (growth may be None without ScaleDepVelocity), the same on
        every rank; pos [n, 3]: the undisplaced positions this rank holds, in any distribution over the ranks.  Returns dict(Pos, Vel,
        Density, Disp, maxdisp, maxvel) in the caller's order, the two maxima the same on every rank.  Bad input on any rank raises
        ValueError on every rank: the ranks agree on it in one reduced flag, the first collective of the call."""
        c, d, ops, N, L = self.comm, self.d, self.ops, self.N, self.L
        pos = np.require(pos, dtype=np.float64, requirements=["C", "W"])      # torch takes no read-only array
        delta = np.ascontiguousarray(delta, dtype=np.float64)
        growth = None if growth is None else np.ascontiguousarray(growth, dtype=np.float64)
        why = self._refusal(params, delta, growth, pos)
        if c.allreduce_max_vec(np.array([0.0 if why is None else 1.0]))[0] > 0:
            raise ValueError(why or "zeldovich: another rank refused its input")
        scaledep = bool(params.ScaleDepVelocity)
        self.rows_sent = self.nalltoall = 0
        # ---- to the owner of the particle's CIC base plane; rows already at home stay in the self block
        # SlabDecomp.owner_of's floor(x / cell) % N, taken on the host: numpy divides as cic_setup does, while torch on the device
        # multiplies by the reciprocal of a scalar divisor - at nextafter(BoxSize, 0) that is plane N - 1 where the kernel sees cell
        # N = 0, and the particle would sit on the last rank with its corners on the first
        rows = torch.from_numpy(pos).to(ops.device)
        plane = np.floor(pos[:, 0] / d.cell).astype(np.int64) % N
        owner = torch.from_numpy(np.searchsorted(np.asarray(d.bounds[1:-1], dtype=np.int64), plane, side="right")).to(ops.device)
        mine, route = self.to_owners(rows, owner)
        mine = mine.contiguous()
        # ---- the Gaussian field of this rank's y-slab, kept across calls
        P, nxl = c.size, d.nxl
        nyl, y0 = N // P, c.rank * (N // P)
        key = (N, int(params.Seed), int(bool(params.UnitaryAmplitude)), int(bool(params.InvertPhase)))
        self.filled = self._key != key
        if self.filled:
            self._key = self._spec = None
            self._spec = ops.fill(*key, y0, nyl)
            self._key = key
        ops.tables(N, L, delta, growth if scaledep else None)
        nf = 7 if scaledep else 4
        fld = ops.full((7, mine.shape[0]), 0.0, torch.float64)
        (self._loop_bespoke if self.bespoke(ops.pitch(N)) else self._loop_torch)(mine, fld, nf)
        # ---- the particle loop, the two maxima, and the way back along the same counts: no key travels
        pos_out, vel, disp, mx = ops.finalize(mine, fld, scaledep, float(params.vel_prefac), L)
        mx = c.allreduce_max_vec(np.asarray(mx, dtype=np.float64))
        res = self.back(route, torch.cat([pos_out, vel, disp, fld[0][:, None]], dim=1).contiguous())
        return dict(Pos=res[:, 0:3].copy(), Vel=res[:, 3:6].copy(), Disp=res[:, 6:9].copy(), Density=res[:, 9].copy(), maxdisp=float(mx[0]),
                    maxvel=float(mx[1]))

    def _loop_bespoke(self, pos, fld, nf):
        """The library's own FFT passes (csrc/fft3d.hip).  Per field: the transfer pass out of place on the kept y-slab, ONE
        all-to-all, the Y/Z inverse from the packed buffer, the neighbour's plane, the gather.  Field f + 1's pass is queued before
        field f's exchange is waited for."""
        c, ops, N, L, P, nxl, plane0 = self.comm, self.ops, self.N, self.L, self.comm.size, self.d.nxl, self.d.plane0
        zp = ops.pitch(N)
        nyl, y0 = N // P, c.rank * (N // P)
        spec = self._spec
        nalloc = N if P == 1 else nxl + 1
        ext = ops.full((nalloc, N, zp), 0.0, torch.float64)
        own = ext[:nxl]
        for f in self.back_bespoke([own] * nf, spec, lambda f, out: ops.xtransfer(N, L, spec, out, y0, nyl, f),
                                   lambda f, packed: ops.fft_yz(N, own, nxl, packed, P)):
            self.neighbour_plane(ext, nxl)
            ops.gather(N, L, pos, ext, plane0, nxl, fld[f])

    def _loop_torch(self, pos, fld, nf):
        """The same loop with torch.fft for mesh sizes without a bespoke transform, and on the CPU stand-in: the field is kept as
        [x][y_l][z'], x slowest, dense."""
        c, ops, N, L, P, nxl, plane0 = self.comm, self.ops, self.N, self.L, self.comm.size, self.d.nxl, self.d.plane0
        Nc, nyl, y0 = N // 2 + 1, N // P, c.rank * (N // P)
        spec = self._spec if self._spec.shape[2] == Nc else self._spec[:, :, :Nc].contiguous()
        nalloc = N if P == 1 else nxl + 1
        ext = ops.full((nalloc, N, N + 2), 0.0, torch.float64)
        for f in range(nf):
            ext[:nxl, :, :N] = self.back_torch(ops.transfer(N, L, spec, y0, nyl, f))
            self.neighbour_plane(ext, nxl)
            ops.gather(N, L, pos, ext, plane0, nxl, fld[f])


class GpuZeldovichOps(_DeviceOps):
    """DistZeldovich's phases on the device library (shq_zeldovich_slab_*), on torch tensors of the context's device."""

    def pitch(self, N):
        return int(capi.hip.shq_zeldovich_slab_pitch(int(N)))

    def fill(self, N, Seed, unitary, invert, y0, nyl):
        spec = torch.empty((N, nyl, self.pitch(N) // 2 or N // 2 + 1), dtype=torch.complex128, device=self.device)
        self._call(capi.hip.shq_zeldovich_slab_fill, N, Seed, unitary, invert, y0, nyl, self._p(spec))
        return spec

    def tables(self, N, L, delta, growth):
        self._call(capi.hip.shq_zeldovich_slab_tables, N, L, capi.ptr(delta), capi.ptr(growth))

    def xtransfer(self, N, L, spec, out, y0, nyl, field):
        assert spec.is_contiguous() and out.is_contiguous() and out.dtype == spec.dtype == torch.complex128 and out.shape == spec.shape
        self._call(capi.hip.shq_zeldovich_slab_xtransfer, N, L, self._p(spec), self._p(out), y0, nyl, field)

    def transfer(self, N, L, spec, y0, nyl, field):
        assert spec.is_contiguous() and spec.dtype == torch.complex128 and spec.shape == (N, nyl, N // 2 + 1)
        out = torch.empty_like(spec)
        self._call(capi.hip.shq_zeldovich_slab_transfer, N, L, self._p(spec), self._p(out), y0, nyl, field)
        return out

    def fft_yz(self, N, planes, nplanes, packed, nranks):
        assert planes.is_contiguous() and (packed is None or (packed.is_contiguous() and packed.dtype == torch.complex128))
        self._call(capi.hip.shq_zeldovich_slab_fft_yz, N, self._p(planes), nplanes, self._p(packed), nranks)

    def gather(self, N, L, pos, window, plane0, nxl, out):
        assert pos.is_contiguous() and window.is_contiguous() and out.is_contiguous() and window.dtype == out.dtype == torch.float64
        assert window.shape[1:] == (N, self.pitch(N) or N + 2)
        self._call(capi.hip.shq_zeldovich_slab_gather, N, L, self._p(pos), pos.shape[0], self._p(window), plane0, nxl, window.shape[0], self._p(out))

    def finalize(self, pos, fld, scaledep, vel_prefac, L):
        n = pos.shape[0]
        assert pos.is_contiguous() and fld.is_contiguous() and fld.shape == (7, n)
        out = [torch.empty((n, 3), dtype=torch.float64, device=self.device) for _ in range(3)]
        mx = (C.c_double * 2)()
        self._call(capi.hip.shq_zeldovich_slab_finalize, n, self._p(pos), self._p(fld), int(scaledep), vel_prefac, L, *[self._p(o) for o in out],
                   C.byref(mx))
        return out[0], out[1], out[2], list(mx)


class _GlassState:
    """the particles a rank owns during a resident glass loop: Pos f64 [m, 3], Vel f32 [m, 3], Mass f32 [m], the origin tag (rank,
    index) as f64 [m, 2] (exact), and Disp f32 [m, 3], which every force writes here and which never travels"""

    def __init__(self, rows, ops):
        self.pos = rows[:, 0:3].contiguous()
        self.vel = rows[:, 3:6].to(torch.float32).contiguous()
        self.mass = rows[:, 6].to(torch.float32).contiguous()
        self.tag = rows[:, 7:9].contiguous()
        self.disp = ops.full((rows.shape[0], 3), 0.0, torch.float32)

    def rows(self, sel):
        """the travelling rows of the particles sel: one float64 row each; float Vel and Mass are exact in it"""
        return torch.cat([self.pos[sel], self.vel[sel].to(torch.float64), self.mass[sel].to(torch.float64)[:, None], self.tag[sel]], dim=1)


class DistGlass(SlabMesh):
    """glass_evolve (libgenic/glass.cpp:76-360) on x-slabs of the Nmesh mesh, one per rank: whole planes of equal width.  Nmesh must
    be divisible by the rank count (equal y-slabs of the spectrum): otherwise the constructor raises ValueError on every rank, before
    any collective.

    The particles move between the nsteps + 1 forces of a call, so their state lives on the slab owners for the whole loop: a row -
    Pos (3 f64), Vel (3 f32), Mass (f32) and an origin tag (rank, index) - sits with the owner of its CIC base plane, which the device
    takes with the kernels' own cell arithmetic (ops.planes).  After every drift ONE all-to-all re-homes the rows whose base plane
    changed owner, and only those; Disp is written on the owner by every force and read there by the next particle kernel, so it
    does not travel.  At the end every row goes back to its origin by its tag.

    One force: the zeroed window deposit (own planes and one behind) in fixed point with the exponent of the GLOBAL total mass, one
    shift that adds the ghost plane into the right-hand neighbour's plane 0 as int64, Y/Z forward packed, one all-to-all, X forward
    on the y-slab (both of the reference's power additions on the way when the step's spectrum is saved); then per axis the
    potential and force transfer fused into the out-of-place X inverse, one all-to-all, Y/Z inverse from the packed buffer, the
    neighbour's first plane by one shift, and the window gather into float Disp.  Axis a + 1's transfer pass is queued before axis
    a's exchange is waited for.  Mesh sizes without a bespoke transform take the same steps with torch.fft.

    The deposit adds integers and a mesh line sees the same kernel arithmetic on any rank, so on the bespoke route Pos, Vel and Disp
    do not depend on the rank count or on who held which particle - provided totmass is the same double: it is the all-reduced sum
    of the ranks' double sums of their float masses, which is independent of the rank count only when that sum is exact (it is for
    setup_glass's equal masses up to 2^29 particles).  The statistics and spectrum sums are added in any order.

    ops (GpuGlassOps below; the CPU tests use a numpy stand-in) works on torch tensors:
      ops.pitch(N) -> doubles per z row of the bespoke passes, 0 without them;  ops.tables(N, L, totmass);
      ops.planes(N, L, pos) -> int32 [m];  ops.deposit(N, L, pos, mass, exp, plane0, nxl, buf) into int64 [nalloc, N, pitch or N + 2];
      ops.gather(N, L, pos, window, plane0, nxl, disp, axis);  ops.particles(pos, vel, disp, ending, beginning) -> [sum Disp^2, sum Vel^2];
      bespoke route: ops.fft_yz(N, planes, nxl, direction, exp, packed, P), ops.xforward(N, spec, y0, nyl, sums or None),
      ops.xtransfer(N, spec, out, y0, nyl, axis);
      torch.fft route: ops.to_real(mesh_i, exp), ops.power(N, spec, y0, nyl, sums), ops.transfer(N, spec, y0, nyl, axis) -> a new tensor.
      sums is float64 [3 N + 1]: power, kk, nmodes (int64 bits), norm; the ops add to it.
    Counters of the last call: rows_sent (rows that left this rank in the opening routing), rehomed (per step the rows this rank sent
    away after the drift: over the ranks they add up to the owner changes of that step) and nalltoall, the all-to-alls and shifts
    started: 2 + nsteps + (nsteps + 1) * F with F = 4 on a one-rank group and 8 on several ranks - the opening routing and the
    return, one re-homing per step, and per force the spectrum's exchange and three force exchanges, on several ranks also the ghost
    shift and three neighbour-plane shifts.  (A lone process without a group has F = 0 on the bespoke route: its planes are the
    y-slab already.)  The all-reduces - the opening vector, the statistics and the spectra at the end - are not counted.
    Nothing here has run on more than one GPU."""

    def __init__(self, comm, Nmesh, BoxSize, ops, bounds=None):
        super().__init__(comm, int(Nmesh), float(BoxSize), ops, bounds)
        self._equal_widths()
        self.rehomed = []

    def _refusal(self, pos, vel, mass, nsteps):
        """what is wrong with this rank's input, or None: the checks of shq_glass_evolve"""
        N, L, n = self.N, self.L, len(pos)
        if not (4 <= N <= 2048 and N % 2 == 0):
            return "glass: Nmesh must be even and in [4, 2048] (got %d)" % N
        if nsteps < 0:
            return "glass: nsteps %d < 0" % nsteps
        if not (math.isfinite(L) and L > 0):
            return "glass: BoxSize must be finite and > 0"
        if pos.shape != (n, 3) or vel.shape != (n, 3) or mass.shape != (n,):
            return "glass: pos and vel are [n][3], mass is [n]"
        if n >= 2 ** 31:
            return "glass: %d particles on one rank (< 2^31)" % n
        if not np.isfinite(mass).all():
            return "glass: non-finite mass"
        if not np.isfinite(vel).all():
            return "glass: non-finite velocity"
        with np.errstate(invalid="ignore", over="ignore"):
            if not (np.isfinite(pos).all() and (np.abs(pos / (L / N)) < 1073741824.0).all()):
                return "glass: a position is not finite or beyond 2^30 cells"
        return None

    def _owner(self, pos):
        """the owner of each position's CIC base plane, which the device takes with the kernels' own cell arithmetic"""
        return torch.div(self.ops.planes(self.N, self.L, pos), self.d.nxl, rounding_mode="floor").to(torch.int64)

    def _home(self, rows):
        """rows (positions in columns 0 .. 2) to the owners of their CIC base planes; the block that stays is not copied through
        the network.  Returns the rows this rank owns now; how many left it is rows_sent."""
        mine, _ = self.to_owners(rows, self._owner(rows[:, 0:3].contiguous()))
        return mine.contiguous()

    def _rehome(self, S):
        """after a drift: the rows whose base plane changed owner travel in one all-to-all; the others stay where they are"""
        owner = self._owner(S.pos)
        away = owner != self.comm.rank
        idx = torch.nonzero(away).flatten()
        got = self._send_sorted(S.rows(idx), owner[idx])[0]
        self.rehomed.append(int(idx.numel()))
        if idx.numel() or got.shape[0]:
            keep = torch.nonzero(~away).flatten()
            S.__init__(torch.cat([S.rows(keep), got], dim=0), self.ops)

    def evolve(self, pos, vel, mass, nsteps, spectra=False, wrap=False):
        """pos f64 [n, 3] (unwrapped, any finite value), vel f32 [n, 3] or None, mass f32 [n] or a scalar: the particles this rank
        holds, in any distribution over the ranks; nsteps, spectra and wrap are the same on every rank.  Returns dict(Pos, Vel,
        Disp) in the caller's order, steps (dicts of t_f, t_v, t_x, force_std, vel_std, the same on every rank) and, with spectra,
        kk / power / nmodes [nsteps][Nmesh] and norm [nsteps]: the all-reduced raw sums of every step (glass_finish_power finishes
        one).  wrap=True applies the periodic wrap to the returned Pos.  Bad input on any rank raises ValueError on every rank, with
        nothing changed: the ranks agree on it in one reduced vector, the first collective of the call, which also carries the
        total mass and the particle count."""
        c, d, ops, N, L = self.comm, self.d, self.ops, self.N, self.L
        pos = np.array(pos, dtype=np.float64, order="C")
        n = len(pos)
        vel = np.zeros((n, 3), dtype=np.float32) if vel is None else np.array(vel, dtype=np.float32, order="C")
        mass = np.full(n, mass, dtype=np.float32) if np.isscalar(mass) else np.array(mass, dtype=np.float32, order="C")
        nsteps = int(nsteps)
        why = self._refusal(pos, vel, mass, nsteps)
        msum = 0.0 if why is not None else float(mass.astype(np.float64).sum())
        tot = c.allreduce_sum_vec(np.array([0.0 if why is None else 1.0, msum, float(n)]))
        if tot[0] > 0:
            raise ValueError(why or "glass: another rank refused its input")
        totmass, ntot = float(tot[1]), int(tot[2])
        if not (math.isfinite(totmass) and totmass > 0):
            raise ValueError("glass: the total mass must be > 0 (got %g)" % totmass)
        self.rows_sent = self.nalltoall = 0
        self.rehomed = []
        self._exp = math.frexp(totmass)[1]       # the deposit's scale is 2^(61 - exp): the whole mass in one cell stays below 2^61
        ops.tables(N, L, totmass)
        # ---- to the owners of the base planes, with the origin tag
        rows = np.empty((n, 9))
        rows[:, 0:3], rows[:, 3:6], rows[:, 6], rows[:, 7], rows[:, 8] = pos, vel, mass, c.rank, np.arange(n)
        S = _GlassState(self._home(torch.from_numpy(rows).to(ops.device)), ops)
        P, nxl = c.size, d.nxl
        nalloc = N if P == 1 else nxl + 1
        bespoke = self.bespoke(ops.pitch(N))
        zp = ops.pitch(N) if bespoke else N + 2
        self._buf = ops.full((nalloc, N, zp), 0, torch.int64)          # the deposit, then (bespoke) its (y, z) half spectrum
        self._ext = ops.full((nalloc, N, zp), 0.0, torch.float64)      # a force's real mesh and the neighbour's first plane
        force = self._force_bespoke if bespoke else self._force_torch
        save = spectra and nsteps > 0
        sums = ops.full((nsteps, 3 * N + 1), 0.0, torch.float64) if save else None
        # ---- glass_evolve (glass.cpp:76-147): one particle kernel between two forces
        force(S, None)
        stats = []
        for step in range(nsteps):
            part = ops.particles(S.pos, S.vel, S.disp, step > 0, True)
            if step > 0:
                stats.append(part)
            self._rehome(S)
            force(S, sums[step] if save else None)
        if nsteps > 0:
            stats.append(ops.particles(S.pos, S.vel, S.disp, True, False))
        self._buf = self._ext = None
        # ---- the way back by the tag, and the reductions
        back = self._send_sorted(torch.cat([S.pos, S.vel.to(torch.float64), S.disp.to(torch.float64), S.tag[:, 1:2]], dim=1),
                                 S.tag[:, 0].to(torch.int64))[0].cpu().numpy()
        assert len(back) == n
        at = back[:, 9].astype(np.int64)
        out = dict(Pos=np.empty((n, 3)), Vel=np.empty((n, 3), dtype=np.float32), Disp=np.empty((n, 3), dtype=np.float32))
        out["Pos"][at], out["Vel"][at], out["Disp"][at] = back[:, 0:3], back[:, 3:6], back[:, 6:9]
        st = c.allreduce_sum_vec(np.asarray(stats, dtype=np.float64).reshape(nsteps, 2))
        out["steps"] = []
        hdt = 0.5 * (math.pi / 2)
        t_x = t_v = 0.0
        for step in range(nsteps):
            t_x += hdt
            t_v += math.pi / 2
            t_f = t_x
            t_x += hdt
            out["steps"].append(dict(t_f=t_f, t_v=t_v, t_x=t_x, force_std=math.sqrt(st[step, 0] / float(ntot)),
                                     vel_std=math.sqrt(st[step, 1] / float(ntot))))
        if spectra:
            h = sums.cpu().numpy() if save else np.zeros((0, 3 * N + 1))
            nm = np.ascontiguousarray(h[:, 2 * N:3 * N]).view(np.int64)
            kk, power, nmodes, norm = [], [], [], []
            if save:
                f = c.allreduce_sum_vec(np.concatenate([h[:, :2 * N], h[:, 3 * N:]], axis=1))
                nm = c.allreduce_sum_vec(nm)
                power, kk, norm = f[:, :N], f[:, N:2 * N], f[:, 2 * N]
            out.update(kk=np.array(kk).reshape(max(nsteps, 0), N), power=np.array(power).reshape(max(nsteps, 0), N),
                       nmodes=nm.reshape(max(nsteps, 0), N), norm=np.array(norm).reshape(max(nsteps, 0)))
        if wrap:
            p = out["Pos"]
            while (p >= L).any():
                p[p >= L] -= L
            while (p < 0).any():
                p[p < 0] += L
        return out

    def _deposit(self, S):
        """the window deposit; on several ranks one shift adds the ghost plane into the right-hand neighbour's plane 0: integers, exact"""
        self.ops.deposit(self.N, self.L, S.pos, S.mass, self._exp, self.d.plane0, self.d.nxl, self._buf)
        self.add_ghosts([self._buf], self.d.nxl)

    def _gather(self, S, axis):
        """the right-hand neighbour's first plane behind the own ones by one shift to the left, then the window gather"""
        self.neighbour_plane(self._ext, self.d.nxl)
        self.ops.gather(self.N, self.L, S.pos, self._ext, self.d.plane0, self.d.nxl, S.disp, axis)

    def _force_bespoke(self, S, sums):
        """glass_force with the library's own FFT passes (csrc/fft3d.hip): the deposit's buffer becomes its (y, z) half spectrum,
        the spectrum is kept on the y-slab for the three axes, a force's planes land in the gather's window"""
        c, ops, N, P, nxl = self.comm, self.ops, self.N, self.comm.size, self.d.nxl
        nyl, y0 = N // P, c.rank * (N // P)
        self._deposit(S)
        own = self._buf[:nxl]
        spec = self.forward_bespoke(own, lambda packed: ops.fft_yz(N, own, nxl, 0, self._exp, packed, P)).wait().contiguous()
        ops.xforward(N, spec, y0, nyl, sums)
        real = self._ext[:nxl]
        for axis in self.back_bespoke([real] * 3, spec, lambda axis, out: ops.xtransfer(N, spec, out, y0, nyl, axis),
                                      lambda axis, packed: ops.fft_yz(N, real, nxl, 1, 0, packed, P)):
            self._gather(S, axis)

    def _force_torch(self, S, sums):
        """the same force with torch.fft, for mesh sizes without a bespoke transform and on the CPU stand-in: the spectrum is kept
        as [x][y_l][z'], x slowest, dense"""
        c, ops, N, P, nxl = self.comm, self.ops, self.N, self.comm.size, self.d.nxl
        nyl, y0 = N // P, c.rank * (N // P)
        self._deposit(S)
        spec = self.forward_torch(ops.to_real(self._buf[:nxl, :, :N], self._exp))
        if sums is not None:
            ops.power(N, spec, y0, nyl, sums)
        for axis in range(3):
            self._ext[:nxl, :, :N] = self.back_torch(ops.transfer(N, spec, y0, nyl, axis))
            self._gather(S, axis)


class GpuGlassOps(_DeviceOps):
    """DistGlass's phases on the device library (shq_glass_slab_*), on torch tensors of the context's device."""

    def pitch(self, N):
        return int(capi.hip.shq_glass_slab_pitch(int(N)))

    def tables(self, N, L, totmass):
        self._call(capi.hip.shq_glass_slab_tables, N, L, totmass)

    def planes(self, N, L, pos):
        assert pos.is_contiguous() and pos.dtype == torch.float64
        out = torch.empty((pos.shape[0],), dtype=torch.int32, device=self.device)
        self._call(capi.hip.shq_glass_slab_planes, N, L, self._p(pos), pos.shape[0], self._p(out))
        return out

    def deposit(self, N, L, pos, mass, exp, plane0, nxl, buf):
        assert pos.is_contiguous() and mass.is_contiguous() and mass.dtype == torch.float32 and buf.is_contiguous() and buf.dtype == torch.int64
        assert buf.shape[1:] == (N, self.pitch(N) or N + 2)
        self._call(capi.hip.shq_glass_slab_deposit, N, L, self._p(pos), self._p(mass), pos.shape[0], exp, plane0, nxl, buf.shape[0], self._p(buf))

    def fft_yz(self, N, planes, nplanes, direction, exp, packed, nranks):
        assert planes.is_contiguous() and (packed is None or (packed.is_contiguous() and packed.dtype == torch.complex128))
        self._call(capi.hip.shq_glass_slab_fft_yz, N, self._p(planes), nplanes, direction, exp, self._p(packed), nranks)

    def xforward(self, N, spec, y0, nyl, sums):
        assert spec.is_contiguous() and spec.dtype == torch.complex128 and (sums is None or (sums.is_contiguous() and sums.shape == (3 * N + 1,)))
        self._call(capi.hip.shq_glass_slab_xforward, N, self._p(spec), y0, nyl, self._p(sums))

    def xtransfer(self, N, spec, out, y0, nyl, axis):
        assert spec.is_contiguous() and out.is_contiguous() and out.dtype == spec.dtype == torch.complex128 and out.shape == spec.shape
        self._call(capi.hip.shq_glass_slab_xtransfer, N, self._p(spec), self._p(out), y0, nyl, axis)

    def power(self, N, spec, y0, nyl, sums):
        assert spec.is_contiguous() and spec.dtype == torch.complex128 and spec.shape == (N, nyl, N // 2 + 1) and sums.is_contiguous()
        self._call(capi.hip.shq_glass_slab_power, N, self._p(spec), y0, nyl, self._p(sums))

    def transfer(self, N, spec, y0, nyl, axis):
        assert spec.is_contiguous() and spec.dtype == torch.complex128 and spec.shape == (N, nyl, N // 2 + 1)
        out = torch.empty_like(spec)
        self._call(capi.hip.shq_glass_slab_transfer, N, self._p(spec), self._p(out), y0, nyl, axis)
        return out

    def gather(self, N, L, pos, window, plane0, nxl, disp, axis):
        assert pos.is_contiguous() and window.is_contiguous() and disp.is_contiguous() and window.dtype == torch.float64 and disp.dtype == torch.float32
        assert window.shape[1:] == (N, self.pitch(N) or N + 2)
        self._call(capi.hip.shq_glass_slab_gather, N, L, self._p(pos), pos.shape[0], self._p(window), plane0, nxl, window.shape[0], self._p(disp), axis)

    def particles(self, pos, vel, disp, ending, beginning):
        assert pos.is_contiguous() and vel.is_contiguous() and disp.is_contiguous() and vel.dtype == disp.dtype == torch.float32
        sums = (C.c_double * 2)()
        self._call(capi.hip.shq_glass_slab_particles, pos.shape[0], self._p(pos), self._p(vel), self._p(disp), int(ending), int(beginning), C.byref(sums))
        return list(sums)


# ---------------------------------------------------------------------------------------------------------------------
# Helium reionisation by quasar bubbles across ranks: turn_on_quasars (libgadget/cooling_qso_lightup.cpp:489-596) as its loop runs
# on several tasks.  Every rank holds some of the gas (any particle may sit on any rank: no decomposition, no ghosts) and hosts some
# of the groups.  The reference draws one global position per iteration on every task with the same random number; each task keeps
# its own ncand_before, and choose_QSO_halo (:314-328) decrements it BEFORE the range test.  So when the drawn position is the last
# candidate of all earlier tasks together, a task with a non-empty list returns local index 0 as well: it does not walk (only
# qso_ind > 0 walks) but erases its candidate 0 (:588-589), its list is from then on shorter than the global count assumes, and
# later draws can fall on a position no task hosts.  The outcome therefore depends on how the candidates are split over the tasks;
# what is reproduced here is the reference's loop for the split that is given, not a rank-independent result.
#
# Which quasars are drawn depends only on the random table and the candidate counts, so every rank replays every rank's counters
# (HeiiiDraws) without communication.  The lit bubbles of a batch of draws are swept on every rank against its own eligible gas (the
# walk of the hosting task reaches gas on every task; for R >= 0, +inf or NaN the particle test !(r2 > R*R) alone decides membership),
# the per-draw counts are all-reduced as one vector, and every rank replays the loop's control (:551-590) on the global counts.
#
# Culling.  A rank may leave a bubble (c, R) out of its sweep only if every eligible particle is proven outside by one axis alone.
# The sweep forms dx = NEAREST(fl(c - x)) and r2 = fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz)); rounding is monotone and the added
# terms are >= 0, so r2 >= fl(dx dx).  For the rank's eligible coordinates x in [lo, hi] (extents taken at open; the list only
# shrinks afterwards) t = fl(c - x) is non-increasing in x, so t lies in [a, b] with a = fl(c - hi), b = fl(c - lo).  f(t) =
# |NEAREST(t)| is, in the sweep's own floating-point operations, non-decreasing on -L <= t < -L/2 (fl(t + L) >= 0), non-increasing
# on [-L/2, 0], non-decreasing on [0, L/2] and non-increasing on L/2 < t <= L (|fl(t - L)| = fl(L - t)): on an interval inside
# [-L, L] that does not contain 0 its minimum is taken at an end, d = min(f(a), f(b)), computed with the same operations.  Then
# |dx| >= d >= 0 gives fl(dx dx) >= fl(d d), and fl(d d) > fl(R R) proves r2 > R*R for every eligible particle.  NEAREST wraps
# once only, so beyond |t| = L the outer pieces turn (|fl(t - L)| rises again) and the minimum can lie inside [a, b]: the proof
# needs |a| <= L and |b| <= L.  The reference keeps Pos in (0, L] and CM in [0, L), so that holds in a run, but it is checked, not
# assumed.  Kept without a proof: an interval that contains t = 0, an interval that leaves [-L, L], an interval at least L/2 wide,
# a non-finite centre or extent, and every bubble whose R is NaN or infinite.
def heiii_nearest(x, L):
    """NEAREST (partmanager.h:99) on Python floats: the operations of the sweep kernel"""
    return x - L if x > 0.5 * L else (x + L if x < -0.5 * L else x)


def heiii_bubble_reaches(c, R, lo, hi, L):
    """False only with a proof (above) that no coordinate box [lo, hi] particle passes the sweep's test for bubble (c, R)"""
    if not math.isfinite(R):
        return True
    R2 = R * R
    for d in range(3):
        if not (hi[d] - lo[d] < 0.5 * L):       # also extents that are not numbers
            continue
        a, b = c[d] - hi[d], c[d] - lo[d]
        if not (a > 0 or b < 0):      # 0 inside [a, b], or a centre that is not a number
            continue
        if not (abs(a) <= L and abs(b) <= L):   # NEAREST wraps once: beyond |t| = L the pieces of f are no longer monotone
            continue
        g = min(abs(heiii_nearest(a, L)), abs(heiii_nearest(b, L)))
        if g * g > R2:
            return False
    return True


class HeiiiDraws:
    """choose_QSO_halo's counters of every rank, replayed as written.  ncands: candidates per rank, in rank order; the candidates
    are numbered globally in that order.  batch(nd) makes up to nd draws and returns per draw the global number of the lit
    candidate, or -1 when no rank walked; `ended` is set by the draw that leaves ncand_tot <= 0, which lights nothing.  events counts
    two_host (two ranks with new_qso >= 0: the spurious erase), unhosted (no rank has the position), index0 (position 0 of some
    rank and nobody walks)."""

    def __init__(self, ncands, TotNgroups, rnd):
        off = np.concatenate([[0], np.cumsum(ncands)]).astype(np.int64)
        self.cand = [list(range(int(off[r]), int(off[r + 1]))) for r in range(len(ncands))]
        self.before = [int(x) for x in off[:-1]]          # count_QSO_halos (:283-304)
        self.ncand_tot = int(off[-1])
        self.seed, self.rnd = int(TotNgroups), rnd
        self.ndrawn, self.ended = 0, False
        self.events = dict(two_host=0, unhosted=0, index0=0)

    def batch(self, nd):
        out = []
        for _ in range(nd):
            drand = float(self.rnd[(self.seed + self.ndrawn) % len(self.rnd)])
            qso = int(drand * self.ncand_tot)
            self.ncand_tot -= 1
            new = []
            for r, cand in enumerate(self.cand):
                if qso < self.before[r]:
                    self.before[r] -= 1
                new.append(-1 if (qso < self.before[r] or qso >= self.before[r] + len(cand)) else qso - self.before[r])
            if self.ncand_tot <= 0:     # "not enough quasars": the loop ends before this one
                self.ended = True
                break
            walkers = [r for r, q in enumerate(new) if q > 0]
            assert len(walkers) <= 1, "two ranks walk in one iteration"
            out.append(self.cand[walkers[0]][new[walkers[0]]] if walkers else -1)
            hosts = sum(q >= 0 for q in new)
            self.events["two_host"] += hosts >= 2
            self.events["unhosted"] += hosts == 0
            self.events["index0"] += not walkers and hosts > 0
            for r, q in enumerate(new):
                if q >= 0:
                    del self.cand[r][q]
            self.ndrawn += 1
        return out


class DistHeIII:
    """run(P, SphP, groups, TotNgroups, params, rnd) -> (log, result), the same on every rank.
    P: numpy PARTICLE_DTYPE array of everything this rank owns (gas PI -> SphP), flag bit and Entropy of the ionised gas are written
    at the end; groups: the catalogue this rank hosts, in the order given (DistFOF.fof's list of dicts, or a FOF_GROUP_DTYPE array);
    TotNgroups: the global group count (the seed of the draws); params: capi.HeiiiParams (n_gas_tot is replaced by the all-reduced
    len(SphP)); rnd: RandTable::Table.  log: the FdHelium lines as (host rank, local group index, pos, ionfrac, n_ionized), with
    (-1, -1, zeros) when nothing was walked; result: shq_heiii_result's fields with global values.
    ops.open(P, SphP, params) -> (n_flash, n_ionized_now, n_eligible, lo[3], hi[3]); ops.sweep(bubbles, nseq) -> counts[nseq];
    ops.commit(seq_stop) -> particles committed; ops.close(P, SphP) -> rows written (GpuHeiiiOps below; the CPU tests use the
    restatement); ops.cull: leave out the bubbles that provably cannot reach this rank's eligible gas.
    The whole run is refused (ValueError on every rank) when ANY candidate of the gathered list has a radius below 0, -inf included,
    even one that would never be drawn: for such a radius the walk's node test decides too (at -inf cull_node rejects the root and
    the walk takes nothing, while the particle test alone would take everything), so membership would depend on each rank's tree.
    The radii are all known before the first draw, and refusing up front keeps every rank on the same path.  The run is closed on
    every way out, and after a refusal only the flash, if the target called for one, has been applied.
    Counters of the last run: nsweeps (batches), kept (bubbles this rank swept, per batch), ntests (eligible x kept, summed),
    events (HeiiiDraws').  Nothing here has run on more than one GPU."""

    FIRST_BATCH, MAX_BATCH = 32, capi.HEIII_MAX_SEQ      # the one call's schedule: 32, 64, ... 1024 draws per sweep

    def __init__(self, comm, ops):
        self.comm, self.ops = comm, ops
        self.nsweeps = self.ntests = self.nrows = 0
        self.kept, self.events = [], {}

    def _candidates(self, groups, p):
        """this rank's rows of build_qso_candidate_list (:260-276): (rank, local index, MinID, CM) as six 64-bit words each"""
        if isinstance(groups, np.ndarray):
            mass, minid, cm = groups["Mass"], groups["MinID"], groups["CM"]
        else:
            mass = np.array([g["Mass"] for g in groups], dtype=np.float64)
            minid = np.array([g["MinID"] for g in groups], dtype=np.uint64)
            cm = np.array([g["CM"] for g in groups], dtype=np.float64).reshape(len(groups), 3)
        sel = np.flatnonzero(~(mass < p.qso_candidate_min_mass) & ~(mass > p.qso_candidate_max_mass))
        rows = np.zeros((len(sel), 6), dtype=np.uint64)
        rows[:, 0], rows[:, 1], rows[:, 2] = self.comm.rank, sel, np.asarray(minid, dtype=np.uint64)[sel]
        rows[:, 3:] = np.ascontiguousarray(np.asarray(cm, dtype=np.float64)[sel]).view(np.uint64)
        return rows

    def run(self, P, SphP, groups, TotNgroups, params, rnd):
        rnd = np.ascontiguousarray(rnd, dtype=np.float64)
        p = capi.HeiiiParams.from_buffer_copy(params)
        p.n_gas_tot = int(self.comm.allreduce_sum_vec(np.array([len(SphP)], dtype=np.int64))[0])       # :492
        self.nsweeps = self.ntests = self.nrows = 0
        self.kept, self.events = [], {}
        opened = self.ops.open(P, SphP, p)
        try:
            return self._loop(p, groups, TotNgroups, rnd, *opened)
        finally:
            self.nrows = self.ops.close(P, SphP)

    def _loop(self, p, groups, TotNgroups, rnd, n_flash, n_ionized_now, m, lo, hi):
        comm, ops, L = self.comm, self.ops, p.BoxSize
        tot = comm.allreduce_sum_vec(np.array([n_ionized_now, n_flash], dtype=np.int64))                # :344-345, :510
        ngas = float(p.n_gas_tot)
        cur = int(tot[0]) / ngas
        res = dict(init_ionfrac=cur, final_ionfrac=cur, n_candidates=0, n_iterations=0, n_flash=int(tot[1]), n_ionized=0)
        log = []
        if not (cur < p.desired_ion_frac):
            return log, res
        cand = comm.allgather_u64(self._candidates(groups, p).reshape(-1)).reshape(-1, 6)
        res["n_candidates"] = len(cand)
        if len(cand) == 0:                                                                                 # :534-536
            return log, res
        crank, cindex = cand[:, 0].astype(np.int64), cand[:, 1].astype(np.int64)
        minid, cm = np.ascontiguousarray(cand[:, 2]), np.ascontiguousarray(cand[:, 3:]).view(np.float64)
        from . import heiii_host_numbers
        radii, threshold = heiii_host_numbers(p, minid, rnd)
        if np.any(radii < 0):
            raise ValueError("DistHeIII: candidate %d has the negative radius %g: membership would depend on each rank's tree"
                             % (int(np.flatnonzero(radii < 0)[0]), float(radii[radii < 0][0])))
        draws = HeiiiDraws(np.bincount(crank, minlength=comm.size), TotNgroups, rnd)
        self.events = draws.events
        cull = getattr(ops, "cull", True)
        batch, iteration, stopped = self.FIRST_BATCH, 0, False
        while not stopped and not draws.ended:
            drawn = draws.batch(batch)
            lit = [(k, g) for k, g in enumerate(drawn) if g >= 0]
            kept = [(k, g) for k, g in lit if m > 0 and (not cull or heiii_bubble_reaches(cm[g], float(radii[g]), lo, hi, L))]
            counts = np.zeros(len(drawn))
            if kept:
                bub = np.zeros(len(kept), dtype=capi.HEIII_BUBBLE_DTYPE)
                bub["seq"], gk = [k for k, _ in kept], [g for _, g in kept]
                bub["c"], bub["R"] = cm[gk], radii[gk]
                counts = ops.sweep(bub, len(drawn)).astype(np.float64)
            if lit:
                counts = comm.allreduce_sum_vec(counts)          # exact: counts are integers far below 2^53 (:554)
            self.nsweeps += 1
            self.kept.append(len(kept))
            self.ntests += m * len(kept)
            seq_stop = 0
            for k, g in enumerate(drawn):                         # the loop's control (:551-590), the same on every rank
                n_ionized = int(counts[k]) if g >= 0 else 0
                seq_stop = k + 1
                cur += n_ionized / ngas
                res["n_ionized"] += n_ionized
                if g >= 0:
                    pos = []
                    for d in range(3):                           # the MPI_MAX of :574 returns the host's wrapped CM: in (0, BoxSize]
                        x = float(cm[g, d]) - p.CurrentParticleOffset[d]
                        if math.isfinite(x):
                            while x > L:
                                x -= L
                            while x <= 0:
                                x += L
                        pos.append(x)
                    log.append((int(crank[g]), int(cindex[g]), tuple(pos), cur, n_ionized))
                else:
                    log.append((-1, -1, (0.0, 0.0, 0.0), cur, n_ionized))
                insufficient = n_ionized < 0.01 * threshold and iteration > 10
                iteration += 1
                if insufficient or not (cur < p.desired_ion_frac):
                    stopped = True
                    break
            if kept:
                m -= ops.commit(seq_stop)
            batch = min(2 * batch, self.MAX_BATCH)
        res.update(final_ionfrac=cur, n_iterations=iteration)
        return log, res


class GpuHeiiiOps:
    """DistHeIII's four steps on the device library (shq_heiii_open / _sweep / _commit / _close)"""

    def __init__(self, ctx, BoxSize, cull=True):
        import shenqi_amd as sq
        self.sq, self.ctx, self.L, self.cull = sq, ctx, BoxSize, cull
        self._pman = None

    def open(self, P, SphP, p):
        self._pman = records_pman(self.sq, self.L, P)
        pv, sv = self._pman.view(), capi.sph_view(SphP)
        nf, ni, ne = C.c_int64(), C.c_int64(), C.c_int64()
        lo, hi = np.zeros(3), np.zeros(3)
        capi.check(capi.hip.shq_heiii_open(self.ctx.h, C.byref(p), C.byref(pv), C.byref(sv), C.byref(nf), C.byref(ni), C.byref(ne), capi.ptr(lo), capi.ptr(hi)))
        return nf.value, ni.value, ne.value, lo, hi

    def sweep(self, bubbles, nseq):
        bubbles = np.ascontiguousarray(bubbles, dtype=capi.HEIII_BUBBLE_DTYPE)
        counts = np.zeros(nseq, dtype=np.uint64)
        capi.check(capi.hip.shq_heiii_sweep(self.ctx.h, capi.ptr(bubbles), len(bubbles), nseq, capi.ptr(counts)))
        return counts

    def commit(self, seq_stop):
        n = C.c_int64()
        capi.check(capi.hip.shq_heiii_commit(self.ctx.h, seq_stop, C.byref(n)))
        return n.value

    def close(self, P, SphP):
        pman, self._pman = self._pman, None
        pv, sv = pman.view(), capi.sph_view(SphP)
        n = C.c_int64()
        capi.check(capi.hip.shq_heiii_close(self.ctx.h, C.byref(pv), C.byref(sv), C.byref(n)))
        P["Flags"] = pman.Base["Flags"]
        return n.value


# ---------------------------------------------------------------------------------------------------------------------
# The domain decomposition itself: domain_decompose_full (libgadget/domain.cpp:174-277).  The particle loops run in `ops` (GpuDomainOps:
# shq_domain_* on the device; the tests' CPU stand-in: the restated procedures), the small serial stages are host functions, and this
# class holds what the reference does between them: the policy table, the retry with more top nodes, the global sample sort, the
# limits, the pairwise combine in the reference's own order (merge order changes the result), the all-reduce of the leaf counts.
class DistDomain:
    """One rank of a full domain decomposition.  params: DomainOverDecompositionFactor, TopNodeAllocFactor, SetAsideFactor (1).
    ops holds the rank's particles and offers samples / local_toptree / merge / finish / install / leaf_counts / balance /
    particle_topleaves / exchange / gc_sorted and `numpart`.  After decompose(): TopNodes, TopLeaves (with the sentinel entry), Tasks,
    policy (the index that worked; the next call starts there) and factor (TopNodeAllocFactor as the retries left it)."""
    NPOLICY = 16

    def __init__(self, comm, ops, params):
        self.comm, self.ops = comm, ops
        self.dodf = int(params["DomainOverDecompositionFactor"])
        self.factor = float(params["TopNodeAllocFactor"])
        self.setaside = float(params.get("SetAsideFactor", 1.0))
        self.policy = 0                 # LastSuccessfulPolicy
        self.TopNodes = self.TopLeaves = self.Tasks = None
        self.policies = []
        for i in range(self.NPOLICY):   # domain_policies_init, :378-403
            d = 256
            if i > 4 and self.policies[i - 1]["SubSampleDistance"] > 2:
                d = self.policies[i - 1]["SubSampleDistance"] // 2
            self.policies.append(dict(PreSort=int(i >= 2), SubSampleDistance=d, NTopLeaves=self.dodf * comm.size * (i + 1)))

    def _any(self, flag):
        return int(self.comm.allreduce_sum_vec(np.array([int(bool(flag))], dtype=np.int64))[0]) > 0

    # -- domain_nonrecursively_combine_topTree, :1178-1261
    def _combine(self, tree, MaxTopNodes):
        comm = self.comm
        errorflag = 0
        size = len(tree)
        sep = 1
        while sep < comm.size:
            if comm.rank % sep == 0:
                if (comm.rank // sep) % 2 == 0:
                    src = comm.rank + sep
                    if src < comm.size:
                        imp = comm.recv_array(src, capi.LOCAL_TOPNODE_DTYPE)
                        if size + len(imp) > MaxTopNodes:
                            errorflag = 1
                        elif len(imp) > 0 and not errorflag:
                            merged = self.ops.merge(tree, imp, MaxTopNodes)
                            if merged is None:
                                errorflag = 1
                            else:
                                tree, size = merged, len(merged)
                else:
                    dst = comm.rank - sep
                    if dst >= 0:
                        comm.send_array(tree, dst)
                    size = -1
            sep *= 2
        tree = comm.bcast_array(tree, capi.LOCAL_TOPNODE_DTYPE)
        if len(tree) >= MaxTopNodes:
            errorflag = 1
        return (None if self._any(errorflag) else tree)

    # -- domain_attempt_decompose / domain_determine_global_toptree, :452-500, :1269-1318
    def _attempt(self, pol, MaxTopNodes):
        ops, comm = self.ops, self.comm
        mine = np.asarray(ops.samples(pol["SubSampleDistance"], pol["PreSort"]), dtype=np.uint64)
        # mpsort_mpi: sorted across the ranks, every rank keeps as many as it gave
        allk = np.sort(comm.allgather_u64(mine), kind="stable")
        if comm.multi:
            n = comm.gather_scalar(len(mine), np.int64)
            off = int(n[:comm.rank].sum())
            mine = allk[off:off + len(mine)]
        else:
            mine = allk
        # topTree[0].Count == topTree[0].Cost == the rank's samples: the limits of :1287-1291 need no tree
        limit = len(allk) // pol["NTopLeaves"]
        tree = ops.local_toptree(mine, limit, limit, MaxTopNodes)
        if self._any(tree is None):
            return True
        tree = self._combine(tree, MaxTopNodes)
        if tree is None:
            return True
        res = ops.finish(tree, MaxTopNodes, limit, limit)
        if self._any(res is None):
            return True
        self.TopNodes, self.TopLeaves = res
        if len(self.TopLeaves) - 1 < comm.size:
            raise RuntimeError("Number of Topleaves is less than NTask")
        return False

    def decompose(self):
        ops, comm = self.ops, self.comm
        done = False
        for i in range(self.policy, self.NPOLICY):
            pol = self.policies[i]
            while True:
                MaxTopNodes = int(self.factor * (ops.numpart + 1))
                if not self._attempt(pol, MaxTopNodes):
                    break
                self.factor *= 1.2
                if self.factor > 10:
                    raise RuntimeError("TopNodeAllocFactor = %g, unreasonably large!" % self.factor)
            # domain_balance, :506-527
            ops.install(self.TopNodes, self.TopLeaves)
            count = comm.allreduce_sum_vec(np.asarray(ops.leaf_counts(), dtype=np.int64))
            self.Tasks, status = ops.balance(self.TopNodes, self.TopLeaves, count, comm.size, self.setaside)
            if status and i < self.NPOLICY - 1:
                continue
            ops.install(self.TopNodes, self.TopLeaves)
            ops.particle_topleaves()
            if ops.exchange(comm):
                if i == self.NPOLICY - 1:
                    raise RuntimeError("Ran out of policies!")
                continue
            self.policy = i
            done = True
            break
        if not done:
            raise RuntimeError("No suitable domain decomposition policy worked for this particle distribution")
        ops.gc_sorted()
        comm.barrier()
        return self


class GpuDomainOps:
    """DistDomain's operators on the device: parts is a device uint8 tensor of MaxPart particle_data records (layout: the
    ExchangeLayout DistExchange takes, off_pos / off_topleaf the byte offsets of Pos and TopLeaf), slots / slot_size the per-type slot
    arrays.  `tables` is the key automaton (capi.peano_tables_from_key of the reference's peano_hilbert_key)."""

    def __init__(self, ctx, tables, layout, off_pos, off_topleaf, BoxSize, parts, numpart, slots, slot_size):
        self.ctx, self.tables, self.L = ctx, tables, layout
        self.off_pos, self.off_topleaf, self.box = int(off_pos), int(off_topleaf), float(BoxSize)
        self.parts, self.numpart, self.slots, self.slot_size = parts, int(numpart), slots, [int(x) for x in slot_size]
        self.esz = int(layout.part_elsize)
        self.MaxPart = parts.numel() // self.esz
        self.keys = None

    def _pv(self):
        return capi.DomainParts(self.parts.data_ptr(), self.esz, int(self.L.off_flags), self.off_pos, self.numpart, self.box)

    def _sync(self):
        torch.cuda.current_stream(self.parts.device).synchronize()

    def samples(self, dist_, presort):
        out = torch.empty(self.numpart // dist_ + 1, dtype=torch.int64, device=self.parts.device)
        n = C.c_int64()
        self._sync()
        capi.check(capi.hip.shq_domain_samples(self.ctx.h, C.byref(self.tables), C.byref(self._pv()), int(dist_), int(presort), out.data_ptr(), C.byref(n)))
        self.ctx.synchronize()
        return out[:n.value].cpu().numpy().view(np.uint64)

    def local_toptree(self, lp, countlimit, costlimit, MaxTopNodes):
        d = torch.from_numpy(np.ascontiguousarray(lp, dtype=np.uint64).view(np.int64).copy()).to(self.parts.device)
        tree = np.zeros(MaxTopNodes, dtype=capi.LOCAL_TOPNODE_DTYPE)
        size = C.c_int()
        self._sync()
        rc = capi.hip.shq_domain_local_toptree(self.ctx.h, d.data_ptr(), len(lp), int(countlimit), int(costlimit), int(MaxTopNodes), tree.ctypes.data, C.byref(size))
        if rc == capi.ERR_RETRY:
            return None
        capi.check(rc)
        return tree[:size.value].copy()

    @staticmethod
    def merge(A, B, MaxTopNodes):
        buf = np.zeros(MaxTopNodes, dtype=capi.LOCAL_TOPNODE_DTYPE)
        buf[:len(A)] = A
        size = C.c_int(len(A))
        B = np.ascontiguousarray(B)
        rc = capi.hip.shq_domain_toptree_merge(buf.ctypes.data, C.byref(size), B.ctypes.data, len(B), int(MaxTopNodes))
        if rc == capi.ERR_RETRY:
            return None
        capi.check(rc)
        return buf[:size.value].copy()

    @staticmethod
    def finish(T, MaxTopNodes, countlimit, costlimit):
        buf = np.zeros(MaxTopNodes, dtype=capi.LOCAL_TOPNODE_DTYPE)
        buf[:len(T)] = T
        size, nl = C.c_int(len(T)), C.c_int()
        N = np.zeros(MaxTopNodes, dtype=capi.TOPNODE_DTYPE)
        L = np.zeros(MaxTopNodes + 1, dtype=capi.TOPLEAF_DTYPE)
        rc = capi.hip.shq_domain_toptree_finish(buf.ctypes.data, C.byref(size), int(MaxTopNodes), int(countlimit), int(costlimit), N.ctypes.data, L.ctypes.data,
                                                C.byref(nl))
        if rc == capi.ERR_RETRY:
            return None
        capi.check(rc)
        return N[:size.value].copy(), L[:nl.value + 1].copy()

    def balance(self, N, L, count, NTask, SetAsideFactor):
        Tasks = np.zeros(NTask + 1, dtype=capi.TASK_LEAFS_DTYPE)
        status = C.c_int()
        count = np.ascontiguousarray(count, dtype=np.int64)
        capi.check(capi.hip.shq_domain_balance(N.ctypes.data, len(N), L.ctypes.data, len(L) - 1, count.ctypes.data, int(NTask), int(self.MaxPart), float(SetAsideFactor),
                                               Tasks.ctypes.data, C.byref(status)))
        return Tasks, int(status.value)

    def install(self, N, L, geo=None):
        capi.check(capi.hip.shq_domain_install(self.ctx.h, C.byref(self.tables), N.ctypes.data, len(N), L.ctypes.data, len(L) - 1,
                                               None if geo is None else geo.ctypes.data))
        self.ntopleaves = len(L) - 1

    def leaf_counts(self):
        out = np.zeros(self.ntopleaves, dtype=np.int64)
        self._sync()
        capi.check(capi.hip.shq_domain_leaf_counts(self.ctx.h, C.byref(self._pv()), out.ctypes.data))
        return out

    def _topleaf_field(self):
        """the TopLeaf members of the records as an int32 view [MaxPart]"""
        return self.parts.view(-1, self.esz)[:, self.off_topleaf:self.off_topleaf + 4]

    def particle_topleaves(self):
        n, dev = self.numpart, self.parts.device
        leaf = self._topleaf_field()[:n].contiguous().view(torch.int32).reshape(-1)      # garbage keeps its old leaf
        self.target = torch.full((max(n, 1),), -1, dtype=torch.int32, device=dev)
        self._sync()
        capi.check(capi.hip.shq_domain_particle_topleaves(self.ctx.h, C.byref(self._pv()), leaf.data_ptr(), self.target.data_ptr()))
        self.ctx.synchronize()
        self._topleaf_field()[:n] = leaf.view(torch.uint8).view(-1, 4)
        return self.target[:n]

    def exchange(self, comm):
        """DomainExchangePlan::domain_exchange with the targets of particle_topleaves; 1 where the reference reports "Could not exchange" """
        def layoutfn(parts, numpart):
            # layoutfunc (:159-164) every round, arrivals included: their keys name the leaves they were sent for
            self.numpart = numpart
            return self.particle_topleaves()
        try:
            self.numpart, self.slot_size = DistExchange(comm, self.ctx, self.L).exchange(self.parts, self.numpart, self.slots, self.slot_size, layoutfn)
        except MemoryError:
            return 1
        return 0

    def gc_sorted(self):
        n, dev = self.numpart, self.parts.device
        keys = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        self._sync()
        capi.check(capi.hip.shq_peano_keys(self.ctx.h, C.byref(self.tables), self.parts.data_ptr() + self.off_pos, self.esz, n, self.box, keys.data_ptr()))
        np_ = C.c_int64(n)
        sz = (C.c_int64 * 6)(*self.slot_size)
        sp = (C.c_void_p * 6)(*[None if s is None else s.data_ptr() for s in self.slots])
        capi.check(capi.hip.shq_slots_gc_sorted(self.ctx.h, C.byref(self.L), self.parts.data_ptr(), C.byref(np_), self.MaxPart, sp, sz, keys.data_ptr()))
        self.ctx.synchronize()
        self.numpart, self.slot_size = int(np_.value), [int(x) for x in sz]
