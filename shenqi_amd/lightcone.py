"""Light-cone crossings (libgadget/lightcone.cpp; csrc/lightcone.hip): the horizon table, the state lightcone_set_time keeps (horizons,
replica list, SampleFraction) and the device call that turns device-resident records into the ordered rows of lightcone_compute.

Records live in device memory behind objects with a data_ptr() (torch uint8 tensors); rows come back as torch tensors on that device."""
import collections
import ctypes as C

import numpy as np

from . import capi

MODES = {"consistent": capi.LIGHTCONE_CONSISTENT, "as_written": capi.LIGHTCONE_AS_WRITTEN}

LightconeStateView = collections.namedtuple(
    "LightconeStateView", "HorizonDistance HorizonDistance2 HorizonDistancePrev HorizonDistance2Prev HorizonDistanceRef SampleFraction Nreplica Reps")


def lightcone_layout(part_dtype=None):
    """shq_lightcone_layout of the record dtype: Type, Pos, Vel, ID"""
    P = capi.PARTICLE_DTYPE if part_dtype is None else part_dtype
    f = P.fields
    return capi.LightconeLayout(P.itemsize, f["Type"][1], f["Pos"][1], f["Vel"][1], f["ID"][1])


def lightcone_table(E, timeBegin, DH, nentry=4096):
    """(tab_loga, tab_Dc, dloga) in the layout of lightcone_init: tab_loga[i] = -dloga * (nentry - i - 1) with dloga = -log(timeBegin) /
    (nentry - 1), tab_Dc[i] = DH * integral of 1 / (E(a) a) d log a from tab_loga[i] to 0, by one 64-point Gauss-Legendre rule per entry.
    E(a) = H(a) / H0 is called with a float; DH is the Hubble distance in internal length units."""
    nentry = int(nentry)
    if nentry < 2 or not 0 < timeBegin < 1:
        raise ValueError("lightcone_table: nentry >= 2 and 0 < timeBegin < 1")
    dloga = (0.0 - np.log(float(timeBegin))) / (nentry - 1)
    tab_loga = np.array([-dloga * (nentry - i - 1) for i in range(nentry)], dtype=np.float64)
    x, w = np.polynomial.legendre.leggauss(64)
    tab_Dc = np.empty(nentry, dtype=np.float64)
    for i in range(nentry):
        half = -0.5 * tab_loga[i]                    # the interval is [tab_loga[i], 0]
        a = np.exp(half * x - half)
        f = np.array([1.0 / (float(E(float(ai))) * ai) for ai in a])
        tab_Dc[i] = float(DH) * half * float(np.dot(w, f))
    return tab_loga, tab_Dc, float(dloga)


def _table(tab_loga, tab_Dc, dloga=None):
    la = np.ascontiguousarray(tab_loga, dtype=np.float64)
    dc = np.ascontiguousarray(tab_Dc, dtype=np.float64)
    if la.ndim != 1 or la.shape != dc.shape or len(la) < 2:
        raise ValueError("lightcone: tab_loga and tab_Dc are two 1-d arrays of one length >= 2")
    if dloga is None:
        dloga = (0.0 - la[0]) / (len(la) - 1)    # lightcone_init's own expression, from log(timeBegin) = tab_loga[0]
    return capi.LightconeTable(la.ctypes.data, dc.ctypes.data, len(la), 0, float(dloga)), (la, dc)


def lightcone_horizon(tab_loga, tab_Dc, a, dloga=None):
    """shq_lightcone_horizon: lightcone_get_horizon(a) on the table"""
    t, keep = _table(tab_loga, tab_Dc, dloga)
    out = C.c_double()
    capi.check(capi.hip.shq_lightcone_horizon(C.byref(t), float(a), C.byref(out)), "lightcone_horizon")
    return out.value


def lightcone_compute_raw(ctx, layout, d_parts, numpart, state, mode, ddrift, offset, rnd_table, d_rows, d_index, d_replica, capacity):
    """shq_lightcone_compute as it is: (status, nrows).  d_rows / d_index / d_replica are device tensors (or None); nothing is raised."""
    rnd = np.ascontiguousarray(rnd_table, dtype=np.float64)
    off = (C.c_double * 3)(*[float(x) for x in offset])
    nrows = C.c_int64(-1)
    dp = None if d_parts is None else d_parts.data_ptr()
    rc = capi.hip.shq_lightcone_compute(ctx.h, C.byref(layout), dp, int(numpart), C.byref(state), int(mode), float(ddrift), off, capi.ptr(rnd), len(rnd),
                                        None if d_rows is None else d_rows.data_ptr(), None if d_index is None else d_index.data_ptr(),
                                        None if d_replica is None else d_replica.data_ptr(), int(capacity), C.byref(nrows))
    return rc, nrows.value


def lightcone_phase_ms(ctx):
    """shq_lightcone_phase_ms: device times of the last compute that launched, in ms: pass A, the scan, pass B"""
    ms = (C.c_double * 3)()
    capi.check(capi.hip.shq_lightcone_phase_ms(ctx.h, ms), "lightcone_phase_ms")
    return list(ms)


class Lightcone:
    """The file statics of lightcone.cpp for one run: the table, the parameters and the state set_time moves."""

    first_capacity = 1024     # rows compute() makes room for before it knows better (or a 64th of the particles, if that is more)

    def __init__(self, tab_loga, tab_Dc, BoxSize, zmin=0.1, zmax=80.0, ReferenceRedshift=2.0, BoxBoost=20, dloga=None):
        self._table, self._keep = _table(tab_loga, tab_Dc, dloga)
        self.BoxSize = float(BoxSize)
        self.params = capi.LightconeParams(float(zmin), float(zmax), float(ReferenceRedshift), int(BoxBoost), 0)
        self._state = capi.LightconeState()
        capi.check(capi.hip.shq_lightcone_init(C.byref(self._table), C.byref(self.params), C.byref(self._state)), "lightcone_init")

    def horizon(self, a):
        out = C.c_double()
        capi.check(capi.hip.shq_lightcone_horizon(C.byref(self._table), float(a), C.byref(out)), "lightcone_horizon")
        return out.value

    def set_time(self, a):
        """lightcone_set_time(a, BoxSize)"""
        capi.check(capi.hip.shq_lightcone_set_time(C.byref(self._table), C.byref(self.params), float(a), self.BoxSize, C.byref(self._state)), "lightcone_set_time")

    @property
    def state(self):
        s = self._state
        reps = np.array(s.Reps, dtype=np.float64).reshape(capi.LIGHTCONE_MAXREPLICA, 3)[:s.Nreplica].copy()
        reps.setflags(write=False)
        return LightconeStateView(s.HorizonDistance, s.HorizonDistance2, s.HorizonDistancePrev, s.HorizonDistance2Prev, s.HorizonDistanceRef, s.SampleFraction,
                                  int(s.Nreplica), reps)

    def compute(self, ctx, d_parts, numpart, ddrift, offset, rnd_table, mode="consistent", capacity=None, layout=None):
        """shq_lightcone_compute on the current state: (rows [nrows, 4] float64, index [nrows] int32, replica [nrows] int32), device tensors
        in (particle, replica) order.  capacity None: the buffers grow once when the first guess is too small and the call is repeated;
        a given capacity that is too small raises."""
        import torch
        L = lightcone_layout() if layout is None else layout
        m = MODES[mode] if isinstance(mode, str) else int(mode)
        cap = max(int(self.first_capacity), int(numpart) // 64) if capacity is None else int(capacity)
        for _ in range(2):
            rows = torch.empty((max(cap, 1), 4), dtype=torch.float64, device=d_parts.device)
            index = torch.empty(max(cap, 1), dtype=torch.int32, device=d_parts.device)
            replica = torch.empty(max(cap, 1), dtype=torch.int32, device=d_parts.device)
            rc, n = lightcone_compute_raw(ctx, L, d_parts, numpart, self._state, m, ddrift, offset, rnd_table, rows, index, replica, cap)
            if rc == capi.ERR_NOMEM and capacity is None and n > cap:
                cap = n
                continue
            break
        capi.check(rc, "lightcone_compute")
        return rows[:n], index[:n], replica[:n]
