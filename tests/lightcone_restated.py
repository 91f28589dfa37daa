"""libgadget/lightcone.cpp restated in numpy / math, and the cases the CPU and GPU tests share.

  lightcone_get_horizon (:101-115)                       horizon()
  lightcone_init (:95), the statics' start               State()
  lightcone_set_time, update_replicas (:118-200)         set_time(), update_replicas()
  lightcone_compute over lightcone_cross (:159-168, :203-250), on one thread     cross()

No output of the reference's light cone is stored here: it needs a running simulation.  Parity rests on reading its code, as for the other
*_restated.py files.  math.log is the C library's log, which is what the host code calls; every other operation is an IEEE double
operation in the reference's order (numpy's elementwise +, -, *, /, sqrt are correctly rounded, so running cross() over all particles
of one replica at a time changes no bit; the rows are put back into the order of the serial loop at the end).

cross() carries both forms of :219-220:
  "as_written"   pold = Pos + Reps[i] - off,  pnew = Pos + Base[i].Vel * ddrift - off          (record i, the replica index; no shift)
  "consistent"   pold = Pos + Reps[i] - off,  pnew = Pos + Reps[i] + Base[p].Vel * ddrift - off
MyFloat is double in these records (LOW_PRECISION's default), so Vel needs no widening."""
import ctypes as C
import functools
import math

import numpy as np

from shenqi_amd import capi

SEED = 20261019
COUNTS = (0, 1, 63, 65, 257, 1000, 5000)   # nothing, one lane, a wave less and more one, two workgroups, four, and past the scan's blocks
MAXREPLICA = 1000
BOXSIZE = 1.0
BOXBOOST = 5
OFFSET = (0.375, -0.25, 0.0625)
ZERO = (0.0, 0.0, 0.0)
DDRIFT = 0.05
VMAX = 1.0          # |Vel[k]| <= VMAX, so a drift moves a coordinate by at most VMAX * DDRIFT = 0.05
RNDSIZE = 997
TINY = 3e-17       # between half an ulp of [0.25, 0.5) and half an ulp of [0.5, 1)
U64 = 1 << 64
# (mode, (H, Hprev), offset): what the GPU test runs, each with both fractions
GEOMETRIES = (("consistent", (2.30, 2.40), OFFSET), ("consistent", (2.30, 2.31), OFFSET), ("consistent", (1.20, 1.30), ZERO), ("as_written", (1.20, 1.30), ZERO))
FRACTIONS = (1.0, 0.3)
NREPLICA = {(2.30, 2.40): 16, (2.30, 2.31): 16, (1.20, 1.30): 4}


class TooManyReplica(Exception):
    """endrun(951234, "too many replica")"""


# ---- the table ------------------------------------------------------------------------------------------------------------------------

def horizon(tab_loga, tab_Dc, dloga, a):
    """:101-115"""
    nentry = len(tab_loga)
    loga = math.log(a)
    bin_ = int((math.log(a) - tab_loga[0]) / dloga)   # C's conversion to int truncates toward zero, as int() does
    if bin_ < 0:
        return float(tab_Dc[0])
    if bin_ >= nentry - 1:
        return float(tab_Dc[nentry - 1])
    u1 = loga - tab_loga[bin_]
    u2 = tab_loga[bin_ + 1] - loga
    u1 /= (tab_loga[bin_ + 1] - tab_loga[bin_])
    u2 /= (tab_loga[bin_ + 1] - tab_loga[bin_])
    return float(tab_Dc[bin_] * u2 + tab_Dc[bin_ + 1] * u1)


def eds_table(timeBegin, DH, nentry=4096):
    """Einstein-de Sitter in the layout of lightcone_init: Dc = 2 DH (1 - sqrt(a))"""
    dloga = (0.0 - math.log(timeBegin)) / (nentry - 1)
    tab_loga = np.array([-dloga * (nentry - i - 1) for i in range(nentry)], dtype=np.float64)
    tab_Dc = np.array([2.0 * DH * (1.0 - math.sqrt(math.exp(x))) for x in tab_loga], dtype=np.float64)
    return tab_loga, tab_Dc, dloga


# ---- the state ------------------------------------------------------------------------------------------------------------------------

class State:
    """the file statics, zero at the start; Reps keeps what earlier calls left behind Nreplica, as a static array does"""

    def __init__(self, HorizonDistanceRef=0.0):
        self.HorizonDistance = self.HorizonDistance2 = self.HorizonDistancePrev = self.HorizonDistance2Prev = 0.0
        self.HorizonDistanceRef = HorizonDistanceRef
        self.SampleFraction = 0.0
        self.Nreplica = 0
        self.Reps = np.zeros((MAXREPLICA, 3), dtype=np.float64)

    def struct(self):
        s = capi.LightconeState()
        for f in ("HorizonDistance", "HorizonDistance2", "HorizonDistancePrev", "HorizonDistance2Prev", "HorizonDistanceRef", "SampleFraction"):
            setattr(s, f, getattr(self, f))
        s.Nreplica = self.Nreplica
        C.memmove(C.addressof(s.Reps), self.Reps.ctypes.data, self.Reps.nbytes)
        return s

    def bytes(self):
        return bytes(self.struct())


def init_state(tab_loga, tab_Dc, dloga, ReferenceRedshift=2.0):
    return State(horizon(tab_loga, tab_Dc, dloga, 1 / (1 + ReferenceRedshift)))


def update_replicas(st, BoxSize, BoxBoost):
    """:118-154"""
    Nmax = BoxBoost * BoxBoost * BoxBoost
    rx = ry = rz = 0
    st.Nreplica = 0
    for _ in range(Nmax):
        dx = BoxSize * rx
        dy = BoxSize * ry
        dz = BoxSize * rz
        d1 = dx * dx + dy * dy + dz * dz
        dx += BoxSize
        dy += BoxSize
        dz += BoxSize
        d2 = dx * dx + dy * dy + dz * dz
        if d1 <= st.HorizonDistance2 and d2 >= st.HorizonDistance2:
            if st.Nreplica >= MAXREPLICA:
                raise TooManyReplica()
            st.Reps[st.Nreplica] = (rx * BoxSize, ry * BoxSize, rz * BoxSize)
            st.Nreplica += 1
        rz += 1
        if rz == BoxBoost:
            rz = 0
            ry += 1
        if ry == BoxBoost:
            ry = 0
            rx += 1


def count_straddling(H, BoxSize, BoxBoost):
    """how many boxes update_replicas would list, without the limit"""
    r = BoxSize * np.arange(BoxBoost, dtype=np.float64)
    x, y, z = np.meshgrid(r, r, r, indexing="ij")
    d1 = x * x + y * y + z * z
    x, y, z = x + BoxSize, y + BoxSize, z + BoxSize
    d2 = x * x + y * y + z * z
    return int(np.count_nonzero((d1 <= H * H) & (d2 >= H * H)))


def set_time(st, tab_loga, tab_Dc, dloga, a, BoxSize, zmin=0.1, zmax=80.0, ReferenceRedshift=2.0, BoxBoost=20):
    """:170-200"""
    z = 1 / a - 1
    if z > zmin and z < zmax:
        st.HorizonDistancePrev = st.HorizonDistance
        st.HorizonDistance2Prev = st.HorizonDistance2
        st.HorizonDistance = horizon(tab_loga, tab_Dc, dloga, a)
        st.HorizonDistance2 = st.HorizonDistance * st.HorizonDistance
        update_replicas(st, BoxSize, BoxBoost)
        if z < ReferenceRedshift:
            st.SampleFraction = 1.0
        else:
            st.SampleFraction = st.HorizonDistanceRef / st.HorizonDistance
            st.SampleFraction *= st.SampleFraction
            st.SampleFraction *= st.SampleFraction
    else:
        st.SampleFraction = 0


def hand_state(H, Hprev, fraction, BoxSize=BOXSIZE, BoxBoost=BOXBOOST):
    """a state with these horizons and the replica list update_replicas makes for H"""
    st = State()
    st.HorizonDistance, st.HorizonDistance2 = H, H * H
    st.HorizonDistancePrev, st.HorizonDistance2Prev = Hprev, Hprev * Hprev
    update_replicas(st, BoxSize, BoxBoost)
    st.SampleFraction = fraction
    return st


# ---- the crossings ----------------------------------------------------------------------------------------------------------------------

class Rows:
    """rows [m, 4], index [m], replica [m] in the order of the serial loop, and what the CPU test asks about them"""

    def __init__(self, rows, index, replica, half, wrapped, geometric, drawn_out):
        self.rows, self.index, self.replica = rows, index, replica
        self.half = half            # rows that took u1 = u2 = 0.5
        self.wrapped = wrapped      # rows whose ID + i wrapped
        self.geometric = geometric  # pairs that pass the distance test
        self.drawn_out = drawn_out  # ... of which the draw rejected


def cross(P, st, mode, ddrift, offset, rnd, pos="Pos", vel="Vel", ident="ID", typ="Type"):
    """lightcone_compute's loop on one thread: for p, for i.  P is a record array; the field names can be redirected for other layouts."""
    n = len(P)
    H, H2, Hp, H2p, frac = st.HorizonDistance, st.HorizonDistance2, st.HorizonDistancePrev, st.HorizonDistance2Prev, st.SampleFraction
    empty = Rows(np.zeros((0, 4)), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), 0, 0, 0, 0)
    if frac <= 0.0 or n == 0 or st.Nreplica == 0:
        return empty
    if mode == "as_written" and n < st.Nreplica:
        raise IndexError("Base[i] does not exist")
    who = np.flatnonzero(P[typ] == 1)                 # "DM only"; no garbage test
    X = np.ascontiguousarray(P[pos][who], dtype=np.float64)
    V = np.ascontiguousarray(P[vel], dtype=np.float64)
    ids = [int(x) for x in P[ident][who]]
    off = [float(x) for x in offset]
    tsize = len(rnd)
    out, half, wrapped, geometric, drawn_out = [], 0, 0, 0, 0
    for i in range(st.Nreplica):
        r = np.array([rnd[(q + i) % U64 % tsize] for q in ids], dtype=np.float64)   # get_random_number(ID + i): the sum wraps in uint64
        wraps = np.array([q + i >= U64 for q in ids], dtype=bool)
        pold = np.empty_like(X)
        pnew = np.empty_like(X)
        dnew = np.zeros(len(who))
        dold = np.zeros(len(who))
        for k in range(3):
            pold[:, k] = X[:, k] + st.Reps[i][k] - off[k]
            if mode == "as_written":
                pnew[:, k] = X[:, k] + V[i, k] * ddrift - off[k]
            else:
                pnew[:, k] = X[:, k] + st.Reps[i][k] + V[who, k] * ddrift - off[k]
            dnew += pnew[:, k] * pnew[:, k]
            dold += pold[:, k] * pold[:, k]
        geo = (dold <= H2p) & (dnew >= H2)
        keep = geo & ~(r > frac)                       # "if(r > SampleFraction) continue"
        geometric += int(geo.sum())
        drawn_out += int((geo & ~keep).sum())
        for j in np.flatnonzero(keep):
            if dold[j] != dnew[j]:
                sn, so = np.sqrt(dnew[j]), np.sqrt(dold[j])
                cnew = sn - H
                cold = so - Hp
                u1 = -cold / (cnew - cold)
                u2 = cnew / (cnew - cold)
            else:
                u1 = u2 = 0.5
                half += 1
            wrapped += int(wraps[j])
            p3 = [pold[j, k] * u2 + pnew[j, k] * u1 for k in range(3)] + [frac]
            out.append((int(who[j]), i, p3))
    if not out:
        empty.geometric, empty.drawn_out = geometric, drawn_out
        return empty
    out.sort(key=lambda t: (t[0], t[1]))
    rows = np.array([t[2] for t in out], dtype=np.float64)
    return Rows(rows, np.array([t[0] for t in out], dtype=np.int32), np.array([t[1] for t in out], dtype=np.int32), half, wrapped, geometric, drawn_out)


# ---- the shared cases -------------------------------------------------------------------------------------------------------------------

class Case:
    pass


@functools.lru_cache(maxsize=None)
def case(n, offset=OFFSET):
    """n PARTICLE_DTYPE records, every unused byte noise: positions inside the box that starts at `offset`, types from {0, 1, 1, 1, 4, 5},
    a sixth of the type-1 velocities exactly zero, a few IDs just below 2^64.  Record 0 drifts by TINY: as_written adds that to every
    particle for replica 0, the only replica of (1.20, 1.30) whose unshifted end can reach the horizon, and it changes a coordinate below
    0.5 but none above (half an ulp there is 5.6e-17), so that both dold == dnew and dold != dnew occur"""
    rng = np.random.default_rng([SEED, n, int(offset[0] != 0)])
    c = Case()
    raw = rng.integers(0, 256, size=n * capi.PARTICLE_DTYPE.itemsize, dtype=np.uint8)
    P = raw.view(capi.PARTICLE_DTYPE).copy()
    P["Pos"] = rng.random((n, 3)) * BOXSIZE + np.array(offset)
    P["Vel"] = (2 * rng.random((n, 3)) - 1) * VMAX
    P["Type"] = np.array([0, 1, 1, 1, 4, 5], dtype=np.uint8)[rng.integers(0, 6, size=n)]
    P["ID"] = rng.integers(0, 1 << 63, size=n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=n, dtype=np.uint64)
    ones = np.flatnonzero(P["Type"] == 1)
    still = ones[rng.random(len(ones)) < 1 / 6]
    P["Vel"][still] = 0.0
    if n:
        P["Vel"][0] = TINY / DDRIFT
    near = ones[:: 16][: 1 + n // 16]               # within 1000 of 2^64: ID + i wraps for the later replicas
    P["ID"][near] = np.array([U64 - 1 - int(k) for k in rng.integers(0, 4, size=len(near))], dtype=np.uint64)
    c.n, c.P, c.offset = n, P, tuple(offset)
    c.rnd = np.random.default_rng([SEED, 997]).random(RNDSIZE)
    return c


@functools.lru_cache(maxsize=None)
def expected(n, mode, H, Hprev, fraction, offset):
    """the rows of case(n, offset) under hand_state(H, Hprev, fraction): computed once, shared, not to be changed"""
    c = case(n, offset)
    return cross(c.P, hand_state(H, Hprev, fraction), mode, DDRIFT, offset, c.rnd)


def combos():
    for mode, (H, Hprev), offset in GEOMETRIES:
        for f in FRACTIONS:
            yield mode, H, Hprev, f, offset


def embed(P, itemsize=192):
    """the same particles in `itemsize`-byte records with every member moved, the rest noise: (records, dtype)"""
    dt = np.dtype({"names": ["Type", "ID", "Vel", "Pos"], "formats": ["u1", "<u8", ("<f8", 3), ("<f8", 3)], "offsets": [7, 16, 48, 104], "itemsize": itemsize})
    rng = np.random.default_rng([SEED, itemsize])
    Q = rng.integers(0, 256, size=len(P) * itemsize, dtype=np.uint8).view(dt).copy()
    for f in dt.names:
        Q[f] = P[f]
    return Q, dt
