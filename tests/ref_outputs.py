"""The pieces of the reference that `make -C oracle ref` compiles into oracle/_ref/, or - where they have not been built (no reference
sources on the machine) - the outputs they gave for the inputs the tests use, stored under tests/golden/ by tools/make_ref_golden.py.
tests/test_ref_golden_cpu.py holds the stored outputs to the built pieces wherever both exist."""
import ctypes as C
import hashlib
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFDIR = os.path.join(ROOT, "oracle", "_ref")
GOLD = os.path.join(ROOT, "tests", "golden")

PEANO_LIB = os.path.join(REFDIR, "libpeano_ref.so")
PEANO_GOLD = os.path.join(GOLD, "ref_peano.npz")
LAYOUT_PROBE = os.path.join(REFDIR, "layout_probe")
LAYOUT_GOLD = os.path.join(GOLD, "ref_layout_probe.json")
DENSITYKERNEL_LIB = os.path.join(REFDIR, "libdensitykernel_ref.so")
DENSITYKERNEL_GOLD = os.path.join(GOLD, "ref_densitykernel.npz")
SHORTRANGE_LIB = os.path.join(REFDIR, "libshortrange_ref.so")
SHORTRANGE_GOLD = os.path.join(GOLD, "ref_shortrange_table.json")
HK_BITS = (1, 2, 3)        # ref_peano_hilbert_key tables stored for every (x, y, z) below 2^bits (top trees of depth <= 3)


def peano_lib():
    """ref_peano_hilbert_key / ref_PEANO of oracle/ref_peano_driver.cpp over libgadget/utils/peano.cpp, or None when not built"""
    if not os.path.exists(PEANO_LIB):
        return None
    lib = C.CDLL(PEANO_LIB)
    lib.ref_peano_hilbert_key.restype = C.c_uint64
    lib.ref_peano_hilbert_key.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    lib.ref_PEANO.restype = C.c_uint64
    lib.ref_PEANO.argtypes = [C.c_void_p, C.c_double]
    return lib


def _pos_key(p, box):
    return np.ascontiguousarray(p, dtype=np.float64).tobytes() + np.float64(box).tobytes()


def fingerprint(pos, box):
    """SHA-256 of a position array (float64, row-major) and the box: names the exact inputs a stored case belongs to"""
    return hashlib.sha256(_pos_key(pos, box)).hexdigest()


class Peano:
    """The reference's Peano-Hilbert key: the built library, or what it gave for the tests' inputs.  Stored are ref_peano_hilbert_key
    for coordinates below 2^bits (bits in HK_BITS), ref_PEANO for the few positions whose full keys the tests use (key(); others raise
    KeyError), and, per named case, the top leaf domain_get_topleaf(PEANO(pos)) of every position (topleaves())."""

    def __init__(self, lib=None, gold=None):
        self.lib = lib
        if lib is None:
            g = np.load(gold or PEANO_GOLD)
            self.gold = g
            self.hk = {b: g["hk%d" % b] for b in HK_BITS}
            self.stored = {_pos_key(p, b): int(k) for p, b, k in zip(g["pos"], g["box"], g["key"])}

    def hilbert_key(self, x, y, z, bits):
        if self.lib is not None:
            return int(self.lib.ref_peano_hilbert_key(x, y, z, bits))
        return int(self.hk[bits][x, y, z])

    def key(self, p, box):
        if self.lib is not None:
            return int(self.lib.ref_PEANO(np.ascontiguousarray(p, dtype=np.float64).ctypes.data, box))
        try:
            return self.stored[_pos_key(p, box)]
        except KeyError:
            raise KeyError("no stored reference key for position %r (box %r): rebuild oracle/_ref or rerun tools/make_ref_golden.py"
                           % (tuple(p), box)) from None

    def keys(self, pos, box):
        return np.array([self.key(p, box) for p in np.asarray(pos)], dtype=np.uint64)

    def topleaves(self, case, pos, box, leaf_of_key):
        """leaf_of_key(PEANO(p)) for every p in pos (leaf_of_key: domain_get_topleaf over the case's top tree); without the library,
        the stored leaves of `case`, which must be for exactly these positions"""
        if self.lib is not None:
            return np.array([leaf_of_key(self.key(p, box)) for p in np.asarray(pos)], dtype=np.int32)
        fp = fingerprint(pos, box)
        assert str(self.gold["fp_" + case]) == fp, \
            "positions of case %r differ from the stored ones: rebuild oracle/_ref or rerun tools/make_ref_golden.py" % case
        return self.gold["leaf_" + case].astype(np.int32)


def peano():
    """the built library when there is one, else the stored keys"""
    lib = peano_lib()
    return Peano(lib=lib) if lib is not None else Peano()


def peano_store(peano):
    """What tests/golden/ref_peano.npz holds, computed with `peano` (the built library): the hilbert_key tables, full keys of the
    golden-key and slot-GC positions, and the top leaves of the geometric-descent and top-leaf-maintenance cases"""
    import common as cm
    import test_exchange_cpu as tex
    import test_gpu_dynamics as tdyn
    import test_gpu_toptree_build as ttb
    import test_peano_ref_cpu as tp
    out = {}
    for b in HK_BITS:
        m = 1 << b
        out["hk%d" % b] = np.array([[[peano.hilbert_key(x, y, z, b) for z in range(m)] for y in range(m)] for x in range(m)], dtype=np.uint64)
    P, numpart, _, _ = tex.gc_sorted_setup(np.random.default_rng(5))
    sets = [(tp.golden_positions(), 4.0), (P["Pos"][:numpart], 25000.0)]
    out["pos"] = np.concatenate([np.asarray(p, dtype=np.float64).reshape(-1, 3) for p, _ in sets])
    out["box"] = np.concatenate([np.full(len(p), b) for p, b in sets])
    out["key"] = np.array([peano.key(p, b) for p, b in zip(out["pos"], out["box"])], dtype=np.uint64)
    cases = []
    for seed in tp.DESCENT_SEEDS:
        nodes, pos = tp.descent_case(seed)
        cases.append(("descent%d" % seed, pos, cm.BOX, nodes))
    nodes, _, _, _, pos_all, _, _, pman = ttb.topleaf_case(peano)
    drifted, _ = tdyn.ref_drift(pman.Base, ttb.TOPLEAF_DRIFT, cm.BOX, 0.0)   # what shq_drift gives, bit for bit (test_drift_bit_exact)
    cases += [("topleaf_initial", pos_all, cm.BOX, nodes), ("topleaf_drifted", drifted, cm.BOX, nodes)]
    for name, pos, box, nodes in cases:
        leaves = peano.topleaves(name, pos, box, lambda k, nodes=nodes: tp.domain_get_topleaf(k, nodes))
        assert leaves.min() >= 0 and leaves.max() < 1 << 16
        out["leaf_" + name] = leaves.astype(np.uint16)
        out["fp_" + name] = np.array(fingerprint(pos, box))
    return out


def layout():
    """what oracle/_ref/layout_probe prints (the reference's struct layouts), or the stored copy of it"""
    if os.path.exists(LAYOUT_PROBE):
        import subprocess
        return json.loads(subprocess.check_output([LAYOUT_PROBE]).decode())
    return json.load(open(LAYOUT_GOLD))


def densitykernel_lib():
    if not os.path.exists(DENSITYKERNEL_LIB):
        return None
    lib = C.CDLL(DENSITYKERNEL_LIB)
    lib.ref_density_kernel.argtypes = [C.c_int, C.c_double, C.c_double, C.c_double, C.c_void_p]
    return lib


def densitykernel_args():
    """the draws of test_oracle_cpu.py::test_density_kernel_vs_reference_build: (ktype, H, u, eta) rows"""
    rng = np.random.default_rng(7)
    rows = []
    for ktype in (1, 2, 4):
        for _ in range(200):
            H, u, eta = rng.uniform(0.01, 5), rng.uniform(0, 1.05), rng.uniform(0.5, 2)
            rows.append((ktype, H, u, eta))
    return rows


def densitykernel_outputs(lib=None):
    """(desnumngb, volume, wk, dwk, dW) of the reference's kernels for densitykernel_args(): computed by the built library when
    there is one, else the stored values"""
    lib = lib if lib is not None else densitykernel_lib()
    if lib is None:
        return np.load(DENSITYKERNEL_GOLD)["out"]
    out = np.zeros((len(densitykernel_args()), 5))
    for i, (ktype, H, u, eta) in enumerate(densitykernel_args()):
        assert lib.ref_density_kernel(ktype, H, u, eta, out[i].ctypes.data) == 0
    return out


def shortrange_table_lib():
    """the reference's tabulated TreePM window (shortrange-kernel.c compiled as it lies), or None when not built"""
    if not os.path.exists(SHORTRANGE_LIB):
        return None
    ref = C.CDLL(SHORTRANGE_LIB)
    arr = (C.c_double * (512 * 5)).in_dll(ref, "shortrange_force_kernels")
    return np.frombuffer(arr, dtype=np.float64).reshape(512, 5).copy()


def table_digest(tab):
    tab = np.ascontiguousarray(tab, dtype="<f8")
    return {"shape": list(tab.shape), "sha256": hashlib.sha256(tab.tobytes()).hexdigest()}


def shortrange_table_digest():
    """shape and SHA-256 of the reference's table: from the built library when there is one, else the stored digest"""
    tab = shortrange_table_lib()
    return table_digest(tab) if tab is not None else json.load(open(SHORTRANGE_GOLD))
