"""shenqi_amd — MI355X-native TreePM + SPH force engine behind shenqi's operator API.

Thin Python driver over two native libraries:
  lib/libshenqi_hip.so   hand-written HIP (gfx950) kernels + the C-ABI (include/shenqi_hip.h)
  lib/libshenqi_host.so  C++ host mirror of the reference operator interface
                         (force_tree_full, grav_short_tree, gravpm_force, ...)
Names follow the reference (libgadget/gravity.h, forcetree.h, partmanager.h).
"""
import ctypes as C

import numpy as np

from . import capi
from .capi import (PARTICLE_DTYPE, SPH_DTYPE, NODE_DTYPE, WALK_EXACT, WALK_GROUP, WALK_AUTO, WALK_TREE_ORDER, WALK_DEFER_POSTPROCESS, GravParams, PMParams,
                   WalkStats, ShqError)

GASMASK, DMMASK, NUMASK, STARMASK, BHMASK = 1, 2, 4, 16, 32
ALLMASK = (1 << 6) - 1
SHORTRANGE_FORCE_WINDOW_TYPE_EXACT = 1
SHORTRANGE_FORCE_WINDOW_TYPE_ERFC = 2


class Context:
    """One library context per rank / GPU (shq_init)."""

    def __init__(self, device=0, stream=None):
        h = C.c_void_p()
        capi.check(capi.hip.shq_init(device, stream, C.byref(h)), "shq_init")
        self.h = h
        self.stream = stream        # the caller's stream the library works on (None: its own)

    def close(self):
        if self.h:
            capi.hip.shq_shutdown(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def synchronize(self):
        capi.check(capi.hip.shq_synchronize(self.h), "shq_synchronize")

    def timer_begin(self, slot):
        capi.check(capi.hip.shq_timer_begin(self.h, slot))

    def timer_end(self, slot):
        capi.check(capi.hip.shq_timer_end(self.h, slot))

    def timer_ms(self, slot):
        ms = C.c_double()
        capi.check(capi.hip.shq_timer_elapsed_ms(self.h, slot, C.byref(ms)))
        return ms.value


class PartManager:
    """PartManager[1] of the reference: a particle_data array plus NumPart / BoxSize."""

    def __init__(self, numpart, BoxSize):
        self.Base = np.zeros(int(numpart), dtype=PARTICLE_DTYPE)
        self.NumPart = int(numpart)
        self.BoxSize = float(BoxSize)
        self._h = capi.host.shqh_partmanager_create(capi.ptr(self.Base), self.NumPart, self.BoxSize)

    def __del__(self):
        if getattr(self, "_h", None) and capi is not None:   # capi is None when the interpreter is shutting down
            capi.host.shqh_partmanager_free(self._h)
            self._h = None

    def view(self):
        v = capi.PartView()
        capi.host.shqh_part_view(self._h, C.byref(v))
        return v


class ForceTree:
    def __init__(self, handle, pman):
        self._h = handle
        self._pman = pman  # keep the particles alive
        info = (C.c_int64 * 5)()
        capi.host.shqh_tree_info(handle, C.byref(info))
        self.firstnode, self.lastnode, self.numnodes, self.NumParticles, self.full_particle_tree_flag = [int(x) for x in info]
        self.BoxSize = pman.BoxSize

    @property
    def Nodes_base(self):
        p = capi.host.shqh_tree_nodes(self._h)
        buf = (C.c_char * (self.numnodes * 120)).from_address(p)
        return np.frombuffer(buf, dtype=NODE_DTYPE)

    def view(self):
        v = capi.TreeView()
        capi.host.shqh_tree_view(self._h, C.byref(v))
        return v

    def free(self):
        if self._h:
            capi.host.shqh_force_tree_free(self._h)
            self._h = None

    def __del__(self):
        self.free()


def force_tree_rebuild_mask(pman, mask, active=None, full=False):
    act = None if active is None else np.ascontiguousarray(active, dtype=np.int32)
    h = capi.host.shqh_force_tree_rebuild_mask(pman._h, mask, capi.ptr(act), 0 if act is None else len(act), int(full))
    if not h:
        raise ShqError(capi.host.shqh_last_error().decode())
    return ForceTree(h, pman)


def tree_build_device(ctx, BoxSize, mask=None, active=None):
    """shq_tree_build: build the tree of the uploaded particles on the device and install it in `ctx`.
    Returns capi.TreeBuildStats."""
    st = capi.TreeBuildStats()
    act, nact = _active_arg(active)
    capi.check(capi.hip.shq_tree_build(ctx.h, float(BoxSize), ALLMASK if mask is None else int(mask), act, nact, C.byref(st)),
               "shq_tree_build")
    return st


def set_tree_debug(ctx, initial_node_cap=0):
    """shq_set_tree_debug: node pool of the first build attempt (0: the default formula); small values force the retry path."""
    capi.check(capi.hip.shq_set_tree_debug(ctx.h, int(initial_node_cap)), "shq_set_tree_debug")


def tree_build_attempts(ctx):
    """shq_tree_build_attempts: attempts the last device tree build made (1 = the first node pool was enough)."""
    a = C.c_int(0)
    capi.check(capi.hip.shq_tree_build_attempts(ctx.h, C.byref(a)), "shq_tree_build_attempts")
    return a.value


def tree_build_domain(ctx, BoxSize, geo, topleaves, ThisTask, firstnode, mask=None, active=None):
    """shq_tree_build_domain: the device tree under a domain decomposition.  geo: capi.TOPNODE_GEO_DTYPE array, topleaves:
    capi.TOPLEAF_DTYPE array (Task read, treenode written).  Returns (stats, local moments as capi.TOPLEAF_MOMENTS_DTYPE)."""
    st = capi.TreeBuildStats()
    act, nact = _active_arg(active)
    geo = np.ascontiguousarray(geo, dtype=capi.TOPNODE_GEO_DTYPE)
    assert topleaves.dtype == capi.TOPLEAF_DTYPE and topleaves.flags["C_CONTIGUOUS"]
    mom = np.zeros(len(topleaves), dtype=capi.TOPLEAF_MOMENTS_DTYPE)
    capi.check(capi.hip.shq_tree_build_domain(ctx.h, float(BoxSize), ALLMASK if mask is None else int(mask), act, nact, capi.ptr(geo), len(geo),
                                              capi.ptr(topleaves), len(topleaves), int(ThisTask), int(firstnode), capi.ptr(mom), C.byref(st)),
               "shq_tree_build_domain")
    return st, mom


def tree_set_topleaf_moments(ctx, moments):
    """shq_tree_set_topleaf_moments: the all-gathered top-leaf moments (capi.TOPLEAF_MOMENTS_DTYPE) into the pseudo nodes."""
    moments = np.ascontiguousarray(moments, dtype=capi.TOPLEAF_MOMENTS_DTYPE)
    capi.check(capi.hip.shq_tree_set_topleaf_moments(ctx.h, capi.ptr(moments), len(moments)), "shq_tree_set_topleaf_moments")


RESIDENT = "resident"        # the list of the last build_active_particles (SHQ_ACTIVE_RESIDENT)
RESIDENT_SUB = "resident-sub"  # the list of the last build_active_sublist (SHQ_SUBLIST_RESIDENT)


def _active_arg(active):
    """(pointer, count) for the `active` argument of the C-ABI: None, a host index list or a resident handle."""
    if active is None:
        return None, 0
    if isinstance(active, str):
        return {RESIDENT: capi.ACTIVE_RESIDENT, RESIDENT_SUB: capi.SUBLIST_RESIDENT}[active], 0
    act = np.ascontiguousarray(active, dtype=np.int32)
    _active_arg.keep = act
    return capi.ptr(act), len(act)


def toptree_upload(ctx, tree, topleaves):
    """shq_toptree_upload: the TopLevel nodes of the host tree + the domain's TopLeaves (capi.TOPLEAF_DTYPE)."""
    tl = np.ascontiguousarray(topleaves, dtype=capi.TOPLEAF_DTYPE)
    tv = tree.view()
    capi.check(capi.hip.shq_toptree_upload(ctx.h, C.byref(tv), capi.ptr(tl), len(tl)), "shq_toptree_upload")


def _toptree_exports(call, ntargets, active):
    """One call with a generous table; a second, exactly sized one only if that was too small."""
    act, nact = _active_arg(active)
    counts = np.zeros(ntargets, dtype=np.int32)
    n = C.c_int64()
    cap = max(1024, ntargets // 4)
    table = np.zeros(cap, dtype=capi.DATA_INDEX_DTYPE)
    rc = call(act, nact, capi.ptr(counts), capi.ptr(table), cap, C.byref(n))
    if rc != 0 and n.value > cap:
        table = np.zeros(n.value, dtype=capi.DATA_INDEX_DTYPE)
        rc = call(act, nact, capi.ptr(counts), capi.ptr(table), n.value, C.byref(n))
    capi.check(rc, "toptree exports")
    return counts, table[: n.value].copy()


def grav_toptree_exports(ctx, gp, ntargets, active=None):
    """shq_grav_toptree_exports: (exportcounts [ntargets] inclusive scan, DataIndexTable) of
    GravTopTreeWalk::toptree_visit (libgadget/gravshort2.hpp:362-438)."""
    return _toptree_exports(lambda a, na, cnt, tab, cap, n: capi.hip.shq_grav_toptree_exports(ctx.h, C.byref(gp), a, na, cnt, tab, cap, n),
                            ntargets, active)


def ngb_toptree_exports(ctx, symmetric, BoxSize, ntargets, active=None):
    """shq_ngb_toptree_exports: TopTreeWalk::toptree_visit with cull_node (libgadget/localtreewalk2.h:210-259)."""
    return _toptree_exports(lambda a, na, cnt, tab, cap, n: capi.hip.shq_ngb_toptree_exports(ctx.h, int(symmetric), float(BoxSize), a, na, cnt, tab,
                                                                                           cap, n), ntargets, active)


def timebins_upload(ctx, bin_gravity=None, bin_hydro=None):
    bg = None if bin_gravity is None else np.ascontiguousarray(bin_gravity, dtype=np.uint8)
    bh = None if bin_hydro is None else np.ascontiguousarray(bin_hydro, dtype=np.uint8)
    capi.check(capi.hip.shq_timebins_upload(ctx.h, capi.ptr(bg), capi.ptr(bh)), "shq_timebins_upload")


def build_active_particles(ctx, Ti_Current, is_pm_step=False):
    """shq_build_active_particles: build_active_particles (libgadget/timestep.cpp:1286-1349) on the device.
    Returns capi.ActiveInfo; the list stays resident (pass active=RESIDENT)."""
    info = capi.ActiveInfo()
    capi.check(capi.hip.shq_build_active_particles(ctx.h, int(Ti_Current), int(bool(is_pm_step)), C.byref(info)),
               "shq_build_active_particles")
    return info


def build_active_sublist(ctx, maxtimebin, Ti_Current):
    """shq_build_active_sublist: build_active_sublist (libgadget/timestep.cpp:1373-1399). Returns its length."""
    n = C.c_int64()
    capi.check(capi.hip.shq_build_active_sublist(ctx.h, int(maxtimebin), int(Ti_Current), C.byref(n)), "shq_build_active_sublist")
    return n.value


def active_download(ctx, sublist=False):
    n = C.c_int64()
    capi.check(capi.hip.shq_active_download(ctx.h, int(sublist), None, 0, C.byref(n)), "shq_active_download")
    out = np.zeros(n.value, dtype=np.int32)
    capi.check(capi.hip.shq_active_download(ctx.h, int(sublist), capi.ptr(out), n.value, C.byref(n)), "shq_active_download")
    return out


def tree_download(ctx, firstnode, numpart=0):
    """shq_tree_download: the device-built tree as a NODE array (numbered from `firstnode` in pre-order)
    and, if numpart > 0, the Father array."""
    nn = C.c_int64()
    capi.check(capi.hip.shq_tree_download(ctx.h, int(firstnode), None, 0, None, C.byref(nn)), "shq_tree_download")
    nodes = np.zeros(nn.value, dtype=NODE_DTYPE)
    father = np.full(int(numpart), -1, dtype=np.int32) if numpart > 0 else None
    capi.check(capi.hip.shq_tree_download(ctx.h, int(firstnode), capi.ptr(nodes), nn.value, capi.ptr(father), C.byref(nn)),
               "shq_tree_download")
    return nodes, father


def dynamics_upload(ctx, pman):
    pv = pman.view()
    capi.check(capi.hip.shq_dynamics_upload(ctx.h, C.byref(pv)), "shq_dynamics_upload")


def drift(ctx, ddrift, BoxSize, random_shift=None):
    """shq_drift: drift_all_particles (libgadget/drift.cpp:16-99) on the resident particles."""
    rs = None if random_shift is None else np.ascontiguousarray(random_shift, dtype=np.float64)
    capi.check(capi.hip.shq_drift(ctx.h, float(ddrift), float(BoxSize), capi.ptr(rs)), "shq_drift")


def kick_short(ctx, gravkick, active=None, from_accel_store=False):
    """shq_kick_short: gravity part of apply_half_kick (libgadget/timestep.cpp:838-872)."""
    gk = np.ascontiguousarray(gravkick, dtype=np.float64)
    assert gk.shape == (capi.TIMEBINS + 1,)
    act, nact = _active_arg(active)
    capi.check(capi.hip.shq_kick_short(ctx.h, capi.ptr(gk), act, nact, int(from_accel_store)), "shq_kick_short")


def kick_hydro(ctx, hydrokick, dt_entr, atime, MaxGasVel, active=None, from_hydro_output=True):
    """shq_kick_hydro: do_hydro_kick for gas (libgadget/timestep.cpp:970-1003). Returns the number of clamped particles."""
    hk = np.ascontiguousarray(hydrokick, dtype=np.float64)
    de = np.ascontiguousarray(dt_entr, dtype=np.float64)
    assert hk.shape == (capi.TIMEBINS + 1,) and de.shape == (capi.TIMEBINS + 1,)
    act, nact = _active_arg(active)
    nlim = C.c_int64()
    capi.check(capi.hip.shq_kick_hydro(ctx.h, capi.ptr(hk), capi.ptr(de), float(atime), float(MaxGasVel), act, nact, int(from_hydro_output),
                                       C.byref(nlim)), "shq_kick_hydro")
    return nlim.value


def entropy_download(ctx, n):
    out = np.zeros(n)
    capi.check(capi.hip.shq_entropy_download(ctx.h, capi.ptr(out)), "shq_entropy_download")
    return out


def kick_pm(ctx, Fgravkick):
    """shq_kick_pm: apply_PM_half_kick (libgadget/timestep.cpp:937-959)."""
    capi.check(capi.hip.shq_kick_pm(ctx.h, float(Fgravkick)), "shq_kick_pm")


def dynamics_download(ctx, pman):
    pv = pman.view()
    capi.check(capi.hip.shq_dynamics_download(ctx.h, C.byref(pv)), "shq_dynamics_download")


def force_tree_full(pman):
    return force_tree_rebuild_mask(pman, ALLMASK, None, full=True)


def set_gravshort_treepar(ErrTolForceAcc=0.002, BHOpeningAngle=0.175, MaxBHOpeningAngle=0.9, TreeUseBH=2, Rcut=6.0,
                          FractionalGravitySoftening=1.0 / 30.0, ShortRangeForceWindowType=SHORTRANGE_FORCE_WINDOW_TYPE_EXACT):
    capi.host.shqh_set_gravshort_treepar(ErrTolForceAcc, BHOpeningAngle, MaxBHOpeningAngle, TreeUseBH, Rcut,
                                         FractionalGravitySoftening, ShortRangeForceWindowType)


def get_TreeUseBH():
    return capi.host.shqh_get_TreeUseBH()


def gravshort_set_softenings(MeanSeparation):
    capi.host.shqh_gravshort_set_softenings(MeanSeparation)


def FORCE_SOFTENING():
    return capi.host.shqh_FORCE_SOFTENING()


def make_grav_params(BoxSize, Asmth, Nmesh, G, rho0):
    gp = GravParams()
    capi.check_host(capi.host.shqh_make_grav_params(BoxSize, Asmth, Nmesh, G, rho0, C.byref(gp)), "make_grav_params")
    return gp


def grav_short_tree(ctx, act, pm, tree, AccelStore, rho0, Ti_Current=0, UseGPU=True, walk_mode=WALK_EXACT, pman=None):
    """grav_short_tree(act, pm, tree, AccelStore, rho0, Ti_Current, UseGPU), libgadget/gravity.h:89.
    act: int32 index array or None (all). pm: dict(Asmth, Nmesh, G). Returns WalkStats."""
    pman = pman or tree._pman
    stats = WalkStats()
    a = None if act is None else np.ascontiguousarray(act, dtype=np.int32)
    rc = capi.host.shqh_grav_short_tree(ctx.h, pman._h, tree._h, pm["Asmth"], pm["Nmesh"], pm["G"], capi.ptr(a),
                                        0 if a is None else len(a), capi.ptr(AccelStore), rho0, int(UseGPU), walk_mode,
                                        C.byref(stats))
    capi.check_host(rc, "grav_short_tree")
    return stats


def gravpm_force(ctx, pm, pman, UseGPU=True, analysis=None, deposit_types=capi.ALL_TYPES):
    """analysis(kk, power, nmodes, Norm) -> T: the hook between the PM's forward and inverse halves (petapm's global_analysis,
    compute_neutrino_power for MassiveNuLinRespOn); it gets the raw P(k) sums of the density and returns T[k2] for k2 = 0 .. 3 (Nmesh/2)^2.
    A NuLRA with its times set (nu.at(Time, TimeIC)) is such a hook: the resident linear-response state steps on the sums.
    deposit_types: the deposit's type mask (bit t = Type t)."""
    if analysis is None and deposit_types == capi.ALL_TYPES:
        capi.check_host(capi.host.shqh_gravpm_force(ctx.h, pman._h, pm["Asmth"], pm["Nmesh"], pm["G"], int(UseGPU)), "gravpm_force")
        return

    def hook(_, nbins, kk, power, nmodes, norm, nmesh, table):
        try:
            T = analysis(np.ctypeslib.as_array(kk, (nbins,)).copy(), np.ctypeslib.as_array(power, (nbins,)).copy(),
                         np.ctypeslib.as_array(nmodes, (nbins,)).copy(), norm)
            np.ctypeslib.as_array(table, (3 * (nmesh // 2) ** 2 + 1,))[:] = T
            return 0
        except Exception:
            return 1

    fn = capi.GRAVPM_ANALYSIS_FN(hook) if analysis is not None else capi.GRAVPM_ANALYSIS_FN()
    capi.check_host(capi.host.shqh_gravpm_force_hook(ctx.h, pman._h, pm["Asmth"], pm["Nmesh"], pm["G"], int(UseGPU), fn, None,
                                                     int(deposit_types)), "gravpm_force")


def calculate_uvbg(ctx, pman, params, cosmo, fesc, sfr, local_J21, zreion, keep_grids=False):
    """calculate_uvbg (uvbg.cpp:509-597) for one rank on the device.  params: capi.UvbgParams (UVBGParams and BoxSize), cosmo:
    capi.UvbgCosmo (Time, the cosmology's scalars, hubble_function(CP, Time), units).  fesc (in / out), sfr (read with
    ReionUseParticleSFR; may be None otherwise), local_J21 (out) and zreion (in / out) are float64 arrays of NumPart: the EXCUR_REION
    fields of each particle's gas or star slot.  Returns (volume-weighted xHI, mass-weighted xHI, number of radii), UVBGgrids' globals;
    with keep_grids also the J21 and xHI grids, float32 [UVBGdim]^3, as save_uvbg_grids writes them."""
    n = pman.NumPart
    arrs = [fesc, sfr, local_J21, zreion]
    for a in arrs:
        if a is not None and (a.dtype != np.float64 or a.shape != (n,) or not a.flags["C_CONTIGUOUS"]):
            raise ValueError("fesc, sfr, local_J21 and zreion are contiguous float64 arrays of NumPart")
    pv = pman.view()
    res = capi.UvbgResult()
    capi.check(capi.hip.shq_uvbg_keep_grids(ctx.h, int(bool(keep_grids))), "shq_uvbg_keep_grids")
    try:
        capi.check(capi.hip.shq_uvbg_calculate(ctx.h, C.byref(params), C.byref(cosmo), C.byref(pv), *[capi.ptr(a) for a in arrs],
                                               C.byref(res)), "calculate_uvbg")
        out = (res.volume_weighted_global_xHI, res.mass_weighted_global_xHI, res.nradii)
        if keep_grids:
            N = params.UVBGdim
            J21 = np.empty((N, N, N), dtype=np.float32)
            xHI = np.empty((N, N, N), dtype=np.float32)
            capi.check(capi.hip.shq_uvbg_download_grids(ctx.h, N, capi.ptr(J21), capi.ptr(xHI)), "shq_uvbg_download_grids")
            out += (J21, xHI)
    finally:
        if keep_grids:
            capi.check(capi.hip.shq_uvbg_keep_grids(ctx.h, 0), "shq_uvbg_keep_grids")
    return out


def heiii_reionization(ctx, pman, SphP, params, rnd_table, gas_tree=None, log_capacity=None):
    """turn_on_quasars (cooling_qso_lightup.cpp:489-596) for one rank on the device, on the resident FOF catalogue (shq_fof first).
    params: capi.HeiiiParams; SphP: the gas slots (SPH_DTYPE, Density and Entropy read through PI); rnd_table: RandTable::Table as
    float64; gas_tree: the GASMASK | BHMASK ForceTree, needed when var_bubble > 0.  Ionised particles get the HeIIIionized bit and their
    heating in pman.Base and SphP.  Returns (capi.HeiiiResult, the FdHelium lines as a HEIII_QUASAR_DTYPE array)."""
    rnd = np.ascontiguousarray(rnd_table, dtype=np.float64)
    pv, sv = pman.view(), capi.sph_view(SphP)
    tv = gas_tree.view() if gas_tree is not None else None
    res = capi.HeiiiResult()
    nlog = C.c_int64()
    cap = int(log_capacity) if log_capacity is not None else 0
    if log_capacity is None:   # the draws are bounded by the candidate count, which only the call knows: ask it once with room for all
        cap = 1 << 20
    log = np.zeros(cap, dtype=capi.HEIII_QUASAR_DTYPE)
    capi.check(capi.hip.shq_heiii_reionization(ctx.h, C.byref(params), C.byref(pv), C.byref(sv), C.byref(tv) if tv is not None else None,
                                               capi.ptr(rnd), len(rnd), capi.ptr(log), cap, C.byref(nlog), C.byref(res)),
               "heiii_reionization")
    if nlog.value > cap:
        raise ShqError(f"heiii_reionization: {nlog.value} FdHelium lines, room for {cap}")
    return res, log[:nlog.value].copy()


def heiii_host_numbers(params, minids, rnd_table):
    """The numbers of the quasar loop that must be glibc's (host only): gaussian_rng's bubble radius per MinID (cooling_qso_lightup.cpp:
    249-255) and non_overlapping_bubble_number (:514-518), from the functions shq_heiii_reionization itself uses.  The phases of the
    same operator (shq_heiii_open / _sweep / _commit / _close) are driven by dist.DistHeIII with dist.GpuHeiiiOps."""
    rnd = np.ascontiguousarray(rnd_table, dtype=np.float64)
    minids = np.ascontiguousarray(minids, dtype=np.uint64)
    radii = np.zeros(len(minids))
    nn = C.c_int64()
    capi.check(capi.hip.shq_heiii_host_numbers(C.byref(params), capi.ptr(minids), len(minids), capi.ptr(rnd), len(rnd), capi.ptr(radii), C.byref(nn)),
               "heiii_host_numbers")
    return radii, nn.value


def lens_count_active(ctx, pman, exclude_type2=False):
    """plane_count_active_particles' local count (plane.cpp:72-83) on the device: not Swallowed, not Type 2 under exclude_type2"""
    pv = pman.view()
    out = C.c_int64()
    capi.check(capi.hip.shq_lens_count_active(ctx.h, C.byref(pv), int(bool(exclude_type2)), C.byref(out)), "lens_count_active")
    return out.value


def lens_planes(ctx, pman, Resolution, Normals, CutPoints=None, Thickness=0.0, CurrentParticleOffset=(0.0, 0.0, 0.0), exclude_type2=False,
                atime=1.0, comoving_distance=1.0, HubbleParam=0.7, omega_source=0.3, num_particles_tot=None, nu=None, counts=True):
    """write_plane's compute (plane.cpp:565-588) for one rank on the device: every (cut, normal) potential plane in one call.
    CutPoints None or empty: the default list (0.5 + i) Thickness; Thickness <= 0: BoxSize.  num_particles_tot None: this rank's
    active count (one rank).  nu: None, or dict(Nmesh, x0, real [nx][Nmesh][Nmesh] float64, inv_fft_norm, mean_mass_cell), the rank's
    x-slab of the PM neutrino correction mesh.  Returns (planes [ncuts][nnormals][R][R] float64, num_particles_plane [ncuts][nnormals]
    int64, counts [ncuts][nnormals][R][R] uint32 or None)."""
    normals = np.ascontiguousarray(Normals, dtype=np.int32)
    cuts = np.ascontiguousarray([] if CutPoints is None else CutPoints, dtype=np.float64)
    lp = capi.LensParams()
    lp.Resolution, lp.ncuts, lp.nnormals, lp.exclude_type2 = int(Resolution), len(cuts), len(normals), int(bool(exclude_type2))
    lp.CutPoints, lp.Normals = capi.ptr(cuts) if len(cuts) else None, capi.ptr(normals) if len(normals) else None
    lp.Thickness, lp.BoxSize = float(Thickness), pman.BoxSize
    lp.CurrentParticleOffset[:] = [float(x) for x in CurrentParticleOffset]
    if num_particles_tot is None:
        num_particles_tot = lens_count_active(ctx, pman, exclude_type2)
    lc = capi.LensCosmo(float(atime), float(comoving_distance), float(HubbleParam), float(omega_source), int(num_particles_tot))
    nm = None
    if nu is not None:
        real = np.ascontiguousarray(nu["real"], dtype=np.float64)
        nm = capi.LensNuMesh(int(nu["Nmesh"]), int(nu["x0"]), real.shape[0] if real.ndim == 3 else 0, 0, float(nu["inv_fft_norm"]),
                             float(nu["mean_mass_cell"]), real.ctypes.data_as(C.c_void_p))
        if real.ndim != 3 or real.shape[1:] != (nm.Nmesh, nm.Nmesh):
            raise ValueError("nu['real'] must be [nx][Nmesh][Nmesh]")
    nc = C.c_int32()
    capi.check(capi.hip.shq_lens_num_cuts(C.byref(lp), C.byref(nc)), "lens_planes")
    R = max(int(Resolution), 0)
    planes = np.zeros((nc.value, len(normals), R, R))
    npl = np.zeros((nc.value, len(normals)), dtype=np.int64)
    cnt = np.zeros((nc.value, len(normals), R, R), dtype=np.uint32) if counts else None
    pv = pman.view()
    capi.check(capi.hip.shq_lens_planes(ctx.h, C.byref(lp), C.byref(lc), C.byref(pv), C.byref(nm) if nm is not None else None,
                                        capi.ptr(planes), capi.ptr(npl), capi.ptr(cnt)), "lens_planes")
    return planes, npl, cnt


def cosmic_time_table(hubble_function, amin, amax, n, UnitTime_in_s, SEC_PER_MEGAYEAR=3.155e13):
    """The table shq_yields_init takes in place of atime_to_myr (metal_return.cpp:170-178): n nodes uniform in ln a over [amin, amax];
    dTdloga = UnitTime_in_s / SEC_PER_MEGAYEAR / hubble_function(a), T = its integral from the first node (scipy's quad, node to node).
    Returns (loga0, dloga, T, dTdloga)."""
    from scipy.integrate import quad
    loga0, dloga = np.log(amin), (np.log(amax) - np.log(amin)) / (n - 1)
    fac = UnitTime_in_s / SEC_PER_MEGAYEAR
    lna = loga0 + dloga * np.arange(n)
    dT = np.array([fac / hubble_function(np.exp(x)) for x in lna])
    steps = [quad(lambda x: fac / hubble_function(np.exp(x)), lna[k], lna[k + 1], epsrel=1e-13, epsabs=0)[0] for k in range(n - 1)]
    return float(loga0), float(dloga), np.concatenate([[0.0], np.cumsum(steps)]), dT


def yields_init(ctx, tables, time_table, Sn1aN0, HubbleParam, imf_norm, MAXMASS=None, SNAGBSWITCH=None):
    """shq_yields_init: upload the caller's yield tables (a mapping with the array names of libgadget/metal_tables.h, each laid out as
    there) and cosmic-time table (loga0, dloga, T, dTdloga); returns maxmassfrac (metal_return.cpp:425)."""
    a = {k: np.ascontiguousarray(tables[k], dtype=np.float64) for k in (
        "lifetime_metallicity", "lifetime_masses", "lifetime", "agb_metallicities", "agb_masses", "agb_total_mass", "agb_total_metals", "agb_yield",
        "snii_metallicities", "snii_masses", "snii_total_mass", "snii_total_metals", "snii_yield", "sn1a_yields")}
    yt = capi.YieldTables()
    yt.life_nmet, yt.life_nmass = len(a["lifetime_metallicity"]), len(a["lifetime_masses"])
    yt.agb_nmet, yt.agb_nmass = len(a["agb_metallicities"]), len(a["agb_masses"])
    yt.snii_nmet, yt.snii_nmass = len(a["snii_metallicities"]), len(a["snii_masses"])
    if (a["lifetime"].size != yt.life_nmet * yt.life_nmass or a["agb_total_mass"].size != yt.agb_nmet * yt.agb_nmass
            or a["agb_total_metals"].size != a["agb_total_mass"].size or a["snii_total_mass"].size != yt.snii_nmet * yt.snii_nmass
            or a["snii_total_metals"].size != a["snii_total_mass"].size or a["agb_yield"].size != len(a["sn1a_yields"]) * a["agb_total_mass"].size
            or a["snii_yield"].size != len(a["sn1a_yields"]) * a["snii_total_mass"].size):
        raise ValueError("yields_init: table sizes do not match their axes")
    for k, v in a.items():
        if k != "sn1a_yields":
            setattr(yt, k, v.ctypes.data)
    yt.nmetals, yt.sn1a_total_metals, yt.sn1a_yields = len(a["sn1a_yields"]), float(np.asarray(tables["sn1a_total_metals"]).ravel()[0]), a["sn1a_yields"].ctypes.data
    loga0, dloga, T, dT = time_table
    T, dT = np.ascontiguousarray(T, dtype=np.float64), np.ascontiguousarray(dT, dtype=np.float64)
    if len(T) != len(dT):
        raise ValueError("yields_init: T and dTdloga differ in length")
    ct = capi.CosmicTimeTable(len(T), float(loga0), float(dloga), T.ctypes.data, dT.ctypes.data)
    yp = capi.YieldParams(float(Sn1aN0), float(HubbleParam), float(imf_norm), float(np.asarray(tables["MAXMASS"] if MAXMASS is None else MAXMASS).ravel()[0]),
                          float(np.asarray(tables["SNAGBSWITCH"] if SNAGBSWITCH is None else SNAGBSWITCH).ravel()[0]))
    mmf = C.c_double()
    capi.check(capi.hip.shq_yields_init(ctx.h, C.byref(yt), C.byref(ct), C.byref(yp), C.byref(mmf)), "yields_init")
    return mmf.value


def metal_yields(ctx, pman, StarP, atime, active=None, out=None):
    """metal_return_init + the yields of metal_return_copy (metal_return.cpp:410-462, 539-569) on the device: shq_metal_yields.
    StarP: the star slots (capi.STAR_DTYPE; LastEnrichmentMyr is rewritten where the reference does).  Returns a dict: StellarAges,
    LowDyingMass, HighDyingMass, MassReturn by star slot (`out`, a dict of such arrays, is updated in place where given: slots of stars
    outside the list keep their values), queue (particle indices, active-list order), MassGenerated, MetalGenerated,
    MetalSpeciesGenerated by queue position."""
    act = None if active is None else np.ascontiguousarray(active, dtype=np.int32)
    cnt = pman.NumPart if act is None else len(act)
    r = {k: (out[k] if out is not None else np.zeros(len(StarP))) for k in ("StellarAges", "LowDyingMass", "HighDyingMass", "MassReturn")}
    queue = np.zeros(max(cnt, 1), dtype=np.int32)
    mg, zg, sg = np.zeros(max(cnt, 1)), np.zeros(max(cnt, 1)), np.zeros((max(cnt, 1), 9))
    nq, nbad = C.c_int64(), C.c_int64()
    pv, sv = pman.view(), capi.star_yield_view(StarP)
    rc = capi.hip.shq_metal_yields(ctx.h, C.byref(pv), C.byref(sv), capi.ptr(act), cnt, float(atime), capi.ptr(r["StellarAges"]), capi.ptr(r["LowDyingMass"]),
                                   capi.ptr(r["HighDyingMass"]), capi.ptr(r["MassReturn"]), capi.ptr(queue), C.byref(nq), capi.ptr(mg), capi.ptr(zg),
                                   capi.ptr(sg), C.byref(nbad))
    if rc != 0 and nbad.value:
        msg = capi.hip.shq_last_error().decode()
        e = ShqError(f"metal_yields failed with status {rc}: {msg}")
        e.status, e.nbad = rc, nbad.value
        raise e
    capi.check(rc, "metal_yields")
    n = nq.value
    r.update(queue=queue[:n].copy(), MassGenerated=mg[:n].copy(), MetalGenerated=zg[:n].copy(), MetalSpeciesGenerated=sg[:n].copy())
    return r


def metal_return_postprocess(ctx, pman, StarP, queue, MassReturn, StellarAges):
    """metal_return_postprocess (metal_return.cpp:581-589) for the stars of `queue`: Mass, TotalMassReturned, LastEnrichmentMyr"""
    q = np.ascontiguousarray(queue, dtype=np.int32)
    mr, ages = np.ascontiguousarray(MassReturn, dtype=np.float64), np.ascontiguousarray(StellarAges, dtype=np.float64)
    if len(mr) != len(q) or len(ages) != len(StarP):
        raise ValueError("metal_return_postprocess: MassReturn is indexed by queue position, StellarAges by star slot")
    pv, sv = pman.view(), capi.star_yield_view(StarP)
    capi.check(capi.hip.shq_metal_return_postprocess(ctx.h, C.byref(pv), C.byref(sv), capi.ptr(q), len(q), capi.ptr(mr), capi.ptr(ages)),
               "metal_return_postprocess")


def cooling_tables(rate_tables, cooling=2, SelfShieldingOn=1, MinGasTemp=100.0, CMBTemperature=2.7255, HeliumHeatOn=0, HeliumHeatThresh=10.0,
                   HeliumHeatAmp=1.0, HeliumHeatExp=0.0, rho_crit_baryon=0.0, fBar=0.17, density_in_phys_cgs=1.0, uu_in_cgs=1.0, tt_in_s=1.0,
                   metal=None, metal_min=None, metal_max=None, zreion=None, zreion_boxsize=0.0):
    """shq_cooling_tables from the caller's data: rate_tables is init_cooling_rates' temp_tab, [14][1000]; metal the NetCoolingRate table
    [nz][nnH][nT] with the first and last node of each axis; zreion the UVF table [Nside]^3.  The struct keeps the arrays alive."""
    t = capi.CoolingTables()
    keep = [np.ascontiguousarray(rate_tables, dtype=np.float64)]
    if keep[0].shape != (14, 1000):
        raise ValueError("cooling_tables: rate_tables must be [14][1000]")
    t.rate_tables = keep[0].ctypes.data
    t.cooling, t.SelfShieldingOn, t.HeliumHeatOn = int(cooling), int(SelfShieldingOn), int(HeliumHeatOn)
    t.MinGasTemp, t.CMBTemperature, t.HeliumHeatThresh, t.HeliumHeatAmp, t.HeliumHeatExp = MinGasTemp, CMBTemperature, HeliumHeatThresh, HeliumHeatAmp, HeliumHeatExp
    t.rho_crit_baryon, t.fBar = rho_crit_baryon, fBar
    t.density_in_phys_cgs, t.uu_in_cgs, t.tt_in_s = density_in_phys_cgs, uu_in_cgs, tt_in_s
    if metal is not None:
        m = np.ascontiguousarray(metal, dtype=np.float64)
        if m.ndim != 3:
            raise ValueError("cooling_tables: the metal table has three axes")
        keep.append(m)
        t.metal = m.ctypes.data
        for d in range(3):
            t.metal_dims[d], t.metal_min[d], t.metal_max[d] = m.shape[d], metal_min[d], metal_max[d]
    if zreion is not None:
        z = np.ascontiguousarray(zreion, dtype=np.float64)
        if z.ndim != 3 or len(set(z.shape)) != 1:
            raise ValueError("cooling_tables: the Zreion table is a cube")
        keep.append(z)
        t.zreion, t.zreion_nside, t.zreion_boxsize = z.ctypes.data, z.shape[0], zreion_boxsize
    t._keep = keep
    return t


def cooling_uvbg(**kw):
    """shq_cooling_uvbg (struct UVBG) from keywords or a mapping's items"""
    u = capi.CoolingUVBG()
    for k, v in kw.items():
        setattr(u, k, float(v))
    return u


def cooling_set_tables(ctx, tables):
    """shq_cooling_set_tables: copy the per-run cooling data (cooling_tables) to the device"""
    capi.check(capi.hip.shq_cooling_set_tables(ctx.h, C.byref(tables)), "cooling_set_tables")


def cooling_set_refill(ctx, on):
    capi.check(capi.hip.shq_cooling_set_refill(ctx.h, int(bool(on))), "cooling_set_refill")


def _cooling_eval(call, head, what, rho, u, ne, Z, heiii, dt, uvbg, redshift, min_egy_spec, lmfp_heat, tail=()):
    rho, u = np.ascontiguousarray(rho, dtype=np.float64), np.ascontiguousarray(u, dtype=np.float64)
    n = len(rho)
    ne = np.array(np.broadcast_to(np.asarray(ne, dtype=np.float64), (n,)))
    opt = [None if a is None else np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=t), (n,))) for a, t in ((Z, np.float64), (heiii, np.uint8), (dt, np.float64))]
    out, status, steps = np.full(n, np.nan), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    capi.check(call(head, capi.COOL_WHAT[what], n, capi.ptr(rho), capi.ptr(u), capi.ptr(ne), capi.ptr(opt[0]), capi.ptr(opt[1]), capi.ptr(opt[2]), C.byref(uvbg),
                    float(redshift), float(min_egy_spec), float(lmfp_heat), capi.ptr(out), capi.ptr(status), capi.ptr(steps), *tail), "cooling_eval")
    return out, ne, status, steps


def cooling_eval(ctx, what, rho, u, ne, uvbg, redshift, Z=None, heiii=None, dt=None, min_egy_spec=0.0, lmfp_heat=0.0):
    """shq_cooling_eval: one of "UNEW" (DoCooling), "TCOOL" (GetCoolingTime), "NH0", "HE0", "HEP", "HEPP", "TEMP", "LAMBDANET" for arrays of
    internal-unit physical densities and energies on the device.  Returns (out, ne after, status, engine steps); out is NaN where the
    status is not capi.COOL_OK."""
    return _cooling_eval(capi.hip.shq_cooling_eval, ctx.h, what, rho, u, ne, Z, heiii, dt, uvbg, redshift, min_egy_spec, lmfp_heat)


def cooling_eval_host(tables, what, rho, u, ne, uvbg, redshift, Z=None, heiii=None, dt=None, min_egy_spec=0.0, lmfp_heat=0.0, nthreads=0):
    """shq_cooling_eval_host: cooling_eval on the CPU with the same engine; needs no context and no GPU"""
    return _cooling_eval(capi.hip.shq_cooling_eval_host, C.byref(tables), what, rho, u, ne, Z, heiii, dt, uvbg, redshift, min_egy_spec, lmfp_heat, (int(nthreads),))


def cooling(ctx, pman, SphP, step, active=None, on_eeqos=None):
    """shq_cooling: cooling_direct (sfr_eff.cpp:430-481) for the active gas on the device.  step: capi.CoolingStep.  Cooled particles get Ne,
    Entropy and Sfr = 0 in SphP.  Returns (capi.CoolingResult, the particles on the effective equation of state, the deferred ones), both
    lists in list order."""
    pv, sv = pman.view(), capi.sph_view(SphP)
    f = SphP.dtype.fields
    cf = capi.CoolingFields(f["Ne"][1], f["Metallicity"][1], f["Sfr"][1], f["DelayTime"][1])
    act = None if active is None else np.ascontiguousarray(active, dtype=np.int32)
    cnt = pman.NumPart if act is None else len(act)
    mask = None if on_eeqos is None else np.ascontiguousarray(on_eeqos, dtype=np.uint8)
    if mask is not None and len(mask) != pman.NumPart:
        raise ValueError("cooling: on_eeqos has one byte per particle")
    eeqos, deferred = np.zeros(max(cnt, 1), dtype=np.int32), np.zeros(max(cnt, 1), dtype=np.int32)
    res = capi.CoolingResult()
    capi.check(capi.hip.shq_cooling(ctx.h, C.byref(pv), C.byref(sv), C.byref(cf), capi.ptr(act), cnt, C.byref(step), capi.ptr(mask), capi.ptr(eeqos), cnt,
                                    capi.ptr(deferred), cnt, C.byref(res)), "cooling")
    return res, eeqos[:res.n_eeqos].copy(), deferred[:res.n_deferred].copy()


def cooling_last_kernel(ctx):
    """(HIP-event ms, engine steps) of the context's last cooling kernel"""
    ms, st = C.c_double(), C.c_int64()
    capi.check(capi.hip.shq_cooling_last_kernel(ctx.h, C.byref(ms), C.byref(st)), "cooling_last_kernel")
    return ms.value, st.value


def sfr_params(**kw):
    """shq_sfr_params (what the engine reads of sfr_params) from keywords; the reference's defaults where it has one"""
    p = capi.SfrParams()
    p.StarformationCriterion, p.Generations, p.FactorSN, p.FactorEVP = 1, 2, 0.1, 1000.0
    p.QuickLymanAlphaTempThresh, p.BoostSFOverDenseFactor = 1e5, 1000.0
    for k, v in kw.items():
        if k not in dict(capi.SfrParams._fields_) or k == "pad_":
            raise ValueError(f"sfr_params: no field {k}")
        setattr(p, k, v)
    return p


class SfrResult:
    """what shq_sfr_eval returns: every row of `out` by name (capi.SFR_OUT), flags, decision, branch, status, steps.  Rows and bytes are
    NaN / 255 where the status is not capi.COOL_OK."""

    def __init__(self, out, flags, decision, branch, status, steps):
        self.out, self.flags, self.decision, self.branch, self.status, self.steps = out, flags, decision, branch, status, steps
        for r, k in enumerate(capi.SFR_OUT):
            setattr(self, k, out[r])

    def arrays(self):
        return [self.out, self.flags, self.decision, self.branch, self.status, self.steps]


def _sfr_eval(call, head, par, what, parts, uvbg_global, uvbg_local, redshift, a3inv, hubble, rnd_table, tail=()):
    n = len(parts["Density"])
    a, keep = capi.SfrArrays(), []
    for k in capi.SFR_ARRAYS:
        v = parts.get(k)
        if v is None:
            continue
        t = np.uint64 if k == "ID" else (np.uint8 if k in ("timebin", "flags") else np.float64)
        v = np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=t), (n,)))
        keep.append(v)
        setattr(a, k, v.ctypes.data)
    rnd = np.ascontiguousarray(rnd_table, dtype=np.float64)
    st = capi.SfrEvalStep(float(redshift), float(a3inv), float(hubble), uvbg_global, uvbg_global if uvbg_local is None else uvbg_local, rnd.ctypes.data, len(rnd))
    out = np.full((len(capi.SFR_OUT), n), np.nan)
    flags, decision, branch = (np.full(n, 255, dtype=np.uint8) for _ in range(3))
    status, steps = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    capi.check(call(head, C.byref(par), capi.SFR_WHAT[what], n, C.byref(a), C.byref(st), capi.ptr(out), capi.ptr(flags), capi.ptr(decision), capi.ptr(branch),
                    capi.ptr(status), capi.ptr(steps), *tail), "sfr_eval")
    return SfrResult(out, flags, decision, branch, status, steps)


def sfr_eval(ctx, par, what, parts, uvbg_global, redshift, a3inv, hubble, rnd_table, uvbg_local=None):
    """shq_sfr_eval: "STARFORM" (starformation() per particle, or quicklyastarformation under QuickLymanAlphaProbability > 0), "EGYEFF"
    (get_egyeff), "NH0" / "HE0" / "HEP" / "HEPP" (the *_sfreff fractions) or "ON_EEQOS" (sfreff_on_eeqos, all four clauses) on the device.
    parts: a mapping with the arrays of capi.SFR_ARRAYS (Hsml, DivVel, CurlVel, GradRho, DelayTime optional).  par: sfr_params().
    Needs cooling_set_tables first.  Returns an SfrResult."""
    return _sfr_eval(capi.hip.shq_sfr_eval, ctx.h, par, what, parts, uvbg_global, uvbg_local, redshift, a3inv, hubble, rnd_table)


def sfr_eval_host(tables, par, what, parts, uvbg_global, redshift, a3inv, hubble, rnd_table, uvbg_local=None, nthreads=0):
    """shq_sfr_eval_host: sfr_eval on the CPU with the same engine; needs no context and no GPU"""
    return _sfr_eval(capi.hip.shq_sfr_eval_host, C.byref(tables), par, what, parts, uvbg_global, uvbg_local, redshift, a3inv, hubble, rnd_table, (int(nthreads),))


def sfr_on_eeqos(ctx, pman, SphP, par, step, active=None):
    """shq_sfr_on_eeqos: sfreff_on_eeqos with all four clauses for the active particles on the device; returns one byte per particle, the
    form cooling()'s on_eeqos takes"""
    pv, sv = pman.view(), capi.sph_view(SphP)
    act = None if active is None else np.ascontiguousarray(active, dtype=np.int32)
    cnt = pman.NumPart if act is None else len(act)
    mask = np.zeros(max(pman.NumPart, 1), dtype=np.uint8)
    capi.check(capi.hip.shq_sfr_on_eeqos(ctx.h, C.byref(pv), C.byref(sv), C.byref(par), capi.ptr(act), cnt, C.byref(step), capi.ptr(mask)), "sfr_on_eeqos")
    return mask[:pman.NumPart]


def starformation(ctx, pman, SphP, par, step, eeqos, ids, rnd_table, GradRho=None, capacity=None):
    """shq_starformation: the star-forming branch of cooling_and_starformation for the particles of `eeqos` (what cooling() returned; under
    QuickLymanAlphaProbability > 0 the active list) on the device.  OK particles get Sfr, Ne, Metallicity, Entropy and the cleared BHHeated
    bit in pman / SphP.  Returns (capi.SfrResultC, (NewParents, mass_of_star, split), (MaybeWind, sm), deferred), all in list order.
    capacity: room in each list (default: the list's length); the ShqError of a call that ran out of room carries the counts as .result."""
    pv, sv = pman.view(), capi.sph_view(SphP)
    f = SphP.dtype.fields
    sf = capi.SfrFields(f["Ne"][1], f["Metallicity"][1], f["Sfr"][1], f["DelayTime"][1])
    lst = np.ascontiguousarray(eeqos, dtype=np.int32)
    ids = np.ascontiguousarray(ids, dtype=np.uint64)
    rnd = np.ascontiguousarray(rnd_table, dtype=np.float64)
    if len(ids) != pman.NumPart:
        raise ValueError("starformation: ids has one entry per particle")
    grad = None if GradRho is None else np.ascontiguousarray(GradRho, dtype=np.float64)
    if grad is not None and len(grad) != len(SphP):
        raise ValueError("starformation: GradRho has one entry per gas slot")
    cap = len(lst) if capacity is None else int(capacity)
    m = max(cap, 1)
    parents, mos, split = np.zeros(m, dtype=np.int32), np.zeros(m), np.zeros(m, dtype=np.uint8)
    wind, sm, deferred = np.zeros(m, dtype=np.int32), np.zeros(m), np.zeros(m, dtype=np.int32)
    res = capi.SfrResultC()
    rc = capi.hip.shq_starformation(ctx.h, C.byref(pv), C.byref(sv), C.byref(sf), capi.ptr(ids), capi.ptr(grad), C.byref(par), capi.ptr(lst), len(lst), C.byref(step),
                                    capi.ptr(rnd), len(rnd), capi.ptr(parents), capi.ptr(mos), capi.ptr(split), cap, capi.ptr(wind), capi.ptr(sm), cap,
                                    capi.ptr(deferred), cap, C.byref(res))
    try:
        capi.check(rc, "starformation")
    except capi.ShqError as e:
        e.result = res      # the counts of a call that ran out of room
        raise
    ns, nw, nd = res.n_newstars, res.n_maybewind, res.n_deferred
    return res, (parents[:ns].copy(), mos[:ns].copy(), split[:ns].copy()), (wind[:nw].copy(), sm[:nw].copy()), deferred[:nd].copy()


def sfr_set_refill(ctx, on):
    capi.check(capi.hip.shq_sfr_set_refill(ctx.h, int(bool(on))), "sfr_set_refill")


def sfr_last_kernel(ctx):
    """(HIP-event ms, engine steps) of the context's last star-formation kernel"""
    ms, st = C.c_double(), C.c_int64()
    capi.check(capi.hip.shq_sfr_last_kernel(ctx.h, C.byref(ms), C.byref(st)), "sfr_last_kernel")
    return ms.value, st.value


class IDGenerator:
    """idgen_init (libgenic/zeldovich.cpp:46-65) for task ThisTask2d of an NTask2d task grid: the sub-block x in [offset[0],
    offset[0] + size[0]), y likewise, every z, with offset[k] = ThisTask2d[k] * Ngrid / NTask2d[k] and size[k] reaching to the next
    task's offset.  The defaults are one rank: the whole Ngrid^3 lattice."""

    def __init__(self, Ngrid, BoxSize, ThisTask2d=(0, 0), NTask2d=(1, 1)):
        self.Ngrid, self.BoxSize = int(Ngrid), float(BoxSize)
        offset, size = [0, 0, 0], [self.Ngrid] * 3
        for k in range(2):
            t, nt = int(ThisTask2d[k]), int(NTask2d[k])
            if nt < 1 or not 0 <= t < nt:
                raise ValueError("IDGenerator: task %d of %d along axis %d" % (t, nt, k))
            offset[k] = t * self.Ngrid // nt
            size[k] = (t + 1) * self.Ngrid // nt - offset[k]
        self.offset, self.size = tuple(offset), tuple(size)
        self.NumPart = size[0] * size[1] * size[2]


def idgen_create_id_from_index(idgen, index):
    """zeldovich.cpp:67-75, for an index or an array of them"""
    index = np.asarray(index, dtype=np.int64)
    i = index // (idgen.size[2] * idgen.size[1]) + idgen.offset[0]
    j = (index % (idgen.size[1] * idgen.size[2])) // idgen.size[2] + idgen.offset[1]
    k = (index % idgen.size[2]) + idgen.offset[2]
    return (i.astype(np.uint64) * np.uint64(idgen.Ngrid) * np.uint64(idgen.Ngrid) + j.astype(np.uint64) * np.uint64(idgen.Ngrid)
            + k.astype(np.uint64) + np.uint64(1))


def idgen_create_pos_from_index(idgen, index):
    """zeldovich.cpp:77-87: [..., 3] positions x * BoxSize / Ngrid"""
    index = np.asarray(index, dtype=np.int64)
    x = index // (idgen.size[2] * idgen.size[1]) + idgen.offset[0]
    y = (index % (idgen.size[1] * idgen.size[2])) // idgen.size[2] + idgen.offset[1]
    z = (index % idgen.size[2]) + idgen.offset[2]
    return np.stack([x * idgen.BoxSize / idgen.Ngrid, y * idgen.BoxSize / idgen.Ngrid, z * idgen.BoxSize / idgen.Ngrid], axis=-1)


def setup_grid(idgen, shift, mass):
    """zeldovich.cpp:89-104: the lattice positions plus shift, and the masses"""
    pos = idgen_create_pos_from_index(idgen, np.arange(idgen.NumPart)) + float(shift)
    return np.ascontiguousarray(pos), np.full(idgen.NumPart, float(mass))


def tabulate_by_k2(fn, Nmesh, BoxSize):
    """fn(kmag) by integer k2 for shq_pm_apply / displacement_fields: kmag = sqrt(k2) * 2 * M_PI / BoxSize as the zeldovich transfers
    form it, 3 (Nmesh/2)^2 + 1 entries; entry 0 (never read) is 0.  fn is called once per k2 with a float."""
    n = 3 * (int(Nmesh) // 2) ** 2 + 1
    t = np.zeros(n)
    for k2 in range(1, n):
        t[k2] = fn(float(np.sqrt(np.float64(k2)) * 2 * np.pi / BoxSize))
    return t


def zeldovich_seed_table(Nmesh, Seed):
    """the seed tables [0][0] and [1][1] of pmesh.h:74-90 (host only, no device needed): two [Nmesh][Nmesh] uint32 arrays"""
    t00 = np.zeros((Nmesh, Nmesh), dtype=np.uint32)
    t11 = np.zeros((Nmesh, Nmesh), dtype=np.uint32)
    capi.check(capi.hip.shq_zeldovich_seed_table(int(Nmesh), int(Seed), capi.ptr(t00), capi.ptr(t11)), "zeldovich_seed_table")
    return t00, t11


def zeldovich_field(ctx, Nmesh, Seed, UnitaryAmplitude=0, InvertPhase=0):
    """fill (or reuse) the resident Gaussian field and download it in petapm's Fourier layout: complex [y][z'][x]"""
    capi.check(capi.hip.shq_zeldovich_fill(ctx.h, int(Nmesh), int(Seed), int(UnitaryAmplitude), int(InvertPhase)), "zeldovich_fill")
    spec = np.zeros((Nmesh, Nmesh // 2 + 1, Nmesh), dtype=np.complex128)
    capi.check(capi.hip.shq_zeldovich_download_field(ctx.h, int(Nmesh), capi.ptr(spec)), "zeldovich_download_field")
    return spec


def displacement_fields(ctx, pos, Nmesh, BoxSize, Seed, DeltaSpec, dlogGrowth=None, vel_prefac=1.0, ScaleDepVelocity=False,
                        UnitaryAmplitude=False, InvertPhase=False, want_disp=True):
    """displacement_fields (libgenic/zeldovich.cpp:150-264) for one rank on the device.  pos: [n][3] undisplaced positions in
    [0, BoxSize).  DeltaSpec / dlogGrowth: tables by k2 (tabulate_by_k2) or callables of kmag.  Returns dict(Pos, Vel, Density, Disp,
    maxdisp, maxvel, phase_ms); the Gaussian field stays resident in ctx for the next species."""
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    n = len(pos)
    delta = tabulate_by_k2(DeltaSpec, Nmesh, BoxSize) if callable(DeltaSpec) else np.ascontiguousarray(DeltaSpec, dtype=np.float64)
    growth = None
    if dlogGrowth is not None:
        growth = tabulate_by_k2(dlogGrowth, Nmesh, BoxSize) if callable(dlogGrowth) else np.ascontiguousarray(dlogGrowth, dtype=np.float64)
    nk2 = 3 * (int(Nmesh) // 2) ** 2 + 1
    if len(delta) != nk2 or (growth is not None and len(growth) != nk2):
        raise ValueError(f"the tables by k2 need {nk2} entries")
    zp = capi.ZeldovichParams(int(Nmesh), int(Seed), int(bool(UnitaryAmplitude)), int(bool(InvertPhase)), int(bool(ScaleDepVelocity)), 0,
                              float(BoxSize), float(vel_prefac))
    out = dict(Pos=np.zeros((n, 3)), Vel=np.zeros((n, 3)), Density=np.zeros(n), Disp=np.zeros((n, 3)) if want_disp else None)
    maxdisp, maxvel = C.c_double(), C.c_double()
    capi.check(capi.hip.shq_zeldovich_displacements(ctx.h, C.byref(zp), capi.ptr(delta), capi.ptr(growth), n, capi.ptr(pos), capi.ptr(out["Pos"]),
                                                    capi.ptr(out["Vel"]), capi.ptr(out["Density"]), capi.ptr(out["Disp"]), C.byref(maxdisp),
                                                    C.byref(maxvel)), "displacement_fields")
    ms = (C.c_double * 4)()
    capi.check(capi.hip.shq_zeldovich_phase_ms(ctx.h, C.byref(ms)), "zeldovich_phase_ms")
    out.update(maxdisp=maxdisp.value, maxvel=maxvel.value, phase_ms=list(ms))
    return out


def glass_setup_positions(Ngrid, BoxSize, shift=0.0, seed=0):
    """setup_glass's perturbed lattice (libgenic/glass.cpp:49-66) for the whole Ngrid^3 lattice on one rank (host only): [Ngrid^3][3]"""
    pos = np.zeros((int(Ngrid) ** 3, 3))
    capi.check(capi.hip.shq_glass_setup_positions(int(Ngrid), float(BoxSize), float(shift), int(seed), capi.ptr(pos)), "glass_setup_positions")
    return pos


def glass_setup_positions_block(Ngrid, BoxSize, shift, seed, offset, size):
    """setup_glass's loop for one task's sub-block of the lattice (host only): x in [offset[0], offset[0] + size[0]), y likewise, every z,
    in idgen_create_pos_from_index's order - an IDGenerator's offset and size.  The reference seeds task ThisTask with seed + ThisTask:
    pass that sum.  [size[0] * size[1] * Ngrid][3]"""
    off, sz = (C.c_int * 2)(int(offset[0]), int(offset[1])), (C.c_int * 2)(int(size[0]), int(size[1]))
    pos = np.zeros((max(sz[0], 0) * max(sz[1], 0) * int(Ngrid), 3))
    capi.check(capi.hip.shq_glass_setup_positions_block(int(Ngrid), float(BoxSize), float(shift), int(seed), C.byref(off), C.byref(sz), capi.ptr(pos)),
               "glass_setup_positions_block")
    return pos


def glass_finish_power(BoxSize_in_MPC, kk, power, nmodes, norm):
    """powerspectrum_sum's tail (powerspectrum.cpp:71-87) on one step's raw sums: (kk, power, nmodes) of the non-empty bins"""
    kk, power = np.array(kk, dtype=np.float64), np.array(power, dtype=np.float64)
    nmodes = np.array(nmodes, dtype=np.int64)
    nz = C.c_int(0)
    capi.check(capi.hip.shq_glass_finish_power(len(kk), float(BoxSize_in_MPC), capi.ptr(kk), capi.ptr(power), capi.ptr(nmodes), float(norm),
                                               C.byref(nz)), "glass_finish_power")
    return kk[:nz.value], power[:nz.value], nmodes[:nz.value]


def glass_evolve(ctx, Nmesh, BoxSize, pos, vel, mass, nsteps=14, spectra=False, wrap=False):
    """glass_evolve (libgenic/glass.cpp:76-147) for one rank on the device: nsteps kick-drift-kick steps of reversed gravity, nsteps + 1
    PM forces.  pos [n][3] float64 (any finite value: positions are not wrapped), vel [n][3] float32, mass [n] float32 or a scalar; the
    inputs are not modified.  Returns dict(Pos, Vel, Disp, steps, phase_ms) and, with spectra, kk / power / nmodes [nsteps][Nmesh] and
    norm [nsteps]: the raw sums of every step (glass_finish_power finishes one).  The positions leave the loop unwrapped, as in the
    reference; wrap=True applies periodic_wrap to the returned Pos, which shq_zeldovich_displacements needs."""
    pos = np.array(pos, dtype=np.float64, order="C")
    n = len(pos)
    vel = np.zeros((n, 3), dtype=np.float32) if vel is None else np.array(vel, dtype=np.float32, order="C")
    mass = np.full(n, mass, dtype=np.float32) if np.isscalar(mass) else np.ascontiguousarray(mass, dtype=np.float32)
    if pos.shape != (n, 3) or vel.shape != (n, 3) or mass.shape != (n,):
        raise ValueError("glass_evolve: pos and vel are [n][3], mass is [n]")
    nsteps = int(nsteps)
    disp = np.zeros((n, 3), dtype=np.float32)
    steps = (capi.GlassStep * max(nsteps, 1))()
    out = dict(Pos=pos, Vel=vel, Disp=disp)
    if spectra:
        out.update(kk=np.zeros((max(nsteps, 0), Nmesh)), power=np.zeros((max(nsteps, 0), Nmesh)),
                   nmodes=np.zeros((max(nsteps, 0), Nmesh), dtype=np.int64), norm=np.zeros(max(nsteps, 0)))
    gp = capi.GlassParams(int(Nmesh), nsteps, float(BoxSize))
    sp = [capi.ptr(out[k]) if spectra else None for k in ("kk", "power", "nmodes", "norm")]
    capi.check(capi.hip.shq_glass_evolve(ctx.h, C.byref(gp), n, capi.ptr(pos), capi.ptr(vel), capi.ptr(disp), capi.ptr(mass),
                                         C.cast(steps, C.c_void_p), *sp), "glass_evolve")
    ms = (C.c_double * 4)()
    capi.check(capi.hip.shq_glass_phase_ms(ctx.h, C.byref(ms)), "glass_phase_ms")
    out["steps"] = [dict(t_f=s.t_f, t_v=s.t_v, t_x=s.t_x, force_std=s.force_std, vel_std=s.vel_std) for s in steps[:max(nsteps, 0)]]
    out["phase_ms"] = list(ms)
    if wrap:
        L = float(BoxSize)
        while (pos >= L).any():
            pos[pos >= L] -= L
        while (pos < 0).any():
            pos[pos < 0] += L
    return out


def thermal_seed_table(Seed, Ngrid):
    """init_rng (libgenic/thermal.cpp:77-91; host only): Ngrid^2 uint32 in the reference's storage order, draw (i outer, j inner) at
    [i + Ngrid * j]; column (x, y) of the lattice is seeded with entry x * Ngrid + y"""
    table = np.zeros(int(Ngrid) ** 2, dtype=np.uint32)
    capi.check(capi.hip.shq_thermal_seed_table(int(Seed), int(Ngrid), capi.ptr(table)), "thermal_seed_table")
    return table


def thermal_tables(max_fd, min_fd=0.0):
    """init_thermalvel's tables (thermal.cpp:44-75; host only): (fermi_dirac_vel [2000], fermi_dirac_cumprob [2000], total_frac)"""
    vel, cumprob = np.zeros(capi.THERMAL_NKNOTS), np.zeros(capi.THERMAL_NKNOTS)
    frac = C.c_double()
    capi.check(capi.hip.shq_thermal_tables(float(max_fd), float(min_fd), capi.ptr(vel), capi.ptr(cumprob), C.byref(frac)), "thermal_tables")
    return vel, cumprob, frac.value


def thermal_speeds(ctx, vel, Ngrid, v_amp, seedtable, cumprob, fdvel, x0=0, nx=None, y0=0, ny=None, want_dvel=False, want_speed=False):
    """add_thermal_speeds over one rank's particles (genic/main.cpp:176-184, 218-226) on the device.  vel: float32 [n][3] of the
    sub-block x in [x0, x0 + nx), y in [y0, y0 + ny), every z, in the rank's particle order (the whole lattice by default); it is not
    modified.  seedtable as thermal_seed_table returns it, cumprob / fdvel as thermal_tables does.  Returns dict(Vel, dvel, speed,
    phase_ms): the new velocities, and on request the double increments [n][3] and the speeds [n]."""
    Ngrid = int(Ngrid)
    nx = Ngrid - int(x0) if nx is None else int(nx)
    ny = Ngrid - int(y0) if ny is None else int(ny)
    vel = np.array(vel, dtype=np.float32, order="C")
    n = len(vel)
    if vel.shape != (n, 3):
        raise ValueError("thermal_speeds: vel is [n][3]")
    seedtable = np.ascontiguousarray(seedtable, dtype=np.uint32).ravel()
    cumprob = np.ascontiguousarray(cumprob, dtype=np.float64)
    fdvel = np.ascontiguousarray(fdvel, dtype=np.float64)
    if len(seedtable) != Ngrid * Ngrid or cumprob.shape != (capi.THERMAL_NKNOTS,) or fdvel.shape != (capi.THERMAL_NKNOTS,):
        raise ValueError(f"thermal_speeds: the seed table has Ngrid^2 entries, the tables {capi.THERMAL_NKNOTS}")
    tp = capi.ThermalParams(Ngrid, int(x0), nx, int(y0), ny, 0, float(v_amp))
    out = dict(Vel=vel, dvel=np.zeros((n, 3)) if want_dvel else None, speed=np.zeros(n) if want_speed else None)
    capi.check(capi.hip.shq_thermal_speeds(ctx.h, C.byref(tp), capi.ptr(seedtable), capi.ptr(cumprob), capi.ptr(fdvel), n, capi.ptr(vel),
                                           capi.ptr(out["dvel"]), capi.ptr(out["speed"])), "thermal_speeds")
    ms = (C.c_double * 3)()
    capi.check(capi.hip.shq_thermal_phase_ms(ctx.h, C.byref(ms)), "thermal_phase_ms")
    out["phase_ms"] = list(ms)
    return out


def synth_positions(kind, n, seed=20240601, L=1.0):
    """SURVEY §8(d) synthetic inputs: kind 'grid' | 'uniform' | 'cluster'."""
    k = {"grid": 0, "uniform": 1, "cluster": 2}[kind]
    pos = np.empty((int(n), 3), dtype=np.float64)
    capi.host.shqh_synth_positions(k, int(n), seed, L, capi.ptr(pos))
    return pos


def synth_positions_range(kind, nglobal, first, count, seed=20240601, L=1.0):
    """particles [first, first + count) of one global synthetic set of nglobal particles, the same for any split over ranks"""
    k = {"grid": 0, "uniform": 1, "cluster": 2}[kind]
    pos = np.empty((int(count), 3), dtype=np.float64)
    capi.host.shqh_synth_positions_range(k, int(nglobal), int(first), int(count), seed, L, capi.ptr(pos))
    return pos


def make_density_params(BoxSize, kernel=1, eta=1.0, MaxNumNgbDeviation=0.5, BlackHoleNgbFactor=2.0, update_hsml=1, DoEgyDensity=1, BlackHoleOn=0, MinGasHsml=0.006):
    """POD mirror of DensityPriv (densitytree2.hpp:10-52) for the C-ABI: DesNumNgb from DensityKrnl::desnumngb (densitykernel.hpp:36-41);
    kick factors all zero"""
    support = {1: 4, 2: 6, 4: 5}[kernel]
    des = 4.0 / 3 * np.pi * (support / 2.0 * eta) ** 3
    dp = capi.DensityParams()
    dp.BoxSize, dp.DesNumNgb, dp.DesNumNgbBH, dp.MinGasHsml = BoxSize, des, des * BlackHoleNgbFactor, MinGasHsml
    dp.MaxNumNgbDeviation = MaxNumNgbDeviation
    dp.update_hsml, dp.BlackHoleOn, dp.DoEgyDensity, dp.WindsDecouple = update_hsml, BlackHoleOn, DoEgyDensity, 0
    dp.DensityKernelType = kernel
    return dp


def make_hydro_params(BoxSize, atime=0.1, hubble=0.1, kernel=1, DensityIndependentSphOn=1, DensityContrastLimit=100.0, ArtBulkViscConst=0.75):
    """POD mirror of HydroPriv (hydratree2.hpp:83-119) for the C-ABI; kick factors and drifts all zero"""
    g = 5.0 / 3.0
    hp = capi.HydroParams()
    hp.BoxSize, hp.atime = BoxSize, atime
    hp.fac_mu = atime ** (3 * (g - 1) / 2) / atime
    hp.fac_vsic_fix = hubble * atime ** (3 * (g - 1))
    hp.hubble_a2 = hubble * atime * atime
    hp.ArtBulkViscConst, hp.DensityContrastLimit = ArtBulkViscConst, DensityContrastLimit
    hp.DensityIndependentSphOn, hp.DensityKernelType = DensityIndependentSphOn, kernel
    return hp


def morton_order(pos, L):
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    order = np.empty(len(pos), dtype=np.int32)
    capi.host.shqh_morton_order(capi.ptr(pos), len(pos), L, capi.ptr(order))
    return order


def hilbert_order(pos, L):
    """Peano-Hilbert order (what the reference keeps particles in, domain.cpp:268)."""
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    order = np.empty(len(pos), dtype=np.int32)
    capi.host.shqh_hilbert_order(capi.ptr(pos), len(pos), L, capi.ptr(order))
    return order


# ---- SPH operators (libgadget/density2.h, hydra2.h) ---------------------------------------------
from .capi import KickFactors, DensityParams, HydroParams, SphStats  # noqa: E402

DENSITY_KERNEL_CUBIC_SPLINE, DENSITY_KERNEL_QUINTIC_SPLINE, DENSITY_KERNEL_QUARTIC_SPLINE = 1, 2, 4
BH_SLOT_DTYPE = np.dtype([("Density", "<f8"), ("DivVel", "<f8")])


def set_densitypar(DensityResolutionEta=1.0, MaxNumNgbDeviation=0.5, DensityKernelType=DENSITY_KERNEL_CUBIC_SPLINE,
                   BlackHoleNgbFactor=2.0, MinGasHsml=0.006):
    capi.host.shqh_set_densitypar(DensityResolutionEta, MaxNumNgbDeviation, DensityKernelType, BlackHoleNgbFactor, MinGasHsml)


def GetNumNgb():
    return capi.host.shqh_GetNumNgb()


def set_hydropar(DensityIndependentSphOn=1, DensityContrastLimit=100.0, ArtBulkViscConst=0.75):
    capi.host.shqh_set_hydropar(DensityIndependentSphOn, DensityContrastLimit, ArtBulkViscConst)


def set_init_hsml(tree, MeanGasSeparation, pman):
    capi.check_host(capi.host.shqh_set_init_hsml(tree._h, MeanGasSeparation, pman._h), "set_init_hsml")


def force_tree_update_hmax(tree, pman):
    capi.host.shqh_force_tree_update_hmax(tree._h, pman._h)


def density(ctx, act, update_hsml, DoEgyDensity, BlackHoleOn, kick, tree, pman, SphP, BhP=None, GradRho_mag=None,
            UseGPU=True):
    """density(act, update_hsml, DoEgyDensity, BlackHoleOn, times..., &EntVarPred, GradRho_mag, tree, UseGPU),
    libgadget/density2.h:42.  Returns (EntVarPred, SphStats)."""
    a = None if act is None else np.ascontiguousarray(act, dtype=np.int32)
    evp = np.zeros(max(len(SphP), 1))
    st = SphStats()
    kick = kick if kick is not None else KickFactors()
    rc = capi.host.shqh_density(ctx.h, pman._h, tree._h, capi.ptr(SphP), len(SphP), capi.ptr(BhP), 0 if BhP is None else len(BhP),
                                capi.ptr(a), 0 if a is None else len(a), int(update_hsml), int(DoEgyDensity), int(BlackHoleOn),
                                C.byref(kick), capi.ptr(evp), capi.ptr(GradRho_mag), int(UseGPU), C.byref(st))
    capi.check_host(rc, "density")
    return evp, st


def hydro_force(ctx, act, atime, hubble, EntVarPred, kick, tree, pman, SphP, drifts=None, UseGPU=True):
    """hydro_force(act, atime, EntVarPred, times..., tree, UseGPU), libgadget/hydra2.h:9."""
    a = None if act is None else np.ascontiguousarray(act, dtype=np.int32)
    st = SphStats()
    kick = kick if kick is not None else KickFactors()
    d = None if drifts is None else np.ascontiguousarray(drifts, dtype=np.float64)
    rc = capi.host.shqh_hydro_force(ctx.h, pman._h, tree._h, capi.ptr(SphP), len(SphP), capi.ptr(a), 0 if a is None else len(a),
                                    atime, hubble, capi.ptr(EntVarPred), C.byref(kick), capi.ptr(d), int(UseGPU), C.byref(st))
    capi.check_host(rc, "hydro_force")
    return st

# ---- snapshot blocks: selection, typed columns, readout (csrc/snapshot.hip; snapshot.py) ----------
from .snapshot import (IOBlock, io_blocks, io_layout, io_conv, io_select, io_gather, io_scatter, io_ion_fractions, snapshot_columns,  # noqa: E402,F401
                       snapshot_readout)
from .capi import IO_SELECT_ALL, IO_SELECT_FOF, IO_ORDER_INDEX, IO_ORDER_GRNR  # noqa: E402,F401

# ---- light-cone crossings: replicas, sampling, ordered rows (csrc/lightcone.hip; lightcone.py) ----------
from .lightcone import (Lightcone, LightconeStateView, lightcone_layout, lightcone_table, lightcone_horizon, lightcone_compute_raw,  # noqa: E402,F401
                        lightcone_phase_ms)
from .capi import LIGHTCONE_CONSISTENT, LIGHTCONE_AS_WRITTEN, LIGHTCONE_MAXREPLICA  # noqa: E402,F401

# ---- run start-up: init()'s loops, the first Hsml, the initial entropy (csrc/startup.hip; startup.py) ----------
from .startup import (StartupError, StartupReport, SmlStats, startup_layout, startup_params, startup_particles, check_density_entropy,  # noqa: E402,F401
                      set_init_hsml_device, init_entropy, setup_smoothinglengths, mean_separation, u_init, check_omega, meanbar)
from .capi import STARTUP_OMEGA, STARTUP_POSITIONS, STARTUP_HSML, STARTUP_INIT, STARTUP_ALL  # noqa: E402,F401

# ---- run logs: energy statistics, black-hole totals and details, the log lines (csrc/stats.hip; stats.py) ----------
from .stats import (BHINFO_DTYPE, stats_layout, stats_params, energy_statistics, stats_finish, bh_totals, bh_detail_layout, bh_detail_arrays,  # noqa: E402,F401
                    bh_details, energy_line, blackholes_line, sfr_line)

# ---- linear-response massive neutrinos: resident state, delta_nu from the PM's P(k), the mode table (csrc/nulra.hip; nulra.py) ----------
from .nulra import NuLRA, pack_sums  # noqa: E402,F401
