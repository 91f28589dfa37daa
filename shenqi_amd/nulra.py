"""Linear-response massive neutrinos (csrc/nulra.hip, csrc/nulra_host.hip): the resident state of init_neutrinos_lra and
delta_nu_from_power between the PM's forward and its finish.

    nu = NuLRA(ctx, nk_allocated=..., TimeTransfer=..., ..., hubble=H, omega_nu_nopart=f, omega_nu_single=g)
    shq_pm_forward(...); nu.step(Time, TimeIC); shq_pm_run(...)          # one rank: the table never leaves the device
    DistTreePM.step(gp, analysis=nu.at(Time, TimeIC))                     # sharded: fed the all-reduced sums, hands back the table
    gravpm_force(ctx, pm, pman, analysis=nu.at(Time, TimeIC))             # the host mirror's hook

ctx = None runs the same engine on the host (no device)."""
import ctypes as C

import numpy as np

from . import capi


def pack_sums(kk, power, nmodes, norm):
    """the raw P(k) sums in the layout shq_nulra_step reads: [nbins] power, [nbins] kk, [nbins] modes (uint64), norm"""
    n = len(kk)
    out = np.empty(3 * n + 1, dtype=np.float64)
    out[:n] = power
    out[n:2 * n] = kk
    out[2 * n:3 * n] = np.asarray(nmodes, dtype=np.int64).view(np.float64)
    out[3 * n] = norm
    return out


class NuLRA:
    """The state and the step.  The three callbacks take a scale factor (omega_nu_single also the species) and return a float; they are
    called on the host, about 10^4 times per step, at arguments that do not depend on k."""

    def __init__(self, ctx, *, nk_allocated, TimeTransfer, TimeMax, light, delta_nu_prefac, Omeganonu, OmegaNu1, kBtnu, mnu, degeneracy, BoxSize_in_MPC,
                 logk, T_nu, hubble, omega_nu_nopart, omega_nu_single, hybrid=None):
        self.ctx = ctx
        self._h = None
        self._logk = np.ascontiguousarray(logk, dtype=np.float64)
        self._tnu = np.ascontiguousarray(T_nu, dtype=np.float64)
        # the CFUNCTYPE objects must outlive the state: the library keeps the pointers
        self._cb = (capi.NULRA_COSMO_FN(lambda a, mi, u: float(hubble(a))), capi.NULRA_COSMO_FN(lambda a, mi, u: float(omega_nu_nopart(a))),
                    capi.NULRA_COSMO_FN(lambda a, mi, u: float(omega_nu_single(a, mi))))
        p = capi.NulraParams()
        p.nk_allocated, p.TimeTransfer, p.TimeMax = int(nk_allocated), TimeTransfer, TimeMax
        p.light, p.delta_nu_prefac, p.Omeganonu, p.OmegaNu1, p.kBtnu = light, delta_nu_prefac, Omeganonu, OmegaNu1, kBtnu
        p.mnu[:] = list(mnu)
        p.degeneracy[:] = list(degeneracy)
        if hybrid is not None:
            p.hybrid_enabled = 1
            p.vcrit_by_light, p.nu_crit_time = hybrid["vcrit_by_light"], hybrid["nu_crit_time"]
            p.nufrac_low[:] = list(hybrid["nufrac_low"])
        p.BoxSize_in_MPC = BoxSize_in_MPC
        p.NPowerTable = len(self._logk)
        p.logk, p.T_nu = capi.ptr(self._logk), capi.ptr(self._tnu)
        p.hubble, p.omega_nu_nopart, p.omega_nu_single = self._cb
        self.params = p
        self.nk_allocated = int(nk_allocated)
        self.Time = self.TimeIC = None
        if ctx is None:
            h = C.c_void_p()
            capi.check(capi.hip.shq_nulra_host_create(C.byref(p), C.byref(h)), "shq_nulra_host_create")
            self._h = h
            self._pre = "shq_nulra_host_"
        else:
            capi.check(capi.hip.shq_nulra_init(ctx.h, C.byref(p)), "shq_nulra_init")
            self._h = ctx.h
            self._pre = "shq_nulra_"

    def _fn(self, name):
        return getattr(capi.hip, self._pre + name)

    def close(self):
        if self._h is not None:
            if self.ctx is None:
                capi.hip.shq_nulra_host_destroy(self._h)
            else:
                capi.check(capi.hip.shq_nulra_free(self._h))
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def try_step(self, Time, TimeIC, sums=None, nbins=0):
        """shq_nulra_step's status.  sums: None (the context's own sums of shq_pm_forward), a host array in pack_sums' layout (uploaded when
        the state is on the device), or anything with data_ptr() in device memory"""
        ptr = None
        if sums is not None and hasattr(sums, "data_ptr"):
            ptr = C.c_void_p(sums.data_ptr())
        elif sums is not None:
            sums = np.ascontiguousarray(sums, dtype=np.float64)
            nbins = (len(sums) - 1) // 3
            ptr = capi.ptr(sums)   # a host array: the device engine uploads it and waits for the copy
        return self._fn("step")(self._h, Time, TimeIC, ptr, int(nbins))

    def step(self, Time, TimeIC, sums=None, nbins=0):
        capi.check(self.try_step(Time, TimeIC, sums, nbins), self._pre + "step")

    def mode_table(self, Nmesh, add_one=True):
        T = np.zeros(3 * (Nmesh // 2) ** 2 + 1)
        capi.check(self._fn("mode_table")(self._h, int(Nmesh), int(bool(add_one)), capi.ptr(T)), self._pre + "mode_table")
        return T

    def info(self):
        info = capi.NulraInfo()
        capi.check(self._fn("download")(self._h, None, None, C.byref(info)), self._pre + "download")
        return info

    def download(self):
        """(delta_nu_last[nk], kk[nonzero], info) of the last step"""
        delta = np.zeros(self.nk_allocated)
        kk = np.zeros(max(self.nk_allocated, 1 << 14))
        info = capi.NulraInfo()
        capi.check(self._fn("download")(self._h, capi.ptr(delta), capi.ptr(kk), C.byref(info)), self._pre + "download")
        return delta[:info.nk].copy(), kk[:info.nonzero].copy(), info

    def delta_nu(self, a):
        """get_delta_nu_combined at a over the stored history; changes nothing"""
        st = capi.NulraState()
        capi.check(self._fn("get_state")(self._h, C.byref(st)))
        out = np.zeros(st.nk)
        capi.check(self._fn("delta_nu")(self._h, a, capi.ptr(out)), self._pre + "delta_nu")
        return out

    def get_state(self):
        """dict(ia, nk, scalefact[ia], delta_tot[nk, ia], delta_nu_init[nk], kvalue[nk], delta_nu_last[nk])"""
        st = capi.NulraState()
        capi.check(self._fn("get_state")(self._h, C.byref(st)))
        ia, nk = st.ia, st.nk
        out = dict(ia=ia, nk=nk, scalefact=np.zeros(ia), delta_tot=np.zeros((nk, ia)), delta_nu_init=np.zeros(nk), kvalue=np.zeros(nk),
                   delta_nu_last=np.zeros(nk))
        for k in ("scalefact", "delta_tot", "delta_nu_init", "kvalue", "delta_nu_last"):
            setattr(st, k, capi.ptr(out[k]))
        capi.check(self._fn("get_state")(self._h, C.byref(st)), self._pre + "get_state")
        return out

    def try_set_state(self, state):
        st = capi.NulraState()
        st.ia, st.nk = int(state["ia"]), int(state["nk"])
        keep = []
        for k in ("scalefact", "delta_tot", "delta_nu_init", "kvalue", "delta_nu_last"):
            v = state.get(k)
            if v is not None:
                v = np.ascontiguousarray(v, dtype=np.float64)
                keep.append(v)
            setattr(st, k, capi.ptr(v))
        return self._fn("set_state")(self._h, C.byref(st))

    def set_state(self, state):
        """state as get_state returns it; without delta_nu_last (a snapshot of the reference) the next step recomputes it"""
        capi.check(self.try_set_state(state), self._pre + "set_state")

    # ---- as the analysis hook of gravpm_force / SlabPM.force / DistTreePM.step ----
    def at(self, Time, TimeIC):
        """sets the times of the next hook call; returns self"""
        self.Time, self.TimeIC = Time, TimeIC
        return self

    def __call__(self, kk, power, nmodes, norm):
        """analysis(kk, power, nmodes, norm) -> T: a step on the (all-reduced) raw sums, then the table for Nmesh = len(kk)"""
        if self.Time is None:
            raise ValueError("NuLRA used as an analysis hook: set the times with .at(Time, TimeIC) first")
        self.step(self.Time, self.TimeIC, pack_sums(kk, power, nmodes, norm))
        return self.mode_table(len(kk))
