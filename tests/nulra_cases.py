"""The cases shared by tests/test_nulra_cpu.py and tests/test_gpu_nulra.py: cosmologies, history tables, synthetic P(k) sums and the
constructor of a shenqi_amd.NuLRA (on a context, or on the host with ctx = None) from a nulra_restated.Cosmo."""
import numpy as np

import shenqi_amd as sq
import nulra_restated as nr

GATE = 1.49e-8          # sqrt(epsilon): the tolerance the reference's own quadrature is run at
TIME_TRANSFER = 0.01
BOXMPC = 2 * np.pi      # k = kk / nmodes
TLOGK = np.linspace(-3.0, 3.0, 20)
TNU = 0.4 / (1 + (10**TLOGK / 0.5) ** 2)
NAS = (1, 2, 3, 4, 5, 40)

HYBRID = dict(vcrit_by_light=850.0 / nr.LIGHT, nu_crit_time=0.1, nufrac_low=[0.3, 0.3, 0.3])


def cosmo(name):
    """The non-hybrid cases keep the kpc/h lengths of the reference's own unit test beside k in h/Mpc: k fs is 1000 times what it would be
    in one unit, the harshest spike at the upper limit.  The hybrid cases use Mpc/h for both.  There the truncated J oscillates as
    cos(vcrit k fs) and decays only as x^-2: its phase reaches 2.7e4 rad at k = 100, which a quadrature can resolve; in the mixed units it
    would be 2.7e7 rad, beyond the 2^15 x 61 points that the reference's adaptive rule may spend, so there is nothing to compare against."""
    if name == "equal":
        return nr.Cosmo([0.15, 0.15, 0.15], [3, 0, 0])
    if name == "mixed":
        return nr.Cosmo([0.2, 0.05, 0.0], [1, 1, 1])
    if name == "equal_mpc":
        return nr.Cosmo([0.15, 0.15, 0.15], [3, 0, 0], H0=100.0)
    if name == "mixed_mpc":
        return nr.Cosmo([0.2, 0.05, 0.0], [1, 1, 1], H0=100.0)
    if name == "hybrid":
        return nr.Cosmo([0.15, 0.15, 0.15], [3, 0, 0], hybrid=HYBRID, H0=100.0)
    if name == "allparticles":   # 1 - partnu < 1e-3 past nu_crit_time
        return nr.Cosmo([0.15, 0.15, 0.15], [3, 0, 0], hybrid=dict(vcrit_by_light=850.0 / nr.LIGHT, nu_crit_time=0.03, nufrac_low=[0.9995] * 3), H0=100.0)
    raise KeyError(name)


COSMOS = ("equal", "mixed", "hybrid")


def make(ctx, c, nk_allocated=32, TimeMax=1.0):
    return sq.NuLRA(ctx, nk_allocated=nk_allocated, TimeTransfer=TIME_TRANSFER, TimeMax=TimeMax, light=nr.LIGHT, delta_nu_prefac=c.delta_nu_prefac,
                    Omeganonu=c.Omeganonu, OmegaNu1=c.OmegaNu1, kBtnu=nr.KBTNU, mnu=c.mnu, degeneracy=c.deg, BoxSize_in_MPC=BOXMPC, logk=TLOGK, T_nu=TNU,
                    hubble=c.hubble, omega_nu_nopart=c.omega_nu_nopart, omega_nu_single=c.omega_nu_single, hybrid=c.hybrid)


def restated(c, nk_allocated=32, TimeMax=1.0):
    return nr.Restated(c, nk_allocated, TIME_TRANSFER, TimeMax, BOXMPC, TLOGK, TNU)


def history(Na, nk=10):
    """nk = 10 bins k = 0.01 .. 100 and Na stored spectra at unequal steps a = 0.01 .. 0.5 (Na = 1: the initial time alone)"""
    k = 0.01 * 10 ** (4.0 * np.arange(nk) / (nk - 1))
    a = np.array([TIME_TRANSFER]) if Na == 1 else TIME_TRANSFER * 50 ** ((np.arange(Na) / (Na - 1.0)) ** 1.3)
    dt = 1e-3 * (a[None, :] / TIME_TRANSFER) * (1 + 0.3 * np.sin(np.arange(nk)[:, None] + 3 * a[None, :])) / (1 + np.sqrt(k[:, None] / 5))
    return dict(ia=Na, nk=nk, scalefact=np.log(a), delta_tot=np.ascontiguousarray(dt), delta_nu_init=1e-3 / (1 + k), kvalue=k)


def restated_delta_nu(c, st):
    a = float(np.exp(st["scalefact"][-1]))
    return nr.get_delta_nu_combined(c, TIME_TRANSFER, st["scalefact"], st["delta_tot"], st["kvalue"], st["delta_nu_init"], a)


def bins(nbins=10, kmin=2.0, kmax=10.0, empty=()):
    """the wavenumbers and mode counts of synthetic P(k) bins (empty: bins without a mode)"""
    k = kmin * (kmax / kmin) ** (np.arange(nbins) / (nbins - 1.0))
    nm = (3 + 2 * np.arange(nbins)).astype(np.int64)
    nm[list(empty)] = 0
    return k, nm


def growth(k, a):
    return 1e-3 * (a / TIME_TRANSFER) / (1 + k / 3)


def sums(k, nm, a, norm=2.5):
    """raw sums (kk, power, nmodes, norm) whose powerspectrum_sum is (k, growth(k, a)^2) on the non-empty bins"""
    d = growth(k, a)
    power = d * d * nm * norm / BOXMPC**3
    kk = k * nm / (2 * np.pi / BOXMPC)
    return kk, power, nm, norm


def rel(x, ref):
    """the worst |x / ref - 1| over every entry (0 where both are exactly 0)"""
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert x.shape == ref.shape and np.isfinite(x).all() and np.isfinite(ref).all()
    both0 = (x == 0) & (ref == 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.abs(x / np.where(both0, 1.0, ref) - 1)
    return float(np.where(both0, 0.0, r).max())


TIMES = (0.01, 0.012, 0.016, 0.022, 0.022, 0.035, 0.05, 0.052, 0.07, 0.1, 0.14, 0.2)


def run_sequence(nu, ref, times=TIMES, nbins=10, TimeIC=TIME_TRANSFER):
    """the same steps on a NuLRA and (ref may be None) on the restatement; returns [(info, delta_nu_last, state)] per step"""
    k, nm = bins(nbins)
    out = []
    for t in times:
        s = sums(k, nm, t)
        nu.step(t, TimeIC, sq.pack_sums(*s))
        if ref is not None:
            ref.step(t, TimeIC, *s)
        d, _, info = nu.download()
        out.append((info, d, nu.get_state()))
    return out
