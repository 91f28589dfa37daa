/* nulra_host.hip — the linear-response neutrino engine of nulra_math.hpp / nulra_engine.hpp on the host: the stages driven in plain
 * loops over host arrays, behind shq_nulra_host_*.  No kernel and no HIP call here: the file also builds with a plain C++ compiler into a
 * stand-alone host program (with the sanitizers, for instance) beside a main that defines shq_set_error. */
#include "nulra_engine.hpp"
#include <string.h>
#include <chrono>

/* the backend of nulra_engine_step on host arrays */
struct NuHostBackend {
    NuArr A = {};
    std::vector<double> d;   /* every double array */
    std::vector<int32_t> nz; /* nzidx */
    int32_t status = 0;

    void alloc(const NuEngine &E, int nbins_cap)
    {
        const size_t nk = (size_t) E.p.nk_allocated, nb = (size_t) nbins_cap;
        std::vector<double> nd((8 + (size_t) E.namax + 3) * nk + 7 * nb, 0.0);
        /* keep what the state holds across a growth of the bin arrays */
        if(!d.empty())
            memcpy(nd.data(), d.data(), sizeof(double) * (8 + (size_t) E.namax + 3) * nk);
        d.swap(nd);
        nz.assign(nb, 0);
        double *q = d.data();
        A.nk_alloc = (int) nk;
        A.namax = E.namax;
        A.nbins_cap = nbins_cap;
        A.wavenum = q; q += nk;
        A.delta_nu_last = q; q += nk;
        A.delta_nu_init = q; q += nk;
        A.power_in = q; q += nk;
        A.ratio_raw = q; q += nk;
        A.logwav = q; q += nk;
        A.slope_w = q; q += nk;
        q += nk; /* spare */
        A.delta_tot = q; q += nk * E.namax;
        A.partial = q; q += 3 * nk;
        A.kk_nz = q; q += nb;
        A.pw_nz = q; q += nb;
        A.logk_nz = q; q += nb;
        A.logp_nz = q; q += nb;
        A.slope_nz = q; q += nb;
        A.ratio_nz = q; q += nb;
        A.slope_r = q; q += nb;
        A.nzidx = nz.data();
        A.status = &status;
        A.ntab = (int) E.tlogk.size();
        A.tlogk = E.tlogk.data();
        A.tT = E.tT.data();
        A.tslope = E.tslope.data();
    }

    const NuEngine *E = nullptr;

    int load_bins(const double *sums, int nbins, double BoxMpc, int *nnz)
    {
        NU_CHECK(sums && nbins >= 4 && nbins <= (1 << 20), SHQ_ERR_INVALID, "nulra_step: null sums or %d bins", nbins);
        if(nbins > A.nbins_cap)
            alloc(*E, nbins);
        int n = 0;
        for(int b = 0; b < nbins; b++) {
            int64_t nm;
            memcpy(&nm, sums + 2 * (size_t) nbins + b, sizeof(nm));
            if(nm != 0)
                A.nzidx[n++] = b;
        }
        for(int i = 0; i < n; i++)
            nulra_op_compact(A, sums, nbins, BoxMpc, i);
        *nnz = n;
        return SHQ_OK;
    }
    int last_wavenumber(int nnz, double *k)
    {
        *k = A.kk_nz[nnz - 1];
        return SHQ_OK;
    }
    int first_init(int nk, double OmegaNua3, double Omeganonu, double OmegaNu1, double partnu)
    {
        for(int i = 0; i < nk; i++)
            nulra_op_first_init(A, i, OmegaNua3, Omeganonu, OmegaNu1, partnu);
        return SHQ_OK;
    }
    int power_in(int rebin, int nnz, int nk, int ia)
    {
        if(rebin)
            for(int i = 0; i < nnz; i++)
                nulra_op_slope_nz(A, nnz, i);
        for(int i = 0; i < nk; i++)
            nulra_op_power_in(A, i, rebin, nnz, ia);
        return SHQ_OK;
    }
    int update_delta_tot(int nk, int col, double OmegaNua3, double Omeganonu, double OmegaNu1, double partnu)
    {
        for(int i = 0; i < nk; i++)
            nulra_op_update(A, i, col, OmegaNua3, Omeganonu, OmegaNu1, partnu);
        return SHQ_OK;
    }
    int delta_nu(const NuNodeTable &T, int Na, const double *sf, double deriv_prefac, double delta_nu_prefac, double nufrac_low, const NuSpecies *S, int ns,
                 int nk)
    {
        const NuNodes N{T.n, T.W.data(), T.fs.data(), T.h.data(), T.iv.data()};
        std::vector<double> row((size_t) nulra_row_len(Na)), lanes((size_t) SHQ_NULRA_LANES);
        double frac[SHQ_NULRA_NUSPECIES] = {0, 0, 0};
        for(int s = 0; s < ns; s++) {
            frac[s] = S[s].frac;
            for(int i = 0; i < nk; i++) {
                double integral = 0;
                if(S[s].integrate) {
                    for(int e = 0; e < nulra_row_len(Na); e++)
                        row[e] = nulra_row_entry(Na, sf, A.delta_tot + (size_t) i * A.namax, e);
                    const double kfac = A.wavenum[i] / S[s].mnubykT;
                    for(int lane = 0; lane < SHQ_NULRA_LANES; lane++)
                        lanes[lane] = nulra_lane_sum(N, row.data(), kfac, S[s].qc, nufrac_low, lane);
                    for(int half = SHQ_NULRA_LANES / 2; half >= 1; half >>= 1)
                        for(int l = 0; l < half; l++)
                            nulra_fold(lanes.data(), l, half);
                    integral = lanes[0];
                }
                A.partial[(size_t) s * A.nk_alloc + i] =
                    nulra_delta_nu_single(A.wavenum[i], A.delta_nu_init[i], T.fsl_A0a, deriv_prefac, delta_nu_prefac, S[s], integral);
            }
        }
        for(int i = 0; i < nk; i++)
            nulra_op_combine(A, i, ns, frac);
        return SHQ_OK;
    }
    int finish(int rebin, int nnz, int nk)
    {
        for(int i = 0; i < nk; i++)
            nulra_op_ratio_raw(A, i);
        if(rebin)
            for(int i = 0; i < nk; i++)
                nulra_op_slope_w(A, nk, i);
        for(int i = 0; i < nnz; i++)
            nulra_op_ratio_nz(A, i, rebin, nk);
        for(int i = 0; i < nnz; i++)
            nulra_op_slope_r(A, nnz, i);
        return SHQ_OK;
    }
};

struct shq_nulra_host {
    NuEngine E;
    NuHostBackend be;
    int kept = -1;
};

extern "C" int shq_nulra_host_create(const shq_nulra_params *params, shq_nulra_host **out)
{
    NU_CHECK(out, SHQ_ERR_INVALID, "null argument");
    shq_nulra_host *h = new shq_nulra_host();
    const int rc = nulra_engine_init(h->E, params);
    if(rc != SHQ_OK) {
        delete h;
        return rc;
    }
    h->be.E = &h->E;
    h->be.alloc(h->E, h->E.p.nk_allocated);
    *out = h;
    return SHQ_OK;
}

extern "C" void shq_nulra_host_destroy(shq_nulra_host *h) { delete h; }

extern "C" int shq_nulra_host_step(shq_nulra_host *h, double Time, double TimeIC, const void *sums, int nbins)
{
    NU_CHECK(h, SHQ_ERR_INVALID, "null argument");
    NU_CHECK(!h->be.status, SHQ_ERR_DEVICE, "nulra: an earlier step left a NaN in delta_nu_last");
    const auto t0 = std::chrono::steady_clock::now();
    NU_TRY(nulra_engine_step(h->E, h->be, Time, TimeIC, (const double *) sums, nbins, &h->kept));
    h->E.callback_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    NU_CHECK(!h->be.status, SHQ_ERR_DEVICE, "nulra_step: NaN in delta_nu_last");
    return SHQ_OK;
}

extern "C" int shq_nulra_host_mode_table(shq_nulra_host *h, int Nmesh, int add_one, double *table)
{
    NU_CHECK(h && table, SHQ_ERR_INVALID, "null argument");
    NU_CHECK(!h->be.status, SHQ_ERR_DEVICE, "nulra: an earlier step left a NaN in delta_nu_last");
    NU_CHECK(h->E.have_step, SHQ_ERR_STATE, "nulra_mode_table: no step yet");
    NU_CHECK(Nmesh >= 2 && Nmesh % 2 == 0 && Nmesh <= 16384, SHQ_ERR_INVALID, "nulra_mode_table: Nmesh %d", Nmesh);
    const long long nk2 = 3ll * (Nmesh / 2) * (Nmesh / 2) + 1;
    const NuArr &A = h->be.A;
    table[0] = add_one ? 1.0 : 0.0;
    for(long long k2 = 1; k2 < nk2; k2++)
        table[k2] = (add_one ? 1.0 : 0.0) + nulra_mode_factor(h->E.nnz, A.logk_nz, A.ratio_nz, A.slope_r, h->E.nu_prefac, h->E.p.BoxSize_in_MPC, k2);
    return SHQ_OK;
}

extern "C" int shq_nulra_host_download(shq_nulra_host *h, double *delta_nu_last, double *kk, shq_nulra_info *info)
{
    NU_CHECK(h, SHQ_ERR_INVALID, "null argument");
    NU_CHECK(!h->be.status, SHQ_ERR_DEVICE, "nulra: an earlier step left a NaN in delta_nu_last");
    if(delta_nu_last)
        memcpy(delta_nu_last, h->be.A.delta_nu_last, sizeof(double) * h->E.nk);
    if(kk)
        memcpy(kk, h->be.A.kk_nz, sizeof(double) * h->E.nnz);
    if(info)
        nulra_fill_info(h->E, h->kept, info);
    return SHQ_OK;
}

extern "C" int shq_nulra_host_delta_nu(shq_nulra_host *h, double a, double *delta_nu)
{
    NU_CHECK(h && delta_nu, SHQ_ERR_INVALID, "null argument");
    NU_CHECK(h->E.ia >= 1 && h->E.nk >= 1, SHQ_ERR_STATE, "nulra_delta_nu: the history is empty");
    NU_CHECK(std::isfinite(a) && a > 0, SHQ_ERR_INVALID, "nulra_delta_nu: a = %g", a);
    std::vector<double> keep(h->be.A.delta_nu_last, h->be.A.delta_nu_last + h->E.nk);
    NU_TRY(nulra_delta_nu_combined(h->E, h->be, a));
    memcpy(delta_nu, h->be.A.delta_nu_last, sizeof(double) * h->E.nk);
    memcpy(h->be.A.delta_nu_last, keep.data(), sizeof(double) * h->E.nk);
    return SHQ_OK;
}

extern "C" int shq_nulra_host_get_state(shq_nulra_host *h, shq_nulra_state *st)
{
    NU_CHECK(h && st, SHQ_ERR_INVALID, "null argument");
    const NuEngine &E = h->E;
    const NuArr &A = h->be.A;
    st->ia = E.ia;
    st->nk = E.nk;
    if(st->scalefact)
        memcpy(st->scalefact, E.scalefact.data(), sizeof(double) * E.ia);
    if(st->delta_tot)
        for(int k = 0; k < E.nk; k++)
            memcpy(st->delta_tot + (size_t) k * E.ia, A.delta_tot + (size_t) k * A.namax, sizeof(double) * E.ia);
    if(st->delta_nu_init)
        memcpy(st->delta_nu_init, A.delta_nu_init, sizeof(double) * E.nk);
    if(st->kvalue)
        memcpy(st->kvalue, A.wavenum, sizeof(double) * E.nk);
    if(st->delta_nu_last)
        memcpy(st->delta_nu_last, A.delta_nu_last, sizeof(double) * E.nk);
    return SHQ_OK;
}

extern "C" int shq_nulra_host_set_state(shq_nulra_host *h, const shq_nulra_state *st)
{
    NU_CHECK(h && st && st->scalefact && st->delta_tot && st->delta_nu_init && st->kvalue, SHQ_ERR_INVALID, "null argument");
    NuEngine &E = h->E;
    const NuArr &A = h->be.A;
    NU_CHECK(st->nk >= 1 && st->ia >= 1 && st->nk <= E.p.nk_allocated && st->ia <= E.namax, SHQ_ERR_INVALID,
             "nulra_set_state: allocated nk %d na %d for neutrino power but need nk %d na %d", E.p.nk_allocated, E.namax, st->nk, st->ia);
    E.ia = st->ia;
    E.nk = st->nk;
    memcpy(E.scalefact.data(), st->scalefact, sizeof(double) * E.ia);
    for(int k = 0; k < E.nk; k++)
        memcpy(A.delta_tot + (size_t) k * A.namax, st->delta_tot + (size_t) k * E.ia, sizeof(double) * E.ia);
    memcpy(A.delta_nu_init, st->delta_nu_init, sizeof(double) * E.nk);
    memcpy(A.wavenum, st->kvalue, sizeof(double) * E.nk);
    E.kmax = *std::max_element(st->kvalue, st->kvalue + E.nk);
    E.init_done = st->delta_nu_last != nullptr;
    if(st->delta_nu_last)
        memcpy(A.delta_nu_last, st->delta_nu_last, sizeof(double) * E.nk);
    E.have_step = false;
    return SHQ_OK;
}
