/* nulra.hip — linear-response massive neutrinos on the device: compute_neutrino_power (gravpm.cpp:308-321) and delta_nu_from_power
 * (neutrinos_lra.cpp:136-241) between shq_pm_forward and the finish, with potential_transfer's nufac table (gravpm.cpp:412-427) filled
 * where the finish reads it.  The contract is in shenqi_hip.h; the arithmetic in nulra_math.hpp, the state machine in nulra_engine.hpp,
 * shared with the host engine (nulra_host.hip).
 *
 * The hot path is nulra_delta_nu_kernel: one workgroup of 256 lanes per (k bin, species).  The bin's history row and its makima slopes
 * are made in LDS; the lanes stride over the k-independent node table (coalesced: W, fs, four Hermite weights, the interval), each node
 * four multiply-adds on the row and one specialJ; the lanes' sums are folded by a fixed tree in LDS.  No floating-point atomics: two
 * runs give the same bits.  Everything else is one thread per bin or per mode.
 * A steady-state step waits for nothing: the host builds the node table from scalefact, which it owns, stages it in one of two pinned
 * blocks and queues one upload and the kernels behind the forward.  The first step, a new number of bins and a restored state wait. */
#include "common.hpp"
#include "nulra_engine.hpp"
#include <string.h>
#include <chrono>

namespace {

template <class F> __global__ void nulra_for_kernel(int n, F f)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if(i < n)
        f(i);
}

template <class F> int nulra_for(hipStream_t s, int n, F f)
{
    if(n <= 0)
        return SHQ_OK;
    nulra_for_kernel<<<dim3(nblk(n, 256)), dim3(256), 0, s>>>(n, f);
    SHQ_HIP(hipGetLastError());
    return SHQ_OK;
}

struct NuSpecies3 {
    NuSpecies s[SHQ_NULRA_NUSPECIES];
};

/* grid (nk, species): partial[s][i] = get_delta_nu of bin i for species s */
__global__ __launch_bounds__(SHQ_NULRA_LANES) void nulra_delta_nu_kernel(NuArr A, NuNodes N, const double *__restrict__ sf, int Na, double fsl_A0a,
                                                                         double deriv_prefac, double delta_nu_prefac, double nufrac_low, NuSpecies3 S)
{
    extern __shared__ double lds[]; /* the row, then the lanes' sums */
    const int i = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
    const NuSpecies sp = S.s[s];
    const int rowlen = nulra_row_len(Na);
    double *row = lds, *lanes = lds + rowlen;
    double integral = 0;
    if(sp.integrate) { /* the same in every lane */
        for(int e = tid; e < rowlen; e += SHQ_NULRA_LANES)
            row[e] = nulra_row_entry(Na, sf, A.delta_tot + (size_t) i * A.namax, e);
        __syncthreads();
        lanes[tid] = nulra_lane_sum(N, row, A.wavenum[i] / sp.mnubykT, sp.qc, nufrac_low, tid);
        __syncthreads();
        for(int half = SHQ_NULRA_LANES / 2; half >= 1; half >>= 1) {
            if(tid < half)
                nulra_fold(lanes, tid, half);
            __syncthreads();
        }
        integral = lanes[0];
    }
    if(tid == 0)
        A.partial[(size_t) s * A.nk_alloc + i] = nulra_delta_nu_single(A.wavenum[i], A.delta_nu_init[i], fsl_A0a, deriv_prefac, delta_nu_prefac, sp, integral);
}

} // namespace

/* the resident state: what the host owns (NuEngine) and the device arrays */
struct NuLraDev {
    NuEngine E;
    NuArr A = {};
    shq_context *ctx = nullptr;
    DevBuf<double> d, bins, tab, nodes, table, tmp, sums_up;
    DevBuf<int32_t> i32; /* [0] status, then nzidx */
    size_t node_cap = 0; /* nodes the device block holds */
    PinBuf<double> stage[2];
    hipEvent_t stage_ev[2] = {nullptr, nullptr}, ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    bool stage_used[2] = {false, false}, timed = false, timed_table = false;
    int cur = 0;
    PinBuf<int> status_host;
    int nz_nbins = 0, nnz = 0, kept = -1;

    hipStream_t stream() const { return ctx->stream; }

    int bind_state()
    {
        const size_t nk = (size_t) E.p.nk_allocated;
        SHQ_TRY(d.reserve((7 + (size_t) E.namax + 3) * nk));
        SHQ_HIP(hipMemsetAsync(d.ptr, 0, sizeof(double) * (7 + (size_t) E.namax + 3) * nk, stream()));
        double *q = d.ptr;
        A.nk_alloc = (int) nk;
        A.namax = E.namax;
        A.wavenum = q; q += nk;
        A.delta_nu_last = q; q += nk;
        A.delta_nu_init = q; q += nk;
        A.power_in = q; q += nk;
        A.ratio_raw = q; q += nk;
        A.logwav = q; q += nk;
        A.slope_w = q; q += nk;
        A.delta_tot = q; q += nk * E.namax;
        A.partial = q; q += 3 * nk;
        const int nt = (int) E.tlogk.size();
        SHQ_TRY(tab.reserve(3 * (size_t) nt));
        SHQ_HIP(hipMemcpy(tab.ptr, E.tlogk.data(), sizeof(double) * nt, hipMemcpyHostToDevice));
        SHQ_HIP(hipMemcpy(tab.ptr + nt, E.tT.data(), sizeof(double) * nt, hipMemcpyHostToDevice));
        SHQ_HIP(hipMemcpy(tab.ptr + 2 * nt, E.tslope.data(), sizeof(double) * nt, hipMemcpyHostToDevice));
        A.ntab = nt;
        A.tlogk = tab.ptr;
        A.tT = tab.ptr + nt;
        A.tslope = tab.ptr + 2 * nt;
        SHQ_TRY(bind_bins(std::max(E.p.nk_allocated, 8)));
        SHQ_TRY(status_host.reserve(1));
        status_host.ptr[0] = 0;
        SHQ_TRY(tmp.reserve(nk));
        /* room for the nodes of the longest history: 16 Na fs samples and Na knots, 30 levels, a few graded intervals */
        SHQ_TRY(reserve_nodes((size_t) SHQ_NULRA_GL * (19 * (size_t) E.namax + 64)));
        for(int b = 0; b < 2; b++)
            SHQ_HIP(hipEventCreateWithFlags(&stage_ev[b], hipEventDisableTiming));
        for(int e = 0; e < 5; e++)
            SHQ_HIP(hipEventCreate(&ev[e]));
        return SHQ_OK;
    }
    int bind_bins(int nb)
    {
        if(nb <= A.nbins_cap)
            return SHQ_OK;
        SHQ_TRY(bins.reserve(7 * (size_t) nb));
        SHQ_TRY(i32.reserve(1 + (size_t) nb));
        SHQ_HIP(hipMemsetAsync(i32.ptr, 0, sizeof(int32_t), stream()));
        double *q = bins.ptr;
        A.nbins_cap = nb;
        A.kk_nz = q; q += nb;
        A.pw_nz = q; q += nb;
        A.logk_nz = q; q += nb;
        A.logp_nz = q; q += nb;
        A.slope_nz = q; q += nb;
        A.ratio_nz = q; q += nb;
        A.slope_r = q; q += nb;
        A.status = i32.ptr;
        A.nzidx = i32.ptr + 1;
        nz_nbins = 0;
        return SHQ_OK;
    }
    /* doubles of a staged node block of n nodes: W, fs, h[4], scalefact[namax], then the intervals as int32 */
    size_t block_doubles(size_t n) const { return 6 * n + (size_t) E.namax + (n + 1) / 2; }
    int reserve_nodes(size_t n)
    {
        if(n <= node_cap)
            return SHQ_OK;
        n = std::max(n, node_cap + node_cap / 2);
        SHQ_HIP(hipStreamSynchronize(stream())); /* nothing may still read the blocks that go */
        SHQ_TRY(nodes.reserve(block_doubles(n)));
        for(int b = 0; b < 2; b++) {
            SHQ_TRY(stage[b].reserve(block_doubles(n)));
            stage_used[b] = false;
        }
        node_cap = n;
        return SHQ_OK;
    }
    void release()
    {
        (void) hipStreamSynchronize(stream());
        d.release(); bins.release(); tab.release(); nodes.release(); table.release(); tmp.release(); sums_up.release(); i32.release();
        stage[0].release(); stage[1].release(); status_host.release();
        for(int b = 0; b < 2; b++)
            if(stage_ev[b])
                (void) hipEventDestroy(stage_ev[b]);
        for(int e = 0; e < 5; e++)
            if(ev[e])
                (void) hipEventDestroy(ev[e]);
    }

    /* ---- the backend of nulra_engine_step ---- */
    int load_bins(const double *sums, int nbins, double BoxMpc, int *out_nnz)
    {
        SHQ_CHECK(sums && nbins >= 4 && nbins <= (1 << 20), SHQ_ERR_INVALID, "nulra_step: null sums or %d bins", nbins);
        SHQ_TRY(bind_bins(nbins));
        if(nz_nbins != nbins) { /* the non-empty bins depend on Nmesh alone: found once, from the mode counts */
            std::vector<int64_t> nm((size_t) nbins);
            SHQ_HIP(hipMemcpyAsync(nm.data(), sums + 2 * (size_t) nbins, sizeof(int64_t) * nbins, hipMemcpyDeviceToHost, stream()));
            SHQ_HIP(hipStreamSynchronize(stream()));
            std::vector<int32_t> idx;
            for(int b = 0; b < nbins; b++)
                if(nm[b] != 0)
                    idx.push_back(b);
            nnz = (int) idx.size();
            if(nnz > 0)
                SHQ_HIP(hipMemcpy(A.nzidx, idx.data(), sizeof(int32_t) * nnz, hipMemcpyHostToDevice));
            nz_nbins = nbins;
        }
        const NuArr a = A;
        SHQ_TRY(nulra_for(stream(), nnz, [=] __device__(int i) { nulra_op_compact(a, sums, nbins, BoxMpc, i); }));
        *out_nnz = nnz;
        return SHQ_OK;
    }
    int last_wavenumber(int n, double *k)
    {
        SHQ_HIP(hipMemcpyAsync(k, A.kk_nz + n - 1, sizeof(double), hipMemcpyDeviceToHost, stream()));
        SHQ_HIP(hipStreamSynchronize(stream()));
        return SHQ_OK;
    }
    int first_init(int nk, double OmegaNua3, double Omeganonu, double OmegaNu1, double partnu)
    {
        const NuArr a = A;
        return nulra_for(stream(), nk, [=] __device__(int i) { nulra_op_first_init(a, i, OmegaNua3, Omeganonu, OmegaNu1, partnu); });
    }
    int power_in(int rebin, int n, int nk, int ia)
    {
        const NuArr a = A;
        if(rebin)
            SHQ_TRY(nulra_for(stream(), n, [=] __device__(int i) { nulra_op_slope_nz(a, n, i); }));
        return nulra_for(stream(), nk, [=] __device__(int i) { nulra_op_power_in(a, i, rebin, n, ia); });
    }
    int update_delta_tot(int nk, int col, double OmegaNua3, double Omeganonu, double OmegaNu1, double partnu)
    {
        const NuArr a = A;
        return nulra_for(stream(), nk, [=] __device__(int i) { nulra_op_update(a, i, col, OmegaNua3, Omeganonu, OmegaNu1, partnu); });
    }
    int delta_nu(const NuNodeTable &T, int Na, const double *sf, double deriv_prefac, double delta_nu_prefac, double nufrac_low, const NuSpecies *S, int ns,
                 int nk)
    {
        const size_t n = (size_t) T.n;
        SHQ_TRY(reserve_nodes(n));
        /* stage the block in the pinned buffer whose last upload is over (two steps back in a steady run) */
        const int b = cur;
        cur ^= 1;
        if(stage_used[b])
            SHQ_HIP(hipEventSynchronize(stage_ev[b]));
        double *h = stage[b].ptr;
        if(n > 0) {
            memcpy(h, T.W.data(), sizeof(double) * n);
            memcpy(h + n, T.fs.data(), sizeof(double) * n);
            memcpy(h + 2 * n, T.h.data(), sizeof(double) * 4 * n);
        }
        memcpy(h + 6 * n, sf, sizeof(double) * (size_t) std::max(Na, 1));
        if(n > 0)
            memcpy(h + 6 * n + E.namax, T.iv.data(), sizeof(int32_t) * n);
        SHQ_HIP(hipEventRecord(ev[0], stream()));
        SHQ_HIP(hipMemcpyAsync(nodes.ptr, h, sizeof(double) * block_doubles(n), hipMemcpyHostToDevice, stream()));
        SHQ_HIP(hipEventRecord(stage_ev[b], stream()));
        stage_used[b] = true;
        SHQ_HIP(hipEventRecord(ev[1], stream()));
        const NuNodes N{(int) n, nodes.ptr, nodes.ptr + n, nodes.ptr + 2 * n, reinterpret_cast<const int32_t *>(nodes.ptr + 6 * n + E.namax)};
        NuSpecies3 S3 = {};
        double frac[SHQ_NULRA_NUSPECIES] = {0, 0, 0};
        for(int s = 0; s < ns; s++) {
            S3.s[s] = S[s];
            frac[s] = S[s].frac;
        }
        if(ns > 0 && nk > 0) {
            const size_t lds = sizeof(double) * ((size_t) nulra_row_len(Na) + SHQ_NULRA_LANES);
            nulra_delta_nu_kernel<<<dim3((unsigned) nk, (unsigned) ns), dim3(SHQ_NULRA_LANES), lds, stream()>>>(A, N, nodes.ptr + 6 * n, Na, T.fsl_A0a, deriv_prefac,
                                                                                                               delta_nu_prefac, nufrac_low, S3);
            SHQ_HIP(hipGetLastError());
        }
        const NuArr a = A;
        const double f0 = frac[0], f1 = frac[1], f2 = frac[2];
        SHQ_TRY(nulra_for(stream(), nk, [=] __device__(int i) {
            const double f[SHQ_NULRA_NUSPECIES] = {f0, f1, f2};
            nulra_op_combine(a, i, ns, f);
        }));
        SHQ_HIP(hipEventRecord(ev[2], stream()));
        timed = true;
        return SHQ_OK;
    }
    int finish(int rebin, int n, int nk)
    {
        const NuArr a = A;
        SHQ_TRY(nulra_for(stream(), nk, [=] __device__(int i) { nulra_op_ratio_raw(a, i); }));
        if(rebin)
            SHQ_TRY(nulra_for(stream(), nk, [=] __device__(int i) { nulra_op_slope_w(a, nk, i); }));
        SHQ_TRY(nulra_for(stream(), n, [=] __device__(int i) { nulra_op_ratio_nz(a, i, rebin, nk); }));
        return nulra_for(stream(), n, [=] __device__(int i) { nulra_op_slope_r(a, n, i); });
    }

    /* T[k2] = add + nu_prefac spline(log |k|) for k2 = 1 .. nk2 - 1, T[0] = add, into device memory */
    int fill_table(int Nmesh, double add, double *d_out)
    {
        const long long nk2 = 3ll * (Nmesh / 2) * (Nmesh / 2) + 1;
        const NuArr a = A;
        const int n = E.nnz;
        const double prefac = E.nu_prefac, box = E.p.BoxSize_in_MPC;
        return nulra_for(stream(), (int) nk2, [=] __device__(int k2) {
            d_out[k2] = k2 == 0 ? add : add + nulra_mode_factor(n, a.logk_nz, a.ratio_nz, a.slope_r, prefac, box, k2);
        });
    }
    /* the sticky NaN status as the last finished copy shows it; sync: wait for the device first */
    int check_status(bool sync)
    {
        if(sync) {
            SHQ_HIP(hipMemcpyAsync(status_host.ptr, A.status, sizeof(int), hipMemcpyDeviceToHost, stream()));
            SHQ_HIP(hipStreamSynchronize(stream()));
        }
        SHQ_CHECK(status_host.ptr[0] == 0, SHQ_ERR_DEVICE, "nulra: a step left a NaN in delta_nu_last");
        return SHQ_OK;
    }
};

#define NU_STATE(D)                                                                                \
    SHQ_CHECK(ctx, SHQ_ERR_INVALID, "null context");                                               \
    SHQ_CHECK(ctx->nulra, SHQ_ERR_STATE, "nulra: shq_nulra_init first");                           \
    SHQ_HIP(hipSetDevice(ctx->device));                                                            \
    NuLraDev &D = *ctx->nulra

extern "C" int shq_nulra_free(shq_context *ctx)
{
    SHQ_CHECK(ctx, SHQ_ERR_INVALID, "null context");
    if(ctx->nulra) {
        (void) hipSetDevice(ctx->device);
        ctx->nulra->release();
        delete ctx->nulra;
        ctx->nulra = nullptr;
    }
    return SHQ_OK;
}

extern "C" int shq_nulra_init(shq_context *ctx, const shq_nulra_params *params)
{
    SHQ_CHECK(ctx, SHQ_ERR_INVALID, "null context");
    SHQ_HIP(hipSetDevice(ctx->device));
    SHQ_TRY(shq_nulra_free(ctx));
    NuLraDev *D = new NuLraDev();
    D->ctx = ctx;
    int rc = nulra_engine_init(D->E, params);
    if(rc == SHQ_OK)
        rc = D->bind_state();
    if(rc != SHQ_OK) {
        D->release();
        delete D;
        return rc;
    }
    ctx->nulra = D;
    return SHQ_OK;
}

extern "C" int shq_nulra_step(shq_context *ctx, double Time, double TimeIC, const void *d_sums, int nbins)
{
    NU_STATE(D);
    SHQ_TRY(D.check_status(false));
    const double *sums = (const double *) d_sums;
    if(!sums) {
        SHQ_CHECK(ctx->pm_spec_pending && ctx->have_power, SHQ_ERR_STATE, "nulra_step: no pending spectrum (shq_pm_forward first)");
        sums = ctx->ps_sums.ptr;
        nbins = ctx->ps_nbins;
    } else {
        SHQ_CHECK(nbins >= 4 && nbins <= (1 << 20), SHQ_ERR_INVALID, "nulra_step: %d bins", nbins);
        if(ctx->pm_spec_pending)
            SHQ_CHECK(nbins == ctx->pm_spec_params.Nmesh, SHQ_ERR_INVALID, "nulra_step: %d bins, the pending spectrum has Nmesh %d", nbins,
                      ctx->pm_spec_params.Nmesh);
        /* sums in host memory (a caller that reduced them on the host): uploaded, and this step waits for the copy */
        hipPointerAttribute_t at;
        const hipError_t e = hipPointerGetAttributes(&at, sums);
        if(e != hipSuccess)
            (void) hipGetLastError();
        if(e != hipSuccess || (at.type != hipMemoryTypeDevice && at.type != hipMemoryTypeManaged)) {
            const size_t n = 3 * (size_t) nbins + 1;
            SHQ_TRY(D.sums_up.reserve(n));
            SHQ_HIP(hipMemcpyAsync(D.sums_up.ptr, sums, sizeof(double) * n, hipMemcpyHostToDevice, ctx->stream));
            SHQ_HIP(hipStreamSynchronize(ctx->stream));
            sums = D.sums_up.ptr;
        }
    }
    SHQ_TRY(shq_join_pm(ctx)); /* the forward's sums */
    D.timed = D.timed_table = false;
    const auto t0 = std::chrono::steady_clock::now();
    SHQ_TRY(nulra_engine_step(D.E, D, Time, TimeIC, sums, nbins, &D.kept));
    D.E.callback_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if(ctx->pm_spec_pending) { /* the rules of shq_pm_set_mode_factor: for this spectrum only, the finish consumes it */
        const int Nmesh = ctx->pm_spec_params.Nmesh;
        SHQ_TRY(ctx->pm_fac.reserve(3 * (size_t) (Nmesh / 2) * (Nmesh / 2) + 1));
        SHQ_HIP(hipEventRecord(D.ev[3], ctx->stream));
        SHQ_TRY(D.fill_table(Nmesh, 1.0, ctx->pm_fac.ptr));
        SHQ_HIP(hipEventRecord(D.ev[4], ctx->stream));
        D.timed_table = true;
        ctx->pm_fac_set = true;
    }
    SHQ_HIP(hipMemcpyAsync(D.status_host.ptr, D.A.status, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    return SHQ_OK;
}

extern "C" int shq_nulra_mode_table(shq_context *ctx, int Nmesh, int add_one, double *table)
{
    NU_STATE(D);
    SHQ_CHECK(table, SHQ_ERR_INVALID, "null argument");
    SHQ_CHECK(D.E.have_step, SHQ_ERR_STATE, "nulra_mode_table: no step yet");
    SHQ_CHECK(Nmesh >= 2 && Nmesh % 2 == 0 && Nmesh <= 16384, SHQ_ERR_INVALID, "nulra_mode_table: Nmesh %d", Nmesh);
    const size_t nk2 = 3 * (size_t) (Nmesh / 2) * (Nmesh / 2) + 1;
    SHQ_TRY(D.table.reserve(nk2));
    SHQ_TRY(D.fill_table(Nmesh, add_one ? 1.0 : 0.0, D.table.ptr));
    SHQ_HIP(hipMemcpyAsync(table, D.table.ptr, sizeof(double) * nk2, hipMemcpyDeviceToHost, ctx->stream));
    return D.check_status(true);
}

extern "C" int shq_nulra_download(shq_context *ctx, double *delta_nu_last, double *kk, shq_nulra_info *info)
{
    NU_STATE(D);
    if(delta_nu_last && D.E.nk > 0)
        SHQ_HIP(hipMemcpyAsync(delta_nu_last, D.A.delta_nu_last, sizeof(double) * D.E.nk, hipMemcpyDeviceToHost, ctx->stream));
    if(kk && D.E.nnz > 0)
        SHQ_HIP(hipMemcpyAsync(kk, D.A.kk_nz, sizeof(double) * D.E.nnz, hipMemcpyDeviceToHost, ctx->stream));
    const int rc = D.check_status(true);
    if(info) {
        nulra_fill_info(D.E, D.kept, info);
        float ms = 0;
        if(D.timed) {
            if(hipEventElapsedTime(&ms, D.ev[0], D.ev[1]) == hipSuccess)
                info->ms[0] = ms;
            if(hipEventElapsedTime(&ms, D.ev[1], D.ev[2]) == hipSuccess)
                info->ms[1] = ms;
        }
        if(D.timed_table && hipEventElapsedTime(&ms, D.ev[3], D.ev[4]) == hipSuccess)
            info->ms[2] = ms;
    }
    return rc;
}

extern "C" int shq_nulra_delta_nu(shq_context *ctx, double a, double *delta_nu)
{
    NU_STATE(D);
    SHQ_CHECK(delta_nu, SHQ_ERR_INVALID, "null argument");
    SHQ_CHECK(D.E.ia >= 1 && D.E.nk >= 1, SHQ_ERR_STATE, "nulra_delta_nu: the history is empty");
    SHQ_CHECK(std::isfinite(a) && a > 0, SHQ_ERR_INVALID, "nulra_delta_nu: a = %g", a);
    const size_t bytes = sizeof(double) * D.E.nk;
    SHQ_HIP(hipMemcpyAsync(D.tmp.ptr, D.A.delta_nu_last, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    SHQ_TRY(nulra_delta_nu_combined(D.E, D, a));
    SHQ_HIP(hipMemcpyAsync(delta_nu, D.A.delta_nu_last, bytes, hipMemcpyDeviceToHost, ctx->stream));
    SHQ_HIP(hipMemcpyAsync(D.A.delta_nu_last, D.tmp.ptr, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    SHQ_HIP(hipStreamSynchronize(ctx->stream));
    return SHQ_OK;
}

extern "C" int shq_nulra_get_state(shq_context *ctx, shq_nulra_state *st)
{
    NU_STATE(D);
    SHQ_CHECK(st, SHQ_ERR_INVALID, "null argument");
    const NuEngine &E = D.E;
    st->ia = E.ia;
    st->nk = E.nk;
    if(E.ia == 0 || E.nk == 0)
        return SHQ_OK;
    hipStream_t s = ctx->stream;
    if(st->scalefact)
        memcpy(st->scalefact, E.scalefact.data(), sizeof(double) * E.ia);
    if(st->delta_tot)
        SHQ_HIP(hipMemcpy2DAsync(st->delta_tot, sizeof(double) * E.ia, D.A.delta_tot, sizeof(double) * D.A.namax, sizeof(double) * E.ia, (size_t) E.nk,
                                 hipMemcpyDeviceToHost, s));
    if(st->delta_nu_init)
        SHQ_HIP(hipMemcpyAsync(st->delta_nu_init, D.A.delta_nu_init, sizeof(double) * E.nk, hipMemcpyDeviceToHost, s));
    if(st->kvalue)
        SHQ_HIP(hipMemcpyAsync(st->kvalue, D.A.wavenum, sizeof(double) * E.nk, hipMemcpyDeviceToHost, s));
    if(st->delta_nu_last)
        SHQ_HIP(hipMemcpyAsync(st->delta_nu_last, D.A.delta_nu_last, sizeof(double) * E.nk, hipMemcpyDeviceToHost, s));
    return D.check_status(true);
}

extern "C" int shq_nulra_set_state(shq_context *ctx, const shq_nulra_state *st)
{
    NU_STATE(D);
    SHQ_CHECK(st && st->scalefact && st->delta_tot && st->delta_nu_init && st->kvalue, SHQ_ERR_INVALID, "null argument");
    NuEngine &E = D.E;
    SHQ_CHECK(st->nk >= 1 && st->ia >= 1 && st->nk <= E.p.nk_allocated && st->ia <= E.namax, SHQ_ERR_INVALID,
              "nulra_set_state: allocated nk %d na %d for neutrino power but need nk %d na %d", E.p.nk_allocated, E.namax, st->nk, st->ia);
    hipStream_t s = ctx->stream;
    E.ia = st->ia;
    E.nk = st->nk;
    memcpy(E.scalefact.data(), st->scalefact, sizeof(double) * E.ia);
    SHQ_HIP(hipMemcpy2DAsync(D.A.delta_tot, sizeof(double) * D.A.namax, st->delta_tot, sizeof(double) * E.ia, sizeof(double) * E.ia, (size_t) E.nk,
                             hipMemcpyHostToDevice, s));
    SHQ_HIP(hipMemcpyAsync(D.A.delta_nu_init, st->delta_nu_init, sizeof(double) * E.nk, hipMemcpyHostToDevice, s));
    SHQ_HIP(hipMemcpyAsync(D.A.wavenum, st->kvalue, sizeof(double) * E.nk, hipMemcpyHostToDevice, s));
    E.kmax = *std::max_element(st->kvalue, st->kvalue + E.nk);
    E.init_done = st->delta_nu_last != nullptr;
    if(st->delta_nu_last)
        SHQ_HIP(hipMemcpyAsync(D.A.delta_nu_last, st->delta_nu_last, sizeof(double) * E.nk, hipMemcpyHostToDevice, s));
    E.have_step = false;
    SHQ_HIP(hipStreamSynchronize(s)); /* the caller's arrays are free when the call returns */
    return SHQ_OK;
}
