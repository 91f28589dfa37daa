/* call_scope.hpp — what one call of a mesh or particle operator owns on the device: buffers, hipFFT plans and the events of its
 * phase timers, given back on every way out of the call. */
#pragma once
#include "common.hpp"

struct CallScope {
    shq_context *ctx;
    const char *who; /* the operator's name: opens every error text */
    std::vector<void *> bufs;
    std::vector<hipfftHandle> plans;
    std::vector<hipEvent_t> ev;
    CallScope(shq_context *c, const char *w) : ctx(c), who(w) {}
    CallScope(const CallScope &) = delete;
    CallScope &operator=(const CallScope &) = delete;

    /* n elements (one at least) of device memory */
    template <typename T> int alloc(T **p, size_t n)
    {
        *p = nullptr;
        const hipError_t e = hipMalloc((void **) p, (n ? n : 1) * sizeof(T));
        if(e != hipSuccess) {
            shq_set_error("%s: hipMalloc of %zu bytes failed: %s", who, n * sizeof(T), hipGetErrorString(e));
            *p = nullptr;
            return SHQ_ERR_NOMEM;
        }
        bufs.push_back((void *) *p);
        return SHQ_OK;
    }
    /* a plan on the context's stream; the scope owns the handle from the moment it exists */
    int plan3d(int N, hipfftType type, hipfftHandle *h)
    {
        const hipfftResult r = hipfftPlan3d(h, N, N, N, type);
        SHQ_CHECK(r == HIPFFT_SUCCESS, SHQ_ERR_DEVICE, "%s: hipfftPlan3d(%s, %d) failed: %d", who, type == HIPFFT_D2Z ? "D2Z" : "Z2D", N, (int) r);
        return own(*h);
    }
    int plan_many(int rank, int *dims, hipfftType type, int batch, hipfftHandle *h)
    {
        const hipfftResult r = hipfftPlanMany(h, rank, dims, nullptr, 1, 0, nullptr, 1, 0, type, batch);
        SHQ_CHECK(r == HIPFFT_SUCCESS, SHQ_ERR_DEVICE, "%s: hipfftPlanMany(%d x %d, batch %d) failed: %d", who, dims[0], dims[rank - 1], batch, (int) r);
        return own(*h);
    }
    /* a new event, recorded on s: event number ev.size() - 1 */
    int mark(hipStream_t s)
    {
        hipEvent_t e = nullptr;
        SHQ_HIP(hipEventCreate(&e));
        ev.push_back(e);
        SHQ_HIP(hipEventRecord(e, s));
        return SHQ_OK;
    }
    /* milliseconds from event a to event b, 0 where the runtime cannot say */
    double ms(size_t a, size_t b) const
    {
        float t = 0;
        if(a >= ev.size() || b >= ev.size() || hipEventElapsedTime(&t, ev[a], ev[b]) != hipSuccess)
            t = 0;
        return t;
    }
    /* between the last two marks */
    double last_ms() const { return ev.size() >= 2 ? ms(ev.size() - 2, ev.size() - 1) : 0.0; }
    /* The stream drains first, so that nothing in flight still uses what is freed.  hipFree synchronises the device by itself, so a
     * scope that used to free without draining (heiii's) behaves as before. */
    ~CallScope()
    {
        (void) hipStreamSynchronize(ctx->stream);
        for(void *b : bufs)
            (void) hipFree(b);
        for(hipfftHandle h : plans)
            hipfftDestroy(h);
        for(hipEvent_t e : ev)
            (void) hipEventDestroy(e);
    }

private:
    int own(hipfftHandle h)
    {
        plans.push_back(h);
        SHQ_CHECK(hipfftSetStream(h, ctx->stream) == HIPFFT_SUCCESS, SHQ_ERR_DEVICE, "%s: hipfftSetStream failed", who);
        return SHQ_OK;
    }
};
