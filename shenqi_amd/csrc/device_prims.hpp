/* device_prims.hpp — the device sort / select / scan calls of the library and their scratch.
 *
 * Every helper asks rocPRIM for its scratch size, reserves ctx->prim_temp and makes the call, on ctx->stream.
 * The one scratch buffer is sound only because every call is ordered on ctx->stream: a caller on another stream needs a buffer of its own.
 *
 * Counts (select, partition): d_count is the caller's device word, or null for a word the helper owns.  A non-null host_count makes the
 * helper copy the count to the host and synchronise the stream; with a null one the count stays on the device and nothing waits.
 * n == 0 enqueues no primitive: the count (the caller's device word, *host_count) is 0. */
#ifndef SHQ_DEVICE_PRIMS_HPP
#define SHQ_DEVICE_PRIMS_HPP

#include "common.hpp"
#include <iterator>
#include <rocprim/device/device_partition.hpp>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/functional.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

/* Bytes of ctx->prim_temp behind every request.  They keep the scratch pointer non-null when a primitive asks for zero bytes (rocPRIM
 * reads a null scratch pointer as a size query and would do no work), and they hold the helpers' own count word. */
#define SHQ_PRIM_PAD 16

/* `tmp` bytes of scratch, contents undefined: valid until the next helper call on this context (shq_context::prim_temp) */
inline int prim_scratch(shq_context *ctx, size_t tmp, void **scratch)
{
    SHQ_TRY(ctx->prim_temp.reserve(tmp + SHQ_PRIM_PAD));
    *scratch = ctx->prim_temp.ptr;
    return SHQ_OK;
}

/* size query, scratch, call; call(scratch, tmp, d_count) is the rocPRIM call with everything else bound */
template <typename Call> inline int prim_run(shq_context *ctx, size_t n, unsigned long long *d_count, int64_t *host_count, Call call)
{
    if(host_count)
        *host_count = 0;
    if(n == 0) {
        if(d_count)
            SHQ_HIP(hipMemsetAsync(d_count, 0, sizeof(*d_count), ctx->stream));
        return SHQ_OK;
    }
    size_t tmp = 0;
    void *scratch = nullptr;
    SHQ_HIP(call(scratch, tmp, d_count));
    SHQ_TRY(prim_scratch(ctx, tmp, &scratch));
    if(!d_count)
        d_count = reinterpret_cast<unsigned long long *>(ctx->prim_temp.ptr + ((tmp + 7) & ~size_t(7))); /* in the pad, 8-byte aligned */
    SHQ_HIP(call(scratch, tmp, d_count));
    if(host_count) {
        unsigned long long h = 0;
        SHQ_HIP(hipMemcpyAsync(&h, d_count, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
        SHQ_HIP(hipStreamSynchronize(ctx->stream));
        *host_count = (int64_t) h;
    }
    return SHQ_OK;
}

/* stable sort of (key, value) pairs by the key bits [begin_bit, end_bit); vin may be any iterator */
template <typename KeyIn, typename KeyOut, typename ValIn, typename ValOut>
inline int prim_sort_pairs(shq_context *ctx, KeyIn kin, KeyOut kout, ValIn vin, ValOut vout, size_t n, unsigned begin_bit, unsigned end_bit)
{
    return prim_run(ctx, n, nullptr, nullptr, [&](void *scratch, size_t &tmp, unsigned long long *) {
        return rocprim::radix_sort_pairs(scratch, tmp, kin, kout, vin, vout, n, begin_bit, end_bit, ctx->stream);
    });
}

template <typename KeyIn, typename KeyOut> inline int prim_sort_keys(shq_context *ctx, KeyIn in, KeyOut out, size_t n, unsigned begin_bit, unsigned end_bit)
{
    return prim_run(ctx, n, nullptr, nullptr, [&](void *scratch, size_t &tmp, unsigned long long *) {
        return rocprim::radix_sort_keys(scratch, tmp, in, out, n, begin_bit, end_bit, ctx->stream);
    });
}

/* the items of `in` that pred accepts, order kept */
template <typename In, typename Out, typename Pred>
inline int prim_select_if(shq_context *ctx, In in, Out out, size_t n, Pred pred, unsigned long long *d_count, int64_t *host_count)
{
    return prim_run(ctx, n, d_count, host_count, [&](void *scratch, size_t &tmp, unsigned long long *d_n) {
        return rocprim::select(scratch, tmp, in, out, d_n, n, pred, ctx->stream);
    });
}

/* the items of `in` whose flag is set, order kept */
template <typename In, typename Flags, typename Out>
inline int prim_select_flagged(shq_context *ctx, In in, Flags flags, Out out, size_t n, unsigned long long *d_count, int64_t *host_count)
{
    return prim_run(ctx, n, d_count, host_count, [&](void *scratch, size_t &tmp, unsigned long long *d_n) {
        return rocprim::select(scratch, tmp, in, flags, out, d_n, n, ctx->stream);
    });
}

/* flagged items to out_sel, the others to out_rej, order kept in both; the count is that of out_sel */
template <typename In, typename Flags, typename OutSel, typename OutRej>
inline int prim_partition_two_way(shq_context *ctx, In in, Flags flags, OutSel out_sel, OutRej out_rej, size_t n, unsigned long long *d_count,
                                  int64_t *host_count)
{
    return prim_run(ctx, n, d_count, host_count, [&](void *scratch, size_t &tmp, unsigned long long *d_n) {
        return rocprim::partition_two_way(scratch, tmp, in, flags, out_sel, out_rej, d_n, n, ctx->stream);
    });
}

/* sums with rocprim::plus of the type of init / of the input's values */
template <typename In, typename Out, typename T> inline int prim_exclusive_scan(shq_context *ctx, In in, Out out, T init, size_t n)
{
    return prim_run(ctx, n, nullptr, nullptr, [&](void *scratch, size_t &tmp, unsigned long long *) {
        return rocprim::exclusive_scan(scratch, tmp, in, out, init, n, rocprim::plus<T>(), ctx->stream);
    });
}

template <typename In, typename Out> inline int prim_inclusive_scan(shq_context *ctx, In in, Out out, size_t n)
{
    using T = typename std::iterator_traits<In>::value_type;
    return prim_run(ctx, n, nullptr, nullptr, [&](void *scratch, size_t &tmp, unsigned long long *) {
        return rocprim::inclusive_scan(scratch, tmp, in, out, n, rocprim::plus<T>(), ctx->stream);
    });
}

#endif
