/* recalgo_feed.h — a C-ABI header of librecalgo_hip.so: the scatter's `prepare` launch that also FEEDS a captured step, i.e.
 * moves the step's batch into the graph's static input span by further workgroups of the same grid.  Self-contained (it repeats
 * the stream typedef: an identical typedef twice is valid C11 and C++); the descriptors are those of recalgo.h and are declared
 * `const void*` here, each with the type it points to.  The conventions are those of recalgo.h: hipError_t as int, asynchronous
 * on `stream`, no hidden allocation, no host read-back, descriptor arrays are HOST arrays read at launch time.
 */
#ifndef RECALGO_FEED_H_
#define RECALGO_FEED_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* recalgo_stream_t; /* hipStream_t */

/* ABI version of THIS header; include/recalgo_feed.abi records the hash of the declarations each version stands for. */
#define RECALGO_FEED_ABI_VERSION 1
int recalgo_feed_abi_version(void);

/* recalgo_scatter_prepare (n_sources <= 1; sources == NULL or n_sources == 0: no lookup, as its source == NULL; a companion arena
 * may ride) or recalgo_scatter_prepare_multi (n_sources 2 .. 4, companion_deferred NULL and companion_rows 0), both recalgo.h, in
 * the SAME single launch and with the same results, which also writes  feed_dst[0, feed_bytes) = feed_src[0, feed_bytes)  by
 * workgroups of their own, the last of the grid (16 bytes per thread between a head and a tail of single bytes: any length).
 *   sources              const recalgo_scatter_source_t[n_sources]
 *   first_requests       int64_t[n_sources]: the first plan slot of every source (recalgo_scatter_prepare's first_request)
 *   deferred, companion_deferred    const recalgo_deferred_adam_t*, or NULL
 *   every argument from K to step_offset: that of recalgo_scatter_prepare
 *   feed_dst, feed_src   device spans of feed_bytes bytes in the same 16-byte phase and disjoint.  feed_src == NULL,
 *                        feed_bytes == 0 or feed_dst == feed_src: nothing is copied, the launch is exactly that of the entries
 *                        above.  No workgroup of the launch reads feed_dst: a caller that feeds a step's id matrix points the
 *                        sources' `ids` INTO feed_src, and whatever is enqueued behind the launch reads feed_dst.
 * recalgo_scatter_prepare_feed_supported -> 1 when the launch accepts the feed, 0 when it refuses it: feed_bytes < 0, a copy with
 * feed_dst NULL, the two spans in different 16-byte phases, or overlapping without being the same.  A refused feed returns
 * hipErrorInvalidValue before anything is launched. */
int recalgo_scatter_prepare_feed_supported(const void* feed_dst, const void* feed_src, int64_t feed_bytes);
int recalgo_scatter_prepare_feed(const void* sources, int n_sources, const int64_t* first_requests, int K, void* plan_workspace,
                                 int64_t plan_requests, int nb_log2, int flags, const void* deferred,
                                 const void* companion_deferred, int64_t rows, int64_t companion_rows, int sweep_period,
                                 const int64_t* step_dev, int step_offset, void* feed_dst, const void* feed_src,
                                 int64_t feed_bytes, recalgo_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* RECALGO_FEED_H_ */
