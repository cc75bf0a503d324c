/*
 * lachesis_mediantime.h -- C ABI of MedianTime on the HIP index.
 *
 * The reference's vecengine is generic over its vectors (vecengine/vector.go:
 * 8-22, vecengine/index.go:16-25) so that a caller can carry more than seqs
 * along HighestBefore.  The production consumers of lachesis-base carry each
 * event's creation time beside HighestBeforeSeq ("vecmt") and ask
 * MedianTime(atropos, genesisTime): the stake-weighted median of the creation
 * times of the highest events the Atropos observes -- the block's timestamp.
 *
 * The library carries no time plane.  hb[e][j] is the highest seq of branch j
 * that e observes, and a branch is a self-parent chain of consecutive seqs, so
 * (branch, seq) names exactly one event: the time vecmt carries for branch j
 * is that event's creation time.  The caller hands the creation time of every
 * event over once (lx_mt_set_times, keyed by dense index); the queries gather
 * from the index's HighestBefore plane on the device.
 *
 * Merged time vector of event e (V entries, validator idx order; the gather
 * of GetMergedHighestBefore, vecengine/index.go:235-250, vecfc/vector_ops.go:
 * 81-96):
 *   - e sees validator v as fork-detected: (fork, time 0);
 *   - else, over v's branches in BranchIDByCreators order, the first branch
 *     with the strictly greatest observed seq s: s = 0 gives (unobserved,
 *     time 0), else (s, creation time of the event of that branch at seq s).
 * MedianTime(e, default_time): per validator the pair (time, weight) =
 * (0, 0) for a fork, (default_time, weight) when unobserved, else (merged
 * time, weight); honest = the sum of those weights, half = honest / 2; the
 * pairs in ascending time (unsigned), the time of the first pair at which the
 * running weight is >= half.  With half = 0 that is the smallest time of all V
 * pairs, the cheaters' zeros included.
 *
 * Conventions of lachesis_hip.h (dense event indices of the index's epoch,
 * validator idx order, caller-owned buffers, 0 = ok / < 0 = error, one host
 * thread per handle and its index).  Up to 8192 validators.
 *
 * The handle follows its index by itself:
 *   - lx_reset of the index (a new epoch) or a reload (lx_load_rows): no times
 *     are held any more; the new validators are taken over;
 *   - lx_drop_not_flushed that dropped events (directly, or inside the abft
 *     handle: lx_abft_build, a wrong claimed frame): dense indices at or above
 *     the flushed count name other events afterwards, so every time at or
 *     above it is forgotten, whether it was set ahead of Add or not.  Set them
 *     again with the events added in their place.  lx_abft_build_frames asks
 *     the same question without adding the event: it does not roll back, and
 *     times set ahead stay.
 * Nothing about times is persisted: after a restart (lx_load_rows /
 * lx_load_finish) the caller sets the times of the loaded events again.
 *
 * The queries only read the index, so unlike any call into an lx_abft handle
 * they may be made from inside the begin_block, apply_event and end_block
 * callbacks of lx_abft_process_batch (a block's time is asked in BeginBlock,
 * and a sealing block resets the index right after EndBlock).
 * lx_mt_set_times may be called there too.
 *
 * Out of scope: column-sharded and row-segment handles (LX_ERR_STATE),
 * vecmt's raw per-branch time rows (the time of a fork-marked entry is stale
 * and depends on parent order; neither the merged vector nor the median reads
 * it), persistence of times.
 */
#ifndef LACHESIS_MEDIANTIME_H
#define LACHESIS_MEDIANTIME_H

#include "lachesis_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lx_mt lx_mt;

/* For the index's current validators.  LX_ERR_STATE for a column shard or a
 * row-segment rank, LX_ERR_ARG for more than 8192 validators. */
int lx_mt_create(lx_index *index, lx_mt **out);
void lx_mt_destroy(lx_mt *m);
const char *lx_mt_last_error(const lx_mt *m);
/* New epoch: validators from the index, no times held. */
int lx_mt_reset(lx_mt *m);

/* Creation times of the dense events [first_event, first_event + n).
 * first_event <= lx_mt_num_times (no holes; earlier entries may be
 * overwritten).  The range may run ahead of lx_num_events: the table is keyed
 * by dense index, so a batch's times can be handed over before the batch is
 * added.  The times live in device memory. */
int lx_mt_set_times(lx_mt *m, uint64_t first_event, uint64_t n, const uint64_t *creation_time);
/* Times held: events [0, lx_mt_num_times) have one. */
uint64_t lx_mt_num_times(lx_mt *m);

/* MedianTime of n events, one launch.  LX_ERR_STATE "time not set" for
 * ev[i] >= lx_mt_num_times (events are added parents first, so every event
 * ev[i] observes has a lower index and this one check covers them; it is made
 * first, so an index a rollback dropped answers this), LX_ERR_ARG "unknown
 * event" for ev[i] >= lx_num_events. */
int lx_mt_median_time(lx_mt *m, uint32_t n, const uint32_t *ev, uint64_t default_time, uint64_t *out);
/* Merged times of n events, row-major: out[i * V + v]; 0 for a fork-detected
 * or unobserved validator.  On a little-endian host row i is vecmt's merged
 * HighestBeforeTime byte layout (8 bytes LE per validator).  Errors as above. */
int lx_mt_merged_times(lx_mt *m, uint32_t n, const uint32_t *ev, uint64_t *out);

#ifdef __cplusplus
}
#endif
#endif
