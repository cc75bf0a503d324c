/*
 * lachesis_ancestry.h -- C ABI of ancestry queries on the HIP index: the set
 * of events a block confirms, read from the vector clock.
 *
 * The reference walks the DAG for this: Engine.DfsSubgraph(head, walk)
 * (vecengine/traversal.go:10-37) and, the same traversal, Lachesis.
 * confirmEvents (abft/lachesis.go:40-55, abft/traversal.go:13-37), which gives
 * every not yet confirmed ancestor of a decided Atropos the decided frame --
 * one store get and one put per visited event.
 *
 * The index holds the answer already.  For events x <= a in Add order (a
 * later event is never an ancestor):
 *   - x is a or an ancestor of a  <=>  0 < LowestAfter(x)[branch(a)] <= seq(a).
 *     Always exact: LowestAfter is set by the reference's DFS whatever the
 *     fork markers, and a branch is a chain of consecutive seqs.
 *   - x is a or an ancestor of a  <=>  HighestBefore(a)[branch(x)].Seq >=
 *     seq(x), wherever that entry is no fork marker.
 * The queries read one HighestBefore entry per pair and fall back to the
 * LowestAfter entry where a sees the creator of x as a cheater.  No parent
 * list is read and no stack is kept.
 *
 * Labels.  The handle keeps one 32-bit label per dense event in device
 * memory, 0 = none: the confirmed-on table (GetEventConfirmedOn) when the
 * labels are decided frames.  lx_anc_confirm is confirmEvents on it.
 *
 * What lx_anc_confirm returns is the SET the reference's DFS visits, not its
 * order: a caller that needs the ApplyEvent order keeps the host walk.  The
 * reference's DFS stops at a labelled event and never looks behind it, so the
 * sets are equal whenever the labelled set is ancestor-closed.  It always is
 * when the labels come from lx_anc_confirm itself or from a confirmed-on
 * table the reference wrote.  After an arbitrary lx_anc_set_labels the call
 * still labels EVERY unlabelled ancestor of a head, also those behind a
 * labelled one.
 *
 * Conventions of lachesis_hip.h (dense event indices of the index's epoch,
 * caller-owned buffers, 0 = ok / < 0 = error with the message in
 * lx_anc_last_error, one host thread per handle and its index).  All input is
 * checked before any device work: LX_ERR_ARG for a head or x that is no
 * indexed event, for a label of 0 and for a null argument; LX_ERR_STATE while
 * the index is loading (between lx_load_rows and lx_load_finish).
 *
 * The handle follows its index by itself, as an lx_mt handle does:
 *   - lx_reset of the index (a new epoch) or a reload: no labels are held;
 *   - lx_drop_not_flushed that dropped events (directly, or inside the abft
 *     handle): dense indices at or above the flushed count name other events
 *     afterwards, so every label at or above it is gone, the low-water mark is
 *     clamped to it and lx_anc_last_confirmed is empty.  lx_abft_build_frames
 *     does not roll back (lx_abft_build does): the labels stay.
 * Nothing is persisted: after a restart the caller hands the stored table
 * back with lx_anc_set_labels.
 *
 * The queries only read the index, so like the lx_mt calls they may be made
 * from inside the begin_block, apply_event and end_block callbacks of
 * lx_abft_process_batch.
 *
 * Fork evidence.  The cheaters of a block (applyAtropos, abft/lachesis.go:
 * 56-74) and the fork markers of a merged HighestBefore row only name a
 * creator.  lx_anc_fork_pairs / lx_anc_cheaters name the two events that prove
 * it, by the reference's own definition of a fork (the naive detection of
 * testForksDetected, vecfc/forkless_cause_test.go:490-518): head observes a
 * fork of creator c  <=>  two different events of c with the same seq are head
 * or ancestors of head.  With S(head, c) = the events of c that are head or
 * ancestors of it, the answer is canonical:
 *   - seq* = the lowest seq two events of S share;
 *   - x < y = the two lowest dense indices among the events of S with seq*
 *     (three and more events in one slot do occur);
 *   - (LX_ANC_NONE, LX_ANC_NONE, 0) where no two events of S share a seq.
 * No parent list is read: a branch is a chain of consecutive seqs, so head's
 * view of a branch is an interval of seqs whose end a binary search over the
 * branch's events finds, and seq* is the lowest seq two intervals of c's
 * branches share.  The search asks the LowestAfter rule above, not
 * HighestBefore: once head has detected the fork EVERY branch entry of c in
 * its row is a marker (Seq 0) and says nothing of how far head sees.  The
 * marker only serves as the quick "none": the reference marks a creator
 * exactly where S holds such a pair.
 * The calls keep no state but the list of the last lx_anc_cheaters (empty
 * after a new epoch or a rollback that dropped events, as
 * lx_anc_last_confirmed), and neither read nor write labels.
 *
 * Out of scope: column-sharded and row-segment handles (LX_ERR_STATE), the
 * reference's DFS order, the general walk filter of DfsSubgraph, evidence
 * other than the canonical lowest pair.
 */
#ifndef LACHESIS_ANCESTRY_H
#define LACHESIS_ANCESTRY_H

#include "lachesis_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lx_anc lx_anc;

/* LX_ERR_STATE for a column shard or a row-segment rank. */
int lx_anc_create(lx_index *index, lx_anc **out);
void lx_anc_destroy(lx_anc *a);
const char *lx_anc_last_error(const lx_anc *a);
/* No labels held (also noticed without this call after a new epoch). */
int lx_anc_reset(lx_anc *a);

/* out[i] = 1 iff x[i] is head[i] or an ancestor of head[i], else 0. */
int lx_anc_observes(lx_anc *a, uint64_t n, const uint32_t *head, const uint32_t *x, uint8_t *out);

/* confirmEvents for n_heads blocks in call order: every event that carries no
 * label and is head[k] or an ancestor of it takes label[k] (non-zero, e.g. the
 * decided frame) from the first k in call order that observes it.  n_new[k] =
 * the events head k labelled.  Heads may be any indexed events (not flushed
 * ones included), in any order, with duplicates; n_heads is unbounded: the
 * call is split into launches of at most 16 heads, fewer where their
 * HighestBefore rows would not fit 64 KiB of LDS.  LX_ERR_ARG for an index of
 * more than 16384 branches. */
int lx_anc_confirm(lx_anc *a, uint32_t n_heads, const uint32_t *head, const uint32_t *label, uint32_t *n_new);

/* The events the last lx_anc_confirm labelled: grouped by head in call order,
 * ascending dense index inside a group.  *n = their number; the first
 * min(cap, *n) are written (out_ev may be NULL with cap 0). */
int lx_anc_last_confirmed(lx_anc *a, uint32_t *out_ev, uint64_t cap, uint64_t *n);

/* GetEventConfirmedOn in bulk, out[i] = label of event first + i (0 = none),
 * and its inverse for a restart (a label of 0 takes the label away).
 * LX_ERR_ARG for first + n > lx_num_events. */
int lx_anc_labels(lx_anc *a, uint64_t first, uint64_t n, uint32_t *out);
int lx_anc_set_labels(lx_anc *a, uint64_t first, uint64_t n, const uint32_t *labels);
/* The lowest dense index without a label (= lx_num_events when all have one):
 * no event below it is looked at by lx_anc_confirm. */
int lx_anc_low_water(lx_anc *a, uint64_t *ev);

/* "no event" in the answers of the fork-evidence calls */
#define LX_ANC_NONE 0xFFFFFFFFu

/* Pairwise: out_x[i] < out_y[i] = the canonical pair for (head[i], creator[i])
 * (creator = validator idx), out_seq[i] (optional, may be NULL) their seq;
 * LX_ANC_NONE, LX_ANC_NONE, 0 where head[i] observes no fork of creator[i].
 * LX_ERR_ARG for a head that is no indexed event, a creator >= the number of
 * validators, and an index in which one creator has more than 1024 branches.
 * A fork-free epoch answers without a launch. */
int lx_anc_fork_pairs(lx_anc *a, uint64_t n, const uint32_t *head, const uint32_t *creator,
                      uint32_t *out_x, uint32_t *out_y, uint32_t *out_seq);

/* Every cheater each head observes (= the fork-detected entries of its merged
 * HighestBefore, the cheaters of applyAtropos when head is an Atropos) with
 * the pair: n_found[k] of them for head k.  The list is read with
 * lx_anc_last_cheaters: grouped by head in call order (duplicates repeat),
 * ascending creator idx inside a group. */
int lx_anc_cheaters(lx_anc *a, uint32_t n_heads, const uint32_t *head, uint32_t *n_found);
/* *n = the entries of the last lx_anc_cheaters; the first min(cap, *n) are
 * written (with cap > 0, out_creator, out_x and out_y are required, out_seq
 * may be NULL). */
int lx_anc_last_cheaters(lx_anc *a, uint32_t *out_creator, uint32_t *out_x, uint32_t *out_y,
                         uint32_t *out_seq, uint64_t cap, uint64_t *n);

#ifdef __cplusplus
}
#endif
#endif
