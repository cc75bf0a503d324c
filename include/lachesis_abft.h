/*
 * lachesis_abft.h -- C ABI of the batched abft caller on top of the HIP index.
 *
 * Drop-in for the consensus loop that drives the index in the reference:
 * abft.IndexedLachesis (abft/indexed_lachesis.go:17-107) = abft.Lachesis
 * (abft/lachesis.go) over abft.Orderer (abft/orderer.go, event_processing.go,
 * frame_decide.go, bootstrap.go) and election.Election (abft/election/).
 * Results -- frames, roots, decided frames, Atropos, cheaters, the order in
 * which confirmed events are applied, epoch sealing -- are those of calling the
 * reference's Process(e) once per event in the given order.  What changes is
 * how the ForklessCause questions are asked: frames of a whole batch are
 * computed level by level in frames, every question of a frame in one GPU
 * tile launch (events x roots of the frame), and election votes of a whole
 * round in one launch.
 *
 * Conventions are those of lachesis_hip.h: dense event indices (Add order of
 * the current epoch; they restart at 0 when an epoch is sealed or reset),
 * validator idx order, caller-owned buffers, 0 = ok / < 0 = error.  The abft
 * handle drives the index handle it was created on (Add, Flush,
 * DropNotFlushed, Reset): do not add events to that index directly (the one
 * exception is the reload of a persisted epoch before lx_abft_restore).
 * One host thread per handle; callbacks must not call back into the handle.
 * The lx_mt calls of lachesis_mediantime.h on the same index are the
 * exception: they only read the index, so BeginBlock can ask the block's
 * MedianTime(atropos) (lx_mt_median_time, lx_mt_merged_times, lx_mt_set_times).
 */
#ifndef LACHESIS_ABFT_H
#define LACHESIS_ABFT_H

#include "lachesis_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LX_ERR_FRAME -7        /* ErrWrongFrame: claimed frame mismatched (abft/event_processing.go:11-13) */
#define LX_ERR_BYZANTINE -8    /* election sanity errors (abft/election/election_math.go:68-90, sort_roots.go:23) */
#define LX_FRAME_BUILD 0xFFFFFFFFu   /* claimed_frame entry: compute as Build does (cap selfParentFrame+100) */

typedef struct lx_abft lx_abft;

/* lachesis.ConsensusCallbacks + BlockCallbacks (lachesis/consensus.go:21-44).
 * begin_block: decided frame, its Atropos, and the cheaters seen by the Atropos
 *   (validator idxs in idx order; abft/lachesis.go:57-73).
 * apply_event: every event newly confirmed by the block, in the reference's
 *   DFS order from the Atropos (abft/lachesis.go:40-55, abft/traversal.go:13-37).
 * end_block: return 0 to continue the epoch, or 1 to seal it; then
 *   *n_validators / *weights (idx order, valid until the next call into the
 *   library) give the next epoch's validators (frame_decide.go:11-35).
 * Any pointer may be NULL. */
typedef struct lx_abft_callbacks {
    void *user;
    void (*begin_block)(void *user, uint32_t frame, uint32_t atropos, const uint32_t *cheaters, uint32_t n_cheaters);
    void (*apply_event)(void *user, uint32_t ev);
    int (*end_block)(void *user, uint32_t *n_validators, const uint32_t **weights);
} lx_abft_callbacks;

/* NewIndexedLachesis (abft/indexed_lachesis.go:42-51) over an index handle
 * (unsharded). */
int lx_abft_create(lx_index *index, lx_abft **out);
void lx_abft_destroy(lx_abft *a);
const char *lx_abft_last_error(const lx_abft *a);
/* Path selection (results never change):
 *   "spec_depth" self-children evaluated speculatively per frame step (0..16,
 *                default 4)
 *   "fc16"       1 (default): fork-free epochs whose seqs fit 16 bits take the
 *                packed root-FC kernel (two columns per dword); 0: the 32-bit
 *                kernel always
 *   "claimed_batch" 1 (default): a batch whose every event claims its frame
 *                enqueues all its frame steps and waits once; 0: step by step
 *                as in Build
 *   "elect_ahead" rounds per election when the elections of every frame are
 *                enqueued together and read back with one wait (2..8, default
 *                2; 0: round by round, one wait per round)
 *   "block_log"  without a begin_block callback: 1 = the handle logs each
 *                decided block (frame, Atropos, cheaters) and runs the
 *                confirmation as a BeginBlock would, never sealing (no
 *                EndBlock); 2 = also the confirmed events in ApplyEvent order;
 *                read with lx_abft_block_log after the batch.  0 (default):
 *                nil BeginBlock semantics */
int lx_abft_set_option(lx_abft *a, const char *name, int64_t value);

/* ApplyGenesis + Bootstrap (abft/apply_genesis.go:17-44, bootstrap.go:30-52):
 * epoch and validators (weights in idx order); resets the index. */
int lx_abft_bootstrap(lx_abft *a, uint32_t epoch, uint32_t n_validators, const uint32_t *weights,
                      const lx_abft_callbacks *cb);

/* IndexedLachesis.Bootstrap over a persisted epoch (abft/indexed_lachesis.go:84-99,
 * abft/bootstrap.go:34-55, abft/lachesis.go:88-99): resumes an epoch after a
 * restart from what Orderer.Bootstrap reads back -- epoch, validators, last
 * decided frame, the roots table (abft/store_roots.go:56-93) and the
 * confirmed-on table -- instead of replaying the epoch's events.
 *
 * Precondition: the caller has reloaded the handle's index for this epoch
 * (lx_reset with the same validators, lx_load_rows ..., lx_load_finish) with
 * the same n_events events in the same dense order.  This is the one exception
 * to "do not add events to that index directly".
 *
 * Events: creator_idx / seq / parent_off / parent_idx are the arrays given to
 * lx_load_rows (self-parent first); ev_frame[e] is the event's frame,
 * ev_confirmed_on[e] GetEventConfirmedOn (0 = not confirmed).
 * Roots: frame f (1 .. n_frames) has the slots
 * root_ev[root_off[f-1] .. root_off[f]) in the order the caller read them
 * (append order of the cache, or key order of the kvdb table); an event that
 * is a root of several frames appears in each (AddRoot, store_roots.go:23-27).
 * The engine keeps that order; new roots are appended behind it.
 *
 * The call rebuilds the observed-roots bit rows of every slot above
 * last_decided_frame (one merged root-ForklessCause launch for all frames) and
 * then does what bootstrapElection does (event_processing.go:102-146): an
 * election for last_decided_frame + 1 over every known root, repeated while
 * frames decide.  As in the reference, Bootstrap runs before the callbacks are
 * assigned (lachesis.go:92-98): a frame decided during the call advances the
 * last decided frame with nil-BeginBlock semantics -- no callback, no
 * confirmation, no seal.  cb takes effect for later batches.
 *
 * Errors (message in lx_abft_last_error; all input is checked before any
 * device work or allocation sized by it): LX_ERR_STATE "already bootstrapped"
 * on a bootstrapped or restored handle, for a sharded index, an index in the
 * middle of loading, or validators other than the index's; LX_ERR_ARG for
 * n_events != lx_num_events(index), a non-monotone root_off, a frame without
 * roots, more than 16384 roots in a frame, a root index >= n_events or listed
 * twice in a frame, a slot of frame f whose event does not satisfy
 * frame(self-parent) < f <= ev_frame[e], a roots table that misses a slot the
 * event tables imply, last_decided_frame > n_frames, ev_confirmed_on[e] >
 * last_decided_frame, or event arrays that are not parents-first.  A failed
 * call leaves the handle not bootstrapped: a second lx_abft_restore or a
 * plain lx_abft_bootstrap works. */
int lx_abft_restore(lx_abft *a, uint32_t epoch, uint32_t n_validators, const uint32_t *weights,
                    uint32_t last_decided_frame, uint32_t n_events, const uint32_t *creator_idx, const uint32_t *seq,
                    const uint64_t *parent_off, const uint32_t *parent_idx, const uint32_t *ev_frame,
                    const uint32_t *ev_confirmed_on, uint32_t n_frames, const uint64_t *root_off,
                    const uint32_t *root_ev, const lx_abft_callbacks *cb);

/* The bulk inverse of lx_abft_restore: the abft state of the current epoch as
 * a caller persists it (or copies it, abft/restart_test.go:159-175).
 * lx_abft_state_sizes gives the counts; lx_abft_state_fetch fills ev_frame and
 * ev_confirmed_on (n_events entries), root_off (n_frames + 1 entries) and
 * root_ev (n_slots entries, frames 1 .. n_frames in slot order).  Any pointer
 * may be NULL.  n_frames = the highest frame holding a root. */
typedef struct lx_abft_state {
    uint32_t epoch, last_decided_frame, n_events, n_frames;
    uint64_t n_slots;
} lx_abft_state;
int lx_abft_state_sizes(lx_abft *a, lx_abft_state *out);
int lx_abft_state_fetch(lx_abft *a, uint32_t *ev_frame, uint32_t *ev_confirmed_on, uint64_t *root_off,
                        uint32_t *root_ev);

/* Orderer.Reset (bootstrap.go:54-65): switch to a new empty epoch. */
int lx_abft_reset(lx_abft *a, uint32_t epoch, uint32_t n_validators, const uint32_t *weights);

/* IndexedLachesis.Process (indexed_lachesis.go:65-82) for n events in
 * processing order (parents first; parent_off/parent_idx as lx_add_batch,
 * dense indices of this epoch, self-parent first).  claimed_frame[i] is the
 * event's Frame() field (LX_FRAME_BUILD: trust the computation, i.e. Build
 * then Process).  out_frame (optional) receives every consumed event's frame.
 * Callbacks fire for every frame decided inside the batch, in order.
 * *consumed = events processed: n, or less when
 *   - an event's claimed frame is wrong: returns LX_ERR_FRAME and *consumed is
 *     its position (the events before it are processed, as the reference
 *     processes them before returning ErrWrongFrame for it);
 *   - a block sealed the epoch: returns 0, *consumed counts the events up to
 *     the one whose processing decided the sealing frame; the rest belong to
 *     no epoch and must be re-submitted by the caller (as the reference test
 *     drivers do, abft/event_processing_test.go:145-150).
 * Every claim of the batch is checked before its elections run, so events
 * past a sealing frame carry this epoch's frame or LX_FRAME_BUILD; a wrong
 * claim there only costs work: the events up to the seal are processed again
 * alone and the call returns as for a seal.
 * Work on untrusted claims: a batch in which every event claims a frame is
 * evaluated before any claim is verified, claim - selfParentFrame frame steps
 * per event.  One pass queues at most 2 n + 4 n_validators + 64 such steps
 * (or one event's alone, however long its climb); a batch that asks for more
 * is processed in several passes inside the call, each over verified frames,
 * with the same results, *consumed and return code.  Inflated claims therefore
 * cost at most one such budget of discarded steps before LX_ERR_FRAME. */
int lx_abft_process_batch(lx_abft *a, uint32_t n, const uint32_t *creator_idx, const uint32_t *seq,
                          const uint64_t *parent_off, const uint32_t *parent_idx, const uint32_t *claimed_frame,
                          uint32_t *out_frame, uint32_t *consumed);

/* The blocks the last lx_abft_process_batch decided (option block_log):
 * block k = frame[k], atropos[k], cheaters[cheat_off[k] .. cheat_off[k+1]),
 * confirmed[conf_off[k] .. conf_off[k+1]) (block_log 2; empty ranges with 1).
 * Pointers stay valid until the next call into the handle; any may be NULL. */
int lx_abft_block_log(const lx_abft *a, uint32_t *n_blocks, const uint32_t **frame, const uint32_t **atropos,
                      const uint32_t **cheat_off, const uint32_t **cheaters, const uint32_t **conf_off,
                      const uint32_t **confirmed);

/* IndexedLachesis.Build (indexed_lachesis.go:53-63): frame of a self-emitted
 * event (added, evaluated, then dropped again).  The drop is a rollback of the
 * index: handles that follow rollbacks react (lachesis_mediantime.h,
 * lachesis_ancestry.h).  lx_abft_build_frames below answers without it; this
 * call remains the one for a candidate that would open a new branch. */
int lx_abft_build(lx_abft *a, uint32_t creator_idx, uint32_t seq, uint32_t n_parents, const uint32_t *parents,
                  uint32_t *out_frame);

/* Orderer.Build (abft/event_processing.go:15-30, calcFrameIdx :163-189 with
 * checkOnly = false) for n candidate events that are NOT added: each is judged
 * alone against the current epoch, candidates never see each other.
 * parent_off / parent_idx as lx_add_batch (dense indices of existing events,
 * self-parent first).  out_frame[i] is what lx_abft_build would return for
 * candidate i; out_is_root[i] (optional) = frame != selfParentFrame.
 * Reads only: no event is added, no rollback counted, no root slot, no
 * callback, no election.  Handles that follow rollbacks of the index (lx_mt,
 * lx_anc, the pending small-batch run's tables) keep what they hold; the stats
 * of lx_abft_last_stats stay those of the last lx_abft_process_batch.
 *
 * All input is checked before any device work; *err_index (optional) receives
 * the first offending candidate.  LX_ERR_STATE: the handle is not
 * bootstrapped.  LX_ERR_ARG: creator >= V; seq == 0; a parent >=
 * lx_num_events; a duplicate parent; seq > 1 without a first parent of the
 * same creator at seq - 1; seq == 1 with a first parent of the same creator;
 * or a candidate that would open a new branch -- its self-parent is not the
 * last event of its branch, or seq == 1 while the creator already has events
 * (fillGlobalBranchID, vecengine/index.go:105-141, would append a branch).
 * lx_abft_build remains the call for that case.  A candidate may extend any
 * existing branch tip, a cheater's fork branch included.  n == 0 is ok and
 * launches nothing. */
int lx_abft_build_frames(lx_abft *a, uint32_t n, const uint32_t *creator_idx, const uint32_t *seq,
                         const uint64_t *parent_off, const uint32_t *parent_idx,
                         uint32_t *out_frame, uint8_t *out_is_root, uint32_t *err_index);

/* Frame progress of candidate events that are NOT added: how far each is from
 * the next frame.  All quantities are those of the index with the candidate
 * added (what Add would produce: DESIGN.md sections 9c, 9d).
 *   stake(e, r)  0 if HighestBefore(e)[branch(r)] is a fork marker, otherwise
 *                the weight of the distinct creators c with a branch j where
 *                LowestAfter(r)[j] != 0 && LowestAfter(r)[j] <= HighestBefore(e)[j].Seq
 *                -- the WeightCounter of forklessCause before HasQuorum:
 *                ForklessCause(e, r) <=> stake(e, r) >= quorum.
 * Per frame f, over the engine's root slots of f in its order, a slot whose
 * event is e itself left out of the three sums:
 *   out_n_roots    the slots of f (own slot included)
 *   out_n_caused   the slots with stake(e, r) >= quorum
 *   out_stake      the weight of the distinct creators of those slots (the
 *                  counter of forklessCausedByQuorumOn without its break)
 *   out_root_stake the sum over the slots of min(stake(e, r), quorum)
 * Frame asked: at_frame == NULL or an entry LX_FRAME_BUILD asks candidate i at
 * its Build frame, the value lx_abft_build_frames returns; there out_stake <
 * quorum, unless the Build cap of 100 frames stopped the loop or the candidate
 * has no self-parent (frame 1 is given without asking roots(1); its progress
 * over roots(1) is reported as it is).  An entry f >= 1 asks frame f alone, no
 * frame loop; a frame without roots answers zeros.  out_frame[i] = the frame
 * the numbers are about.  Every out_* is optional except out_frame.
 * flags: LX_PROGRESS_PAIRS keeps stake(e, r) of every slot for
 * lx_abft_last_progress_pairs.
 *
 * Reads only, with the guarantee of lx_abft_build_frames: no event added, no
 * root slot, no election, no callback, no rollback counted; lx_mt and lx_anc
 * handles keep what they hold; the stats of lx_abft_last_stats stay those of
 * the last lx_abft_process_batch.
 * Inputs, checks and refusals are those of lx_abft_build_frames, all before
 * any device work, plus LX_ERR_ARG for an at_frame entry 0 and for unknown
 * flag bits; *err_index (optional) receives the first offending candidate.
 * n == 0 is ok and launches nothing. */
#define LX_PROGRESS_PAIRS 1u   /* keep the per-pair stakes for lx_abft_last_progress_pairs */
int lx_abft_build_progress(lx_abft *a, uint32_t n, const uint32_t *creator_idx, const uint32_t *seq,
                           const uint64_t *parent_off, const uint32_t *parent_idx,
                           const uint32_t *at_frame, uint32_t flags,
                           uint32_t *out_frame, uint32_t *out_n_roots, uint32_t *out_n_caused,
                           uint32_t *out_stake, uint64_t *out_root_stake, uint32_t *err_index);

/* The same for n indexed events (any event of the epoch, not flushed ones
 * included), on the index as it stands.  LX_FRAME_BUILD asks an event at its
 * own frame: there out_stake < quorum, and at each earlier frame back to its
 * self-parent's frame out_stake >= quorum.  An event that is a root of the
 * frame asked leaves its own slot out of the three sums and keeps it in the
 * pair list.  Reads only, as above.  LX_ERR_STATE: not bootstrapped.
 * LX_ERR_ARG: an event >= lx_num_events, an at_frame entry 0, unknown flags. */
int lx_abft_event_progress(lx_abft *a, uint32_t n, const uint32_t *ev, const uint32_t *at_frame,
                           uint32_t flags, uint32_t *out_frame, uint32_t *out_n_roots,
                           uint32_t *out_n_caused, uint32_t *out_stake, uint64_t *out_root_stake,
                           uint32_t *err_index);

/* Per-pair stakes of the last progress call made with LX_PROGRESS_PAIRS:
 * entry i owns [pair_off[i], pair_off[i+1]) (n + 1 offsets), one entry per
 * slot of its frame in slot order, own slot included: the root event and
 * stake(e, r).  *n_pairs = their number; the first min(cap, *n_pairs) are
 * written.  Any pointer but n_pairs may be NULL.  Empty (pair_off[0] = 0,
 * *n_pairs = 0) after any other call that launches work on the handle, a
 * progress call without the flag or a failed one included. */
int lx_abft_last_progress_pairs(lx_abft *a, uint64_t *pair_off, uint32_t *out_root,
                                uint32_t *out_stake, uint64_t cap, uint64_t *n_pairs);

/* GPU work of the last lx_abft_build_frames, lx_abft_build_progress or
 * lx_abft_event_progress, whichever came last (zeros after a call that failed
 * its input checks or had n == 0); in a progress call k_root_progress takes
 * the place of the quorum kernel. */
typedef struct lx_abft_build_stats {
    uint32_t launches;      /* kernel launches: uploads, k_build_rows, root-FC and quorum per round */
    uint32_t frame_steps;   /* (frame, round) steps evaluated */
    uint32_t rounds;        /* waits: one per round of the frame loop */
    uint32_t fc16;          /* 1: the packed 16-bit root-FC kernel ran */
    uint64_t fc_pairs;      /* (candidate, root) pairs evaluated */
} lx_abft_build_stats;
int lx_abft_build_last_stats(const lx_abft *a, lx_abft_build_stats *out);

uint32_t lx_abft_epoch(const lx_abft *a);
uint32_t lx_abft_last_decided_frame(const lx_abft *a);
/* GetFrameRoots (abft/store_roots.go:52-93): root events of a frame. */
int lx_abft_frame_roots(lx_abft *a, uint32_t frame, uint32_t *out_ev, uint32_t cap, uint32_t *n);
int lx_abft_event_frame(const lx_abft *a, uint32_t ev, uint32_t *frame);
/* GetEventConfirmedOn (abft/store_event_confirmed.go:20-30): 0 = not confirmed. */
int lx_abft_event_confirmed_on(const lx_abft *a, uint32_t ev, uint32_t *frame);

/* Wall time of the last lx_abft_process_batch by phase (ms) and its GPU work.
 * After lx_abft_restore: ms_frames = input checks, tables and the rebuild of
 * the bit rows (fc_launches, fc_pairs), ms_election = the elections
 * (vote_launches); ms_index is 0 (the index reload is the caller's). */
typedef struct lx_abft_stats {
    float ms_index;      /* Add of the batch (lx_add_batch) */
    float ms_frames;     /* frames + roots (root ForklessCause tiles) */
    float ms_election;   /* votes, decisions */
    float ms_blocks;     /* cheaters, confirmation DFS, callbacks */
    uint32_t frame_steps, fc_launches, vote_launches, blocks;
    uint64_t fc_pairs;   /* (event, root) pairs evaluated */
    uint64_t fc_pair_cols;   /* pairs x validator columns compared by k_root_fc */
    float ms_root_fc_gpu;    /* k_root_fc time on the stream (HIP events around each launch) */
    uint64_t fc_lane_ops;    /* VALU lane-ops the root-FC inner loops issue (ISA count per pair and
                                column: 2.5 in k_root_fc; 1.5 in k_root_fc16, 2 in its 32-column
                                chunks holding a weight >= 2^16) over the padded columns */
    uint32_t elections_ahead;   /* elections decided by run_elections_ahead (all their rounds
                                   enqueued at once) rather than round by round */
} lx_abft_stats;
int lx_abft_last_stats(const lx_abft *a, lx_abft_stats *out);

#ifdef __cplusplus
}
#endif
#endif
