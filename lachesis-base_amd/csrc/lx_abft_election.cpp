// lx_abft_election.cpp -- elections and blocks of the batched abft caller (lx_abft_engine.h).
//
// Election (abft/election/election_math.go:13-114).  Votes of a root slot
// depend only on the slots it observes, so votes are computed per frame
// (round) for all slots at once, for every subject (k_vote_round).  The
// reference skips subjects already decided when a root is processed; that
// only skips work whose result is never read.  The decision for subject v is
// the vote of the first deciding root in processing order =
// atomicMin over (event << 32 | vote); the frame is decided at
// t = max(previous decision, max_{v <= Atropos subject} first decision(v))
// (chooseAtropos, sort_roots.go:10-25), final once no uncomputed slot is older
// than t.  Frames are replayed after each decision as processKnownRoots does.
// Elections of different frames do not read each other, so all of them run
// side by side first (run_elections_ahead), round by round only what remains.
//
// Blocks (abft/lachesis.go:40-86): cheaters from the Atropos' HighestBefore
// fork markers, confirmation DFS in the reference's stack order on the host.
#include "lx_abft_engine.h"

namespace lxa {

// votes of slots [from, to) of frame g for subjects [v_lo, v_hi) (round g - F)
int vote_slots(lx_abft *a, const IndexView &iv, uint32_t F, uint32_t g, uint32_t from, uint32_t to, uint32_t v_lo,
               uint32_t v_hi) {
    hipStream_t s = iv.stream;
    if (from >= to || v_lo >= v_hi) return 0;
    Frame &fg = frame_at(a, g);
    Frame &fp = frame_at(a, g - 1);
    ARC(sync_frame(a, fg, s));
    ARC(sync_frame(a, fp, s));
    ARC(reserve(a, fg.votes, (uint64_t)fg.ev.size() * a->V, (uint64_t)fg.voted * a->V, s));
    VoteArgs v{};
    v.V = a->V;
    v.voter_ev = fg.d_ev + from;
    v.bm_off = fg.d_bm_off + from;
    v.bm_len = fg.d_bm_len + from;
    v.bm = a->arena;
    v.prev_creator = fp.d_creator;
    v.prev_dup = fp.d_dup;
    v.prev_votes = fp.votes;
    v.prev_has_dup = std::any_of(fp.dup.begin(), fp.dup.end(), [](uint32_t d) { return d != NONE; }) ? 1u : 0u;
    v.v_lo = v_lo;
    v.v_hi = v_hi;
    v.wcreator = iv.wpad;
    v.quorum = a->quorum;
    v.votes = fg.votes + (uint64_t)from * a->V;
    v.dec = a->d_dec;
    v.err = a->d_err;
    ARC(flush_uploads(a, s));
    AHIP(a, lx::launch_votes(v, to - from, g == F + 1, s));
    a->stats.vote_launches++;
    return 0;
}

// new slots of frame g, current subject window
int vote_frame(lx_abft *a, const IndexView &iv, uint32_t F, uint32_t g) {
    Frame &fg = frame_at(a, g);
    const uint32_t from = fg.voted, to = (uint32_t)fg.ev.size();
    if (from == to) return 0;
    ARC(vote_slots(a, iv, F, g, from, to, 0, a->vw));
    a->frames[g].voted = to;
    return 0;
}

// widen the subject window of election F to [0, nw) for every voted slot
int widen_window(lx_abft *a, const IndexView &iv, uint32_t F, uint32_t nw) {
    for (uint32_t g = F + 1; g < a->frames.size(); g++) {
        const uint32_t voted = a->frames[g].voted;
        if (!voted) break;
        ARC(vote_slots(a, iv, F, g, 0, voted, a->vw, nw));
    }
    a->vw = nw;
    return 0;
}

// chooseAtropos (SortedIDs = idx order) over the decisions of subjects
// [0, vw): 0 pending, 1 decided (*t, *atropos slot), 2 every subject decided "no"
int atropos_state(const unsigned long long *dec, uint32_t vw, uint64_t *t, uint32_t *obs) {
    uint64_t tmax = 0;
    for (uint32_t v = 0; v < vw; v++) {
        if (dec[v] == ~0ull) return 0;
        tmax = std::max<uint64_t>(tmax, dec[v] >> 32);
        if (dec[v] & 0x80000000ull) {
            *t = tmax;
            *obs = (uint32_t)(dec[v] & kVoteNoRoot);
            return 1;
        }
    }
    return 2;
}

// decision of election F: 0 pending, 1 decided (*t, *atropos slot),
// 2 every subject of the window decided "no" (widen it)
int check_decision(lx_abft *a, const IndexView &iv, uint32_t F, uint64_t *t, uint32_t *obs, int *state) {
    const uint32_t *rb = nullptr;
    ARC(readback(a, iv.stream, reinterpret_cast<const uint32_t *>(a->d_dec.get()), 2 * a->vw, a->d_err, 1, &rb));
    std::vector<unsigned long long> dec(a->vw);
    memcpy(dec.data(), rb, a->vw * 8ull);
    const uint32_t err = rb[2 * a->vw];
    if (err & kVoteErrTwoRoots)
        return a->fail(LX_ERR_BYZANTINE, "forkless caused by 2 fork roots => more than 1/3W are Byzantine (election frame=%u)", F);
    if (err & kVoteErrQuorum)
        return a->fail(LX_ERR_BYZANTINE, "root must be forkless caused by at least 2/3W of prev roots (election frame=%u)", F);
    if (err & kVoteErrMissing)
        return a->fail(LX_ERR_BYZANTINE, "every root must vote for every not decided subject (election frame=%u)", F);
    *state = atropos_state(dec.data(), a->vw, t, obs);
    if (*state != 2 || a->vw < a->V) return 0;
    return a->fail(LX_ERR_BYZANTINE, "all the roots are decided as 'no', which is possible only if more than 1/3W are Byzantine");
}

int reset_election(lx_abft *a, const IndexView &iv) {
    ARC(reserve(a, a->d_dec, a->V, 0, iv.stream));
    ARC(reserve(a, a->d_err, 1, 0, iv.stream));
    AHIP(a, hipMemsetAsync(a->d_dec, 0xFF, a->V * 8ull, iv.stream));
    AHIP(a, hipMemsetAsync(a->d_err, 0, 4, iv.stream));
    for (uint32_t g = a->last_decided + 1; g < a->frames.size(); g++) a->frames[g].voted = 0;
    a->vw = std::min<uint32_t>(a->V, kVoteWindow);
    a->dec_dirty = false;
    return 0;
}

// The confirmations of the blocks queued by apply_block (block_log 1, no
// ApplyEvent): block F confirms every not yet confirmed ancestor of its
// Atropos (the DFS of lachesis.go:40-55 stops at confirmed events, whose
// ancestors are all confirmed already), so each event takes the first queued
// block whose Atropos it is an ancestor of.  Events are in Add order (parents
// first): one sweep from the highest Atropos down carries the earliest block
// index to the parents -- the same sets as the blocks' DFS, in one pass over
// the parent lists instead of one stack walk per block.
void confirm_sweep(lx_abft *a) {
    const size_t nb = a->sweep_atropos.size();
    if (!nb) return;
    uint32_t hi = 0;
    for (uint32_t e : a->sweep_atropos) hi = std::max(hi, e);
    std::vector<uint32_t> &lab = a->sweep_label;
    lab.assign((size_t)hi + 1, NONE);
    for (size_t k = nb; k-- > 0;) lab[a->sweep_atropos[k]] = (uint32_t)k;   // earliest block wins
    for (uint32_t e = hi + 1; e-- > 0;) {
        const uint32_t k = lab[e];
        if (k == NONE || a->ev_confirmed[e]) continue;
        a->ev_confirmed[e] = a->sweep_frame[k];
        for (uint64_t j = a->par_off[e]; j < a->par_off[e + 1]; j++) {
            const uint32_t p = a->par[j];
            if (!a->ev_confirmed[p] && k < lab[p]) lab[p] = k;
        }
    }
    a->sweep_atropos.clear();
    a->sweep_frame.clear();
}

// cheaters + confirmation DFS + callbacks; returns 1 in *sealed when EndBlock seals
// (row: the Atropos' HB row already read back, or nullptr)
int apply_block(lx_abft *a, const IndexView &iv, uint32_t F, uint32_t atropos, bool *sealed,
                std::vector<uint32_t> *new_w, const uint32_t *row = nullptr) {
    *sealed = false;
    std::vector<uint32_t> cheaters;
    if (!row) ARC(readback(a, iv.stream, iv.hb + (uint64_t)atropos * iv.stride, a->V, nullptr, 0, &row));
    for (uint32_t c = 0; c < a->V; c++)
        if (row[c] & LX_MARK) cheaters.push_back(c);   // GetMergedHighestBefore(atropos)[c].IsForkDetected()
    // BeginBlock == nil: no confirmation, no seal (lachesis.go:69-71) -- unless
    // the handle logs its blocks itself (option block_log: a BeginBlock that
    // records, no EndBlock)
    const uint32_t log = a->cb.begin_block ? 0u : a->block_log;
    if (!a->cb.begin_block && !log) return 0;
    if (a->cb.begin_block) a->cb.begin_block(a->cb.user, F, atropos, cheaters.data(), (uint32_t)cheaters.size());
    if (log) {
        BlockLog &L = a->blog;
        L.frame.push_back(F);
        L.atropos.push_back(atropos);
        L.cheaters.insert(L.cheaters.end(), cheaters.begin(), cheaters.end());
        L.cheat_off.push_back((uint32_t)L.cheaters.size());
    }
    if (log == 1 && !a->cb.apply_event) {
        // nobody sees the order: the confirmations of this batch's blocks are
        // made by one sweep (confirm_sweep) before anything reads them
        a->sweep_atropos.push_back(atropos);
        a->sweep_frame.push_back(F);
        a->blog.conf_off.push_back(0);
        a->stats.blocks++;
        return 0;
    }
    // dfsSubgraph(atropos, filter) (abft/traversal.go:13-37, lachesis.go:40-55)
    std::vector<uint32_t> stack;
    for (uint32_t walk = atropos;;) {
        if (a->ev_confirmed[walk] == 0) {
            a->ev_confirmed[walk] = F;
            if (a->cb.apply_event) a->cb.apply_event(a->cb.user, walk);
            if (log == 2) a->blog.confirmed.push_back(walk);
            // a parent already confirmed would be popped and skipped: not pushed
            for (uint64_t k = a->par_off[walk]; k < a->par_off[walk + 1]; k++)
                if (a->ev_confirmed[a->par[k]] == 0) stack.push_back(a->par[k]);
        }
        if (stack.empty()) break;
        walk = stack.back();
        stack.pop_back();
    }
    if (a->cb.end_block) {
        uint32_t nv = 0;
        const uint32_t *w = nullptr;
        if (a->cb.end_block(a->cb.user, &nv, &w)) {
            if (!nv || !w) return a->fail(LX_ERR_ARG, "end_block sealed the epoch without validators");
            new_w->assign(w, w + nv);
            *sealed = true;
        }
    }
    if (log) a->blog.conf_off.push_back((uint32_t)a->blog.confirmed.size());
    a->stats.blocks++;
    return 0;
}

// Elections decided ahead.  Election F reads only the root slots of frames
// > F (processKnownRoots replays them after every decision), never the
// outcome of election F-1, so the elections of every frame with two frames of
// roots above it are enqueued together: each with its own vote tables over
// the first subject window and its own decision words, for elect_ahead rounds
// (frames F+1 .. F+elect_ahead), read back after one wait.  The host then
// takes them in frame order as the step-by-step loop would: an election
// decided and final within those rounds is applied (the Atropos HB rows of
// all of them come back in a second wait); the first one that is not
// (pending, every subject of the window "no", a vote error, a slot older than
// its decision left unvoted) hands over to the step-by-step loop, which
// redoes it from scratch.  *sealed_at as in run_elections.
int run_elections_ahead(lx_abft *a, const IndexView &iv, uint64_t *sealed_at, std::vector<uint32_t> *new_w) {
    hipStream_t s = iv.stream;
    const uint32_t R = a->elect_ahead, F0 = a->last_decided + 1;
    if (R < 2 || a->frames.size() < F0 + 3) return 0;
    const uint32_t maxf = (uint32_t)a->frames.size() - 1;
    const uint32_t nE = maxf - 1 - F0;    // elections F0 .. maxf - 2
    const uint32_t vw = std::min<uint32_t>(a->V, kVoteWindow);
    PassTimer pt("elect");
    for (uint32_t f = F0; f <= maxf; f++) ARC(sync_frame(a, frame_at(a, f), s));
    pt.mark("sync_frames");
    // vote tables: election e, round g -> slots(g) x vw
    std::vector<uint64_t> voff;
    uint64_t vtot = 0;
    for (uint32_t e = 0; e < nE; e++)
        for (uint32_t g = F0 + e + 1; g <= std::min(F0 + e + R, maxf); g++) {
            voff.push_back(vtot);
            vtot += (uint64_t)a->frames[g].ev.size() * vw;
        }
    ARC(reserve(a, a->ea_votes, std::max<uint64_t>(vtot, 1), 0, s));
    ARC(reserve(a, a->ea_dec, (uint64_t)nE * vw, 0, s));
    ARC(reserve(a, a->ea_err, nE, 0, s));
    ARC(reserve(a, a->ea_args, voff.size(), 0, s));
    // the tables of round r of every election go out in one launch per kernel
    // (args on the device, grouped by round)
    std::vector<std::vector<VoteArgs>> by_round(R);
    size_t vi = 0;
    for (uint32_t e = 0; e < nE; e++) {
        const uint32_t F = F0 + e;
        const uint32_t *prev = nullptr;
        for (uint32_t g = F + 1; g <= std::min(F + R, maxf); g++, vi++) {
            Frame &fg = a->frames[g], &fp = a->frames[g - 1];
            VoteArgs v{};
            v.V = vw;   // row stride of these tables: subjects [0, vw) only
            v.voter_ev = fg.d_ev;
            v.bm_off = fg.d_bm_off;
            v.bm_len = fg.d_bm_len;
            v.bm = a->arena;
            v.prev_creator = fp.d_creator;
            v.prev_dup = fp.d_dup;
            v.prev_votes = prev;
            v.prev_has_dup = std::any_of(fp.dup.begin(), fp.dup.end(), [](uint32_t d) { return d != NONE; }) ? 1u : 0u;
            v.v_lo = 0;
            v.v_hi = vw;
            v.wcreator = iv.wpad;
            v.quorum = a->quorum;
            v.votes = a->ea_votes + voff[vi];
            v.dec = a->ea_dec + (uint64_t)e * vw;
            v.err = a->ea_err + e;
            v.n_voters = (uint32_t)fg.ev.size();
            by_round[g - F - 1].push_back(v);
            prev = v.votes;
        }
    }
    std::vector<uint64_t> aoff(R + 1, 0);
    for (uint32_t r = 0; r < R; r++) {
        aoff[r + 1] = aoff[r] + by_round[r].size();
        a->up.add(a->ea_args + aoff[r], by_round[r].data(), by_round[r].size() * sizeof(VoteArgs));
    }
    ARC(flush_uploads(a, s));
    AHIP(a, hipMemsetAsync(a->ea_dec, 0xFF, (uint64_t)nE * vw * 8, s));
    AHIP(a, hipMemsetAsync(a->ea_err, 0, nE * 4ull, s));
    for (uint32_t r = 0; r < R; r++) {
        uint32_t mx = 0;
        for (const VoteArgs &v : by_round[r]) mx = std::max(mx, v.n_voters);
        AHIP(a, lx::launch_votes_multi(a->ea_args + aoff[r], (uint32_t)by_round[r].size(), mx, vw, r == 0, s));
        a->stats.vote_launches++;
    }
    pt.mark("launch");
    const uint32_t *rb = nullptr;
    ARC(readback(a, s, reinterpret_cast<const uint32_t *>(a->ea_dec.get()), 2 * nE * vw, a->ea_err, nE, &rb));
    pt.mark("wait");
    std::vector<unsigned long long> dec((uint64_t)nE * vw);
    memcpy(dec.data(), rb, dec.size() * 8);
    std::vector<uint32_t> err(rb + 2ull * nE * vw, rb + 2ull * nE * vw + nE);
    // decided prefix of the elections, in frame order
    struct Decided {
        uint32_t F, atropos;
        uint64_t t;
    };
    std::vector<Decided> done;
    std::vector<uint64_t> L(maxf + 2, ~0ull);   // L[h] = oldest slot of frames >= h
    for (uint32_t h = maxf; h >= 1; h--) {
        L[h] = L[h + 1];
        for (uint32_t x : a->frames[h].ev) L[h] = std::min<uint64_t>(L[h], x);
    }
    for (uint32_t e = 0; e < nE; e++) {
        const uint32_t F = F0 + e;
        uint64_t t = 0;
        uint32_t obs = 0;
        if (err[e] || atropos_state(dec.data() + (uint64_t)e * vw, vw, &t, &obs) != 1) break;
        if (t > L[std::min(F + R, maxf) + 1]) break;   // an older slot is not voted yet
        if (obs >= a->frames[F].ev.size()) break;
        done.push_back({F, a->frames[F].ev[obs], t});
    }
    if (done.empty()) return 0;
    std::vector<uint32_t> rows(done.size());
    for (size_t k = 0; k < done.size(); k++) rows[k] = done[k].atropos;
    pt.mark("decide");
    const uint32_t *hb_rows = nullptr;
    ARC(readback_rows(a, iv, rows, &hb_rows));
    pt.mark("rows");
    for (size_t k = 0; k < done.size(); k++) {
        const uint64_t decided_at = std::max<uint64_t>(done[k].t, a->t_prev);
        bool sealed;
        ARC(apply_block(a, iv, done[k].F, done[k].atropos, &sealed, new_w, hb_rows + k * (uint64_t)a->V));
        if (sealed) {
            *sealed_at = decided_at;
            return 0;
        }
        a->t_prev = decided_at;
        a->last_decided = done[k].F;
    }
    pt.mark("apply");
    for (uint32_t g = 1; g <= a->last_decided && g < a->frames.size(); g++) a->frames[g].votes.release();
    a->dec_dirty = true;
    a->stats.elections_ahead += (uint32_t)done.size();
    return 0;
}

// Runs elections over all known root slots; *sealed_at = event that decided a
// sealing frame (NONE if none).
int run_elections(lx_abft *a, uint64_t *sealed_at, std::vector<uint32_t> *new_w) {
    *sealed_at = ~0ull;
    IndexView iv;
    int rc = lx_index_view(a->ix, &iv);
    if (rc) return a->ixfail(rc);
    ARC(run_elections_ahead(a, iv, sealed_at, new_w));
    if (*sealed_at != ~0ull) return 0;
    for (;;) {
        const uint32_t F = a->last_decided + 1;
        if (a->dec_dirty) ARC(reset_election(a, iv));
        const uint32_t maxf = (uint32_t)a->frames.size() - 1;
        if (a->frames.size() <= F + 1) return 0;
        ARC(sync_frame(a, frame_at(a, F), iv.stream));
        int state = 0;
        uint64_t t = 0;
        uint32_t obs = 0;
        bool checked = false;
        for (uint32_t g = F + 1; g <= maxf; g++) {
            const bool fresh = frame_at(a, g).voted < frame_at(a, g).ev.size();
            ARC(vote_frame(a, iv, F, g));
            if (g < F + 2 || (checked && !fresh)) continue;
            ARC(check_decision(a, iv, F, &t, &obs, &state));
            while (state == 2) {   // all subjects so far decided "no": the Atropos is further down
                ARC(widen_window(a, iv, F, std::min<uint32_t>(a->V, a->vw * 2)));
                ARC(check_decision(a, iv, F, &t, &obs, &state));
            }
            checked = true;
            if (state) {
                // final unless a slot not yet voted in this election is older
                uint64_t L = ~0ull;
                for (uint32_t h = g + 1; h <= maxf; h++) {
                    const Frame &fh = a->frames[h];
                    for (size_t k = fh.voted; k < fh.ev.size(); k++) L = std::min<uint64_t>(L, fh.ev[k]);
                }
                if (t <= L) break;
                state = 0;
            }
        }
        if (!state) return 0;
        const Frame &fF = a->frames[F];
        if (obs >= fF.ev.size()) return a->fail(LX_ERR_STATE, "decided Atropos has no root (frame %u)", F);
        const uint32_t atropos = fF.ev[obs];
        const uint64_t decided_at = std::max<uint64_t>(t, a->t_prev);
        bool sealed;
        ARC(apply_block(a, iv, F, atropos, &sealed, new_w));
        if (sealed) {
            *sealed_at = decided_at;
            return 0;
        }
        a->t_prev = decided_at;
        a->last_decided = F;
        for (uint32_t g = 1; g <= F && g < a->frames.size(); g++) a->frames[g].votes.release();
        a->dec_dirty = true;
    }
}

}  // namespace lxa
