// lx_abft.cpp -- batched abft caller (include/lachesis_abft.h).
//
// Same results as abft.IndexedLachesis.Process called once per event
// (abft/indexed_lachesis.go:65-82), reorganised so that the ForklessCause
// questions of the consensus loop become a few large GPU launches: frames
// (lx_abft_frames.cpp), elections and blocks (lx_abft_election.cpp); this file
// holds the epoch, the add and process passes, restore and the C API.  The
// engine's state and what the three sources share: lx_abft_engine.h.
#include "lx_abft_engine.h"

namespace lxa {

void clear_epoch(lx_abft *a) {
    a->frames.clear();   // their device arrays go back to the pool
    a->ev_frame.clear();
    a->ev_sp.clear();
    a->ev_confirmed.clear();
    a->sweep_atropos.clear();
    a->sweep_frame.clear();
    a->par_off.assign(1, 0);
    a->par.clear();
    a->arena_used = 0;
    a->last_decided = 0;
    a->t_prev = 0;
    a->dec_dirty = true;
    a->k_gen = 0;
}

int start_epoch(lx_abft *a, uint32_t epoch, uint32_t nv, const uint32_t *w) {
    if (!nv || !w) return a->fail(LX_ERR_ARG, "genesis validators shouldn't be empty");
    int rc = lx_reset(a->ix, nv, w);
    if (rc) return a->ixfail(rc);
    IndexView iv;
    if ((rc = lx_index_view(a->ix, &iv))) return a->ixfail(rc);
    if (iv.shard_count > 1) return a->fail(LX_ERR_STATE, "abft needs an unsharded index");
    clear_epoch(a);
    a->epoch = epoch;
    a->V = nv;
    a->weights.assign(w, w + nv);
    a->quorum = iv.quorum;
    return 0;
}

// ---------------------------------------------------------------------------- restart

// What lx_abft_restore is given (include/lachesis_abft.h).
struct RestoreIn {
    uint32_t epoch, nv;
    const uint32_t *w;
    uint32_t last_decided, n;
    const uint32_t *creator, *seq;
    const uint64_t *poff;
    const uint32_t *par, *ev_frame, *ev_conf;
    uint32_t nf;
    const uint64_t *root_off;
    const uint32_t *root_ev;
};

// Every check of the input, on the host: nothing is allocated by a size the
// caller claims before that size is tied to the index's own event count (the
// two tables below have n_events entries, checked first; the roots are read in
// place, and a frame's slot list ends at its first repeated event at the
// latest).  *sp_out = self-parent per event (inter/dag/event.go:87-92).
int check_restore(lx_abft *a, const IndexView &iv, const RestoreIn &in, std::vector<uint32_t> *sp_out) {
    if (!in.nv || !in.w) return a->fail(LX_ERR_ARG, "genesis validators shouldn't be empty");
    if (iv.shard_count > 1) return a->fail(LX_ERR_STATE, "abft needs an unsharded index");
    if (iv.loading) return a->fail(LX_ERR_STATE, "index is loading (lx_load_finish first)");
    if (in.nv != iv.V || !std::equal(in.w, in.w + in.nv, iv.weights->begin()))
        return a->fail(LX_ERR_STATE, "validators differ from the ones the index was reloaded with");
    if (in.n != iv.n_events)
        return a->fail(LX_ERR_ARG, "n_events %u, but the index holds %llu events", in.n, (unsigned long long)iv.n_events);
    if (in.n && (!in.creator || !in.seq || !in.poff || !in.ev_frame || !in.ev_conf))
        return a->fail(LX_ERR_ARG, "null event table");
    if (in.nf && !in.root_off) return a->fail(LX_ERR_ARG, "null root_off");
    if (in.last_decided > in.nf)
        return a->fail(LX_ERR_ARG, "last decided frame %u above the %u frames of the roots table", in.last_decided, in.nf);
    std::vector<uint32_t> &sp = *sp_out;
    sp.assign(in.n, NONE);
    uint64_t want_slots = 0;
    for (uint32_t e = 0; e < in.n; e++) {
        const uint64_t p0 = in.poff[e], p1 = in.poff[e + 1];
        if (p1 < p0 || (p1 > p0 && !in.par)) return a->fail(LX_ERR_ARG, "event %u: bad parent_off", e);
        if (in.creator[e] >= in.nv) return a->fail(LX_ERR_ARG, "event %u: creator idx %u", e, in.creator[e]);
        for (uint64_t x = p0; x < p1; x++)
            if (in.par[x] >= e) return a->fail(LX_ERR_ARG, "event %u: parent %u is not before it", e, in.par[x]);
        if (in.seq[e] > 1 && p1 > p0) sp[e] = in.par[p0];
        const uint32_t spf = sp[e] == NONE ? 0 : in.ev_frame[sp[e]], f = in.ev_frame[e];
        if (f == 0 || f < spf || f > in.nf)
            return a->fail(LX_ERR_ARG, "event %u: frame %u (self-parent's frame %u, %u frames of roots)", e, f, spf, in.nf);
        want_slots += f - spf;   // a root of every frame it passes (store_roots.go:23-27)
        if (in.ev_conf[e] > in.last_decided)
            return a->fail(LX_ERR_ARG, "event %u confirmed on frame %u above the last decided frame %u", e, in.ev_conf[e],
                           in.last_decided);
    }
    if (in.nf && in.root_off[0] != 0) return a->fail(LX_ERR_ARG, "root_off must start at 0");
    std::vector<uint32_t> seen(in.n, 0);   // last frame listing the event
    for (uint32_t f = 1; f <= in.nf; f++) {
        const uint64_t lo = in.root_off[f - 1], hi = in.root_off[f];
        if (hi < lo) return a->fail(LX_ERR_ARG, "root_off is not monotone at frame %u", f);
        if (hi == lo) return a->fail(LX_ERR_ARG, "frame %u has no roots", f);
        if (!in.root_ev) return a->fail(LX_ERR_ARG, "null root_ev");
        if (hi - lo > kMaxFrameRoots) return a->fail(LX_ERR_ARG, "frame %u: more than %u roots", f, kMaxFrameRoots);
        for (uint64_t k = lo; k < hi; k++) {
            const uint32_t e = in.root_ev[k];
            if (e >= in.n) return a->fail(LX_ERR_ARG, "frame %u: root %u is not an event of the epoch", f, e);
            if (seen[e] == f) return a->fail(LX_ERR_ARG, "frame %u lists root %u twice", f, e);
            seen[e] = f;
            const uint32_t spf = sp[e] == NONE ? 0 : in.ev_frame[sp[e]];
            if (!(spf < f && f <= in.ev_frame[e]))
                return a->fail(LX_ERR_ARG, "frame %u: event %u (frame %u, self-parent's %u) is no root of it", f, e,
                               in.ev_frame[e], spf);
        }
    }
    const uint64_t slots = in.nf ? in.root_off[in.nf] : 0;
    if (slots != want_slots)
        return a->fail(LX_ERR_ARG, "the roots table holds %llu slots, the event frames imply %llu",
                       (unsigned long long)slots, (unsigned long long)want_slots);
    return 0;
}

// The tables of the persisted epoch, the observed-roots bit rows of the slots
// above the last decided frame, and bootstrapElection (event_processing.go:
// 102-146).  The bit row of a slot of frame f is not persisted (the reference
// asks ForklessCause again, election.go:110-124): it is rebuilt as
// FC(slot, r) over ALL slots r of frame f - 1, one step per frame in one
// merged launch.  While the epoch ran, the row was taken when the event was
// processed and covered only the slots of f - 1 known by then (bm_len); the
// slots added later are later events, not ancestors of this one, so their
// ForklessCause is false and the full-length row reads the same.
int restore_epoch(lx_abft *a, const IndexView &iv, const RestoreIn &in, std::vector<uint32_t> &sp) {
    hipStream_t s = iv.stream;
    const double t0 = now_ms();
    clear_epoch(a);
    a->epoch = in.epoch;
    a->V = in.nv;
    a->weights.assign(in.w, in.w + in.nv);
    a->quorum = iv.quorum;
    a->last_decided = in.last_decided;
    a->ev_sp.swap(sp);
    if (in.n) {
        a->ev_frame.assign(in.ev_frame, in.ev_frame + in.n);
        a->ev_confirmed.assign(in.ev_conf, in.ev_conf + in.n);
        a->par_off.resize((size_t)in.n + 1);
        for (uint32_t e = 0; e <= in.n; e++) a->par_off[e] = in.poff[e] - in.poff[0];
        if (in.poff[in.n] > in.poff[0]) a->par.assign(in.par + in.poff[0], in.par + in.poff[in.n]);
    }
    a->frames.resize((size_t)in.nf + 1);
    std::vector<FcStep> steps;
    uint64_t ncand = 0;
    for (uint32_t f = 1; f <= in.nf; f++) {
        const uint64_t lo = in.root_off[f - 1], hi = in.root_off[f];
        const uint32_t cnt = (uint32_t)(hi - lo);
        const bool rebuild = f > in.last_decided && f >= 2;   // frame 1 observes nothing
        const uint32_t R = rebuild ? (uint32_t)a->frames[f - 1].ev.size() : 0, words = (R + 31) / 32;
        Frame &fr = a->frames[f];
        fr.ev.reserve(cnt);
        fr.creator.reserve(cnt);
        fr.dup.reserve(cnt);
        fr.bm_off.reserve(cnt);
        fr.bm_len.reserve(cnt);
        for (uint32_t k = 0; k < cnt; k++) {
            const uint32_t e = in.root_ev[lo + k];
            add_slot(a, f, e, in.creator[e], rebuild ? a->arena_used + (uint64_t)k * words : 0, R);
        }
        if (rebuild) {
            steps.push_back(FcStep{f - 1, a->frames[f].ev.data(), cnt, R, words, a->arena_used, ncand});
            a->arena_used += (uint64_t)cnt * words;
            ncand += cnt;
        }
    }
    ARC(reserve(a, a->arena, a->arena_used + 1, 0, s));
    ARC(q_buffer(a, std::max<uint64_t>(ncand, 1), s));   // the quorum answers of the steps are not used
    ARC(launch_fc_steps(a, iv, steps, StepSet{}));
    AHIP(a, hipStreamSynchronize(s));
    ARC(collect_fc_times(a));
    a->stats.frame_steps += (uint32_t)steps.size();
    const double t1 = now_ms();
    a->stats.ms_frames += (float)(t1 - t0);
    // Orderer.Bootstrap runs before the callbacks are assigned (lachesis.go:
    // 92-98): frames decided here only move the last decided frame
    // (apply_block without BeginBlock and without the block log)
    const uint32_t block_log = a->block_log;
    a->cb = lx_abft_callbacks{};
    a->block_log = 0;
    uint64_t sealed_at;
    std::vector<uint32_t> new_w;
    const int rc = run_elections(a, &sealed_at, &new_w);
    a->block_log = block_log;
    a->stats.ms_election += (float)(now_ms() - t1);
    return rc;
}

struct Snapshot {
    std::vector<size_t> sizes;
    uint64_t arena_used;
    uint64_t n_events;
};

Snapshot take_snapshot(lx_abft *a) {
    Snapshot s;
    for (const Frame &f : a->frames) s.sizes.push_back(f.ev.size());
    s.arena_used = a->arena_used;
    s.n_events = a->ev_frame.size();
    return s;
}

void restore_snapshot(lx_abft *a, const Snapshot &s) {
    for (size_t f = 0; f < a->frames.size(); f++) {
        Frame &fr = a->frames[f];
        size_t keep = f < s.sizes.size() ? s.sizes[f] : 0;
        while (fr.ev.size() > keep) {
            uint32_t c = fr.creator.back();
            fr.last_of[c] = fr.dup.back();
            fr.ev.pop_back();
            fr.creator.pop_back();
            fr.dup.pop_back();
            fr.bm_off.pop_back();
            fr.bm_len.pop_back();
        }
        fr.synced = std::min<uint32_t>(fr.synced, (uint32_t)keep);
        fr.voted = std::min<uint32_t>(fr.voted, (uint32_t)keep);
    }
    while (a->frames.size() > s.sizes.size() && a->frames.size() > 1 && a->frames.back().ev.empty())
        a->frames.pop_back();
    a->arena_used = s.arena_used;
    a->ev_frame.resize(s.n_events);
    a->ev_sp.resize(s.n_events);
    a->ev_confirmed.resize(s.n_events);
    a->sweep_atropos.clear();
    a->sweep_frame.clear();
    a->par_off.resize(s.n_events + 1);
    a->par.resize(a->par_off.back());
}

// adds the batch to the index and the host event tables
int add_events(lx_abft *a, uint32_t n, const uint32_t *creator, const uint32_t *seq, const uint64_t *poff,
               const uint32_t *par) {
    PassTimer pt("index");
    uint32_t err_index = 0;
    int rc = lx_add_batch(a->ix, n, creator, seq, poff, par, nullptr, &err_index);
    if (rc) return a->ixfail(rc);
    pt.mark("add_batch");
    const uint64_t e0 = a->ev_sp.size();
    a->ev_sp.resize(e0 + n);
    a->ev_frame.resize(e0 + n, 0);
    a->ev_confirmed.resize(e0 + n, 0);
    a->par_off.reserve(a->par_off.size() + n);
    const uint64_t q0 = a->par.size();
    a->par.insert(a->par.end(), par + poff[0], par + poff[n]);
    for (uint32_t i = 0; i < n; i++) {
        const uint64_t p0 = poff[i], p1 = poff[i + 1];
        a->ev_sp[e0 + i] = seq[i] > 1 && p1 > p0 ? par[p0] : NONE;   // inter/dag/event.go:87-92
        a->par_off.push_back(q0 + (p1 - poff[0]));
    }
    pt.mark("tables");
    return 0;
}

// Work bound of the claimed path.  compute_frames_claimed queues claim(i) -
// selfParentFrame(i) frame steps for event i before any claim is verified,
// and its only guard (claim <= top + 1) moves with the claims themselves: V
// events claiming top + 1, top + 2, ... queue ~V^2 / 2 steps that the
// reference refuses after one or two.  One pass therefore takes the longest
// prefix of the batch whose queued steps stay within
//     kStepsPerEvent * n + kStepsPerValidator * V + kStepsFloor
// (n = events of the call), and at least one event: a single long climb, a
// validator back from an outage, is one candidate per step and is always
// taken whole.  The events behind the cut go through the next pass of the
// same call, when every frame below them is a verified one again, so a cut
// changes no result and is never reported as an error; the steps thrown away
// by a call that ends in LX_ERR_FRAME are within one budget.  An honest batch
// queues one step per root slot it adds (~1 per event or less) and is not cut.
constexpr uint64_t kStepsPerEvent = 2, kStepsPerValidator = 4, kStepsFloor = 64;

// events of [0, n) that one claimed pass takes (see above); base = dense
// index of event 0, not yet added
uint32_t claimed_pass_len(const lx_abft *a, uint64_t base, uint32_t n, uint64_t budget, const uint32_t *seq,
                          const uint64_t *poff, const uint32_t *par, const uint32_t *claimed) {
    uint64_t steps = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (seq[i] <= 1 || poff[i + 1] == poff[i]) continue;   // no self-parent: frame 1, no step
        const uint32_t sp = par[poff[i]];
        uint32_t spf;
        if (sp >= base) {
            if (sp - base >= i) continue;   // not an event before it: the index refuses the pass
            spf = claimed[sp - base];
        } else {
            spf = a->ev_frame[sp];
        }
        if (claimed[i] > spf) steps += claimed[i] - spf;
        if (steps > budget && i) return i;
    }
    return n;
}

int process_pass(lx_abft *a, uint32_t n, const uint32_t *creator, const uint32_t *seq, const uint64_t *poff,
                 const uint32_t *par, const uint32_t *claimed, uint32_t *out_frame, uint32_t *consumed) {
    *consumed = 0;
    if (!n) return 0;
    const uint64_t base = a->ev_frame.size();
    Snapshot snap = take_snapshot(a);
    double t0 = now_ms();
    ARC(add_events(a, n, creator, seq, poff, par));
    double t1 = now_ms();
    ARC(compute_frames(a, base, n, creator, claimed));
    double t2 = now_ms();
    a->stats.ms_index += (float)(t1 - t0);
    a->stats.ms_frames += (float)(t2 - t1);
    // checkAndSaveEvent: claimed frame must equal the computed one
    uint32_t bad = n;
    if (claimed)
        for (uint32_t i = 0; i < n; i++)
            if (claimed[i] != LX_FRAME_BUILD && claimed[i] != a->ev_frame[base + i]) { bad = i; break; }
    if (bad < n) {
        // the reference processes the events before the bad one; redo them alone
        restore_snapshot(a, snap);
        int rc = lx_drop_not_flushed(a->ix);
        if (rc) return a->ixfail(rc);
        uint32_t c = 0;
        const uint32_t epoch = a->epoch;
        if (bad) ARC(process_pass(a, bad, creator, seq, poff, par, claimed, out_frame, &c));
        *consumed = c;
        // a seal among the events before it, the last of them included: the
        // bad event belongs to the next epoch, where its frame was not checked
        if (c < bad || a->epoch != epoch) return 0;
        a->err = "claimed frame mismatched with calculated";
        return LX_ERR_FRAME;
    }
    uint64_t sealed_at;
    std::vector<uint32_t> new_w;
    double t3 = now_ms();
    ARC(run_elections(a, &sealed_at, &new_w));
    confirm_sweep(a);
    double t4 = now_ms();
    a->stats.ms_election += (float)(t4 - t3);
    uint32_t done = n;
    if (sealed_at != ~0ull) done = (uint32_t)(sealed_at - base + 1);
    if (out_frame)
        for (uint32_t i = 0; i < done; i++) out_frame[i] = a->ev_frame[base + i];
    *consumed = done;
    if (sealed_at != ~0ull) {
        ARC(start_epoch(a, a->epoch + 1, (uint32_t)new_w.size(), new_w.data()));
    } else {
        int rc = lx_flush(a->ix);
        if (rc) return a->ixfail(rc);
    }
    return 0;
}

// A claimed batch in passes of bounded speculative work (claimed_pass_len);
// every other batch in one.
int process(lx_abft *a, uint32_t n, const uint32_t *creator, const uint32_t *seq, const uint64_t *poff,
            const uint32_t *par, const uint32_t *claimed, uint32_t *out_frame, uint32_t *consumed) {
    *consumed = 0;
    if (!n) return 0;
    if (!claimed_path(a, n, claimed)) return process_pass(a, n, creator, seq, poff, par, claimed, out_frame, consumed);
    const uint64_t budget = kStepsPerEvent * n + kStepsPerValidator * a->V + kStepsFloor;
    std::vector<uint64_t> off;
    for (uint32_t lo = 0; lo < n;) {
        const uint32_t epoch = a->epoch;
        const uint32_t m = claimed_pass_len(a, a->ev_frame.size(), n - lo, budget, seq + lo, poff + lo, par, claimed + lo);
        uint32_t c = 0;
        int rc;
        if (lo == 0 && m == n) {
            rc = process_pass(a, n, creator, seq, poff, par, claimed, out_frame, &c);
        } else {
            off.resize(m + 1);   // parent offsets of the pass from 0
            for (uint32_t i = 0; i <= m; i++) off[i] = poff[lo + i] - poff[lo];
            rc = process_pass(a, m, creator + lo, seq + lo, off.data(), par + poff[lo], claimed + lo,
                              out_frame ? out_frame + lo : nullptr, &c);
        }
        *consumed += c;
        // an error, or a seal (the events behind it belong to the next epoch: the caller's)
        if (rc || c < m || a->epoch != epoch) return rc;
        lo += m;
    }
    return 0;
}

}  // namespace lxa

using namespace lxa;

static void clear_pairs(lx_abft *a) {
    a->pp_ent.clear();
    a->pp_keep.clear();
}

extern "C" {

int lx_abft_create(lx_index *index, lx_abft **out) {
    if (!index || !out) return LX_ERR_ARG;
    lx_abft *a = new lx_abft();
    a->ix = index;
    *out = a;
    return 0;
}

void lx_abft_destroy(lx_abft *a) {
    delete a;   // ~lx_abft waits for the device, then every member frees what it owns
}

const char *lx_abft_last_error(const lx_abft *a) { return a ? a->err.c_str() : "null handle"; }

int lx_abft_bootstrap(lx_abft *a, uint32_t epoch, uint32_t nv, const uint32_t *w, const lx_abft_callbacks *cb) {
    if (!a) return LX_ERR_ARG;
    if (a->booted) return a->fail(LX_ERR_STATE, "already bootstrapped");
    clear_pairs(a);
    a->cb = cb ? *cb : lx_abft_callbacks{};
    ARC(start_epoch(a, epoch, nv, w));
    a->booted = true;
    return 0;
}

int lx_abft_restore(lx_abft *a, uint32_t epoch, uint32_t nv, const uint32_t *w, uint32_t last_decided, uint32_t n,
                    const uint32_t *creator, const uint32_t *seq, const uint64_t *poff, const uint32_t *par,
                    const uint32_t *ev_frame, const uint32_t *ev_conf, uint32_t nf, const uint64_t *root_off,
                    const uint32_t *root_ev, const lx_abft_callbacks *cb) {
    if (!a) return LX_ERR_ARG;
    if (a->booted) return a->fail(LX_ERR_STATE, "already bootstrapped");
    clear_pairs(a);
    IndexView iv;
    int rc = lx_index_view(a->ix, &iv);   // refuses an index without an epoch
    if (rc) return a->ixfail(rc);
    const RestoreIn in{epoch, nv, w, last_decided, n, creator, seq, poff, par, ev_frame, ev_conf, nf, root_off, root_ev};
    std::vector<uint32_t> sp;
    ARC(check_restore(a, iv, in, &sp));
    a->stats = lx_abft_stats{};
    a->blog.clear();
    rc = restore_epoch(a, iv, in, sp);
    if (rc) {
        // not bootstrapped: another restore or a plain bootstrap starts over
        clear_epoch(a);
        a->cb = lx_abft_callbacks{};
        return rc;
    }
    a->cb = cb ? *cb : lx_abft_callbacks{};
    a->booted = true;
    return 0;
}

int lx_abft_state_sizes(lx_abft *a, lx_abft_state *out) {
    if (!a || !out) return LX_ERR_ARG;
    if (!a->booted) return a->fail(LX_ERR_STATE, "not bootstrapped");
    uint32_t nf = 0;
    uint64_t slots = 0;
    for (uint32_t f = 1; f < a->frames.size(); f++)
        if (!a->frames[f].ev.empty()) nf = f;
    for (uint32_t f = 1; f <= nf; f++) slots += a->frames[f].ev.size();
    out->epoch = a->epoch;
    out->last_decided_frame = a->last_decided;
    out->n_events = (uint32_t)a->ev_frame.size();
    out->n_frames = nf;
    out->n_slots = slots;
    return 0;
}

int lx_abft_state_fetch(lx_abft *a, uint32_t *ev_frame, uint32_t *ev_conf, uint64_t *root_off, uint32_t *root_ev) {
    lx_abft_state st;
    ARC(lx_abft_state_sizes(a, &st));
    if (ev_frame) std::copy(a->ev_frame.begin(), a->ev_frame.end(), ev_frame);
    if (ev_conf) std::copy(a->ev_confirmed.begin(), a->ev_confirmed.end(), ev_conf);
    uint64_t off = 0;
    if (root_off) root_off[0] = 0;
    for (uint32_t f = 1; f <= st.n_frames; f++) {
        const auto &ev = a->frames[f].ev;
        if (root_ev) std::copy(ev.begin(), ev.end(), root_ev + off);
        off += ev.size();
        if (root_off) root_off[f] = off;
    }
    return 0;
}

int lx_abft_set_option(lx_abft *a, const char *name, int64_t value) {
    if (!a || !name) return LX_ERR_ARG;
    const std::string k(name);
    if (k == "spec_depth") {
        if (value < 0 || value > 16) return a->fail(LX_ERR_ARG, "spec_depth must be 0..16");
        a->spec_depth = (uint32_t)value;
    } else if (k == "fc16") {
        if (value < 0 || value > 1) return a->fail(LX_ERR_ARG, "fc16 must be 0 or 1");
        a->fc16 = value != 0;
    } else if (k == "claimed_batch") {
        if (value < 0 || value > 1) return a->fail(LX_ERR_ARG, "claimed_batch must be 0 or 1");
        a->claimed_batch = value != 0;
    } else if (k == "block_log") {
        if (value < 0 || value > 2) return a->fail(LX_ERR_ARG, "block_log must be 0, 1 or 2");
        a->block_log = (uint32_t)value;
    } else if (k == "elect_ahead") {
        if (value < 0 || value > 8 || value == 1) return a->fail(LX_ERR_ARG, "elect_ahead must be 0 or 2..8");
        a->elect_ahead = (uint32_t)value;
    } else {
        return a->fail(LX_ERR_ARG, "unknown option %s", name);
    }
    return 0;
}

int lx_abft_reset(lx_abft *a, uint32_t epoch, uint32_t nv, const uint32_t *w) {
    if (!a) return LX_ERR_ARG;
    if (!a->booted) return a->fail(LX_ERR_STATE, "not bootstrapped");
    clear_pairs(a);
    return start_epoch(a, epoch, nv, w);
}

int lx_abft_process_batch(lx_abft *a, uint32_t n, const uint32_t *creator, const uint32_t *seq,
                          const uint64_t *poff, const uint32_t *par, const uint32_t *claimed, uint32_t *out_frame,
                          uint32_t *consumed) {
    if (!a || !consumed) return LX_ERR_ARG;
    if (!a->booted) return a->fail(LX_ERR_STATE, "not bootstrapped");
    a->stats = lx_abft_stats{};
    a->blog.clear();
    clear_pairs(a);
    return process(a, n, creator, seq, poff, par, claimed, out_frame, consumed);
}

int lx_abft_block_log(const lx_abft *a, uint32_t *n_blocks, const uint32_t **frame, const uint32_t **atropos,
                      const uint32_t **cheat_off, const uint32_t **cheaters, const uint32_t **conf_off,
                      const uint32_t **confirmed) {
    if (!a || !n_blocks) return LX_ERR_ARG;
    const BlockLog &L = a->blog;
    *n_blocks = (uint32_t)L.frame.size();
    if (frame) *frame = L.frame.data();
    if (atropos) *atropos = L.atropos.data();
    if (cheat_off) *cheat_off = L.cheat_off.data();
    if (cheaters) *cheaters = L.cheaters.data();
    if (conf_off) *conf_off = L.conf_off.data();
    if (confirmed) *confirmed = L.confirmed.data();
    return 0;
}

int lx_abft_build(lx_abft *a, uint32_t creator, uint32_t seq, uint32_t np, const uint32_t *parents,
                  uint32_t *out_frame) {
    if (!a || !out_frame) return LX_ERR_ARG;
    if (!a->booted) return a->fail(LX_ERR_STATE, "not bootstrapped");
    const uint64_t base = a->ev_frame.size();
    clear_pairs(a);
    Snapshot snap = take_snapshot(a);
    uint64_t poff[2] = {0, np};
    int rc = add_events(a, 1, &creator, &seq, poff, parents);
    if (rc == 0) rc = compute_frames(a, base, 1, &creator, nullptr);
    if (rc == 0) *out_frame = a->ev_frame[base];
    restore_snapshot(a, snap);
    int rc2 = lx_drop_not_flushed(a->ix);
    if (rc) return rc;
    if (rc2) return a->ixfail(rc2);
    return 0;
}

int lx_abft_build_frames(lx_abft *a, uint32_t n, const uint32_t *creator, const uint32_t *seq, const uint64_t *poff,
                         const uint32_t *par, uint32_t *out_frame, uint8_t *out_is_root, uint32_t *err_index) {
    if (!a) return LX_ERR_ARG;
    a->bstats = lx_abft_build_stats{};
    clear_pairs(a);
    if (err_index) *err_index = 0;
    if (!a->booted) return a->fail(LX_ERR_STATE, "not bootstrapped");
    if (!n) return 0;
    if (!creator || !seq || !poff || !out_frame) return a->fail(LX_ERR_ARG, "null input");
    const int rc = build_frames(a, n, creator, seq, poff, par, out_frame, out_is_root, err_index);
    if (rc == LX_ERR_ARG) a->bstats = lx_abft_build_stats{};
    return rc;
}

int lx_abft_build_progress(lx_abft *a, uint32_t n, const uint32_t *creator, const uint32_t *seq, const uint64_t *poff,
                           const uint32_t *par, const uint32_t *at_frame, uint32_t flags, uint32_t *out_frame,
                           uint32_t *out_n_roots, uint32_t *out_n_caused, uint32_t *out_stake,
                           uint64_t *out_root_stake, uint32_t *err_index) {
    if (!a) return LX_ERR_ARG;
    a->bstats = lx_abft_build_stats{};
    clear_pairs(a);
    if (err_index) *err_index = 0;
    if (!a->booted) return a->fail(LX_ERR_STATE, "not bootstrapped");
    if (flags & ~LX_PROGRESS_PAIRS) return a->fail(LX_ERR_ARG, "unknown flags");
    if (!n) return 0;
    if (!creator || !seq || !poff || !out_frame) return a->fail(LX_ERR_ARG, "null input");
    const Progress pg{nullptr, at_frame, (flags & LX_PROGRESS_PAIRS) != 0, out_n_roots, out_n_caused, out_stake,
                      out_root_stake};
    const int rc = build_frames(a, n, creator, seq, poff, par, out_frame, nullptr, err_index, &pg);
    if (rc == LX_ERR_ARG) a->bstats = lx_abft_build_stats{};
    if (rc) clear_pairs(a);
    return rc;
}

int lx_abft_event_progress(lx_abft *a, uint32_t n, const uint32_t *ev, const uint32_t *at_frame, uint32_t flags,
                           uint32_t *out_frame, uint32_t *out_n_roots, uint32_t *out_n_caused, uint32_t *out_stake,
                           uint64_t *out_root_stake, uint32_t *err_index) {
    if (!a) return LX_ERR_ARG;
    a->bstats = lx_abft_build_stats{};
    clear_pairs(a);
    if (err_index) *err_index = 0;
    if (!a->booted) return a->fail(LX_ERR_STATE, "not bootstrapped");
    if (flags & ~LX_PROGRESS_PAIRS) return a->fail(LX_ERR_ARG, "unknown flags");
    if (!n) return 0;
    if (!ev || !out_frame) return a->fail(LX_ERR_ARG, "null input");
    const Progress pg{ev, at_frame, (flags & LX_PROGRESS_PAIRS) != 0, out_n_roots, out_n_caused, out_stake,
                      out_root_stake};
    const int rc = event_progress(a, n, ev, out_frame, err_index, &pg);
    if (rc == LX_ERR_ARG) a->bstats = lx_abft_build_stats{};
    if (rc) clear_pairs(a);
    return rc;
}

int lx_abft_last_progress_pairs(lx_abft *a, uint64_t *pair_off, uint32_t *out_root, uint32_t *out_stake, uint64_t cap,
                                uint64_t *n_pairs) {
    if (!a || !n_pairs) return LX_ERR_ARG;
    uint64_t total = 0;
    for (size_t i = 0; i < a->pp_ent.size(); i++) {
        const lx_abft::PairEnt &e = a->pp_ent[i];
        if (pair_off) pair_off[i] = total;
        const uint64_t w = total < cap ? std::min<uint64_t>(e.n, cap - total) : 0;
        if (w && out_root) std::copy_n(a->frames[e.frame].ev.begin(), w, out_root + total);
        if (w && out_stake) std::copy_n(a->pp_keep.begin() + e.off, w, out_stake + total);
        total += e.n;
    }
    if (pair_off) pair_off[a->pp_ent.size()] = total;
    *n_pairs = total;
    return 0;
}

int lx_abft_build_last_stats(const lx_abft *a, lx_abft_build_stats *out) {
    if (!a || !out) return LX_ERR_ARG;
    *out = a->bstats;
    return 0;
}

uint32_t lx_abft_epoch(const lx_abft *a) { return a ? a->epoch : 0; }
uint32_t lx_abft_last_decided_frame(const lx_abft *a) { return a ? a->last_decided : 0; }

int lx_abft_frame_roots(lx_abft *a, uint32_t f, uint32_t *out, uint32_t cap, uint32_t *n) {
    if (!a || !n) return LX_ERR_ARG;
    *n = 0;
    if (f >= a->frames.size()) return 0;
    const auto &ev = a->frames[f].ev;
    *n = (uint32_t)ev.size();
    if (out) std::copy(ev.begin(), ev.begin() + std::min<size_t>(cap, ev.size()), out);
    return 0;
}

int lx_abft_event_frame(const lx_abft *a, uint32_t ev, uint32_t *frame) {
    if (!a || !frame || ev >= a->ev_frame.size()) return LX_ERR_ARG;
    *frame = a->ev_frame[ev];
    return 0;
}

int lx_abft_event_confirmed_on(const lx_abft *a, uint32_t ev, uint32_t *frame) {
    if (!a || !frame || ev >= a->ev_confirmed.size()) return LX_ERR_ARG;
    *frame = a->ev_confirmed[ev];
    return 0;
}

int lx_abft_last_stats(const lx_abft *a, lx_abft_stats *out) {
    if (!a || !out) return LX_ERR_ARG;
    *out = a->stats;
    return 0;
}

}  // extern "C"