// lx_abft_frames.cpp -- frames of the batched abft caller (lx_abft_engine.h).
//
// Frames (calcFrameIdx, abft/event_processing.go:163-189).  frame(e) is the
// first f >= selfParentFrame(e) at which e is NOT forkless-caused by a quorum
// of roots(f) (capped by the claimed frame, or selfParentFrame+100 in Build);
// roots(f) = events with selfParentFrame < f <= frame.  ForklessCause(e, r)
// can only hold for ancestors r of e, so the answer for e depends only on its
// ancestors and the batch can be solved frame by frame: at step f every
// event still undecided has frame >= f, roots(f) is complete, and every event
// whose loop has reached f asks q_f(e) = quorum(roots(f)) -- all of them in
// one k_root_fc tile launch.  Self-children of those events are evaluated
// speculatively in the same launch (their self-parent usually stops at f).
// An event that passes q_f becomes a root of f+1; its bit row of that launch
// is exactly the observed-roots set the election needs for that root slot.
// A batch in which every event claims its frame needs no steps at all: every
// question is known up front (compute_frames_claimed), one launch answers all.
#include "lx_abft_engine.h"

namespace lxa {

// the step's uploads in one k_scatter launch (stream-ordered before the
// kernels that read them)
int flush_uploads(lx_abft *a, hipStream_t s) {
    Uploader &u = a->up;
    if (!u.pending()) return 0;
    const int k = u.next;
    u.next = (u.next + 1) % Uploader::kSlots;
    if (!u.done[k]) AHIP(a, hipEventCreateWithFlags(&u.done[k].e, hipEventDisableTiming));
    if (u.used[k]) AHIP(a, hipEventSynchronize(u.done[k]));   // the slot's last k_scatter has read it
    const uint64_t dbytes = u.desc.size() * sizeof(ScatterDesc);
    const uint64_t need = dbytes + u.data.size();
    AHIP(a, u.pin[k].grow(need, std::max<uint64_t>(need * 2, 1u << 16), s, false));
    uint64_t max_bytes = 0;
    for (auto &d : u.desc) {
        d.src_off += dbytes;
        max_bytes = std::max<uint64_t>(max_bytes, d.bytes);
    }
    memcpy(u.pin[k].host(), u.desc.data(), dbytes);
    memcpy(u.pin[k].host() + dbytes, u.data.data(), u.data.size());
    const uint8_t *base = u.pin[k].dev();
    AHIP(a, lx::launch_scatter(reinterpret_cast<const ScatterDesc *>(base), (uint32_t)u.desc.size(), max_bytes, base,
                               s));
    AHIP(a, hipEventRecord(u.done[k], s));
    u.used[k] = true;
    u.launches++;
    u.desc.clear();
    u.data.clear();
    return 0;
}

// a->rb_pin holds `need` words (contents not kept)
static int rb_buffer(lx_abft *a, uint64_t need, hipStream_t s) {
    AHIP(a, a->rb_pin.grow(need, std::max<uint64_t>(need * 2, 4096), s, true));
    return 0;
}

// words [0, na) of a and [0, nb) of b (device) into a->rb_pin, then wait for
// the stream: the host reads them at the returned pointer
int readback(lx_abft *a, hipStream_t s, const uint32_t *x, uint32_t na, const uint32_t *y, uint32_t nb,
             const uint32_t **out) {
    ARC(rb_buffer(a, (uint64_t)na + nb, s));
    AHIP(a, lx::launch_readback(a->rb_pin.dev(), x, na, y, nb, s));
    AHIP(a, hipStreamSynchronize(s));
    *out = a->rb_pin.host();
    return 0;
}

// HB rows of events rows[k] into a->rb_pin (k * V), then wait for the stream
int readback_rows(lx_abft *a, const IndexView &iv, const std::vector<uint32_t> &rows, const uint32_t **out) {
    ARC(rb_buffer(a, (uint64_t)rows.size() * a->V, iv.stream));
    AHIP(a, lx::launch_gather_rows(a->rb_pin.dev(), iv.hb, iv.stride, a->V, rows.data(), (uint32_t)rows.size(),
                                   iv.stream));
    AHIP(a, hipStreamSynchronize(iv.stream));
    *out = a->rb_pin.host();
    return 0;
}

Frame &frame_at(lx_abft *a, uint32_t f) {
    if (a->frames.size() <= f) a->frames.resize(f + 1);
    return a->frames[f];
}

void add_slot(lx_abft *a, uint32_t f, uint32_t e, uint32_t creator, uint64_t bm_off, uint32_t bm_len) {
    Frame &fr = frame_at(a, f);
    if (fr.last_of.empty()) fr.last_of.assign(a->V, NONE);
    uint32_t k = (uint32_t)fr.ev.size();
    fr.ev.push_back(e);
    fr.creator.push_back(creator);
    fr.dup.push_back(fr.last_of[creator]);
    fr.last_of[creator] = k;
    fr.bm_off.push_back(bm_off);
    fr.bm_len.push_back(bm_len);
}

int sync_frame(lx_abft *a, Frame &fr, hipStream_t s) {
    uint32_t from = fr.synced;
    if (from == fr.ev.size()) return 0;
    ARC(upload(a, fr.d_ev, fr.ev, from, s));
    ARC(upload(a, fr.d_creator, fr.creator, from, s));
    ARC(upload(a, fr.d_dup, fr.dup, from, s));
    ARC(upload(a, fr.d_bm_len, fr.bm_len, from, s));
    ARC(upload(a, fr.d_bm_off, fr.bm_off, from, s));
    fr.synced = (uint32_t)fr.ev.size();
    return 0;
}

// Cheaters' branch columns, grouped by creator, original first (k_root_fc).
int refresh_cheaters(lx_abft *a, const IndexView &iv) {
    if (a->k_gen == iv.branch_gen) return 0;
    std::vector<uint32_t> col, flag, kw;
    for (uint32_t c = 0; c < iv.V; c++) {
        const auto &l = (*iv.by_creator)[c];
        if (l.size() < 2) continue;
        for (size_t i = 0; i < l.size(); i++) {
            col.push_back(l[i]);
            flag.push_back((i == 0 ? 1u : 0u) | (i + 1 == l.size() ? 2u : 0u));
            kw.push_back(i + 1 == l.size() ? (*iv.weights)[c] : 0u);
        }
    }
    a->n_k = (uint32_t)col.size();
    if (a->n_k) {
        ARC(upload(a, a->d_kcol, col, 0, iv.stream));
        ARC(upload(a, a->d_kflag, flag, 0, iv.stream));
        ARC(upload(a, a->d_kw, kw, 0, iv.stream));
    }
    a->k_gen = iv.branch_gen;
    return 0;
}

// VALU lane-ops per (event, root) pair of the root-FC inner loops (ISA count):
// 2.5 per column in k_root_fc, 1.5 in k_root_fc16 (2 in its 32-column chunks
// holding a weight >= 2^16), over the padded columns
uint64_t fc_ops_per_pair(const lx_abft *a, const IndexView &iv, bool forks, bool seq16, uint32_t ncols) {
    if (forks || !seq16) return 5 * (uint64_t)ncols / 2;
    uint64_t hi_cols = 0;
    for (uint32_t c = 0; c < iv.V; c += 32)
        for (uint32_t j = c; j < std::min(c + 32, iv.V); j++)
            if (a->weights[j] >> 16) {
                hi_cols += 32;
                break;
            }
    return (3 * (uint64_t)ncols + hi_cols) / 2;
}

// after the stream has drained: k_root_fc times of the launches since the last call
int collect_fc_times(lx_abft *a) {
    for (uint32_t k = 0; k < a->fc_ev_used; k++) {
        float ms = 0;
        AHIP(a, hipEventElapsedTime(&ms, a->fc_ev[2 * k], a->fc_ev[2 * k + 1]));
        a->stats.ms_root_fc_gpu += ms;
    }
    a->fc_ev_used = 0;
    return 0;
}

// the next pair of timing events exists (fc_ev[2 k], fc_ev[2 k + 1], k = fc_ev_used)
static int fc_event_pair(lx_abft *a) {
    while (a->fc_ev.size() < 2ull * (a->fc_ev_used + 1)) {
        Event e;
        AHIP(a, hipEventCreate(&e.e));
        a->fc_ev.push_back(std::move(e));
    }
    return 0;
}

// a->q_pin holds the q answers of n candidates (contents not kept)
int q_buffer(lx_abft *a, uint64_t n, hipStream_t s) {
    AHIP(a, a->q_pin.grow(n, std::max<uint64_t>(n, 4096), s, true));
    return 0;
}

// the read-out fields QuorumArgs and ProgressArgs share, for step x behind r
template <typename A>
static void fill_readout(A &q, const lx_abft *a, const IndexView &iv, const Frame &fr, const FcStep &x,
                         const RootFcArgs &r, const uint32_t *cand, uint32_t block0) {
    q.psum = r.psum;
    q.n_split = r.n_split;
    q.words = x.words;
    q.n_roots = x.n_roots;
    q.n_cand = x.n_cand;
    q.cand = cand;
    q.root_ev = fr.d_ev;
    q.creator = fr.d_creator;
    q.dup = fr.d_dup;
    q.wcreator = iv.wpad;
    q.quorum = a->quorum;
    q.q = a->q_pin.dev() + x.qoff;   // answers land in pinned host memory
    q.block0 = block0;
}

// The steps in one k_root_fc launch and one read-out launch (the MULTI forms,
// the steps' arguments uploaded with the candidates; set.by_value: one step
// through the plain kernels).  The read-out's rows and a->q_pin already hold
// room for every step.  Enqueued, nothing waits.
int launch_fc_steps(lx_abft *a, const IndexView &iv, const std::vector<FcStep> &st, const StepSet &set) {
    if (st.empty()) return 0;
    hipStream_t s = iv.stream;
    const uint32_t n = (uint32_t)st.size();
    const bool scratch = set.rows == StepSet::kScratch, prog = set.out == StepSet::kProgress;
    const bool prog_multi = prog && n > 1;   // one progress step takes its args by value
    uint64_t ncand = 0, tiles = 0;
    for (const FcStep &x : st) {
        ARC(sync_frame(a, frame_at(a, x.frame), s));
        ncand += x.n_cand;
        tiles += fc_tiles(x.n_cand, x.n_roots);
    }
    // split the columns when the tiles alone cannot fill the chip
    const uint32_t ncols = (iv.V + 31) / 32 * 32;
    const FcColSplit sp = fc_col_split(tiles, ncols);
    uint64_t npsum = 0;
    for (const FcStep &x : st) npsum += (uint64_t)sp.n_split * x.n_cand * x.words * 32;
    ARC(reserve(a, a->d_cand, ncand, 0, s));
    ARC(reserve(a, a->d_psum, npsum, 0, s));
    if (!set.by_value) {
        ARC(reserve(a, a->d_fcargs, n, 0, s));
        if (prog) ARC(reserve(a, a->d_pgargs, n, 0, s));
        else ARC(reserve(a, a->d_qargs, n, 0, s));
    }
    ARC(refresh_cheaters(a, iv));
    // what the set reads and writes
    RootFcArgs base{};
    base.hb = scratch ? a->b_plane.get() : iv.hb;
    base.la = iv.la;
    base.stride = iv.stride;
    base.ncols = ncols;
    base.wpad = iv.wpad;
    base.quorum = a->quorum;
    base.n_k = a->n_k;
    base.kcol = a->d_kcol;
    base.kflag = a->d_kflag;
    base.kw = a->d_kw;
    base.ev_branch = iv.ev_branch;
    base.own = scratch ? a->b_args.get() : nullptr;
    uint32_t *const bits = set.out == StepSet::kArena ? a->arena.get() : a->b_bits.get();
    uint32_t *const pair_out = set.pairs ? a->pp_pin.dev() : nullptr;
    std::vector<RootFcArgs> fa(n);
    std::vector<QuorumArgs> qa(prog ? 0 : n);
    std::vector<ProgressArgs> pa(prog ? n : 0);
    uint64_t coff = 0, poff = 0, pairs = 0;
    uint32_t blocks = 0, qblocks = 0;
    for (uint32_t j = 0; j < n; j++) {
        const FcStep &x = st[j];
        const Frame &fr = a->frames[x.frame];
        a->up.add(a->d_cand + coff, x.cand, x.n_cand * 4ull);
        // rows of the scratch plane are no events: any root stands in for a dropped slot
        RootFcArgs &r = fa[j] = lx::root_fc_step(base, a->d_cand + coff, x.n_cand, fr.d_ev, x.n_roots,
                                                 scratch ? fr.ev[0] : x.cand[0], a->d_psum + poff, x.words, sp);
        r.block0 = blocks;
        blocks += lx::root_fc_blocks(r);
        // ... and none of them is a root slot the read-out would skip
        const uint32_t *qcand = scratch ? a->b_none.get() : r.cand;
        if (prog) {
            fill_readout(pa[j], a, iv, fr, x, r, qcand, qblocks);
            pa[j].out = a->pg_pin.dev() + x.qoff;
            pa[j].pairs = pair_out ? pair_out + x.pair0 : nullptr;
        } else {
            fill_readout(qa[j], a, iv, fr, x, r, qcand, qblocks);
            qa[j].bits = bits + x.row0;
        }
        qblocks += (x.n_cand + 3) / 4;
        coff += x.n_cand;
        poff += (uint64_t)sp.n_split * x.n_cand * x.words * 32;
        pairs += (uint64_t)x.n_cand * x.n_roots;
    }
    if (!set.by_value) {
        a->up.add(a->d_fcargs, fa.data(), n * sizeof(RootFcArgs));
        if (!prog) a->up.add(a->d_qargs, qa.data(), n * sizeof(QuorumArgs));
        else if (prog_multi) a->up.add(a->d_pgargs, pa.data(), n * sizeof(ProgressArgs));
    }
    if (set.pt) set.pt->mark("args");
    ARC(flush_uploads(a, s));
    if (set.pt) set.pt->mark("upload");
    const bool forks = iv.B > iv.V, seq16 = a->fc16 && iv.max_seq <= 0xFFFFu && set.seq16;
    if (set.first) {
        AHIP(a, lx::launch_build_rows(*set.first, forks, s));
        a->bstats.launches++;
    }
    if (set.engine) {
        ARC(fc_event_pair(a));
        AHIP(a, hipEventRecord(a->fc_ev[2 * a->fc_ev_used], s));
    }
    if (set.by_value) AHIP(a, lx::launch_root_fc(fa[0], forks, seq16, s));
    else if (scratch) AHIP(a, lx::launch_root_fc_own_multi(a->d_fcargs, n, blocks, forks, seq16, s));
    else AHIP(a, lx::launch_root_fc_multi(a->d_fcargs, n, blocks, forks, seq16, s));
    if (set.engine) {
        AHIP(a, hipEventRecord(a->fc_ev[2 * a->fc_ev_used + 1], s));
        a->fc_ev_used++;
    }
    if (prog_multi) AHIP(a, lx::launch_root_progress_multi(a->d_pgargs, n, qblocks, s));
    else if (prog) AHIP(a, lx::launch_root_progress(pa[0], s));
    else if (set.by_value) AHIP(a, lx::launch_root_quorum(qa[0], s));
    else AHIP(a, lx::launch_root_quorum_multi(a->d_qargs, n, qblocks, s));
    if (set.engine) {
        a->stats.fc_launches++;
        a->stats.fc_pairs += pairs;
        a->stats.fc_pair_cols += pairs * iv.V;
        a->stats.fc_lane_ops += pairs * fc_ops_per_pair(a, iv, forks, seq16, ncols);
    } else {
        a->bstats.launches += 2;
        a->bstats.fc_pairs += pairs;
        a->bstats.fc16 = !forks && seq16;
    }
    return 0;
}

// One frame step, answered: bits (cands x roots(f)) into the arena at *row0, q
// per candidate.  One step, its kernel arguments by value.
int eval_frame(lx_abft *a, const IndexView &iv, uint32_t f, const std::vector<uint32_t> &cand, uint64_t *row0,
               uint32_t *words_out, std::vector<uint8_t> &q) {
    hipStream_t s = iv.stream;
    const uint32_t n = (uint32_t)cand.size(), R = (uint32_t)frame_at(a, f).ev.size(), words = (R + 31) / 32;
    ARC(q_buffer(a, n, s));
    *row0 = a->arena_used;
    *words_out = words;
    ARC(reserve(a, a->arena, a->arena_used + (uint64_t)n * words + 1, a->arena_used, s));
    a->arena_used += (uint64_t)n * words;
    if (!words) {
        q.assign(n, 0);   // no roots in frame f: no quorum (WeightCounter of nothing)
        return 0;
    }
    StepSet set;
    set.by_value = true;
    ARC(launch_fc_steps(a, iv, {FcStep{f, cand.data(), n, R, words, *row0, 0}}, set));
    AHIP(a, hipStreamSynchronize(s));
    q.assign(a->q_pin.host(), a->q_pin.host() + n);
    return collect_fc_times(a);
}

// Frames of a batch in which every event claims its frame (Process,
// event_processing.go:163-189 with the claimed frame as the loop bound).
// Taking the claims of in-batch self-parents as given, every question is
// known up front: event i asks q_f(i) for f in [selfParentFrame(i), claim(i)),
// and roots(f) = the roots of f so far plus the batch events claiming f or
// more above a self-parent frame below f (Store.AddRoot adds a root to every
// frame it passes, store_roots.go:23-27), in event order (the order
// per-event Process adds them).  ForklessCause(i, r) is false for every r that is not an ancestor of
// i, so roots later in event order change none of i's answers.  All frame
// steps are enqueued back to back and answered after one wait.  Up to the
// first event whose computed frame differs from its claim, every claim used
// was verified, so the answers are exact there; process() redoes that prefix
// alone (nothing after it is reported).  A claim above every root frame so far
// + 1 cannot verify (frame top+1 has no roots): the batch is cut there.
// Work bound: the queued steps are sum(claim(i) - selfParentFrame(i)), all
// evaluated before the first claim is checked.  process() hands this function
// at most 2 n + 4 V + 64 of them per pass (n = events of the call; see
// claimed_pass_len), or the steps of one event alone, and runs the rest of the
// batch as further passes, so inflated claims cost one such budget at most.
int compute_frames_claimed(lx_abft *a, uint64_t base, uint32_t n, const uint32_t *creator, const uint32_t *claimed) {
    PassTimer pt("frames");
    IndexView iv;
    int rc = lx_index_view(a->ix, &iv);
    if (rc) return a->ixfail(rc);
    pt.mark("view");
    hipStream_t s = iv.stream;
    uint32_t top = 0;   // highest frame with a root
    for (uint32_t f = 1; f < a->frames.size(); f++)
        if (!a->frames[f].ev.empty()) top = f;
    std::vector<uint32_t> spf(n, 0), rf(n, NONE);
    uint32_t cut = n, fmin = NONE, fmax = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t sp = a->ev_sp[base + i];
        if (sp == NONE) {   // f = 0: roots(0) is empty -> frame 1 (:184-187)
            rf[i] = 1;
            top = std::max(top, 1u);
            continue;
        }
        spf[i] = sp < base ? a->ev_frame[sp] : claimed[sp - base];
        const uint32_t c = claimed[i];
        if (spf[i] == 0 || c > top + 1) {
            cut = i;
            break;
        }
        if (c > spf[i]) {
            rf[i] = c;
            top = std::max(top, c);
            fmin = std::min(fmin, spf[i]);
            fmax = std::max(fmax, c - 1);
        }
    }
    pt.mark("scan");
    // candidates per frame step (event order) and each event's q slots
    const uint32_t nf = fmin == NONE ? 0 : fmax - fmin + 1;
    std::vector<std::vector<uint32_t>> cand(nf);
    std::vector<std::vector<uint32_t>> new_roots(top + 2);
    std::vector<uint64_t> qoff(nf + 1, 0), row0(nf, 0);
    std::vector<uint32_t> words(nf, 0), pos0(n, 0);
    {
        // list sizes first: one allocation per list
        std::vector<uint32_t> nc(nf, 0), nr(top + 2, 0);
        for (uint32_t i = 0; i < cut; i++) {
            if (a->ev_sp[base + i] == NONE) {
                nr[1]++;
                continue;
            }
            if (rf[i] == NONE) continue;
            for (uint32_t f = spf[i]; f < rf[i]; f++) {
                nc[f - fmin]++;
                nr[f + 1]++;
            }
        }
        for (uint32_t k = 0; k < nf; k++) cand[k].reserve(nc[k]);
        for (uint32_t f = 0; f < top + 2; f++) new_roots[f].reserve(nr[f]);
    }
    for (uint32_t i = 0; i < cut; i++) {
        if (a->ev_sp[base + i] == NONE) {
            new_roots[1].push_back(i);
            continue;
        }
        if (rf[i] == NONE) continue;
        // a root of every frame it passes: spf+1 .. claim (Store.AddRoot, store_roots.go:23-27)
        for (uint32_t f = spf[i] + 1; f <= rf[i]; f++) new_roots[f].push_back(i);
        pos0[i] = (uint32_t)cand[spf[i] - fmin].size();   // position in its first step
        for (uint32_t f = spf[i]; f < claimed[i]; f++) cand[f - fmin].push_back((uint32_t)(base + i));
    }
    for (uint32_t k = 0; k < nf; k++) qoff[k + 1] = qoff[k] + cand[k].size();
    ARC(q_buffer(a, std::max<uint64_t>(qoff[nf], 1), s));
    std::vector<uint8_t> launched(nf, 0);
    // a root's position in the step at f (binary search: cand lists are sorted)
    auto pos_in = [&](uint32_t f, uint32_t i) {
        const auto &c = cand[f - fmin];
        return (uint32_t)(std::lower_bound(c.begin(), c.end(), (uint32_t)(base + i)) - c.begin());
    };
    pt.mark("cands");
    // layout: step k (frame fmin + k) asks cand[k] against every root of its
    // frame (the ones so far + this batch's), bit rows at row0[k] in the arena
    const uint64_t arena0 = a->arena_used;
    std::vector<uint32_t> nroots(nf, 0);
    for (uint32_t k = 0; k < nf; k++) {
        const uint32_t f = fmin + k;
        nroots[k] = (uint32_t)(frame_at(a, f).ev.size() + (f < new_roots.size() ? new_roots[f].size() : 0));
        words[k] = (nroots[k] + 31) / 32;
        row0[k] = a->arena_used;
        a->arena_used += (uint64_t)cand[k].size() * words[k];
        launched[k] = !cand[k].empty() && words[k];
    }
    pt.mark("layout");
    // the roots, frame by frame in event order: a root of f observes the step at
    // f - 1 (its position there and the roots of f - 1 before it by merge walks:
    // every list is in event order)
    for (uint32_t f = 1; f < new_roots.size(); f++) {
        if (new_roots[f].empty()) continue;
        Frame &fr = frame_at(a, f);
        const size_t want = fr.ev.size() + new_roots[f].size();
        fr.ev.reserve(want);
        fr.creator.reserve(want);
        fr.dup.reserve(want);
        fr.bm_off.reserve(want);
        fr.bm_len.reserve(want);
        if (f == 1) {
            for (uint32_t i : new_roots[1]) add_slot(a, 1, (uint32_t)(base + i), creator[i], 0, 0);
            continue;
        }
        const uint32_t k = f - 1 - fmin;
        const auto &nr = new_roots[f - 1];
        const auto &cl = cand[k];
        const uint32_t old_roots = (uint32_t)(frame_at(a, f - 1).ev.size() - nr.size());
        size_t pc = 0, pb = 0;
        for (uint32_t i : new_roots[f]) {
            const uint32_t e = (uint32_t)(base + i);
            while (pc < cl.size() && cl[pc] < e) pc++;
            while (pb < nr.size() && nr[pb] < i) pb++;
            add_slot(a, f, e, creator[i], row0[k] + (uint64_t)pc * words[k], old_roots + (uint32_t)pb);
        }
    }
    pt.mark("slots");
    // every step in one k_root_fc and one k_root_quorum launch
    ARC(reserve(a, a->arena, a->arena_used + 1, arena0, s));
    std::vector<FcStep> act;
    for (uint32_t k = 0; k < nf; k++)
        if (launched[k])
            act.push_back(FcStep{fmin + k, cand[k].data(), (uint32_t)cand[k].size(), nroots[k], words[k], row0[k], qoff[k]});
    StepSet set;
    set.pt = &pt;
    ARC(launch_fc_steps(a, iv, act, set));
    pt.mark("launch");
    AHIP(a, hipStreamSynchronize(s));
    pt.mark("wait");
    ARC(collect_fc_times(a));
    a->stats.frame_steps += (uint32_t)act.size();
    for (uint32_t i = 0; i < n; i++) {
        if (i >= cut) {
            a->ev_frame[base + i] = NONE;   // never equals a claim: process() stops here
            continue;
        }
        if (a->ev_sp[base + i] == NONE) {
            a->ev_frame[base + i] = 1;
            continue;
        }
        uint32_t f = spf[i];
        for (uint32_t p = pos0[i]; f < claimed[i]; f++) {
            const uint32_t k = f - fmin;
            if (!launched[k] || !a->q_pin.host()[qoff[k] + (f == spf[i] ? p : pos_in(f, i))]) break;
        }
        a->ev_frame[base + i] = f;
    }
    return 0;
}

bool claimed_path(const lx_abft *a, uint32_t n, const uint32_t *claimed) {
    return claimed && a->claimed_batch &&
           std::none_of(claimed, claimed + n, [](uint32_t c) { return c == LX_FRAME_BUILD; });
}

// Frames of events [base, base+n) (all already added to the index).
// cap[i]: claimed frame (Process) or NONE = Build's selfParentFrame + 100.
int compute_frames(lx_abft *a, uint64_t base, uint32_t n, const uint32_t *creator, const uint32_t *claimed) {
    if (claimed_path(a, n, claimed)) return compute_frames_claimed(a, base, n, creator, claimed);
    IndexView iv;
    int rc = lx_index_view(a->ix, &iv);
    if (rc) return a->ixfail(rc);
    std::vector<uint32_t> cur(n, NONE), cap(n, NONE), child_head(n, NONE), child_next(n, NONE);
    std::map<uint32_t, std::vector<uint32_t>> pending;   // frame -> batch positions whose loop is at it
    for (uint32_t i = 0; i < n; i++) {
        uint32_t sp = a->ev_sp[base + i];
        if (sp != NONE && sp >= base) {
            uint32_t p = (uint32_t)(sp - base);
            child_next[i] = child_head[p];
            child_head[p] = i;
        }
    }
    auto cap_of = [&](uint32_t i, uint32_t sp_frame) {
        uint32_t c = claimed ? claimed[i] : LX_FRAME_BUILD;
        return c == LX_FRAME_BUILD ? sp_frame + kBuildCap : c;
    };
    // resolve(i, f): frame(i) = f; self-children start their loop at f.  A
    // child evaluated speculatively in the same launch is handled by the walk
    // below; the others are queued at f by flush().
    std::vector<std::pair<uint32_t, uint32_t>> pushed;
    auto resolve = [&](uint32_t i, uint32_t f) {
        a->ev_frame[base + i] = f;
        for (uint32_t c = child_head[i]; c != NONE; c = child_next[c]) {
            cur[c] = f;
            cap[c] = cap_of(c, f);
            pushed.emplace_back(c, f);
        }
    };
    auto flush = [&]() {
        for (auto &pc : pushed)
            if (a->ev_frame[base + pc.first] == 0 && cur[pc.first] == pc.second) pending[pc.second].push_back(pc.first);
        pushed.clear();
    };
    for (uint32_t i = 0; i < n; i++) {
        uint32_t sp = a->ev_sp[base + i];
        if (sp == NONE) {
            // f = 0: roots(0) is empty, no quorum -> f stays 0 -> frame 1 (:184-187)
            resolve(i, 1);
            add_slot(a, 1, (uint32_t)(base + i), creator[i], 0, 0);
        } else if (sp < base) {
            cur[i] = a->ev_frame[sp];
            cap[i] = cap_of(i, cur[i]);
            pending[cur[i]].push_back(i);
        }
    }
    flush();

    std::vector<uint8_t> spec(n, 0), q;
    std::vector<uint32_t> cand_pos, cand_ev;
    while (!pending.empty()) {
        const uint32_t f = pending.begin()->first;
        std::vector<uint32_t> Q = std::move(pending.begin()->second);
        pending.erase(pending.begin());
        // Events whose loop bound is f stop without asking (:184: the bound is
        // checked before the quorum) -- with claimed frames that is every
        // non-root event -- and their self-children start at f: drain them
        // all before launching.
        std::vector<uint32_t> ask, work = std::move(Q);
        while (!work.empty()) {
            const uint32_t i = work.back();
            work.pop_back();
            if (f < cap[i]) {
                ask.push_back(i);
                continue;
            }
            resolve(i, f);
            for (auto &pc : pushed) work.push_back(pc.first);
            pushed.clear();
        }
        if (ask.empty()) continue;
        std::sort(ask.begin(), ask.end());
        // speculative self-descendants, spec_depth deep
        cand_pos = ask;
        for (uint32_t i : ask) spec[i] = 2;
        {
            std::vector<uint32_t> lvl = ask, nxt;
            for (uint32_t d = 0; d < a->spec_depth && !lvl.empty() && n > 1; d++) {
                nxt.clear();
                for (uint32_t i : lvl)
                    for (uint32_t c = child_head[i]; c != NONE; c = child_next[c])
                        // a claimed frame above f says i passes q_f: its
                        // children cannot be at f, nothing to speculate
                        if (!spec[c] && cur[c] == NONE && (!claimed || claimed[i] == LX_FRAME_BUILD ||
                                                           claimed[i] <= f)) {
                            spec[c] = 1;
                            nxt.push_back(c);
                            cand_pos.push_back(c);
                        }
                lvl.swap(nxt);
            }
        }
        std::sort(cand_pos.begin(), cand_pos.end());
        cand_ev.resize(cand_pos.size());
        for (size_t k = 0; k < cand_pos.size(); k++) cand_ev[k] = (uint32_t)(base + cand_pos[k]);
        uint64_t row0;
        uint32_t words;
        ARC(eval_frame(a, iv, f, cand_ev, &row0, &words, q));
        for (size_t k = 0; k < cand_pos.size(); k++) {
            const uint32_t i = cand_pos[k];
            const bool own = spec[i] == 2;
            spec[i] = 0;
            // a speculative event counts only if its self-parent stopped at f
            // during this walk (then i's loop is at f too)
            if (!own && (cur[i] != f || a->ev_frame[base + i] != 0)) continue;
            if (f >= cap[i]) {
                resolve(i, f);
            } else if (q[k]) {
                cur[i] = f + 1;                      // root of f+1; its bit row observes roots(f)
                add_slot(a, f + 1, cand_ev[k], creator[i], row0 + k * (uint64_t)words, (uint32_t)frame_at(a, f).ev.size());
                pending[f + 1].push_back(i);
            } else {
                resolve(i, f);
            }
        }
        flush();
        a->stats.frame_steps++;
    }
    return 0;
}

// ---------------------------------------------------------------------------- Build without Add
// lx_abft_build_frames.  A candidate's frame depends on
// nothing that is not in the planes already: its HighestBefore row is the join
// of its parents' rows (k_build_rows), and ForklessCause against a frame's
// roots reads that row and the roots' LowestAfter rows, with the own-creator
// term corrected for the entries Add would have written (fc_own_term).  The
// frame loop of calcFrameIdx runs in rounds: every candidate still climbing
// asks q_f at its current frame, the candidates of one frame are one step of a
// merged launch, one wait per round.  Nothing of the engine's state is
// written: the frames' device mirrors are completed (sync_frame), scratch
// buffers grow, and that is all.
// lx_abft_build_progress / lx_abft_event_progress (section 9d) are the same
// steps with k_root_progress in the place of k_root_quorum: the stake sums of
// the step on which an entry stops are reported, not only its frame.
struct BuildCand {
    uint32_t pos;      // position in the call
    uint32_t spf;      // selfParentFrame
    uint32_t f;        // the loop's current frame
    bool last;         // progress calls: asked at f alone, no climb (explicit frame, cap reached, no self-parent, event)
};

// The candidates' tables as the device reads them (BuildArgs), after the input
// checks of lx_abft_build_frames on host tables alone.  act: the candidates
// that ask anything, = rows of the scratch plane, in call order.  pg == NULL
// (lx_abft_build_frames): a candidate without a self-parent asks nothing; a
// progress call gives it a virtual row too (own branch = the creator's
// original column, seq 1) and asks roots(1).
struct BuildTables {
    std::vector<BuildCand> act;
    std::vector<uint32_t> br, seq, cr, poff{0}, par;
    uint32_t max_seq = 0;
};

int build_tables(lx_abft *a, const IndexHostMeta &hm, uint64_t n_ev, uint32_t n, const uint32_t *creator,
                 const uint32_t *seq, const uint64_t *poff, const uint32_t *par, const Progress *pg,
                 uint32_t *err_index, BuildTables *t) {
    auto bad = [&](uint32_t i, const char *what) {
        if (err_index) *err_index = i;
        return a->fail(LX_ERR_ARG, "candidate %u: %s", i, what);
    };
    std::vector<uint32_t> srt;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t c = creator[i], s = seq[i];
        if (c >= a->V) return bad(i, "creator out of range");
        if (s == 0) return bad(i, "seq 0");
        if (poff[i + 1] < poff[i] || poff[i + 1] - poff[i] > 0xFFFFFFFFull) return bad(i, "parent offsets not monotone");
        const uint64_t p0 = poff[i], p1 = poff[i + 1];
        if (p1 > p0 && !par) return bad(i, "null parents");
        for (uint64_t p = p0; p < p1; p++)
            if (par[p] >= n_ev) return bad(i, "parent out of range");
        srt.assign(par + p0, par + p1);
        std::sort(srt.begin(), srt.end());
        if (std::adjacent_find(srt.begin(), srt.end()) != srt.end()) return bad(i, "duplicate parent");
        const uint32_t at = pg && pg->at_frame ? pg->at_frame[i] : LX_FRAME_BUILD;
        if (at == 0) return bad(i, "at_frame 0");
        const bool own_first = p1 > p0 && hm.ev_creator[par[p0]] == c;
        uint32_t br = c, spf = 0;
        if (s == 1) {
            if (own_first) return bad(i, "seq 1 with a self-parent");
            if (hm.branch_len[c]) return bad(i, "would open a new branch (the creator has events); use lx_abft_build");
            if (!pg) continue;   // no self-parent: f = 0, roots(0) is empty -> frame 1
        } else {
            if (!own_first || hm.ev_seq[par[p0]] != s - 1) return bad(i, "no self-parent of the same creator at seq - 1");
            const uint32_t sp = par[p0];
            br = hm.ev_branch[sp];
            if (hm.branch_first[br] + hm.branch_len[br] - 1 != s - 1)
                return bad(i, "would open a new branch (the self-parent is not its branch's last event); use lx_abft_build");
            spf = a->ev_frame[sp];
        }
        if ((uint64_t)t->par.size() + (p1 - p0) > 0xFFFFFFFFull) return bad(i, "too many parents");
        if (at != LX_FRAME_BUILD) t->act.push_back(BuildCand{i, spf, at, true});
        else if (s == 1) t->act.push_back(BuildCand{i, 0, 1, true});
        else t->act.push_back(BuildCand{i, spf, spf, false});
        t->br.push_back(br);
        t->seq.push_back(s);
        t->cr.push_back(c);
        t->par.insert(t->par.end(), par + p0, par + p1);
        t->poff.push_back((uint32_t)t->par.size());
        t->max_seq = std::max(t->max_seq, s);
    }
    return 0;
}

// The virtual rows: the tables go up with the first round's steps, k_build_rows
// runs ahead of them (StepSet::first).  ra must outlive the first round.
int build_plane(lx_abft *a, const IndexView &iv, const BuildTables &t, StepSet *set, BuildRowsArgs *ra) {
    hipStream_t s = iv.stream;
    const uint32_t m = (uint32_t)t.act.size();
    ARC(reserve(a, a->b_plane, (uint64_t)m * iv.stride, 0, s));
    const uint64_t o_seq = m, o_cr = 2ull * m, o_poff = 3ull * m, o_par = 4ull * m + 1;
    ARC(reserve(a, a->b_tab, o_par + t.par.size(), 0, s));
    a->up.add(a->b_tab, t.br.data(), m * 4ull);
    a->up.add(a->b_tab + o_seq, t.seq.data(), m * 4ull);
    a->up.add(a->b_tab + o_cr, t.cr.data(), m * 4ull);
    a->up.add(a->b_tab + o_poff, t.poff.data(), (m + 1) * 4ull);
    a->up.add(a->b_tab + o_par, t.par.data(), t.par.size() * 4ull);
    if (a->b_none_n < m) {
        ARC(reserve(a, a->b_none, m, 0, s));
        const std::vector<uint32_t> none(a->b_none.cap(), NONE);
        a->up.add(a->b_none, none.data(), none.size() * 4ull);
        a->b_none_n = a->b_none.cap();
    }
    BuildArgs ba{};
    ba.br = a->b_tab;
    ba.seq = a->b_tab + o_seq;
    ba.creator = a->b_tab + o_cr;
    ba.par_off = a->b_tab + o_poff;
    ba.par = a->b_tab + o_par;
    ba.ev_seq = iv.ev_seq;
    ba.cheat_of = iv.cheat_of;
    ba.cheat_off = iv.cheat_off;
    ba.cheat_br = iv.cheat_br;
    ARC(reserve(a, a->b_args, 1, 0, s));
    a->up.add(a->b_args, &ba, sizeof ba);
    set->rows = StepSet::kScratch;
    set->seq16 = t.max_seq <= 0xFFFFu;
    *ra = BuildRowsArgs{};
    ra->hb = iv.hb;
    ra->stride = iv.stride;
    ra->B = iv.B;
    ra->plane = a->b_plane;
    ra->n = m;
    ra->c = ba;
    ra->branch_first = iv.branch_first;
    for (const auto &l : *iv.by_creator) ra->n_cheat += l.size() > 1;
    set->first = ra;   // the tables, the first round's steps and candidates go up in one k_scatter launch
    return 0;
}

// The frame loop of calcFrameIdx in rounds, one wait per round: every entry
// still climbing asks q_f at its current frame, the entries of one frame are
// one step of a merged launch.  Entry k is row k of the scratch plane, or
// (pg->events) an indexed event.  pg: the numbers of the step on which an
// entry stops are reported; an entry the Build cap stopped is asked once more
// at the frame it got.
int build_rounds(lx_abft *a, const IndexView &iv, std::vector<BuildCand> &act, StepSet &set, const Progress *pg) {
    hipStream_t s = iv.stream;
    const uint32_t m = (uint32_t)act.size();
    std::vector<uint32_t> live(m);
    for (uint32_t k = 0; k < m; k++) live[k] = k;
    std::map<uint32_t, std::vector<uint32_t>> by_frame, ev_by_frame;
    std::vector<FcStep> st;
    std::vector<const std::vector<uint32_t> *> st_ent;
    while (!live.empty()) {
        by_frame.clear();
        for (uint32_t k : live) by_frame[act[k].f].push_back(k);
        if (pg && pg->events) {
            ev_by_frame.clear();
            for (uint32_t k : live) ev_by_frame[act[k].f].push_back(pg->events[act[k].pos]);
        }
        st.clear();
        st_ent.clear();
        uint64_t rows = 0, qn = 0, pn = 0;
        for (auto &kv : by_frame) {
            const uint32_t f = kv.first;
            const uint32_t R = f < a->frames.size() ? (uint32_t)a->frames[f].ev.size() : 0;
            if (!R) continue;   // no roots: no quorum, the loop stops at f
            const uint32_t words = (R + 31) / 32, nc = (uint32_t)kv.second.size();
            const uint32_t *rows_of = pg && pg->events ? ev_by_frame[f].data() : kv.second.data();
            st.push_back(FcStep{f, rows_of, nc, R, words, rows, qn, pn});
            st_ent.push_back(&kv.second);
            if (!pg) rows += (uint64_t)nc * words;
            else if (pg->pairs) pn += (uint64_t)nc * R;
            qn += nc;
        }
        if (st.empty()) {
            ARC(flush_uploads(a, s));   // nothing asks: leave no upload pending
            break;
        }
        if (pg) {
            // the records and pair stakes of the round: pinned, device-mapped, contents not kept
            AHIP(a, a->pg_pin.grow(qn, std::max<uint64_t>(qn + qn / 2, 4096), s, true));
            if (pn) AHIP(a, a->pp_pin.grow(pn, std::max<uint64_t>(pn + pn / 2, 4096), s, true));
        } else {
            ARC(reserve(a, a->b_bits, rows + 1, 0, s));
        }
        ARC(q_buffer(a, qn, s));
        ARC(launch_fc_steps(a, iv, st, set));
        set.first = nullptr;
        AHIP(a, hipStreamSynchronize(s));
        a->bstats.frame_steps += (uint32_t)st.size();
        a->bstats.rounds++;
        live.clear();
        for (size_t i = 0; i < st.size(); i++) {
            const FcStep &x = st[i];
            for (uint32_t j = 0; j < x.n_cand; j++) {
                const uint32_t k = (*st_ent[i])[j];
                BuildCand &c = act[k];
                if (a->q_pin.host()[x.qoff + j] && !c.last) {
                    c.f++;
                    if (c.f >= c.spf + kBuildCap) c.last = true;
                    if (!c.last || pg) {
                        live.push_back(k);
                        continue;
                    }
                }
                if (!pg) continue;
                const uint4 o = a->pg_pin.host()[x.qoff + j];
                if (pg->n_roots) pg->n_roots[c.pos] = x.n_roots;
                if (pg->n_caused) pg->n_caused[c.pos] = o.x;
                if (pg->stake) pg->stake[c.pos] = o.y;
                if (pg->root_stake) pg->root_stake[c.pos] = ((uint64_t)o.w << 32) | o.z;
                if (pg->pairs) {
                    const uint32_t *src = a->pp_pin.host() + x.pair0 + (uint64_t)j * x.n_roots;
                    a->pp_ent[c.pos] = lx_abft::PairEnt{a->pp_keep.size(), x.n_roots, x.frame};
                    a->pp_keep.insert(a->pp_keep.end(), src, src + x.n_roots);
                }
            }
        }
    }
    return 0;
}

// the step set of a Build-without-Add or progress call: nothing of the engine's
// state or of the last batch's stats is written, the build stats are charged
static StepSet build_set(const Progress *pg) {
    StepSet set;
    set.engine = false;
    set.out = pg ? StepSet::kProgress : StepSet::kScratchBits;
    set.pairs = pg && pg->pairs;
    return set;
}

// an entry that asks nothing reports zeros
static void zero_progress(lx_abft *a, uint32_t n, const Progress *pg) {
    if (pg->n_roots) std::fill(pg->n_roots, pg->n_roots + n, 0u);
    if (pg->n_caused) std::fill(pg->n_caused, pg->n_caused + n, 0u);
    if (pg->stake) std::fill(pg->stake, pg->stake + n, 0u);
    if (pg->root_stake) std::fill(pg->root_stake, pg->root_stake + n, (uint64_t)0);
    if (pg->pairs) a->pp_ent.assign(n, lx_abft::PairEnt{0, 0, 0});
}

int build_frames(lx_abft *a, uint32_t n, const uint32_t *creator, const uint32_t *seq, const uint64_t *poff,
                 const uint32_t *par, uint32_t *out_frame, uint8_t *out_is_root, uint32_t *err_index,
                 const Progress *pg) {
    IndexView iv;
    int rc = lx_index_peek(a->ix, &iv);
    if (rc) return a->ixfail(rc);
    IndexHostMeta hm;
    if ((rc = lx_index_host_meta(a->ix, &hm))) return a->ixfail(rc);
    const uint64_t n_ev = std::min<uint64_t>(iv.n_events, a->ev_frame.size());
    // ---- input checks (host tables only)
    BuildTables t;
    ARC(build_tables(a, hm, n_ev, n, creator, seq, poff, par, pg, err_index, &t));
    for (uint32_t i = 0; i < n; i++) {
        out_frame[i] = 1;
        if (out_is_root) out_is_root[i] = 1;
    }
    if (pg) zero_progress(a, n, pg);
    if (t.act.empty()) return 0;

    // ---- the virtual rows
    if ((rc = lx_index_view(a->ix, &iv))) return a->ixfail(rc);   // the pending small-batch run is in the planes
    if (iv.shard_count > 1 || iv.loading) return a->fail(LX_ERR_STATE, "abft needs an unsharded, loaded index");
    const uint64_t up0 = a->up.launches;
    StepSet set = build_set(pg);
    BuildRowsArgs ra;
    ARC(build_plane(a, iv, t, &set, &ra));

    // ---- the frame loop, one wait per round
    ARC(build_rounds(a, iv, t.act, set, pg));
    a->bstats.launches += (uint32_t)(a->up.launches - up0);
    for (const BuildCand &c : t.act) {
        out_frame[c.pos] = c.f;
        if (out_is_root) out_is_root[c.pos] = c.f != c.spf;
    }
    return 0;
}

// lx_abft_event_progress: indexed events at their own frame (or the frame
// asked), one step per frame, one round; the plain root-FC kernels on the
// index's HB plane.
int event_progress(lx_abft *a, uint32_t n, const uint32_t *ev, uint32_t *out_frame, uint32_t *err_index,
                   const Progress *pg) {
    IndexView iv;
    int rc = lx_index_peek(a->ix, &iv);
    if (rc) return a->ixfail(rc);
    const uint64_t n_ev = std::min<uint64_t>(iv.n_events, a->ev_frame.size());
    std::vector<BuildCand> act(n);
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t at = pg->at_frame ? pg->at_frame[i] : LX_FRAME_BUILD;
        if (ev[i] >= n_ev || at == 0) {
            if (err_index) *err_index = i;
            return a->fail(LX_ERR_ARG, "entry %u: %s", i, at == 0 ? "at_frame 0" : "event out of range");
        }
        const uint32_t f = at == LX_FRAME_BUILD ? a->ev_frame[ev[i]] : at;
        act[i] = BuildCand{i, f, f, true};
    }
    zero_progress(a, n, pg);
    for (uint32_t i = 0; i < n; i++) out_frame[i] = act[i].f;
    if ((rc = lx_index_view(a->ix, &iv))) return a->ixfail(rc);   // the pending small-batch run is in the planes
    if (iv.shard_count > 1 || iv.loading) return a->fail(LX_ERR_STATE, "abft needs an unsharded, loaded index");
    const uint64_t up0 = a->up.launches;
    StepSet set = build_set(pg);   // the plain root-FC kernels on the index's HB plane
    ARC(build_rounds(a, iv, act, set, pg));
    a->bstats.launches += (uint32_t)(a->up.launches - up0);
    return 0;
}

}  // namespace lxa
