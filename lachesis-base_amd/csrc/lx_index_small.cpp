// lx_index_small.cpp -- the small-batch (latency) Add path of the index handle
// (lx_index.h, lx_small.hip): the host mirror, the staging slots, the pending run.
// One translation unit: the latency leg counts these functions in microseconds.
#include <hip/hip_runtime.h>

#include <cstring>

#include "lx_index.h"

using namespace lxi;

#ifdef LX_HOST_PROF
uint64_t g_hprof[16];
extern "C" void lx_host_prof(uint64_t out[16], int reset) {
    memcpy(out, g_hprof, sizeof g_hprof);
    if (reset) memset(g_hprof, 0, sizeof g_hprof);
}
#endif

// Refresh the host mirror after batches the device assigned (big path): the
// immutable per-event fields of the events not mirrored yet, branch lengths whole.
int hm_sync(lx_index *h) {
    if (h->hm.ok) return 0;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const uint64_t n = h->n_events, lo = std::min(h->hm.n, n);
    rawvec<uint32_t> *v[] = {&h->hm.creator, &h->hm.seq, &h->hm.branch, &h->hm.bbefore};
    const uint32_t *d[] = {h->lay.ev_creator, h->lay.ev_seq, h->lay.ev_branch, h->lay.ev_bbefore};
    for (int k = 0; k < 4; k++) {
        v[k]->resize(n);
        if (n > lo) HIPCHK(h, hipMemcpy(v[k]->data() + lo, d[k] + lo, (n - lo) * 4, hipMemcpyDeviceToHost));
    }
    h->hm.blen.resize(h->B);
    HIPCHK(h, hipMemcpy(h->hm.blen.data(), h->lay.branch_len, h->B * 4ull, hipMemcpyDeviceToHost));
    h->hm.n = n;
    h->hm.ok = true;
    return 0;
}

namespace {

// pinned staging image of `words` uint32 (the slot's previous copy has finished
// reading it) and a device image at least as large.  A slot that must grow
// grows every slot to the same size at once: the slots are used in turn, and
// growing them one by one put a pinned allocation (~0.1-0.3 ms) into each of
// the next kSlots calls -- the latency leg's add1024 tail
int stage_slot(lx_index *h, uint64_t words, uint32_t **out, int *slot) {
    const int k = (int)h->st.next;
    h->st.next = (h->st.next + 1) % lx_index::kSlots;
    if (h->st.used[k]) HIPCHK(h, hipEventSynchronize(h->st.copied[k]));
    if (words > h->st.pin[k].cap() || words > h->st.dev[k].cap()) {
        const uint64_t cap = std::max<uint64_t>(words + words / 2, 16384);
        HIPCHK(h, hipStreamSynchronize(h->stream));   // every copy and kernel that read a slot
        for (int j = 0; j < lx_index::kSlots; j++) {
            HIPCHK(h, h->st.pin[j].grow(cap));
            HIPCHK(h, h->st.dev[j].grow(cap));
        }
    }
    *out = h->st.pin[k];
    *slot = k;
    return 0;
}

}  // namespace

// Launch the pending run of small-path events [pend.bs, pend.bs + pend.n): the
// staged image (records, parents, the run's topological levels, new branches,
// touched branch lengths), one k_small, then the fork marks.  Every entry point
// that reads the device state or enqueues after it calls this first.
int flush_pending(lx_index *h) {
    if (!h->pend.n) return 0;
    HP_T(f0);
    const uint32_t n = h->pend.n;
    const uint64_t bs = h->pend.bs;
    const uint32_t B0 = h->pend.B0, B = h->B;
    const uint32_t L = h->pend.maxlvl + 1, nf = B - B0;
    // branches the run touched (each once)
    h->sm.touched.clear();
    if (h->touch.mark.size() < B) h->touch.mark.resize(B, 0);
    const uint32_t tm = ++h->touch.stamp;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t br = h->pend.ev[i].q0.x;
        if (h->touch.mark[br] != tm) { h->touch.mark[br] = tm; h->sm.touched.push_back(br); }
    }
    const uint32_t n_blen = (uint32_t)h->sm.touched.size();
    // in-run parents (run positions) and "old" entries -- parents older than the
    // run, and the older previous branch event of a branch's first event in it
    // -- were split as the events were added (add_batch_small)
    const uint32_t n_pl = (uint32_t)h->pend.pl.size(), n_old = (uint32_t)h->pend.old.size(), nh = h->pend.nh;
    if (small_lds_bytes(n, nh, L, n_pl) > kSmallLds)   // add_batch_small keeps runs within it
        return h->fail(LX_ERR_STATE, "pending run exceeds the k_small LDS budget");
    // regions 16-B aligned: the kernel copies meta and the in-run list to LDS as uint4
    const uint64_t w_ev = 12ull * n, w_meta = (2ull * n + 3) & ~3ull, w_pl = ((n_pl + 7ull) & ~7ull) / 2;
    const uint64_t words = w_ev + w_meta + w_pl + 2ull * n_old + (L + 1) + 2ull * nf + 2ull * n_blen;
    uint32_t *img;
    int slot = -1, rc;
    const bool inl = words <= kSmallInline;   // small enough for the kernel arguments
    HP_T(g0);
    if (inl) img = h->sm.inl.img;
    else if ((rc = stage_slot(h, words, &img, &slot))) return rc;
    HP_ADD(12, g0);
    HP_T(g1);
    memcpy(img, h->pend.ev.data(), w_ev * 4);
    HP_ADD(13, g1);
    HP_T(g2);
    // meta in level order (counting sort; Add order inside a level), level offsets
    uint2 *meta = reinterpret_cast<uint2 *>(img + w_ev);
    uint32_t *ipl = img + w_ev + w_meta;
    uint2 *iold = reinterpret_cast<uint2 *>(ipl + w_pl);
    uint32_t *loff = reinterpret_cast<uint32_t *>(iold + n_old);
    h->sm.cnt.assign(L + 1, 0);
    for (uint32_t i = 0; i < n; i++) h->sm.cnt[h->pend.lvl[i] + 1]++;
    for (uint32_t l = 0; l < L; l++) h->sm.cnt[l + 1] += h->sm.cnt[l];
    for (uint32_t l = 0; l <= L; l++) loff[l] = h->sm.cnt[l];
    for (uint32_t i = 0; i < n; i++) meta[h->sm.cnt[h->pend.lvl[i]]++] = h->pend.meta[i];
    HP_ADD(14, g2);
    HP_T(g3);
    if (n_pl) memcpy(ipl, h->pend.pl.data(), n_pl * 2ull);
    if (n_old) memcpy(iold, h->pend.old.data(), n_old * 8ull);
    uint32_t *nfirst = loff + L + 1, *ncreator = nfirst + nf, *blen = ncreator + nf;
    for (uint32_t x = 0; x < nf; x++) {
        nfirst[x] = h->h_branch_first[B0 + x];
        ncreator[x] = h->h_branch_creator[B0 + x];
    }
    for (uint32_t x = 0; x < n_blen; x++) {
        blen[2 * x] = h->sm.touched[x];
        blen[2 * x + 1] = h->hm.blen[h->sm.touched[x]];
    }
    HP_ADD(15, g3);
    HP_ADD(4, f0);
    HP_T(f1);
    hipStream_t s = h->stream;
    if (!inl) {
        // device image `slot` is free once the kernel that read it finished
        // the copy is a kernel on this stream (a copy-engine transfer waited
        // for the previous run's kernel and then handed over to the compute
        // queue, tens of us between every two runs of a level-fed stream)
        HIPCHK(h, lx::launch_stage(h->st.dev[slot], img, words, s));
        HIPCHK(h, hipEventRecord(h->st.copied[slot], s));
    }
    SmallArgs &a = h->sm.inl.a;
    a = SmallArgs{};
    a.hb = h->lay.hb;
    a.la = h->lay.la;
    a.stride = h->pstride;
    a.bs = (uint32_t)bs;
    a.n = n;
    a.B0 = B0;
    a.B = B;
    a.img = inl ? nullptr : h->st.dev[slot];
    a.o_meta = (uint32_t)w_ev;
    a.o_pl = (uint32_t)(w_ev + w_meta);
    a.o_old = (uint32_t)(w_ev + w_meta + w_pl);
    a.o_loff = (uint32_t)(loff - img);
    a.n_pl = n_pl;
    a.n_old = n_old;
    a.n_h0 = nh;
    a.n_levels = L;
    a.o_nfirst = (uint32_t)(nfirst - img);
    a.o_ncreator = (uint32_t)(ncreator - img);
    a.o_blen = (uint32_t)(blen - img);
    a.n_blen = n_blen;
    a.ev_creator = h->lay.ev_creator;
    a.ev_seq = h->lay.ev_seq;
    a.ev_branch = h->lay.ev_branch;
    a.ev_bbefore = h->lay.ev_bbefore;
    a.ev_sp = h->lay.ev_sp;
    a.first_child = h->lay.first_child;
    a.first_root = h->lay.first_root;
    a.branch_first = h->lay.branch_first;
    a.branch_creator = h->lay.branch_creator;
    a.branch_len = h->lay.branch_len;
    a.brow = h->lay.brow;
    a.s_cap = h->s_cap;
    a.mask = B > h->V ? 1u : 0u;
    if (h->small_timing) HIPCHK(h, hipEventRecord(h->ev[1], s));
    // a deep run of few fork-free branches (per-event Adds of configs[0]: every
    // event its own level) by frontier doubling instead of level by level
    const bool dbl = h->dbl && !inl && !a.mask && B <= kDblMaxB && L >= kSmallDblLevels &&
                     small_dbl_lds_bytes(n, B, nh) <= kDblLds;
    HIPCHK(h, inl ? lx::launch_small_inline(h->sm.inl, s) : dbl ? lx::launch_small_dbl(a, s) : lx::launch_small(a, s));
    if (!inl) h->st.used[slot] = true;
    if (h->small_timing) HIPCHK(h, hipEventRecord(h->ev[2], s));
    if (B > h->V && h->n_cheat) {
        MarkArgs m{};
        m.hb = h->lay.hb;
        m.stride = h->pstride;
        m.batch_start = (uint32_t)bs;
        m.n = n;
        m.V = h->V;
        m.ev_branch = h->lay.ev_branch;
        m.ev_bbefore = h->lay.ev_bbefore;
        m.branch_first = h->lay.branch_first;
        m.n_cheat = h->n_cheat;
        m.cheat_off = h->lay.cheat_off;
        m.cheat_br = h->lay.cheat_br;
        HIPCHK(h, lx::launch_marks(m, s));
    }
    h->pend.n = 0;
    h->stats = lx_stats{};
    h->stats.index_launches = 1;
    h->stats_lazy = h->small_timing;
    HP_ADD(5, f1);
    HP_CNT(9, 1);
    return 0;
}

// The pending run is one fork-free event a: add it and fill the FC cache row
// of a against the n_slots events of evk in one k_add1_row launch (the
// unchanged caller's Add-then-ForklessCause miss; lx_fccache.cpp).  Returns 1
// (nothing enqueued) when the run is not of that shape; the caller then
// flushes and fills separately.
int flush_add1_row(lx_index *h, uint32_t a, uint32_t *evk_dev, uint32_t n_slots, uint8_t *tag_dev, uint8_t *out_dev,
                   uint32_t *psum_dev, const Add1Delta *delta) {
    if (h->pend.n != 1 || h->pend.bs != a || h->B != h->V || h->pend.B0 != h->B || h->n_cheat || h->small_timing ||
        h->sharded() || h->rowseg() || !n_slots)
        return 1;
    const SmallEv &e = h->pend.ev[0];
    // parents: all older than the run (one event), in its "old" entries
    Add1RowArgs r{};
    uint32_t np = 0;
    for (const uint2 &o : h->pend.old)
        if (!(o.x & 0x80000000u)) {
            if (np == kAdd1MaxPar) return 1;
            r.par[np++] = o.y;
        }
    if (np != e.q0.w) return 1;
    r.hb = h->lay.hb;
    r.la = h->lay.la;
    r.stride = h->pstride;
    r.a = a;
    r.e = e;
    r.blen = h->hm.blen[e.q0.x];
    r.B = h->B;
    r.w_br = h->weights[e.q0.x];
    r.ev_creator = h->lay.ev_creator;
    r.ev_seq = h->lay.ev_seq;
    r.ev_branch = h->lay.ev_branch;
    r.ev_bbefore = h->lay.ev_bbefore;
    r.ev_sp = h->lay.ev_sp;
    r.first_child = h->lay.first_child;
    r.first_root = h->lay.first_root;
    r.branch_len = h->lay.branch_len;
    r.brow = h->lay.brow;
    r.branch_first = h->lay.branch_first;
    r.s_cap = h->s_cap;
    r.evk = evk_dev;
    r.n_slots = n_slots;
    r.tag = tag_dev;
    r.out = out_dev;
    r.wpad = h->lay.wpad;
    r.quorum = h->quorum;
    r.psum = psum_dev;
    if (delta) {
        r.nd = delta->n;
        for (uint32_t i = 0; i < delta->n; i++) {
            r.d_slot[i] = delta->slot[i];
            r.d_ev[i] = delta->ev[i];
            r.d_tag[i] = delta->tag[i];
        }
    }
    HIPCHK(h, lx::launch_add1_row(r, h->stream));
    h->pend.n = 0;
    h->stats = lx_stats{};
    h->stats.index_launches = 1;
    h->stats_lazy = false;
    return 0;
}

namespace {

// A run of n events with npar parents fits one k_small workgroup's LDS (the h0
// slots are at most one per branch existing before the run, and levels <= n).
inline bool small_fits(const lx_index *h, uint64_t n, uint64_t npar) {
    return n <= kSmallMaxN && npar <= 0xFFFF &&
           small_lds_bytes(n, std::min<uint64_t>(n, h->B), n, npar + 3 * n) <= kSmallLds;
}

// Add for a batch of at most small_max events, host pointers, unsharded handle.
// Validation and branch assignment run on the host in Add order -- the
// reference's own sequential fillGlobalBranchID (vecengine/index.go:105-141:
// a root continues the creator's branch iff its lastSeq is 0, a self-parented
// event continues its self-parent's branch iff lastSeq + 1 == seq, otherwise a
// new branch) over the mirrored metadata -- with the checks and error codes of
// k_validate_claim.  The batch joins the pending run of small-path events
// (pend); the run is launched as one k_small (level by level inside the
// kernel) when it reaches kPendLaunch events, or before anything reads or
// orders after the device state (flush_pending).  Nothing waits: errors are
// known before anything is enqueued, and a DropNotFlushed of events that are
// still pending costs no device work at all.
int add_batch_small(lx_index *h, uint32_t n, const uint32_t *creator, const uint32_t *seq, const uint64_t *poff,
                    const uint32_t *par, uint32_t *out_branch, uint32_t *err_index) {
    int rc;
    if (!h->hm.ok) {
        HIPCHK(h, set_dev(h->device));
        if ((rc = hm_sync(h))) return rc;
    }
    HP_T(a0);
    const uint64_t bs = h->n_events;
    // events [0, m) have monotone parent offsets (the error at m, if any, is
    // reported after those before it, in Add order)
    uint32_t m = 0;
    while (m < n && poff[m + 1] >= poff[m]) m++;
    const uint64_t npar_b = poff[m] - poff[0];
    HP_ADD(0, a0);
    // the run launches before it would outgrow one k_small (LDS, small_fits)
    if (h->pend.n && !small_fits(h, h->pend.n + n, h->pend.npar + npar_b) &&
        ((rc = h->hip(set_dev(h->device), "set device")) || (rc = flush_pending(h))))
        return rc;
    HP_T(a1);
    if (!h->pend.n) {
        h->pend.bs = bs;
        h->pend.B0 = h->B;
        h->pend.maxlvl = 0;
        h->pend.ev.clear();
        h->pend.lvl.clear();
        h->pend.meta.clear();
        h->pend.pl.clear();
        h->pend.old.clear();
        h->pend.npar = 0;
        h->pend.nh = 0;
    }
    const uint64_t pbs = h->pend.bs;
    const uint32_t B0 = h->B, pn0 = h->pend.n, nh0 = h->pend.nh, maxlvl0 = h->pend.maxlvl;
    const size_t pl0 = h->pend.pl.size(), old0 = h->pend.old.size();
    uint32_t B = B0, bmax = 0;
    if (h->hm.creator.capacity() < bs + n) {
        // the mirror grows with the epoch: reserve for the device capacity at once
        const uint64_t c = std::max<uint64_t>(2 * (bs + n), h->n_cap);
        for (auto *v : {&h->hm.creator, &h->hm.seq, &h->hm.branch, &h->hm.bbefore}) v->reserve(c);
    }
    h->hm.creator.resize(bs + n);
    h->hm.seq.resize(bs + n);
    h->hm.branch.resize(bs + n);
    h->hm.bbefore.resize(bs + n);
    h->pend.ev.resize(pn0 + n);
    h->pend.lvl.resize(pn0 + n);
    h->pend.meta.resize(pn0 + n);
    h->sm.undo.resize(n);
    // the split lists sized for the worst case once, written through raw
    // pointers, trimmed after the loop (the per-parent push_backs of round 3's
    // first version cost a capacity check each)
    h->pend.pl.resize(pl0 + npar_b + 3ull * n);
    h->pend.old.resize(old0 + npar_b + n);
    uint16_t *const plb = h->pend.pl.data();
    uint2 *const ob = h->pend.old.data();
    uint32_t *const lvlb = h->pend.lvl.data();
    uint2 *const metab = h->pend.meta.data();
    SmallEv *const evb = h->pend.ev.data();
    uint32_t *const mc = h->hm.creator.data(), *const ms = h->hm.seq.data(), *const mb = h->hm.branch.data(),
                   *const mbb = h->hm.bbefore.data();
    uint2 *const undo = h->sm.undo.data();   // {branch, length before} per event, for a rollback
    uint32_t *blen = h->hm.blen.data(), *bfirst = h->h_branch_first.data();
    const uint32_t V = h->V;
    size_t npl = pl0, nold = old0;
    uint32_t maxlvl = maxlvl0, nh = nh0;
    int code = 0;
    bool nonmono = false;
    uint32_t bad = 0;
    HP_ADD(1, a1);
    HP_T(a2);
    // validation (the checks and error codes of k_validate_claim), branch
    // assignment and the parent split in one pass; an error rolls the batch
    // back below (nothing of it was enqueued)
    for (uint32_t i = 0; i < n; i++) {
        const uint64_t g = bs + i;
        const uint32_t c = creator[i], s = seq[i];
        if (i == m) { nonmono = true; bad = i; break; }
        const uint64_t p0 = poff[i], p1 = poff[i + 1];
        if (c >= V) { code = LX_ERR_ARG; bad = i; break; }
        if (s == 0 || s >= 0x7FFFFFFEu) { code = LX_ERR_EVENT; bad = i; break; }
        // level inside the run; parents split into in-run positions (chunks of
        // 4, padded with the event's own position) and older events (k_small)
        const uint32_t pi = pn0 + i;
        const uint32_t e_pl = (uint32_t)npl, e_old = (uint32_t)nold;
        uint32_t lvl = 0;
        for (uint64_t x = p0; x < p1; x++) {
            const uint32_t gp = par[x];
            if (gp >= g) { code = LX_ERR_ORDER; break; }
            if (gp >= pbs) {
                lvl = std::max(lvl, lvlb[gp - pbs] + 1);
                plb[npl++] = (uint16_t)(gp - pbs);
            } else {
                ob[nold++] = make_uint2(pi, gp);
            }
        }
        if (code) { bad = i; break; }
        const uint32_t sp = s > 1 ? (p1 > p0 ? par[p0] : LX_NONE) : LX_NONE;
        uint32_t br = 0;
        bool cont = false;
        if (s > 1) {
            // eventcheck: a self-parent of the same creator with seq - 1 (in the
            // mirror already, this batch's earlier events included)
            if (sp == LX_NONE || mc[sp] != c || ms[sp] + 1 != s) { code = LX_ERR_EVENT; bad = i; break; }
            const uint32_t bsp = mb[sp];
            const uint32_t len = blen[bsp];
            const uint32_t last = len ? bfirst[bsp] + len - 1 : 0;
            if (last + 1 == s) { br = bsp; cont = true; }
        } else if (blen[c] == 0) {
            br = c;
            cont = true;
        }
        const uint32_t bb = B;
        if (!cont) {
            br = B++;
            h->h_branch_first.push_back(s);
            h->h_branch_creator.push_back(c);
            h->by_creator[c].push_back(br);
            h->hm.blen.push_back(0);
            blen = h->hm.blen.data();
            bfirst = h->h_branch_first.data();
        }
        undo[i] = make_uint2(br, blen[br]);
        blen[br] = s - bfirst[br] + 1;
        mc[g] = c;
        ms[g] = s;
        mb[g] = br;
        mbb[g] = bb;
        while (npl & 3) plb[npl++] = (uint16_t)pi;
        metab[pi] = make_uint2(pi | ((uint32_t)npl - e_pl) / 4 << 16, e_pl / 4);
        const uint32_t prev = (cont && s > 1) ? sp : LX_NONE;
        uint32_t hslot = LX_NONE;
        if (prev != LX_NONE && prev < pbs) {
            hslot = nh++;
            ob[nold++] = make_uint2(0x80000000u | hslot, prev);
        }
        lvlb[pi] = lvl;
        maxlvl = std::max(maxlvl, lvl);
        bmax = std::max(bmax, s);
        SmallEv &e = evb[pi];
        e.q0 = make_uint4(br, s, prev, (uint32_t)(p1 - p0));
        e.q1 = make_uint4(e_old, bfirst[br], sp, bb);
        e.q2 = make_uint4(c, cont ? kSmallCont : 0u, LX_NONE, hslot);
        if (cont && sp != LX_NONE && sp >= pbs) evb[sp - pbs].q2.z = (uint32_t)g;
        if (out_branch) out_branch[i] = br;
    }
    HP_ADD(2, a2);
    HP_T(a3);
    // the batch rolled back: the host mirror as before it, the run without it
    auto rollback = [&](uint32_t done) {
        for (uint32_t i = done; i-- > 0;)
            if (undo[i].x < B0) h->hm.blen[undo[i].x] = undo[i].y;
        h->hm.blen.resize(B0);
        h->h_branch_first.resize(B0);
        h->h_branch_creator.resize(B0);
        for (auto &l : h->by_creator)
            while (!l.empty() && l.back() >= B0) l.pop_back();
        for (auto *v : {&h->hm.creator, &h->hm.seq, &h->hm.branch, &h->hm.bbefore}) v->resize(bs);
        h->pend.ev.resize(pn0);
        h->pend.lvl.resize(pn0);
        h->pend.meta.resize(pn0);
        h->pend.pl.resize(pl0);
        h->pend.old.resize(old0);
        h->pend.nh = nh0;
        h->pend.maxlvl = maxlvl0;
        for (uint32_t i = 0; i < pn0; i++)
            if (h->pend.ev[i].q2.z != LX_NONE && h->pend.ev[i].q2.z >= bs) h->pend.ev[i].q2.z = LX_NONE;
    };
    if (code || nonmono) {
        rollback(bad);
        if (err_index) *err_index = bad;
        if (nonmono) return h->fail(LX_ERR_ARG, "parent offsets not monotone");
        if (code == LX_ERR_ORDER) return h->fail(code, "event %u: processed out of order, parent not found", bad);
        if (code == LX_ERR_ARG) return h->fail(code, "event %u: creator idx out of range", bad);
        return h->fail(code, "event %u: violates seq/self-parent invariants (eventcheck)", bad);
    }
    h->pend.pl.resize(npl);
    h->pend.old.resize(nold);
    h->pend.nh = nh;
    h->pend.maxlvl = maxlvl;
    // capacity (rare re-layouts sync the stream; the pending run is not on the
    // device yet); on failure the host mirror and the run are rolled back
    h->max_seq = std::max(h->max_seq, bmax);
    const bool grows = bs + n > h->n_cap || B > h->stride || h->max_seq > h->s_cap;
    if (grows || B != B0 || h->ncols == 0 || h->pend.n + n >= kPendLaunch)
        if ((rc = h->hip(set_dev(h->device), "set device"))) return rc;
    if ((rc = grow_events(h, bs + n)) || (rc = grow_branches(h, B)) || (rc = grow_scap(h, h->max_seq))) {
        rollback(n);
        return rc;
    }
    h->wb.ready = false;
    h->B = B;
    h->pcols_used = std::max(h->pcols_used, B);
    if (B != B0 || h->ncols == 0)
        if ((rc = rebuild_columns(h))) return rc;
    h->n_events += n;
    h->hwm = std::max(h->hwm, h->n_events);
    h->hm.n = h->n_events;
    h->last_npar = poff[n] - poff[0];
    h->pend.npar += poff[n] - poff[0];
    h->pend.n = pn0 + n;
    HP_ADD(3, a3);
    if (h->pend.n >= kPendLaunch) return flush_pending(h);
    return 0;
}

}  // namespace

// the host-array Add: the small path when the batch fits it, else staged for the
// device path (add_batch_dev, lx_index_add.cpp)
extern "C" {

int lx_add_batch(lx_index *h, uint32_t n, const uint32_t *creator, const uint32_t *seq, const uint64_t *poff,
                 const uint32_t *par, uint32_t *out_branch, uint32_t *err_index) {
    if (!h) return LX_ERR_ARG;
    HP_T(e0);
    if (n == 0) return 0;
    if (!creator || !seq || !poff) return h->fail(LX_ERR_ARG, "null input");
    uint64_t base = poff[0], npar = poff[n] - poff[0];
    if (poff[n] < poff[0] || npar >= 0xFFFFFFFFull) return h->fail(LX_ERR_ARG, "bad parent offsets");
    if (h->loading) return h->fail(LX_ERR_STATE, "lx_add_batch during a load (lx_load_finish first)");
    // the small path makes no HIP call unless it launches or grows (it sets the device then)
    if (h->have_epoch && !h->sharded() && !h->rowseg() && n <= std::min(h->small_max, kSmallMaxN) &&
        small_fits(h, n, npar)) {
        const int rs = add_batch_small(h, n, creator, seq, poff, par, out_branch, err_index);
        HP_ADD(6, e0);
        HP_CNT(10, n);
        HP_CNT(11, 1);
        return rs;
    }
    HIPCHK(h, set_dev(h->device));
    int rc;
    if ((rc = flush_pending(h))) return rc;
    // the batch goes to the device as one pinned image {creator, seq, parent
    // offsets, parents} (16-B aligned parts) copied by k_stage into a device
    // image the walk reads in place: pageable hipMemcpyAsync of the four arrays
    // cost ~0.5 ms per 50k-event batch
    const uint64_t a4 = (n + 3ull) / 4 * 4, o4 = (n + 4ull) / 4 * 4;
    const uint64_t words = 2 * a4 + o4 + npar;
    uint32_t *img = nullptr;
    int slot = 0;
    if ((rc = stage_slot(h, words, &img, &slot))) return rc;
    memcpy(img, creator, n * 4ull);
    memcpy(img + a4, seq, n * 4ull);
    uint32_t *off = img + 2 * a4;
    for (uint32_t i = 0; i <= n; i++) {
        if (i && poff[i] < poff[i - 1]) return h->fail(LX_ERR_ARG, "parent offsets not monotone");
        off[i] = (uint32_t)(poff[i] - base);
    }
    if (npar) memcpy(img + 2 * a4 + o4, par + base, npar * 4);
    uint32_t *dimg = h->st.dev[slot];
    HIPCHK(h, lx::launch_stage(dimg, img, words, h->stream));
    HIPCHK(h, hipEventRecord(h->st.copied[slot], h->stream));
    h->st.used[slot] = true;
    uint64_t start = h->n_events;
    if ((rc = add_batch_dev(h, n, dimg, dimg + a4, dimg + 2 * a4, dimg + 2 * a4 + o4, err_index))) return rc;
    if (out_branch) HIPCHK(h, hipMemcpy(out_branch, h->lay.ev_branch + start, n * 4ull, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
