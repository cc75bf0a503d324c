// lx_index_add.cpp -- the big Add path of the index handle (lx_index.h): batch
// preparation on the device, the walk the plan picks, the segmented walk.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "lx_index.h"

using namespace lxi;

namespace {

// LX_PROF=1 in a make WPROF=1 build: the walker's per-wave counters of one
// batch (IndexArgs::prof), summed up on stderr
void print_walker_prof(uint32_t n, const std::vector<unsigned long long> &pv) {
    // summary over workgroups: compute waves (lane sums), loader, drains
    double sum[kProfWaves * kProfSlots] = {0};
    uint32_t nb = 0;
    for (uint32_t b = 0; b < (uint32_t)kProfBlocks; b++) {
        const unsigned long long *pb = pv.data() + (size_t)b * kProfWaves * kProfSlots;
        if (!pb[9]) continue;
        nb++;
        for (int i = 0; i < kProfWaves * kProfSlots; i++) sum[i] += (double)pb[i];
    }
    fprintf(stderr, "[lx_prof] n=%u blocks=%u (means per block)\n", n, nb);
    {
        // the slowest workgroups: wall (max over its waves) and the compute waves' no-record passes
        std::vector<std::pair<double, uint32_t>> wb;
        for (uint32_t b = 0; b < (uint32_t)kProfBlocks; b++) {
            const unsigned long long *pb = pv.data() + (size_t)b * kProfWaves * kProfSlots;
            double wmax = 0;
            for (int w = 0; w < kProfWaves; w++) wmax = std::max(wmax, (double)pb[w * kProfSlots + 9]);
            if (wmax > 0) wb.push_back({wmax, b});
        }
        std::sort(wb.rbegin(), wb.rend());
        for (size_t i = 0; i < wb.size() && i < 6; i++) {
            const unsigned long long *pb = pv.data() + (size_t)wb[i].second * kProfWaves * kProfSlots;
            double norec = 0;
            for (int w = 0; w < kProfWaves; w++)
                if (pb[w * kProfSlots + 10] == 0) norec += (double)pb[w * kProfSlots + 7];
            fprintf(stderr, "[lx_prof] slow block %u (xcd %u): wall_us=%.0f compute norec=%.0f\n", wb[i].second,
                    wb[i].second % 8, wb[i].first / 100.0, norec);
        }
        if (!wb.empty())
            fprintf(stderr, "[lx_prof] median block wall_us=%.0f\n", wb[wb.size() / 2].first / 100.0);
    }
    for (int w = 0; w < kProfWaves; w++) {
        const double *q = sum + w * kProfSlots;
        if (!q[9]) continue;
        const double role = q[10] / (nb ? nb : 1);
        if (role > 1.5) {
            fprintf(stderr, "[lx_prof] wave %d drain: wall_us=%.0f rounds=%.0f spin=%.0f busy_us=%.0f fills=%.0f brc_miss=%.0f\n",
                    w, q[9] / nb / 100.0, q[3] / nb, q[0] / nb, q[6] / nb / 100.0, q[4] / nb, q[5] / nb);
        } else if (role > 0.5) {
            fprintf(stderr, "[lx_prof] wave %d loader: wall_us=%.0f rounds=%.0f iter=%.0f slot_wait=%.0f sleeps=%.0f\n", w,
                    q[9] / nb / 100.0, q[3] / nb, q[0] / nb, q[1] / nb, q[2] / nb);
        } else {
            fprintf(stderr, "[lx_prof] wave %d: wall_us=%.0f wave_passes=%.0f lane: pass=%.0f spin=%.0f chunk=%.0f done=%.0f slow=%.0f fill=%.0f wm=%.0f norec=%.0f  ns/pass=%.1f\n",
                    w, q[9] / nb / 100.0, q[8] / nb, q[0] / nb, q[1] / nb, q[2] / nb, q[3] / nb, q[4] / nb, q[5] / nb, q[6] / nb,
                    q[7] / nb, q[9] * 10.0 / (q[8] > 0 ? q[8] : 1));
            if (q[14] == 0 && q[15] > 0)
                fprintf(stderr, "[lx_prof] wave %d blocks ahead of the fetched one: landed records %.1f, issued %.1f; behind it: drained %.1f\n",
                        w, q[11] / q[15], q[12] / q[15], q[13] / q[15]);
            if (q[14] > 0)
                fprintf(stderr, "[lx_prof] wave %d cycles/pass: fetch=%.0f (record rt %.0f) fold=%.0f (ring rt %.0f) ovf=%.0f complete=%.0f total=%.0f\n", w,
                        q[10] / q[8], q[5] / q[8], q[11] / q[8], q[15] / q[8], q[12] / q[8], q[13] / q[8], q[14] / q[8]);
        }
    }
}

// The batch walked as the plan's G Add-order segments, the partial events'
// rows gathered, LowestAfter filled from the final rows (lx_segment.hip,
// DESIGN.md section 6b).  `ia` is the batch's ordinary walk; timings into
// seg_stats.
int seg_walk(lx_index *h, IndexArgs ia, const WalkPlan &plan, hipStream_t s) {
    const uint32_t n = ia.n, bs = ia.batch_start, G = plan.G;
    SegArgs a{};
    a.hb = h->lay.hb;
    a.la = h->lay.la;
    a.stride = h->pstride;
    a.B = h->B;
    a.bs = bs;
    a.n = n;
    a.G = G;
    for (uint32_t k = 0; k < G; k++) a.seg_lo[k] = bs + (uint32_t)((uint64_t)n * k / G / 64 * 64);
    a.seg_lo[G] = bs + n;
    a.ev_branch = h->lay.ev_branch;
    a.ev_seq = h->lay.ev_seq;
    a.branch_first = h->lay.branch_first;
    a.branch_len = h->lay.branch_len;
    a.brow = h->lay.brow;
    a.s_cap = h->s_cap;
    a.own_seg = LX_NONE;
    a.per_rank = 1;
    int rc;
    if ((rc = grow_scratch(h, h->lay.seg_jt, (uint64_t)(G + 1) * h->B)) ||
        (rc = grow_scratch(h, h->lay.seg_cnt, (uint64_t)h->B + 2 * kMaxSegments)) ||
        (rc = grow_scratch(h, h->lay.seg_mf, (uint64_t)n)) ||
        (rc = grow_scratch(h, h->lay.seg_plist, (uint64_t)n)) ||
        (rc = grow_scratch(h, h->lay.seg_elist, (uint64_t)n)))
        return rc;
    a.jt = h->lay.seg_jt;
    a.cnt = h->lay.seg_cnt;
    a.pcount = h->lay.seg_cnt + h->B;
    a.pflag = h->lay.seg_mf;
    a.plist = h->lay.seg_plist;
    a.elist = h->lay.seg_elist;
    a.ecount = a.pcount + G;
    if ((rc = seg_events(h, 2 * G + 3))) return rc;
    const Event *ev = h->seg_ev.data();
    HIPCHK(h, lx::launch_seg_tables(a, s));
    // one launch for all G when they fit the CUs side by side (k_index_segs),
    // otherwise one walk after the other
    const bool conc = plan.one_launch;
    ia.seg = 1;
    ia.ev_branch = h->lay.ev_branch;
    ia.ev_seq = h->lay.ev_seq;
    ia.seg_j = a.jt;
    ia.seg_flag = a.pflag;
    ia.seg_list = a.plist;
    ia.seg_count = a.pcount;
    if (conc) {
        IndexArgs sk = ia;
        sk.seg_g = G;
        sk.seg_B = a.B;
        for (uint32_t k = 0; k <= G; k++) sk.seg_lo[k] = a.seg_lo[k];
        HIPCHK(h, hipEventRecord(ev[0], s));
        HIPCHK(h, lx::launch_index(sk, plan, s));
        for (uint32_t k = 0; k < G; k++) HIPCHK(h, hipEventRecord(ev[2 * k + 1], s));
    }
    for (uint32_t k = 0; k < G && !conc; k++) {
        HIPCHK(h, hipEventRecord(ev[2 * k], s));
        HIPCHK(h, lx::launch_index(seg_window(ia, k, a.seg_lo[k], a.seg_lo[k + 1], a.B), plan, s));
        HIPCHK(h, hipEventRecord(ev[2 * k + 1], s));
    }
    uint32_t pc[kMaxSegments], ec[kMaxSegments];
    HIPCHK(h, hipMemcpyAsync(pc, a.pcount, G * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    for (uint32_t k = 0; k < G; k++) HIPCHK(h, lx::launch_seg_partial(a, k, pc[k], s));
    HIPCHK(h, hipEventRecord(ev[2 * G], s));
    for (uint32_t k = 0; k < G; k++) HIPCHK(h, lx::launch_seg_edges(a, k, pc[k], s));
    HIPCHK(h, hipMemcpyAsync(ec, a.ecount, G * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    for (uint32_t k = 0; k < G; k++) HIPCHK(h, lx::launch_seg_la_edge(a, k, ec[k], s));
    HIPCHK(h, hipEventRecord(ev[2 * G + 1], s));
    HIPCHK(h, hipStreamSynchronize(s));
    lx_seg_stats &st = h->seg_stats;
    st = lx_seg_stats{};
    st.segments = G;
    st.one_launch = conc ? 1u : 0u;
    for (uint32_t k = 0; k < G; k++) {
        st.first_event[k] = a.seg_lo[k];
        st.partial[k] = pc[k];
        HIPCHK(h, hipEventElapsedTime(&st.walk_ms[k], ev[conc ? 0 : 2 * k], ev[2 * k + 1]));
    }
    st.first_event[G] = a.seg_lo[G];
    HIPCHK(h, hipEventElapsedTime(&st.partial_ms, ev[2 * G - 1], ev[2 * G]));
    HIPCHK(h, hipEventElapsedTime(&st.la_ms, ev[2 * G], ev[2 * G + 1]));
    return 0;
}

}  // namespace

// Add of a batch whose arrays are on the device (lx_add_batch_dev, and lx_add_batch's staged image)
int add_batch_dev(lx_index *h, uint32_t n, const uint32_t *creator, const uint32_t *seq, const uint32_t *poff,
                  const uint32_t *par, uint32_t *err_index) {
    if (!h->have_epoch) return h->fail(LX_ERR_STATE, "lx_add_batch before lx_reset");
    if (h->loading) return h->fail(LX_ERR_STATE, "lx_add_batch during a load (lx_load_finish first)");
    if (n == 0) return 0;
    if (h->rowseg()) {
        if (h->n_events || h->rs_state) return h->fail(LX_ERR_STATE, "a row-segment rank takes one batch per epoch");
        if (h->rs_rank >= h->rs_count) return h->fail(LX_ERR_ARG, "seg_rank %u >= seg_count %u", h->rs_rank, h->rs_count);
        if (n < 64ull * h->rs_count) return h->fail(LX_ERR_ARG, "row segments need >= 64 events per rank");
    }
    h->wb.ready = false;
    if (h->n_events + n >= 0xFFFFFFF0ull) return h->fail(LX_ERR_ARG, "too many events in one epoch");
    h->hm.ok = false;           // the device assigns this batch: the host mirror is refreshed on demand
    h->stats_lazy = false;
    int rc;
    if ((rc = grow_events(h, h->n_events + n))) return rc;
    if ((rc = ensure_batch(h, n, 0))) return rc;
    hipStream_t s = h->stream;

    HIPCHK(h, hipEventRecord(h->ev[0], s));
    HIPCHK(h, hipMemsetAsync(h->status, 0, kStatusWords * 4, s));
    HIPCHK(h, hipMemsetAsync(h->status + 8, 0xFF, 8, s));
    BatchArgs a = batch_args(h, n, creator, seq, poff, par);
    HIPCHK(h, lx::launch_batch_prepare(a, h->lay.scan_tmp, h->lay.scan_tmp.cap(), s));
    uint32_t st[16];
    uint32_t nforks = 0;
    HIPCHK(h, hipMemcpyAsync(st, h->status, sizeof st, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(&nforks, h->lay.b_rank + (n - 1), 4, hipMemcpyDeviceToHost, s));
    uint32_t npar32 = 0;
    HIPCHK(h, hipMemcpyAsync(&npar32, poff + n, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    uint64_t e64;
    memcpy(&e64, st + 8, 8);
    if (e64 != ~0ull) {
        HIPCHK(h, lx::launch_undo_claims(a, s));
        HIPCHK(h, hipStreamSynchronize(s));
        uint32_t pos = (uint32_t)(e64 >> 8), code = (uint32_t)(e64 & 0xFF);
        if (err_index) *err_index = pos;
        if (code == 2) return h->fail(LX_ERR_ORDER, "event %u: processed out of order, parent not found", pos);
        if (code == 1) return h->fail(LX_ERR_ARG, "event %u: creator idx out of range", pos);
        return h->fail(LX_ERR_EVENT, "event %u: violates seq/self-parent invariants (eventcheck)", pos);
    }
    uint32_t bmax = st[2];
    h->last_npar = npar32;
    uint32_t B_new = h->B + nforks;
    if ((rc = grow_branches(h, B_new))) return rc;
    h->max_seq = std::max(h->max_seq, bmax);
    if ((rc = grow_scap(h, h->max_seq))) return rc;
    a = batch_args(h, n, creator, seq, poff, par);   // pointers may have moved
    a.nofork = (nforks == 0 && B_new == h->V) ? 1u : 0u;
    // compact records for the 8- / 12-column walks: fork-free epoch, every
    // branch and seq within 16 bits (the packed-slot condition)
    WalkEpoch we = h->walk_epoch();
    we.B = B_new;
    h->b_crec_ok = walk_crec_ok(we, h->crec_opt);
    a.crec = h->b_crec_ok ? h->lay.b_crec : nullptr;
    // pointer jumping along in-batch self-parent chains: a chain has at most
    // min(n, max seq) events, ceil(log2) + 1 rounds resolve it (k_finalize flags
    // an unresolved event, checked below); none without forks
    uint32_t rounds = 1;
    while (rounds < 32 && (1ull << (rounds - 1)) < std::min<uint64_t>(n, bmax)) rounds++;
    HIPCHK(h, lx::launch_batch_finish(a, a.nofork ? 0u : rounds + 1, s));
    if (nforks) {
        std::vector<uint32_t> cr(nforks), fs(nforks);
        HIPCHK(h, hipMemcpyAsync(cr.data(), h->lay.branch_creator + h->B, nforks * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipMemcpyAsync(fs.data(), h->lay.branch_first + h->B, nforks * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipStreamSynchronize(s));
        for (uint32_t i = 0; i < nforks; i++) {
            h->h_branch_creator.push_back(cr[i]);
            h->h_branch_first.push_back(fs[i]);
            h->by_creator[cr[i]].push_back(h->B + i);
            if (h->sharded())
                h->h_cmap.push_back(cr[i] >= h->own_lo && cr[i] < h->own_hi ? h->nloc++ : LX_NONE);
        }
        if (h->sharded()) {
            if ((rc = grow_local(h, h->nloc))) return rc;
            HIPCHK(h, hipMemcpyAsync(h->lay.cmap + h->B, h->h_cmap.data() + h->B, nforks * 4ull, hipMemcpyHostToDevice, s));
        }
    }
    h->B = B_new;
    h->pcols_used = std::max(h->pcols_used, h->sharded() ? h->nloc : h->B);
    if (nforks || h->ncols == 0)
        if ((rc = rebuild_columns(h))) return rc;

    const size_t prof_n = (size_t)kProfBlocks * kProfWaves * kProfSlots;
    if (!h->d_clk) {
        HIPCHK(h, h->d_clk.renew(1 + 3ull * kClkBlocks));
        HIPCHK(h, hipMemsetAsync(h->d_clk, 0, (1 + 3ull * kClkBlocks) * 8, s));
    }
    IndexArgs ia = index_args(h, n, poff, par);
    const WalkPlan plan = walk_plan(h->walk_epoch(), n);   // (a row-segment rank makes its own, rs_begin)
    DevBuf<unsigned long long> d_prof;
    if (h->prof) {
        HIPCHK(h, d_prof.renew(prof_n));
        ia.prof = d_prof;
        HIPCHK(h, hipMemsetAsync(ia.prof, 0, prof_n * 8, s));
    }
    HIPCHK(h, hipEventRecord(h->ev[1], s));
    if (h->rowseg()) {
        if ((rc = rs_planes(h, n))) return rc;   // own rows only (+ the virtual bases)
        ia.hb = h->lay.hb;
        ia.la = h->lay.la;
        if ((rc = rs_begin(h, ia, s))) return rc;
    } else if (plan.G && h->segments > 1) {   // option segments
        if ((rc = seg_walk(h, ia, plan, s))) return rc;
    } else if (h->dbl && h->B <= h->V && !h->sharded() && h->B <= kDblMaxB && n >= 16ull * h->B && n <= 0xFFFFu &&
               dbl_lds_bytes(n, h->B) <= kDblLds) {
        // few branches, no forks: HB by frontier doubling in one workgroup
        // (the walker's time is levels x pass, and such epochs are deep chains)
        DblArgs da{};
        da.hb = h->lay.hb;
        da.la = h->lay.la;
        da.stride = h->pstride;
        da.bs = (uint32_t)h->n_events;
        da.n = n;
        da.B = h->B;
        da.rec = h->lay.b_rec;
        da.par = par;
        da.poff = poff;
        da.ev_branch = h->lay.ev_branch;
        da.ev_seq = h->lay.ev_seq;
        da.branch_first = h->lay.branch_first;
        da.brow = h->lay.brow;
        da.s_cap = h->s_cap;
        HIPCHK(h, lx::launch_dbl(da, s));
    } else if (plan.G) {   // side-by-side segments worth it (walk_seg_pick)
        if ((rc = seg_walk(h, ia, plan, s))) return rc;
    } else {
        HIPCHK(h, lx::launch_index(ia, plan, s));
    }
    HIPCHK(h, hipEventRecord(h->ev[2], s));
    if (h->prof) {
        std::vector<unsigned long long> pv(prof_n);
        HIPCHK(h, hipMemcpyAsync(pv.data(), ia.prof, prof_n * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipStreamSynchronize(s));
        print_walker_prof(n, pv);
    }
    if (h->B > h->V && h->n_cheat && !h->rowseg()) {   // a row-segment rank marks its rows at lx_rowseg_finish
        MarkArgs m{};
        m.hb = h->lay.hb;
        m.stride = h->pstride;
        m.cmap = h->sharded() ? h->lay.cmap : nullptr;
        m.batch_start = (uint32_t)h->n_events;
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
    if (!h->sharded() && !h->rowseg() && h->la_tail) {
        if ((rc = la_tail(h, s))) return rc;
    }
    HIPCHK(h, hipEventRecord(h->ev[3], s));
    h->n_events += n;
    h->hwm = std::max(h->hwm, h->n_events);
    HIPCHK(h, hipStreamSynchronize(s));
    uint32_t unresolved = 0;
    HIPCHK(h, hipMemcpy(&unresolved, h->status + 4, 4, hipMemcpyDeviceToHost));
    if (unresolved) return h->fail(LX_ERR_STATE, "branch assignment left %u events unresolved", unresolved);
    float t0 = 0, t1 = 0, t2 = 0;
    HIPCHK(h, hipEventElapsedTime(&t0, h->ev[0], h->ev[1]));
    HIPCHK(h, hipEventElapsedTime(&t1, h->ev[1], h->ev[2]));
    HIPCHK(h, hipEventElapsedTime(&t2, h->ev[2], h->ev[3]));
    h->stats.ms_assign = t0;
    h->stats.ms_index = t1;
    h->stats.ms_marks = t2;
    h->stats.index_launches = 1;
    return 0;
}

extern "C" {

int lx_add_batch_dev(lx_index *h, uint32_t n, const uint32_t *creator, const uint32_t *seq, const uint32_t *poff,
                     const uint32_t *par, uint32_t *err_index) {
    if (!h) return LX_ERR_ARG;
    HIPCHK(h, set_dev(h->device));
    {
        const int rc = flush_pending(h);
        if (rc) return rc;
    }
    return add_batch_dev(h, n, creator, seq, poff, par, err_index);
}

}  // extern "C"
