// lx_index_layout.cpp -- the device buffers of the index handle (lx_index.h): growth and
// re-layout, the column and cheater tables, the argument builders of the walks.
#include <hip/hip_runtime.h>

#include "lx_index.h"

using namespace lxi;

// a re-layout: every buffer of the old layout goes, with the state that describes them
void free_all(lx_index *h) {
    if (h->rowseg() && h->lay.hb_mem) (void)hipStreamSynchronize(h->stream);   // the walk may still write its rows
    h->lay = Layout{};
    h->wb.ready = false;
    h->fk_hi4 = 0;
    h->sc.events = ~0ull;
    h->sc.cols_gen = 0;
    h->sx.full = true;
    h->sx.active = false;
    h->rs_gen = 0;
    h->rs_state = 0;
    h->n_cap = h->stride = h->pstride = h->s_cap = 0;
}

namespace {

// a shard's produced LowestAfter rows lap[(col * s_cap + s) * stride + j] in a
// new shape (local columns, seq capacity, branch capacity), contents kept
int relayout_lap(lx_index *h, uint32_t ncol, uint32_t nscap, uint32_t nstride) {
    DU32 n;
    const uint64_t words = (uint64_t)ncol * nscap * nstride;
    HIPCHK(h, n.renew(words));
    HIPCHK(h, hipMemsetAsync(n, 0, words * 4, h->stream));
    if (h->lay.lap) {
        const uint32_t oc = std::min(h->pstride, ncol), os = std::min(h->s_cap, nscap);
        for (uint32_t k = 0; k < oc && os; k++)
            HIPCHK(h, lx::launch_copy_rows(n + (uint64_t)k * nscap * nstride, nstride,
                                           h->lay.lap + (uint64_t)k * h->s_cap * h->stride, h->stride, os,
                                           std::min(h->stride, nstride), h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    h->lay.lap = std::move(n);
    return 0;
}

// the ordinary planes in a new row pitch: `rows` rows of `ocols` columns kept
// (none when there is no old plane), the rest zero
int repitch_planes(lx_index *h, uint32_t npitch, uint64_t rows, uint32_t ocols) {
    Layout &l = h->lay;
    for (DU32 *p : {&l.hb_mem, &l.la_mem}) {
        DU32 n;
        HIPCHK(h, n.renew(h->n_cap * npitch));
        HIPCHK(h, hipMemsetAsync(n, 0, h->n_cap * npitch * 4, h->stream));
        if (*p) HIPCHK(h, lx::launch_copy_rows(n, npitch, *p, ocols, rows, ocols, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        *p = std::move(n);
    }
    l.hb = l.hb_mem;
    l.la = l.la_mem;
    return 0;
}

}  // namespace

// per-event arrays + planes for n_cap events (copies the first `keep` events)
int grow_events(lx_index *h, uint64_t need) {
    if (need <= h->n_cap) return 0;
    Layout &l = h->lay;
    uint64_t cap = std::max<uint64_t>({need, h->n_cap + h->n_cap / 2, 4096});
    uint64_t keep = h->hwm;
    for (DU32 *a : {&l.ev_creator, &l.ev_seq, &l.ev_branch, &l.ev_bbefore, &l.ev_sp, &l.first_child})
        HIPCHK(h, a->regrow(cap, keep, Fill::none, h->stream));
    HIPCHK(h, lx::launch_fill_u32(l.first_child + keep, cap - keep, LX_NONE, h->stream));
    // (a row-segment rank allocates the planes of its own rows when it takes
    // its batch: rs_planes)
    if (!h->rowseg()) {
        for (DU32 *p : {&l.hb_mem, &l.la_mem})
            HIPCHK(h, p->regrow(cap * h->pstride, keep * h->pstride, Fill::all, h->stream));
        l.hb = l.hb_mem;
        l.la = l.la_mem;
    }
    h->n_cap = cap;
    return 0;
}

namespace {

// LowestAfter tail state sized to the branch capacity; a new table starts at
// zw = 0 (the next pass re-zeroes every unobserved tail: always correct)
int ensure_tail(lx_index *h) {
    Layout &l = h->lay;
    if (l.tail_cap() >= h->stride && l.tail_zw) return 0;
    const uint64_t t = h->stride;
    HIPCHK(h, l.tail_zw.renew(t * t, h->stream, true));
    HIPCHK(h, l.tail_lo.renew(t * t));
    HIPCHK(h, l.tail_cmin.renew(t));
    HIPCHK(h, hipMemsetAsync(l.tail_zw, 0, t * t * 4, h->stream));
    return 0;
}

}  // namespace

int la_tail(lx_index *h, hipStream_t s) {
    int rc;
    if ((rc = ensure_tail(h))) return rc;
    TailArgs t{};
    t.la = h->lay.la;
    t.hb = h->lay.hb;
    t.stride = h->pstride;
    t.brow = h->lay.brow;
    t.s_cap = h->s_cap;
    t.branch_first = h->lay.branch_first;
    t.branch_len = h->lay.branch_len;
    t.B = h->B;
    t.zw = h->lay.tail_zw;
    t.lo = h->lay.tail_lo;
    t.cmin = h->lay.tail_cmin;
    t.tcap = h->lay.tail_cap();
    HIPCHK(h, lx::launch_la_tail(t, s));
    h->tail_dirty = true;
    return 0;
}

// the tail table starts over (the next pass re-zeroes every unobserved tail)
int restart_tail(lx_index *h) {
    if (h->lay.tail_zw && h->tail_dirty)
        HIPCHK(h, hipMemsetAsync(h->lay.tail_zw, 0, (uint64_t)h->lay.tail_cap() * h->lay.tail_cap() * 4, h->stream));
    h->tail_dirty = false;
    return 0;
}

// branch capacity (= plane stride) and per-branch arrays
int grow_branches(lx_index *h, uint32_t need) {
    if (need <= h->stride) return 0;
    Layout &l = h->lay;
    uint32_t ns = round_up(std::max<uint32_t>(need, h->stride + h->stride / 4), 64);
    uint32_t os = h->stride;
    int rc;
    if (h->sharded()) {
        // planes hold local columns; the produced LowestAfter rows are B wide
        if (l.lap && (rc = relayout_lap(h, h->pstride, h->s_cap, ns))) return rc;
        DU32 nc;   // (filled with LX_NONE, not zeros: spelled out)
        HIPCHK(h, nc.renew(ns));
        HIPCHK(h, lx::launch_fill_u32(nc, ns, LX_NONE, h->stream));
        if (l.cmap)
            HIPCHK(h, hipMemcpyAsync(nc, l.cmap, std::min<uint64_t>(os, l.cmap.cap()) * 4, hipMemcpyDeviceToDevice,
                                     h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        l.cmap = std::move(nc);
    } else if (l.hb && !h->rowseg()) {   // (row-segment planes: rs_planes, at the batch)
        if ((rc = repitch_planes(h, ns, h->hwm, os))) return rc;
    }
    for (DU32 *a : {&l.branch_first, &l.branch_creator, &l.branch_len, &l.wpad, &l.col_list})
        HIPCHK(h, a->regrow(ns, os, Fill::all, h->stream));
    HIPCHK(h, l.brow.regrow((uint64_t)ns * h->s_cap, (uint64_t)os * h->s_cap, Fill::none, h->stream));
    h->stride = ns;
    if (!h->sharded()) h->pstride = ns;
    return 0;
}

int grow_scap(lx_index *h, uint32_t need) {
    if (need <= h->s_cap) return 0;
    uint32_t ns = std::max<uint32_t>({need, h->s_cap + h->s_cap / 2, 256});
    DU32 nb;
    HIPCHK(h, nb.renew((uint64_t)h->stride * ns));
    if (h->lay.brow && h->s_cap) {
        HIPCHK(h, lx::launch_copy_rows(nb, ns, h->lay.brow, h->s_cap, h->stride, h->s_cap, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    h->lay.brow = std::move(nb);
    if (h->sharded()) {
        int rc;
        if ((rc = relayout_lap(h, h->pstride, ns, h->stride))) return rc;
    }
    h->s_cap = ns;
    return 0;
}

// a shard's plane columns (own originals + own fork branches) beyond pstride
int grow_local(lx_index *h, uint32_t need) {
    if (need <= h->pstride) return 0;
    uint32_t np = round_up(std::max<uint32_t>(need, h->pstride + h->pstride / 4), 16);
    int rc;
    if ((rc = relayout_lap(h, np, h->s_cap, h->stride))) return rc;
    if ((rc = repitch_planes(h, np, h->hwm, h->pstride))) return rc;
    // (a shard has wloc from lx_reset on, so regrow waits for the stream here as the planes did)
    HIPCHK(h, h->lay.wloc.regrow(np, h->pstride, Fill::all, h->stream));
    h->pstride = np;
    return 0;
}

int ensure_batch(lx_index *h, uint64_t n, uint64_t npar) {
    Layout &l = h->lay;
    if (n > l.batch_cap) {
        uint64_t cap = std::max<uint64_t>(n, 1024);
        for (DU32 *a : {&l.b_creator, &l.b_seq, &l.b_isfork, &l.b_rank, &l.b_tmpbr, &l.b_jmp}) HIPCHK(h, a->renew(cap));
        HIPCHK(h, l.b_poff.renew(cap + 1));
        HIPCHK(h, l.b_rec.renew((cap + 63) / 64 * 64));   // whole 64-record rounds (round-blocked SoA)
        HIPCHK(h, l.b_crec.renew((cap + 63) / 64 * 64));
        size_t sb = 0;
        HIPCHK(h, lx::scan_tmp_bytes((uint32_t)cap, &sb));
        HIPCHK(h, l.scan_tmp.renew(sb));
        l.batch_cap = cap;
    }
    if (npar > l.b_par.cap()) HIPCHK(h, l.b_par.renew(std::max<uint64_t>(npar, 4096)));
    return 0;
}

// column list of this shard + cheater CSR (restricted to owned creators); runs
// whenever the branch -> creator map changed, so it starts the map's next
// generation (lx_index.h)
int rebuild_columns(lx_index *h) {
    h->branch_gen++;
    std::vector<uint32_t> cols;
    for (uint32_t b = 0; b < h->B; b++) {
        uint32_t c = h->h_branch_creator[b];
        if (c >= h->own_lo && c < h->own_hi) cols.push_back(b);
    }
    h->ncols = (uint32_t)cols.size();
    if (!cols.empty())
        HIPCHK(h, hipMemcpyAsync(h->lay.col_list, cols.data(), cols.size() * 4, hipMemcpyHostToDevice, h->stream));
    std::vector<uint32_t> off{0}, br, cr;
    for (uint32_t c = h->own_lo; c < h->own_hi; c++) {
        const auto &l = h->by_creator[c];
        if (l.size() < 2) continue;
        cr.push_back(c);
        br.insert(br.end(), l.begin(), l.end());
        off.push_back((uint32_t)br.size());
    }
    h->n_cheat = (uint32_t)cr.size();
    const std::vector<uint32_t> cr_glob = cr;   // cr becomes plane columns below (shards)
    HIPCHK(h, h->lay.cheat_of.grow(h->V));
    std::vector<int32_t> co(h->V, -1);   // alive until the sync below
    for (uint32_t k = 0; k < cr.size(); k++) co[cr[k]] = (int32_t)k;
    HIPCHK(h, hipMemcpyAsync(h->lay.cheat_of, co.data(), h->V * 4ull, hipMemcpyHostToDevice, h->stream));
    uint64_t need = std::max<uint64_t>({off.size(), br.size(), 1});
    if (need > h->lay.cheat_off.cap()) {
        uint64_t cap = std::max<uint64_t>(need * 2, 256);
        Layout &l = h->lay;
        HIPCHK(h, renew_guarded(cap, l.cheat_off, l.cheat_br, l.cheat_creator, l.cheat_brl, l.cheat_crl));
    }
    if (h->n_cheat) {
        HIPCHK(h, hipMemcpyAsync(h->lay.cheat_off, off.data(), off.size() * 4, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->lay.cheat_br, br.data(), br.size() * 4, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->lay.cheat_creator, cr.data(), cr.size() * 4, hipMemcpyHostToDevice, h->stream));
        if (h->sharded()) {
            for (auto &x : br) x = h->h_cmap[x];
            for (auto &x : cr) x = h->h_cmap[x];
        }
        HIPCHK(h, hipMemcpyAsync(h->lay.cheat_brl, br.data(), br.size() * 4, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->lay.cheat_crl, cr.data(), cr.size() * 4, hipMemcpyHostToDevice, h->stream));
    }
    // fork-path FC tables (k_fc_fk streams every plane column; <= 64 cheaters
    // per handle, beyond that the cheater fix-up loop of k_fc<.., true>)
    std::vector<uint32_t> fw, fc, wch;   // alive until the sync below
    h->fk_hi4 = 0;
    if (h->fc_fk && h->n_cheat && h->n_cheat <= kFcFkMaxCheaters) {
        const uint32_t npc = h->sharded() ? h->nloc : h->B;
        const uint64_t cap = round_up(npc, 4);
        if (cap > h->lay.fk_w.cap()) HIPCHK(h, renew_guarded(cap + cap / 2, h->lay.fk_w, h->lay.fk_c));
        HIPCHK(h, h->lay.fk_wch.grow(kFcFkMaxCheaters));
        fw.assign(cap, 0);
        fc.assign(cap, LX_NONE);
        for (uint32_t b : cols) {
            const uint32_t c = h->h_branch_creator[b];
            const uint32_t pc = h->sharded() ? h->h_cmap[b] : b;
            if (pc >= cap) return h->fail(LX_ERR_STATE, "fork FC table: plane column %u past %u", pc, npc);
            if (co[c] >= 0) fc[pc] = (uint32_t)co[c];
            else fw[pc] = b < h->V ? h->weights[c] : 0u;
        }
        wch.assign(kFcFkMaxCheaters, 0);
        for (uint32_t k = 0; k < h->n_cheat; k++) wch[k] = h->weights[cr_glob[k]];
        HIPCHK(h, hipMemcpyAsync(h->lay.fk_w, fw.data(), cap * 4, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->lay.fk_c, fc.data(), cap * 4, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->lay.fk_wch, wch.data(), wch.size() * 4, hipMemcpyHostToDevice, h->stream));
        h->fk_hi4 = (uint32_t)(cap / 4);
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

BatchArgs batch_args(lx_index *h, uint32_t n, const uint32_t *creator, const uint32_t *seq, const uint32_t *poff,
                     const uint32_t *par) {
    BatchArgs a{};
    a.n = n;
    a.batch_start = (uint32_t)h->n_events;
    a.V = h->V;
    a.B0 = h->B;
    a.creator = creator;
    a.seq = seq;
    a.poff = poff;
    a.par = par;
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
    a.isfork = h->lay.b_isfork;
    a.rank = h->lay.b_rank;
    a.tmp_br = h->lay.b_tmpbr;
    a.jmp = h->lay.b_jmp;
    a.rec = h->lay.b_rec;
    a.status = h->status;
    return a;
}

// The batch's ordinary walk (the walk plan picks the kernel and the grid,
// seg_window cuts a segment's window from it)
IndexArgs index_args(const lx_index *h, uint32_t n, const uint32_t *poff, const uint32_t *par) {
    IndexArgs ia{};
    ia.hb = h->lay.hb;
    ia.la = h->lay.la;
    ia.stride = h->pstride;
    ia.cmap = h->sharded() ? h->lay.cmap : nullptr;
    ia.lap = h->sharded() ? h->lay.lap : nullptr;
    ia.lap_stride = h->stride;
    ia.batch_start = (uint32_t)h->n_events;
    ia.n = n;
    ia.rec = h->lay.b_rec;
    ia.crec = h->b_crec_ok ? h->lay.b_crec : nullptr;
    ia.par_in = par;
    ia.poff_in = poff;
    ia.col_list = h->lay.col_list;
    ia.ncols = h->ncols;
    ia.branch_first = h->lay.branch_first;
    ia.brow = h->lay.brow;
    ia.s_cap = h->s_cap;
    ia.clk = h->d_clk;
    return ia;
}

// the LowestAfter fills of the events added since the last flush (rollback and write-back)
UnfillArgs unfill_args(lx_index *h) {
    UnfillArgs u{};
    u.hb = h->lay.hb;
    u.la = h->lay.la;
    u.stride = h->pstride;
    u.cmap = h->sharded() ? h->lay.cmap : nullptr;
    u.lap = h->sharded() ? h->lay.lap : nullptr;
    u.lap_stride = h->stride;
    u.lo = (uint32_t)h->n_flushed;
    u.hi = (uint32_t)h->n_events;
    u.B = h->B;
    u.ev_seq = h->lay.ev_seq;
    u.ev_branch = h->lay.ev_branch;
    u.ev_bbefore = h->lay.ev_bbefore;
    u.ev_sp = h->lay.ev_sp;
    u.ev_creator = h->lay.ev_creator;
    u.first_child = h->lay.first_child;
    u.first_root = h->lay.first_root;
    u.branch_len = h->lay.branch_len;
    u.branch_first = h->lay.branch_first;
    u.brow = h->lay.brow;
    u.s_cap = h->s_cap;
    u.B_keep = h->B_flushed;
    return u;
}
