// lx_index_persist.cpp -- write-back of the index handle (lx_index.h) and the two-step load
// from the persisted tables (the RLP of BranchesInfo: lx_rlp.h).
#include <hip/hip_runtime.h>

#include <cstring>

#include "lx_index.h"
#include "lx_rlp.h"

using namespace lxi;

namespace {

// ---- write-back helpers
int ensure_wb(lx_index *h, uint64_t n) {
    if (n <= h->lay.wb_flag.cap() && h->lay.wb_flag) return 0;
    Layout &l = h->lay;
    h->wb.ready = false;
    l.wb_flag.reset();   // (the capacity the check above reads: set last; wb_buf stays)
    const uint64_t cap = std::max<uint64_t>(n, 4096);
    for (DU32 *b : {&l.wb_pos, &l.wb_la_rows, &l.wb_hb_rows}) HIPCHK(h, b->renew(cap));
    for (auto *b : {&l.wb_len, &l.wb_la_off, &l.wb_hb_off}) HIPCHK(h, b->renew(cap + 1));
    size_t tb = 0;
    HIPCHK(h, lx::persist_tmp_bytes((uint32_t)cap, &tb));
    HIPCHK(h, l.wb_tmp.renew(tb));
    HIPCHK(h, l.wb_flag.renew(cap));
    return 0;
}

RowsArgs rows_args(lx_index *h, uint32_t hb, const uint32_t *rows, uint32_t n) {
    RowsArgs a{};
    a.plane = hb ? h->lay.hb : h->lay.la;
    a.stride = h->stride;
    a.rows = rows;
    a.n = n;
    a.B = h->B;
    a.ev_bbefore = h->lay.ev_bbefore;
    a.ev_branch = h->lay.ev_branch;
    a.branch_first = h->lay.branch_first;
    a.hb = hb;
    return a;
}

// encoded rows -> host, in chunks of at most kWbChunk bytes of device staging
constexpr uint64_t kWbChunk = 256ull << 20;

int rows_to_host(lx_index *h, uint32_t hb, const uint32_t *rows, const uint64_t *off_dev, uint32_t n,
                 uint64_t *off_host, uint8_t *bytes) {
    std::vector<uint64_t> off(n + 1);
    HIPCHK(h, hipMemcpyAsync(off.data(), off_dev, (n + 1) * 8ull, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (off_host) memcpy(off_host, off.data(), (n + 1) * 8ull);
    if (!bytes || !n || !off[n]) return 0;
    uint64_t row_max = 0;
    for (uint32_t i = 0; i < n; i++) row_max = std::max(row_max, off[i + 1] - off[i]);
    const uint64_t want = std::max(std::min(off[n], kWbChunk), row_max);
    if (want > h->lay.wb_buf.bytes()) HIPCHK(h, h->lay.wb_buf.renew((want + 3) / 4));
    for (uint32_t i0 = 0; i0 < n;) {
        uint32_t i1 = i0 + 1;
        while (i1 < n && off[i1 + 1] - off[i0] <= h->lay.wb_buf.bytes()) i1++;
        RowsArgs a = rows_args(h, hb, rows + i0, i1 - i0);
        HIPCHK(h, lx::launch_encode_rows(a, off_dev + i0, off[i0], h->lay.wb_buf, h->stream));
        HIPCHK(h, hipMemcpyAsync(bytes + off[i0], h->lay.wb_buf, off[i1] - off[i0], hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        i0 = i1;
    }
    return 0;
}

int branches_info_rlp(lx_index *h, std::string *out) {
    std::vector<uint32_t> len(h->B);
    HIPCHK(h, hipMemcpyAsync(len.data(), h->lay.branch_len, h->B * 4ull, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (uint32_t b = 0; b < h->B; b++) len[b] = len[b] ? h->h_branch_first[b] + len[b] - 1 : 0;   // BranchIDLastSeq
    *out = encode_branches_info(len, h->h_branch_creator, h->by_creator);
    return 0;
}

static int load_fail(lx_index *h, const char *fmt, uint64_t a = 0, uint64_t b = 0) {
    char buf[256];
    snprintf(buf, sizeof buf, fmt, (unsigned long long)a, (unsigned long long)b);
    h->loading = false;
    h->have_epoch = false;   // the handle needs lx_reset
    return h->fail(LX_ERR_STATE, "inconsistent DB: %s", buf);
}

}  // namespace

extern "C" {

int lx_writeback_prepare(lx_index *h, lx_writeback *out) {
    if (!h || !out) return LX_ERR_ARG;
    WHOLE_INDEX(h);
    if (!h->have_epoch) return h->fail(LX_ERR_STATE, "write-back before lx_reset");
    NOT_LOADING(h);
    {
        const int rc = flush_pending(h);
        if (rc) return rc;
    }
    if (h->shard_count > 1) return h->fail(LX_ERR_STATE, "write-back needs an unsharded handle (shards hold partial rows)");
    HIPCHK(h, set_dev(h->device));
    h->wb.ready = false;
    const uint32_t N = (uint32_t)h->n_events, lo = (uint32_t)h->n_flushed;
    int rc;
    if ((rc = ensure_wb(h, N))) return rc;
    hipStream_t s = h->stream;
    uint32_t n_la = 0;
    if (N > lo) {
        HIPCHK(h, hipMemsetAsync(h->lay.wb_flag, 0, N * 4ull, s));
        HIPCHK(h, lx::launch_dirty_la(unfill_args(h), h->lay.wb_flag, s));
        HIPCHK(h, lx::launch_compact(h->lay.wb_flag, h->lay.wb_pos, N, h->lay.wb_tmp, h->lay.wb_tmp.cap(),
                                     h->lay.wb_la_rows, s));
        HIPCHK(h, hipMemcpyAsync(&n_la, h->lay.wb_pos + (N - 1), 4, hipMemcpyDeviceToHost, s));
        HIPCHK(h, lx::launch_iota(h->lay.wb_hb_rows, lo, N - lo, s));
        HIPCHK(h, hipStreamSynchronize(s));
    }
    // byte offsets of both row sets (wb_len is scratch, reused in stream order)
    HIPCHK(h, lx::launch_row_offsets(rows_args(h, 0, h->lay.wb_la_rows, n_la), h->lay.wb_len, h->lay.wb_la_off,
                                     h->lay.wb_tmp, h->lay.wb_tmp.cap(), s));
    HIPCHK(h, lx::launch_row_offsets(rows_args(h, 1, h->lay.wb_hb_rows, N - lo), h->lay.wb_len, h->lay.wb_hb_off,
                                     h->lay.wb_tmp, h->lay.wb_tmp.cap(), s));
    uint64_t tot[2] = {0, 0};
    HIPCHK(h, hipMemcpyAsync(&tot[0], h->lay.wb_la_off + n_la, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(&tot[1], h->lay.wb_hb_off + (N - lo), 8, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    if ((rc = branches_info_rlp(h, &h->wb.bi))) return rc;
    lx_writeback w{};
    w.first_event = lo;
    w.n_events = N - lo;
    w.n_la_rows = n_la;
    w.hb_bytes = tot[1];
    w.la_bytes = tot[0];
    w.bi_bytes = (uint32_t)h->wb.bi.size();
    h->wb.desc = w;
    h->wb.ready = true;
    *out = w;
    return 0;
}

int lx_writeback_fetch(lx_index *h, uint64_t *hb_off, uint8_t *hb_bytes, uint32_t *la_ev, uint64_t *la_off,
                       uint8_t *la_bytes, uint8_t *branch_be, uint8_t *bi_rlp) {
    if (!h) return LX_ERR_ARG;
    if (!h->wb.ready) return h->fail(LX_ERR_STATE, "lx_writeback_fetch without a current lx_writeback_prepare");
    HIPCHK(h, set_dev(h->device));
    const lx_writeback &w = h->wb.desc;
    const uint32_t n = (uint32_t)w.n_events, m = (uint32_t)w.n_la_rows;
    int rc;
    if ((hb_off || hb_bytes) && (rc = rows_to_host(h, 1, h->lay.wb_hb_rows, h->lay.wb_hb_off, n, hb_off,
                                                   hb_bytes))) return rc;
    if (la_ev && m) {
        HIPCHK(h, hipMemcpyAsync(la_ev, h->lay.wb_la_rows, m * 4ull, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    if ((la_off || la_bytes) && (rc = rows_to_host(h, 0, h->lay.wb_la_rows, h->lay.wb_la_off, m, la_off,
                                                   la_bytes))) return rc;
    if (branch_be && n) {
        std::vector<uint32_t> br(n);
        HIPCHK(h, hipMemcpyAsync(br.data(), h->lay.ev_branch + w.first_event, n * 4ull, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        for (uint32_t i = 0; i < n; i++)
            for (int k = 0; k < 4; k++) branch_be[4 * i + k] = (uint8_t)(br[i] >> (24 - 8 * k));
    }
    if (bi_rlp) memcpy(bi_rlp, h->wb.bi.data(), h->wb.bi.size());
    return 0;
}

// ---- restart from the persisted tables (abft/restart_test.go:156-188)

int lx_load_rows(lx_index *h, uint32_t n, const uint32_t *creator, const uint32_t *seq, const uint64_t *poff,
                 const uint32_t *par, const uint8_t *branch_be, const uint64_t *hb_off, const uint8_t *hb_bytes,
                 const uint64_t *la_off, const uint8_t *la_bytes) {
    if (!h) return LX_ERR_ARG;
    WHOLE_INDEX(h);
    if (!h->have_epoch) return h->fail(LX_ERR_STATE, "lx_load_rows before lx_reset");
    if (h->sharded()) return h->fail(LX_ERR_STATE, "lx_load_rows needs an unsharded handle");
    if (!n) return 0;
    if (!creator || !seq || !poff || !branch_be || !hb_off || !hb_bytes || !la_off || !la_bytes)
        return h->fail(LX_ERR_ARG, "null input");
    if (!h->loading) {
        if (h->n_events) return h->fail(LX_ERR_STATE, "lx_load_rows needs a freshly reset handle");
        h->loading = true;
        h->rolled_epoch();   // what a handle keyed on dense indices held is not of this load
        h->ld.first.assign(h->V, 1);
        h->ld.last.assign(h->V, 0);
        h->ld.count.assign(h->V, 0);
        h->ld.tail.assign(h->V, LX_NONE);
        h->ld.creator.resize(h->V);
        for (uint32_t c = 0; c < h->V; c++) h->ld.creator[c] = c;
        h->ld.par.clear();
        h->ld.poff.assign(1, 0);
        h->ld.B = h->V;
    }
    HIPCHK(h, set_dev(h->device));
    const uint64_t bs = h->n_events;
    uint32_t max_hent = 0, max_lent = 0, bmax = h->max_seq;
    for (uint32_t i = 0; i < n; i++) {
        const uint64_t g = bs + i;
        const uint32_t c = creator[i], s = seq[i];
        const uint64_t p0 = poff[i], p1 = poff[i + 1];
        const uint32_t br = ((uint32_t)branch_be[4 * i] << 24) | ((uint32_t)branch_be[4 * i + 1] << 16) |
                            ((uint32_t)branch_be[4 * i + 2] << 8) | branch_be[4 * i + 3];
        if (c >= h->V || s == 0 || s >= 0x7FFFFFFEu || p1 < p0) return load_fail(h, "event %llu: bad creator/seq", g);
        for (uint64_t x = p0; x < p1; x++)
            if (par[x] >= g) return load_fail(h, "event %llu: parent %llu not loaded before it", g, par[x]);
        const uint32_t sp = s > 1 ? (p1 > p0 ? par[p0] : LX_NONE) : LX_NONE;
        if (s > 1 && (sp == LX_NONE || h->hm.creator[sp] != c || h->hm.seq[sp] + 1 != s))
            return load_fail(h, "event %llu: self-parent", g);
        if (br < h->V && br != c) return load_fail(h, "event %llu: branch %llu of another creator", g, br);
        if (br >= (1u << 24)) return load_fail(h, "event %llu: branch ID %llu", g, br);
        if (br >= h->ld.first.size()) {
            h->ld.first.resize(br + 1, 0);
            h->ld.last.resize(br + 1, 0);
            h->ld.count.resize(br + 1, 0);
            h->ld.tail.resize(br + 1, LX_NONE);
            h->ld.creator.resize(br + 1, LX_NONE);
        }
        const bool opens = h->ld.count[br] == 0;
        if (opens) {
            if (br < h->V && s != 1) return load_fail(h, "event %llu: first of branch %llu", g, br);
            h->ld.first[br] = s;
            h->ld.creator[br] = c;
        } else if (h->ld.creator[br] != c || s != h->ld.last[br] + 1 || sp != h->ld.tail[br]) {
            return load_fail(h, "event %llu: does not continue branch %llu", g, br);
        }
        h->ld.last[br] = s;
        h->ld.tail[br] = (uint32_t)g;
        h->ld.count[br]++;
        h->ld.B = std::max(h->ld.B, br + 1);
        // branches before its Add, from the HighestBefore byte length: 8 x (B
        // before + 1) when it opened a fork branch, else 8 x B before
        // (vecengine/index.go:147, vecfc/vector.go:82-89)
        const uint64_t hl = hb_off[i + 1] - hb_off[i], ll = la_off[i + 1] - la_off[i];
        if (hb_off[i + 1] < hb_off[i] || la_off[i + 1] < la_off[i] || hl % 8 || ll % 4 || hl / 8 > 0xFFFFFF || ll / 4 > 0xFFFFFF)
            return load_fail(h, "event %llu: vector byte lengths", g);
        const uint32_t hent = (uint32_t)(hl / 8), lent = (uint32_t)(ll / 4);
        const bool fork_open = opens && br >= h->V;
        const uint32_t bb = fork_open ? br : hent;
        if ((fork_open ? hent != br + 1 : (hent < h->V || br >= hent)) || lent < bb + (fork_open ? 1u : 0u))
            return load_fail(h, "event %llu: vector lengths disagree with branch %llu", g, br);
        max_hent = std::max(max_hent, hent);
        max_lent = std::max(max_lent, lent);
        bmax = std::max(bmax, s);
        h->hm.creator.push_back(c);
        h->hm.seq.push_back(s);
        h->hm.branch.push_back(br);
        h->hm.bbefore.push_back(bb);
        h->ld.par.insert(h->ld.par.end(), par + p0, par + p1);
        h->ld.poff.push_back(h->ld.par.size());
    }
    h->max_seq = bmax;
    int rc;
    if ((rc = grow_events(h, bs + n)) || (rc = grow_branches(h, std::max({h->ld.B, max_hent, max_lent}))) ||
        (rc = grow_scap(h, bmax)))
        return rc;
    hipStream_t st = h->stream;
    // metadata of the chunk (the mirror vectors stay alive until the sync below)
    std::vector<uint32_t> sp(n);
    for (uint32_t i = 0; i < n; i++)
        sp[i] = seq[i] > 1 ? par[poff[i]] : LX_NONE;
    HIPCHK(h, hipMemcpyAsync(h->lay.ev_creator + bs, h->hm.creator.data() + bs, n * 4ull, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(h->lay.ev_seq + bs, h->hm.seq.data() + bs, n * 4ull, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(h->lay.ev_branch + bs, h->hm.branch.data() + bs, n * 4ull, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(h->lay.ev_bbefore + bs, h->hm.bbefore.data() + bs, n * 4ull, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(h->lay.ev_sp + bs, sp.data(), n * 4ull, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(h->lay.branch_first, h->ld.first.data(), h->ld.B * 4ull, hipMemcpyHostToDevice, st));
    // the chunk's table bytes and offsets
    const uint64_t hb_n = hb_off[n] - hb_off[0], la_n = la_off[n] - la_off[0];
    const uint64_t o_hoff = (hb_n + la_n + 15) / 16 * 16, o_loff = o_hoff + 8ull * (n + 1);
    const uint64_t need = o_loff + 8ull * (n + 1);
    HIPCHK(h, h->ld.buf.grow(need, st, true));
    HIPCHK(h, hipMemcpyAsync(h->ld.buf, hb_bytes + hb_off[0], hb_n, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(h->ld.buf + hb_n, la_bytes + la_off[0], la_n, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(h->ld.buf + o_hoff, hb_off, 8ull * (n + 1), hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(h->ld.buf + o_loff, la_off, 8ull * (n + 1), hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemsetAsync(h->status + 5, 0, 4, st));
    LoadArgs a{};
    a.hb = h->lay.hb;
    a.la = h->lay.la;
    a.stride = h->stride;
    a.bs = (uint32_t)bs;
    a.n = n;
    a.B = h->ld.B;
    a.hb_off = reinterpret_cast<const uint64_t *>(h->ld.buf + o_hoff);
    a.la_off = reinterpret_cast<const uint64_t *>(h->ld.buf + o_loff);
    a.hb_base = hb_off[0];
    a.la_base = la_off[0] - hb_n;   // la bytes follow the hb bytes in the staging buffer
    a.hb_bytes = h->ld.buf;
    a.la_bytes = h->ld.buf;
    a.ev_branch = h->lay.ev_branch;
    a.ev_seq = h->lay.ev_seq;
    a.branch_first = h->lay.branch_first;
    a.brow = h->lay.brow;
    a.s_cap = h->s_cap;
    a.bad = h->status + 5;
    HIPCHK(h, lx::launch_load_rows(a, st));
    uint32_t bad = 0;
    HIPCHK(h, hipMemcpyAsync(&bad, h->status + 5, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    if (bad) return load_fail(h, "HighestBefore entries (MinSeq, own seq or branch) in events %llu..%llu", bs, bs + n - 1);
    h->n_events = bs + n;
    h->hwm = std::max(h->hwm, h->n_events);
    h->hm.n = h->n_events;
    return 0;
}

int lx_load_finish(lx_index *h, const uint8_t *bi_rlp, uint32_t bi_len) {
    if (!h) return LX_ERR_ARG;
    if (!h->have_epoch) return h->fail(LX_ERR_STATE, "lx_load_finish before lx_reset");
    if (!h->loading && h->n_events) return h->fail(LX_ERR_STATE, "lx_load_finish without lx_load_rows");
    if (!bi_rlp) return h->fail(LX_ERR_ARG, "null BranchesInfo");
    HIPCHK(h, set_dev(h->device));
    if (!h->loading) {   // an empty epoch: the initial BranchesInfo
        h->ld.first.assign(h->V, 1);
        h->ld.last.assign(h->V, 0);
        h->ld.count.assign(h->V, 0);
        h->ld.creator.resize(h->V);
        for (uint32_t c = 0; c < h->V; c++) h->ld.creator[c] = c;
        h->ld.poff.assign(1, 0);
        h->ld.B = h->V;
        h->loading = true;
    }
    std::vector<uint32_t> last, cr;
    std::vector<std::vector<uint32_t>> by;
    if (!decode_branches_info(bi_rlp, bi_len, last, cr, by)) return load_fail(h, "RLP(BranchesInfo) malformed");
    const uint32_t V = h->V, B = (uint32_t)last.size();
    if (cr.size() != B || by.size() != V || B < V || B < h->ld.B) return load_fail(h, "BranchesInfo sizes (B %llu)", B);
    h->ld.first.resize(B, 0);
    h->ld.last.resize(B, 0);
    h->ld.count.resize(B, 0);
    h->ld.creator.resize(B, LX_NONE);
    std::vector<std::vector<uint32_t>> want(V);
    for (uint32_t b = 0; b < B; b++) {
        if (cr[b] >= V || (b < V && cr[b] != b)) return load_fail(h, "branch %llu creator", b);
        if (b >= V && !h->ld.count[b]) return load_fail(h, "fork branch %llu has no event", b);
        if (h->ld.count[b] && h->ld.creator[b] != cr[b]) return load_fail(h, "branch %llu creator", b);
        if (last[b] != h->ld.last[b]) return load_fail(h, "branch %llu last seq %llu", b, last[b]);   // branches_info.go:11
        want[cr[b]].push_back(b);
    }
    for (uint32_t c = 0; c < V; c++)
        if (by[c] != want[c]) return load_fail(h, "branches of creator %llu", c);
    const uint64_t N = h->n_events;
    int rc;
    if ((rc = grow_branches(h, B))) return rc;
    h->B = h->B_flushed = B;
    h->h_branch_creator = cr;
    h->h_branch_first.assign(B, 1);
    std::vector<uint32_t> blen(B, 0);
    for (uint32_t b = 0; b < B; b++) {
        if (h->ld.count[b]) h->h_branch_first[b] = h->ld.first[b];
        blen[b] = h->ld.count[b];
    }
    h->by_creator = by;
    h->hm.blen = blen;
    h->hm.ok = true;
    h->hm.n = N;
    // claims: the continuing self-child of each event, each creator's first root
    std::vector<uint32_t> fchild(N, LX_NONE), froot(V, LX_NONE);
    for (uint64_t e = 0; e < N; e++) {
        const uint32_t s = h->hm.seq[e], br = h->hm.branch[e];
        if (s > 1) {
            const uint32_t sp = h->ld.par[h->ld.poff[e]];
            if (h->hm.branch[sp] == br) fchild[sp] = (uint32_t)e;
        } else if (br < V) {
            froot[br] = (uint32_t)e;
        }
    }
    hipStream_t st = h->stream;
    HIPCHK(h, hipMemcpyAsync(h->lay.branch_first, h->h_branch_first.data(), B * 4ull, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(h->lay.branch_creator, cr.data(), B * 4ull, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(h->lay.branch_len, blen.data(), B * 4ull, hipMemcpyHostToDevice, st));
    if (N) HIPCHK(h, hipMemcpyAsync(h->lay.first_child, fchild.data(), N * 4ull, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(h->lay.first_root, froot.data(), V * 4ull, hipMemcpyHostToDevice, st));
    h->pcols_used = std::max(h->pcols_used, B);
    if ((rc = rebuild_columns(h))) return rc;   // syncs the stream
    if (N) {
        // fork markers only in cheaters' columns (k_load_raw / k_load_check
        // below verify those); a marker anywhere else is corrupt
        std::vector<uint32_t> cheat_col(B, 0);
        for (uint32_t b = 0; b < B; b++) cheat_col[b] = by[cr[b]].size() > 1 ? 1u : 0u;
        DU32 d_cc;
        HIPCHK(h, d_cc.renew(B));
        HIPCHK(h, hipMemcpyAsync(d_cc, cheat_col.data(), 4ull * B, hipMemcpyHostToDevice, st));
        HIPCHK(h, hipMemsetAsync(h->status + 5, 0, 4, st));
        HIPCHK(h, lx::launch_load_marks_ok(h->lay.hb, h->stride, (uint32_t)N, B, d_cc, h->status + 5, st));
        uint32_t bad = 0;
        HIPCHK(h, hipMemcpyAsync(&bad, h->status + 5, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(h, hipStreamSynchronize(st));
        d_cc.reset();
        if (bad) return load_fail(h, "fork marker in a column of a creator with one branch");
    }
    if (B > V && h->n_cheat && N) {
        // raw seqs behind the fork markers (cheaters' columns), then the markers
        // re-derived from them must be exactly the loaded ones
        std::vector<uint32_t> cols;
        for (uint32_t c = 0; c < V; c++)
            if (by[c].size() > 1) cols.insert(cols.end(), by[c].begin(), by[c].end());
        const uint32_t ncc = (uint32_t)cols.size();
        std::vector<uint32_t> lvl(N), perm(N);
        uint32_t L = 0;
        for (uint64_t e = 0; e < N; e++) {
            uint32_t l = 0;
            for (uint64_t k = h->ld.poff[e]; k < h->ld.poff[e + 1]; k++) l = std::max(l, lvl[h->ld.par[k]] + 1);
            lvl[e] = l;
            L = std::max(L, l + 1);
        }
        std::vector<uint32_t> off(L + 1, 0);
        for (uint64_t e = 0; e < N; e++) off[lvl[e] + 1]++;
        for (uint32_t l = 0; l < L; l++) off[l + 1] += off[l];
        std::vector<uint32_t> cur(off.begin(), off.end() - 1);
        for (uint64_t e = 0; e < N; e++) perm[cur[lvl[e]]++] = (uint32_t)e;
        const uint64_t npar = h->ld.par.size();
        DBytes d_scratch;
        const uint64_t o_perm = 4ull * ncc, o_off = o_perm + 4ull * N, o_poff = (o_off + 4ull * (L + 1) + 7) / 8 * 8,
                       o_par = o_poff + 8ull * (N + 1), o_lm = o_par + 4ull * std::max<uint64_t>(npar, 1);
        HIPCHK(h, d_scratch.renew(o_lm + N * ncc));
        uint8_t *scratch = d_scratch;
        HIPCHK(h, hipMemcpyAsync(scratch, cols.data(), 4ull * ncc, hipMemcpyHostToDevice, st));
        HIPCHK(h, hipMemcpyAsync(scratch + o_perm, perm.data(), 4ull * N, hipMemcpyHostToDevice, st));
        HIPCHK(h, hipMemcpyAsync(scratch + o_off, off.data(), 4ull * (L + 1), hipMemcpyHostToDevice, st));
        HIPCHK(h, hipMemcpyAsync(scratch + o_poff, h->ld.poff.data(), 8ull * (N + 1), hipMemcpyHostToDevice, st));
        if (npar) HIPCHK(h, hipMemcpyAsync(scratch + o_par, h->ld.par.data(), 4ull * npar, hipMemcpyHostToDevice, st));
        HIPCHK(h, hipMemsetAsync(h->status + 5, 0, 4, st));
        LoadRawArgs r{};
        r.hb = h->lay.hb;
        r.stride = h->stride;
        r.cols = reinterpret_cast<const uint32_t *>(scratch);
        r.ncc = ncc;
        r.perm = reinterpret_cast<const uint32_t *>(scratch + o_perm);
        r.lvl_off = reinterpret_cast<const uint32_t *>(scratch + o_off);
        r.n_levels = L;
        r.poff = reinterpret_cast<const uint64_t *>(scratch + o_poff);
        r.par = reinterpret_cast<const uint32_t *>(scratch + o_par);
        r.ev_branch = h->lay.ev_branch;
        r.ev_seq = h->lay.ev_seq;
        r.lm = scratch + o_lm;
        r.bad = h->status + 5;
        HIPCHK(h, lx::launch_load_raw(r, st));
        MarkArgs m{};
        m.hb = h->lay.hb;
        m.stride = h->pstride;
        m.batch_start = 0;
        m.n = (uint32_t)N;
        m.V = V;
        m.ev_branch = h->lay.ev_branch;
        m.ev_bbefore = h->lay.ev_bbefore;
        m.branch_first = h->lay.branch_first;
        m.n_cheat = h->n_cheat;
        m.cheat_off = h->lay.cheat_off;
        m.cheat_br = h->lay.cheat_br;
        HIPCHK(h, lx::launch_marks(m, st));
        HIPCHK(h, lx::launch_load_check(r, (uint32_t)N, st));
        uint32_t bad = 0;
        HIPCHK(h, hipMemcpyAsync(&bad, h->status + 5, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(h, hipStreamSynchronize(st));
        if (bad) return load_fail(h, "fork markers / raw HighestBefore do not follow from the vectors (flags %llu)", bad);
    }
    if (N) {
        LoadVerifyArgs v{};
        v.hb = h->lay.hb;
        v.la = h->lay.la;
        v.stride = h->stride;
        v.n = (uint32_t)N;
        v.B = B;
        v.ev_branch = h->lay.ev_branch;
        v.ev_seq = h->lay.ev_seq;
        v.branch_first = h->lay.branch_first;
        v.branch_len = h->lay.branch_len;
        v.brow = h->lay.brow;
        v.s_cap = h->s_cap;
        v.bad = h->status + 5;
        HIPCHK(h, hipMemsetAsync(h->status + 5, 0, 4, st));
        HIPCHK(h, lx::launch_load_verify_la(v, st));
        uint32_t bad = 0;
        HIPCHK(h, hipMemcpyAsync(&bad, h->status + 5, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(h, hipStreamSynchronize(st));
        if (bad) return load_fail(h, "LowestAfter rows do not follow from the HighestBefore rows (flags %llu)", bad);
    }
    h->n_flushed = N;
    h->loading = false;
    h->ld.par.clear();
    h->ld.par.shrink_to_fit();
    h->ld.poff.clear();
    h->ld.poff.shrink_to_fit();
    return 0;
}

}  // extern "C"
