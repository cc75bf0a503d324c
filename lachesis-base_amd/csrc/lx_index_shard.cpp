// lx_index_shard.cpp -- the column-shard LowestAfter exchange of the index handle
// (lx_index.h): shard bounds, row and column lists, pack / unpack, the
// incremental (dirty-row) exchange.
#include <hip/hip_runtime.h>

#include "lx_index.h"

using namespace lxi;

void shard_bounds(const lx_index *h, uint32_t r, uint32_t *lo, uint32_t *hi) {
    auto bound = [&](uint32_t q) {
        return q >= h->shard_count ? h->V : (uint32_t)((uint64_t)h->V * q / h->shard_count) & ~3u;
    };
    *lo = bound(r);
    *hi = bound(r + 1);
}

namespace {

std::vector<uint32_t> shard_cols(const lx_index *h, uint32_t q) {
    uint32_t lo, hi;
    shard_bounds(h, q, &lo, &hi);
    std::vector<uint32_t> cols;
    for (uint32_t b = 0; b < h->B; b++)
        if (h->h_branch_creator[b] >= lo && h->h_branch_creator[b] < hi) cols.push_back(b);
    return cols;
}

int upload_cols(lx_index *h);
int ensure_shard_cols(lx_index *h);

// rows (events) whose branch belongs to each shard, at the current event count
// (and every shard's column list)
int ensure_shard_rows(lx_index *h) {
    if (h->sc.events == h->n_events && h->sc.gen == h->branch_gen) return 0;
    const uint32_t n = (uint32_t)h->n_events;
    const uint32_t G = h->shard_count;
    if (n > h->lay.sc_flag.cap() || h->lay.sc_rows.size() != G) {
        h->lay.sc_rows = std::vector<DU32>(G);
        uint64_t cap = std::max<uint64_t>(n, 4096);
        for (DU32 &r : h->lay.sc_rows) HIPCHK(h, r.renew(cap));
        h->lay.sc_flag.reset();   // (the capacity the check above reads: set last)
        HIPCHK(h, h->lay.sc_pos.renew(cap));
        size_t sb = 0;
        HIPCHK(h, lx::scan_tmp_bytes((uint32_t)cap, &sb));
        HIPCHK(h, h->lay.sc_tmp.renew(sb));
        HIPCHK(h, h->lay.sc_flag.renew(cap));
    }
    h->lay.sc_nrows.assign(G, 0);
    for (uint32_t q = 0; q < G; q++) {
        uint32_t lo, hi;
        shard_bounds(h, q, &lo, &hi);
        HIPCHK(h, lx::launch_shard_rows(h->lay.ev_branch, h->lay.branch_creator, n, lo, hi, h->lay.sc_flag,
                                        h->lay.sc_pos, h->lay.sc_tmp, h->lay.sc_tmp.cap(), h->lay.sc_rows[q], h->stream));
        if (n) HIPCHK(h, hipMemcpyAsync(&h->lay.sc_nrows[q], h->lay.sc_pos + (n - 1), 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    if (int rc = upload_cols(h)) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->sc.events = h->n_events;
    h->sc.gen = h->branch_gen;
    return 0;
}

// the column lists alone (the incremental exchange lists its rows itself)
int ensure_shard_cols(lx_index *h) {
    if (h->lay.sc_cols && h->sc.cols_gen == h->branch_gen) return 0;
    if (int rc = upload_cols(h)) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

// every shard's column list on the device (rebuilt with the shard rows, when
// the event count or the branch set changed)
int upload_cols(lx_index *h) {
    std::vector<uint32_t> all;
    h->sc.col_off.assign(1, 0);
    for (uint32_t q = 0; q < h->shard_count; q++) {
        std::vector<uint32_t> c = shard_cols(h, q);
        all.insert(all.end(), c.begin(), c.end());
        h->sc.col_off.push_back((uint32_t)all.size());
    }
    HIPCHK(h, h->lay.sc_cols.renew(all.size(), h->stream, true));
    if (!all.empty())
        HIPCHK(h, hipMemcpyAsync(h->lay.sc_cols, all.data(), all.size() * 4, hipMemcpyHostToDevice, h->stream));
    h->sc.cols_gen = h->branch_gen;
    return 0;
}

}  // namespace

extern "C" {

int lx_shard_of(const lx_index *h, uint32_t *rank, uint32_t *count) {
    if (!h) return LX_ERR_ARG;
    if (rank) *rank = h->shard_rank;
    if (count) *count = h->shard_count;
    return 0;
}

int lx_shard_range(const lx_index *h, uint32_t shard, uint32_t *lo, uint32_t *hi) {
    if (!h || shard >= h->shard_count) return LX_ERR_ARG;
    shard_bounds(h, shard, lo, hi);
    return 0;
}

// Wire width of a LowestAfter block entry: LA entries are seqs or 0, so while
// every seq of the epoch is < 2^16 they travel as uint16 (half the all-to-all
// bytes).  max_seq follows the event stream, which every shard indexes whole,
// so all shards agree on the width.  Option shard_wire=4 forces uint32.
static uint32_t shard_wire_bytes(const lx_index *h) {
    return (h->wire_force != 4 && h->max_seq <= 0xFFFFu) ? 2u : 4u;
}

int lx_shard_wire(lx_index *h, uint32_t *bytes_per_entry) {
    if (!h || !bytes_per_entry) return LX_ERR_ARG;
    *bytes_per_entry = shard_wire_bytes(h);
    return 0;
}

int lx_shard_block(lx_index *h, uint32_t src, uint32_t dst, uint64_t *elems) {
    if (!h || !elems || src >= h->shard_count || dst >= h->shard_count) return LX_ERR_ARG;
    HIPCHK(h, set_dev(h->device));
    int rc;
    if ((rc = h->sx.active ? ensure_shard_cols(h) : ensure_shard_rows(h))) return rc;
    const uint64_t nrows = h->sx.active ? h->sx.roff[src + 1] - h->sx.roff[src] : h->lay.sc_nrows[src];
    *elems = nrows * (h->sc.col_off[dst + 1] - h->sc.col_off[dst]);
    return 0;
}

// rows of shard `rows_of` x columns of shard `cols_of`, moved by `mode`
// (0 pack, 1 unpack, 2 own block, 3 byte-wire check into buf[0]); wire 0 = the
// epoch's width (shard_wire_bytes)
static int la_xfer(lx_index *h, uint32_t rows_of, uint32_t cols_of, uint32_t *buf, int mode, uint32_t wire = 0) {
    if (!h->sharded()) return h->fail(LX_ERR_STATE, "LowestAfter exchange needs a column-sharded handle");
    if (!h->have_epoch) return h->fail(LX_ERR_STATE, "exchange before lx_reset");
    HIPCHK(h, set_dev(h->device));
    int rc;
    if ((rc = h->sx.active ? ensure_shard_cols(h) : ensure_shard_rows(h))) return rc;
    const uint32_t c0 = h->sc.col_off[cols_of], c1 = h->sc.col_off[cols_of + 1];
    XferArgs x{};
    x.lap = h->lay.lap;
    x.lap_stride = h->stride;
    x.s_cap = h->s_cap;
    x.la = h->lay.la;
    x.pstride = h->pstride;
    x.cmap = h->lay.cmap;
    x.ev_branch = h->lay.ev_branch;
    x.ev_seq = h->lay.ev_seq;
    x.branch_first = h->lay.branch_first;
    // the dirty rows of an incremental exchange (lx_shard_dirty_set), else every row
    x.rows = h->sx.active ? h->lay.sx_rows + h->sx.roff[rows_of] : h->lay.sc_rows[rows_of];
    x.nrows = h->sx.active ? (uint32_t)(h->sx.roff[rows_of + 1] - h->sx.roff[rows_of]) : h->lay.sc_nrows[rows_of];
    x.cols = h->lay.sc_cols + c0;
    x.ncols = c1 - c0;
    x.buf = buf;
    x.mode = mode;
    x.wire = wire ? wire : shard_wire_bytes(h);
    const bool check = mode == 3 || (mode == 0 && x.wire == 1);
    if (check) {
        HIPCHK(h, h->lay.wire_flag.grow(1));
        HIPCHK(h, hipMemsetAsync(h->lay.wire_flag, 0, 4, h->stream));
        x.flag = h->lay.wire_flag;
        if (mode == 3) x.buf = h->lay.wire_flag;
    }
    HIPCHK(h, lx::launch_la_xfer(x, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (check) {
        uint32_t bad = 0;
        HIPCHK(h, hipMemcpy(&bad, h->lay.wire_flag, 4, hipMemcpyDeviceToHost));
        if (mode == 3) return bad ? 1 : 0;
        if (bad) return h->fail(LX_ERR_WIRE, "LowestAfter block to shard %u does not fit the 1-byte wire", cols_of);
    }
    return 0;
}

int lx_la_pack_dev(lx_index *h, uint32_t dst, uint32_t *out, void *stream) {
    if (!h || dst >= h->shard_count || dst == h->shard_rank || !out) return LX_ERR_ARG;
    (void)stream;
    return la_xfer(h, h->shard_rank, dst, out, 0);
}

int lx_la_unpack_dev(lx_index *h, uint32_t src, const uint32_t *in, void *stream) {
    if (!h || src >= h->shard_count || src == h->shard_rank || !in) return LX_ERR_ARG;
    (void)stream;
    return la_xfer(h, src, h->shard_rank, const_cast<uint32_t *>(in), 1);
}

int lx_shard_block_wire(lx_index *h, uint32_t dst, uint32_t *bytes_per_entry) {
    if (!h || !bytes_per_entry || dst >= h->shard_count || dst == h->shard_rank) return LX_ERR_ARG;
    *bytes_per_entry = shard_wire_bytes(h);
    if (h->wire_force) return 0;               // option shard_wire pins the epoch width
    const int r = la_xfer(h, h->shard_rank, dst, nullptr, 3);
    if (r < 0) return r;
    if (r == 0) *bytes_per_entry = 1;
    return 0;
}

int lx_la_pack_wire_dev(lx_index *h, uint32_t dst, void *out, uint32_t bytes_per_entry) {
    if (!h || dst >= h->shard_count || dst == h->shard_rank || !out) return LX_ERR_ARG;
    if (bytes_per_entry != 1 && bytes_per_entry != 2 && bytes_per_entry != 4) return LX_ERR_ARG;
    if (bytes_per_entry == 1 && h->wire_force)
        return h->fail(LX_ERR_WIRE, "option shard_wire pins the wire to %u bytes", shard_wire_bytes(h));
    return la_xfer(h, h->shard_rank, dst, static_cast<uint32_t *>(out), 0, bytes_per_entry);
}

int lx_la_unpack_wire_dev(lx_index *h, uint32_t src, const void *in, uint32_t bytes_per_entry) {
    if (!h || src >= h->shard_count || src == h->shard_rank || !in) return LX_ERR_ARG;
    if (bytes_per_entry != 1 && bytes_per_entry != 2 && bytes_per_entry != 4) return LX_ERR_ARG;
    return la_xfer(h, src, h->shard_rank, static_cast<uint32_t *>(const_cast<void *>(in)), 1, bytes_per_entry);
}

int lx_la_own_dev(lx_index *h, void *stream) {
    if (!h) return LX_ERR_ARG;
    (void)stream;
    return la_xfer(h, h->shard_rank, h->shard_rank, nullptr, 2);
}

// ---- incremental LowestAfter exchange ("streaming")
//
// An entry LA[(c, s)][j] is written when an event e of branch j first reaches
// (c, s): s in (RAW(prev(e))[c], RAW(e)[c]].  RAW grows
// along a branch, so every entry written since the last exchange lies at
// s > RAW(p_j)[c], p_j = branch j's last event at that exchange (none: from
// the branch's first seq).  dmin[c] = min over the branches with new events
// of RAW(p_j)[c] + 1 is therefore the first row of branch c that can have
// changed; rows below it are unchanged on every receiver.  Only the owner of
// column c holds RAW(.)[c]: each rank reports its own columns, the ranks
// combine them by an element-wise min, and every rank lists the same dirty
// rows for every shard (branch order, then seq).  A DropNotFlushed, reset or
// load makes the next exchange a full one.

int lx_shard_dirty(lx_index *h, uint32_t nb, uint32_t *dmin) {
    if (!h || !dmin) return LX_ERR_ARG;
    if (!h->sharded()) return h->fail(LX_ERR_STATE, "the incremental exchange needs a column-sharded handle");
    if (!h->have_epoch) return h->fail(LX_ERR_STATE, "exchange before lx_reset");
    if (nb < h->B) return h->fail(LX_ERR_ARG, "dmin holds %u branches < %u", nb, h->B);
    HIPCHK(h, set_dev(h->device));
    int rc;
    if ((rc = flush_pending(h)) || (rc = ensure_shard_cols(h))) return rc;
    for (uint32_t b = 0; b < nb; b++) dmin[b] = LX_NONE;
    const uint32_t c0 = h->sc.col_off[h->shard_rank], c1 = h->sc.col_off[h->shard_rank + 1];
    if (h->lay.sx_len.cap() < h->stride || !h->lay.sx_len) {
        HIPCHK(h, renew_guarded(h->stride, h->lay.sx_len, h->lay.sx_dmin));
        HIPCHK(h, hipMemsetAsync(h->lay.sx_len, 0, (uint64_t)h->stride * 4, h->stream));
        h->sx.full = true;
    }
    if (h->sx.full) {
        // whole blocks: every row of every own branch
        const std::vector<uint32_t> own = shard_cols(h, h->shard_rank);
        for (uint32_t c : own) dmin[c] = h->h_branch_first[c];
        return 0;
    }
    if (!h->B || c1 == c0) return 0;
    HIPCHK(h, lx::launch_fill_u32(h->lay.sx_dmin, h->B, LX_NONE, h->stream));
    HIPCHK(h, lx::launch_shard_dmin(h->lay.hb, h->pstride, h->lay.cmap, h->lay.branch_len, h->lay.brow, h->s_cap,
                                    h->lay.branch_first,
                                    h->lay.sx_len, h->B, h->lay.sc_cols + c0, c1 - c0, h->lay.sx_dmin, h->stream));
    HIPCHK(h, hipMemcpyAsync(dmin, h->lay.sx_dmin, 4ull * h->B, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

int lx_shard_dirty_set(lx_index *h, uint32_t nb, const uint32_t *dmin) {
    if (!h || !dmin) return LX_ERR_ARG;
    if (!h->sharded()) return h->fail(LX_ERR_STATE, "the incremental exchange needs a column-sharded handle");
    if (nb < h->B) return h->fail(LX_ERR_ARG, "dmin holds %u branches < %u", nb, h->B);
    HIPCHK(h, set_dev(h->device));
    int rc;
    if ((rc = ensure_shard_cols(h))) return rc;
    const uint32_t B = h->B, G = h->shard_count;
    std::vector<uint32_t> len(B);
    if (B) HIPCHK(h, hipMemcpyAsync(len.data(), h->lay.branch_len, 4ull * B, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    // per shard, its branches in order: {branch, first dirty index, row offset}
    std::vector<uint32_t> meta;
    std::vector<uint64_t> moff;
    h->sx.roff.assign(G + 1, 0);
    uint64_t total = 0;
    for (uint32_t q = 0; q < G; q++) {
        h->sx.roff[q] = total;
        for (uint32_t c : shard_cols(h, q)) {
            const uint32_t first = h->h_branch_first[c];
            uint32_t start = len[c];
            if (dmin[c] != LX_NONE) start = dmin[c] <= first ? 0u : std::min(dmin[c] - first, len[c]);
            if (start == len[c]) continue;
            meta.push_back(c);
            meta.push_back(start);
            meta.push_back((uint32_t)total);
            meta.push_back(len[c] - start);
            total += len[c] - start;
        }
    }
    h->sx.roff[G] = total;
    if (total > 0xFFFFFFFFull) return h->fail(LX_ERR_ARG, "too many dirty rows");
    if ((rc = grow_scratch(h, h->lay.sx_rows, total + 1)) ||
        (rc = grow_scratch(h, h->lay.sx_meta, (uint64_t)meta.size() + 4)))
        return rc;
    if (!meta.empty()) {
        HIPCHK(h, hipMemcpyAsync(h->lay.sx_meta, meta.data(), meta.size() * 4, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, lx::launch_shard_dirty_rows(h->lay.brow, h->s_cap, h->lay.sx_meta, (uint32_t)(meta.size() / 4),
                                              h->lay.sx_rows, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));   // `meta` is a host temporary
    h->sx.active = true;
    return 0;
}

int lx_shard_dirty_commit(lx_index *h) {
    if (!h) return LX_ERR_ARG;
    if (!h->sharded()) return h->fail(LX_ERR_STATE, "the incremental exchange needs a column-sharded handle");
    HIPCHK(h, set_dev(h->device));
    if (h->lay.sx_len && h->B) {
        HIPCHK(h, hipMemcpyAsync(h->lay.sx_len, h->lay.branch_len, 4ull * h->B, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        h->sx.full = false;
    }
    h->sx.active = false;
    return 0;
}

}  // extern "C"
