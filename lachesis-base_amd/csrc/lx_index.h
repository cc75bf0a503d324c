// lx_index.h -- the index handle behind the C ABI (include/lachesis_hip.h) and
// what the sources of the host engine share:
//   lx_capi.cpp           create / destroy, options, Reset, Flush, DropNotFlushed, sync, stats, the index view
//   lx_index_layout.cpp   growth and re-layout of the device buffers, column and cheater tables, argument builders
//   lx_index_add.cpp      the big Add path (device arrays): batch preparation, the walks, the segmented walk
//   lx_index_small.cpp    lx_add_batch and the small (latency) Add path: host mirror, staging slots, the pending run
//   lx_index_fc.cpp       ForklessCause entry points, early-exit counters, the column-shard early exit
//   lx_index_get.cpp      row getters and the resident row server
//   lx_index_shard.cpp    the column-shard LowestAfter exchange, whole and incremental
//   lx_index_persist.cpp  write-back, and the load from persisted tables (RLP: lx_rlp.h)
// and their neighbours (lx_fccache.cpp, lx_rowseg.cpp, the abft engine through
// the index view).  Every device buffer, pinned buffer, stream and event of the
// handle is owned by a type that frees it (lx_devbuf.h): nothing is freed by
// hand.  Internal: not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/lachesis_hip.h"
#include "lx_devbuf.h"
#include "lx_internal.h"

struct FcCache;   // lx_fccache.cpp

namespace lxi {

constexpr uint32_t kStatusWords = 64;   // [1] fc bad flag, [2] max seq, [3] pinned-FC sink, [4] unresolved
                                        // branch, [5] load check flags, [8..9] batch error u64, [16..47] jump flags

using DU32 = DevBuf<uint32_t>;
using DBytes = DevBuf<uint8_t>;   // untyped scratch (its capacity is its size in bytes)

inline uint32_t round_up(uint32_t x, uint32_t m) { return (x + m - 1) / m * m; }

// std::vector whose resize leaves new elements default-initialised (no zero
// fill): the small Add path sizes its lists for the worst case per batch and
// writes every element it keeps
template <class T>
struct NoInitAlloc : std::allocator<T> {
    NoInitAlloc() = default;
    template <class U>
    NoInitAlloc(const NoInitAlloc<U> &) noexcept {}
    template <class U>
    struct rebind {
        using other = NoInitAlloc<U>;
    };
    template <class U>
    void construct(U *p) noexcept {
        ::new (static_cast<void *>(p)) U;
    }
    template <class U, class... A>
    void construct(U *p, A &&...a) {
        ::new (static_cast<void *>(p)) U(std::forward<A>(a)...);
    }
};
template <class T>
using rawvec = std::vector<T, NoInitAlloc<T>>;

// hipSetDevice costs microseconds per call; every entry point makes sure the
// handle's device is current, so switch only when it is not
inline hipError_t set_dev(int device) {
    int cur = -1;
    if (hipGetDevice(&cur) == hipSuccess && cur == device) return hipSuccess;
    return hipSetDevice(device);
}

// The device buffers whose shape follows the epoch's layout (branch capacity,
// local columns, event capacity).  lx_reset drops them all at once when the
// layout changes (free_all: lay = Layout{}); the buffers that live as long as
// the handle are members of lx_index itself.
struct Layout {
    // the planes: hb / la are views.  They are hb_mem / la_mem themselves,
    // except on a row-segment rank, whose planes hold its own rows only
    // (rs_planes): there they are virtual bases (own row e at hb + e * pstride,
    // inside the allocations of rs_mem_rows rows)
    uint32_t *hb = nullptr, *la = nullptr;
    DU32 hb_mem, la_mem;
    uint64_t rs_mem_rows = 0;
    uint32_t rs_mem_pstride = 0;
    // per event, per branch
    DU32 ev_creator, ev_seq, ev_branch, ev_bbefore, ev_sp, first_child;
    DU32 first_root, branch_first, branch_creator, branch_len, brow, wpad, col_list;
    // LowestAfter tail zeroing (unsharded; TailArgs): per-(j, c) done-up-to seqs
    DU32 tail_zw, tail_lo, tail_cmin;
    uint32_t tail_cap() const { return (uint32_t)tail_cmin.cap(); }
    DU32 wire_flag;                        // device flag of the byte-wire fit check (4 B)
    // cheater CSR; cheat_brl / cheat_crl: the same as plane columns (shards)
    DU32 cheat_off, cheat_br, cheat_creator, cheat_brl, cheat_crl;
    DevBuf<int32_t> cheat_of;              // creator -> index into the cheater CSR (-1: one branch)
    // fork-path ForklessCause tables per plane column (k_fc_fk; valid when
    // fk_hi4 != 0): weight of a non-cheater's original, cheater index of a
    // cheater's branches, the cheaters' weights
    DU32 fk_w, fk_c, fk_wch;
    // column shard (shard_count > 1): own columns only (lx_internal.h)
    DU32 cmap, lap, wloc;
    // batch scratch (batch_cap events, b_par.cap() parents)
    uint64_t batch_cap = 0;
    DU32 b_creator, b_seq, b_poff, b_par, b_isfork, b_rank, b_tmpbr, b_jmp;
    DevBuf<EventRec> b_rec;
    DevBuf<CRec> b_crec;                   // compact records (lx_internal.h) of the last batch
    DBytes scan_tmp;
    // query scratch
    DU32 q_a, q_b;
    DBytes q_out;
    // column-shard exchange cache (rows per shard at sc.events)
    std::vector<DU32> sc_rows;
    std::vector<uint32_t> sc_nrows;
    DU32 sc_flag, sc_pos, sc_cols;
    DBytes sc_tmp;
    // incremental LowestAfter exchange (lx_shard_dirty*): per branch the events it
    // had at the last committed exchange; the dirty row lists of every shard
    DU32 sx_len, sx_dmin, sx_rows, sx_meta;
    // write-back (lx_writeback_*): dirty-row flags, row lists, byte offsets
    DU32 wb_flag, wb_pos, wb_la_rows, wb_hb_rows, wb_buf;
    DevBuf<uint64_t> wb_len, wb_la_off, wb_hb_off;
    DBytes wb_tmp;
    // segmented walk (option segments, lx_segment.hip): scratch of the last batch (seg_mf: flags)
    DU32 seg_jt, seg_cnt, seg_mf, seg_plist, seg_elist;
    // row-segment rank (lx_rowseg.cpp)
    DU32 rs_need, rs_req, rs_ctr, rs_ids, rs_out, rs_send;
    // ForklessCause across ranks (lx_rowseg_fc_*): per event the stamp of its LA
    // row (2 gen: asked in batch gen, 2 gen + 1: received), route / sort scratch
    DU32 rs_stamp, rsq_scratch, rsq_list, rsq_ctr;
    DBytes rsq_tmp;
    // rows of other ranks a row-segment rank receives go to receive areas
    // (rows x pstride): HighestBefore rows for the partial fix-up (rs_rhb, row
    // rs_hslot[x]), LowestAfter rows for one ForklessCause batch (rs_rla, row
    // rs_lslot[x])
    DU32 rs_hslot, rs_rhb, rs_lslot, rs_rla;
};

}  // namespace lxi

struct lx_index {
    int device = 0;
    // declared ahead of every buffer and event, so that it is destroyed last
    // (after the buffers whose work ran on it; ~lx_index waits for that work)
    lxi::Stream stream;
    // the caller's stream of an entry point that takes one (null: the handle's)
    hipStream_t stream_or(void *s) const { return s ? (hipStream_t)s : (hipStream_t)stream; }
    lx_index() = default;
    __attribute__((visibility("hidden"))) ~lx_index();   // lx_capi.cpp
    uint32_t shard_rank = 0, shard_count = 1;
    std::string err;

    // epoch
    uint32_t V = 0;
    std::vector<uint32_t> weights;
    uint32_t quorum = 0;
    uint32_t own_lo = 0, own_hi = 0;
    uint64_t n_events = 0, n_flushed = 0, hwm = 0;
    uint32_t B = 0, B_flushed = 0;
    uint32_t max_seq = 0;
    bool la_tail = true;                   // option la_memset=1: zero the whole LA plane at reset instead
    bool tail_dirty = false;               // lay.tail_zw holds progress (a tail pass ran since it was zeroed)
    uint32_t wire_force = 0;               // option shard_wire=4: LowestAfter blocks always uint32
    uint32_t pcols_used = 0;       // plane columns rows may hold non-zero values in (since the last zeroing)
    bool have_epoch = false;

    // host mirror of BranchesInfo (creator / first seq per branch; by creator)
    std::vector<uint32_t> h_branch_creator, h_branch_first;
    std::vector<std::vector<uint32_t>> by_creator;
    // generation of the branch -> creator map, never 0 once an epoch exists:
    // bumped whenever the map changes (rebuild_columns: Reset, an Add that
    // creates forks, a DropNotFlushed that removes them, lx_load_finish).  A
    // drop can take a fork's branch number back and a later Add give it to
    // another creator's fork, so the branch count alone does not identify the
    // map: every table built from it is keyed on this counter
    uint64_t branch_gen = 0;
    // Rollbacks of the dense indices, for handles that key tables of their own
    // on them (lx_mediantime.cpp).  roll_gen counts every event that lets an
    // index name another event: lx_reset and the start of a load (nothing is
    // kept: they also set epoch_gen = roll_gen) and every lx_drop_not_flushed
    // that dropped something; roll_keep[k] is the flushed count rollback
    // epoch_gen + 1 + k kept (lx_index_kept_since)
    uint64_t roll_gen = 0, epoch_gen = 0;
    std::vector<uint64_t> roll_keep;
    void rolled_epoch() {
        epoch_gen = ++roll_gen;
        roll_keep.clear();
    }
    void rolled_back(uint64_t keep) {
        roll_gen++;
        roll_keep.push_back(keep);
    }

    // capacities
    uint64_t n_cap = 0;
    uint32_t stride = 0;   // == branch capacity
    uint32_t pstride = 0;  // row stride of hb / la (= stride; a shard's local column capacity)
    uint32_t s_cap = 0;
    uint64_t cap_hint = 0;
    uint32_t reserve = 0;

    // device state: the buffers of the current layout, the handle's own below
    lxi::Layout lay;
    uint32_t n_cheat = 0, ncols = 0;
    uint32_t fk_hi4 = 0;                   // the fork-path ForklessCause tables (lay.fk_*) are valid
    bool dbl = true;                       // option dbl=0: the column walker for small fork-free batches too
    bool fc_fk = true;                     // option fc_fk=0: the fix-up loop kernel instead
    // column shard (shard_count > 1): own columns only (lx_internal.h)
    std::vector<uint32_t> h_cmap;          // global branch -> plane column / LX_NONE
    uint32_t nloc = 0;                     // plane columns in use
    bool sharded() const { return shard_count > 1; }
    lxi::DU32 status;

    bool b_crec_ok = false;                // lay.b_crec written (fork-free, 16-bit branches and seqs)

    // column-shard exchange cache (lay.sc_*: rows per shard at sc.events)
    struct ShardCache {
        uint64_t events = ~0ull;
        uint64_t gen = 0;                 // branch_gen the rows were listed for
        std::vector<uint32_t> col_off;    // shard q's columns: lay.sc_cols[col_off[q] .. col_off[q+1])
        uint64_t cols_gen = 0;            // branch_gen lay.sc_cols was built for
    } sc;
    // incremental LowestAfter exchange (lay.sx_*)
    struct ShardDirty {
        bool full = true;                 // the next exchange sends whole blocks (reset, drop, load)
        bool active = false;              // pack / unpack / lx_shard_block use the dirty lists
        std::vector<uint64_t> roff;       // shard q's dirty rows: lay.sx_rows[roff[q] .. roff[q + 1])
    } sx;

    // write-back (lx_writeback_*, lay.wb_*)
    struct WriteBack {
        bool ready = false;               // `desc` and `bi` describe the index as it is
        lx_writeback desc{};
        std::string bi;                   // RLP(BranchesInfo)
    } wb;

    // small-batch (latency) path, lx_small.hip: the host assigns branches in Add
    // order from a mirror of the per-event metadata and stages the batch in
    // pinned memory; one H2D copy + one launch, no sync
    uint32_t small_max = kSmallMaxN;       // option small_max: largest batch on this path (0: never)
    struct HostMirror {
        bool ok = false;                   // the mirror equals the device metadata
        uint64_t n = 0;                    // events whose (immutable) metadata the mirror holds
        lxi::rawvec<uint32_t> creator, seq, branch, bbefore;
        std::vector<uint32_t> blen;        // per branch: events on it (= device branch_len)
    } hm;
    struct SmallScratch {
        std::vector<uint32_t> level, cnt, touched;
        lxi::rawvec<uint2> undo;           // add_batch_small: {branch, length before} per event
        SmallInlineArgs inl{};             // arguments of the last launch; images of <= kSmallInline words inline
    } sm;
    // the pending run: small-path events assigned on the host but not launched
    // yet, [pend.bs, pend.bs + pend.n), branches from pend.B0 (flush_pending)
    struct PendingRun {
        uint32_t n = 0, B0 = 0, maxlvl = 0;
        uint64_t bs = 0;
        lxi::rawvec<SmallEv> ev;           // records (q1.x = offset into old, q2.w = h0 slot)
        lxi::rawvec<uint32_t> lvl;         // topological level inside the run
        lxi::rawvec<uint2> meta;           // per event {position | chunks << 16, chunk offset into pl}
        lxi::rawvec<uint16_t> pl;          // in-run parents (run positions), chunks of 4 (k_small)
        lxi::rawvec<uint2> old;            // {target, global event}: parents older than the run, older prevs
        uint64_t npar = 0;                 // parents of the run (LDS budget, small_fits)
        uint32_t nh = 0;                   // h0 slots of the run
    } pend;
    struct Touched {
        std::vector<uint32_t> mark;        // per branch: stamp of the last run that touched it
        uint32_t stamp = 0;
    } touch;
    // staging images in flight: slot k = a pinned image and its device copy,
    // copied by a kernel on the handle's stream (k_stage)
    static constexpr int kSlots = 4;
    struct Staging {
        lxi::PinBuf<uint32_t> pin[kSlots];
        lxi::Event copied[kSlots];         // the copy of slot k finished (its pinned image is free)
        bool used[kSlots] = {};
        uint32_t next = 0;
        lxi::DU32 dev[kSlots];
    } st;
    // restart from the persisted tables (lx_load_rows / lx_load_finish); `loading`
    // stays flat: every entry point reads it (NOT_LOADING)
    bool loading = false;
    struct Load {
        std::vector<uint32_t> first, last, count, creator, tail;   // per branch, as loaded
        std::vector<uint32_t> par;         // parents of every loaded event (dense)
        std::vector<uint64_t> poff;
        uint32_t B = 0;                    // branches seen so far (max ID + 1)
        lxi::DBytes buf;                   // device staging of a chunk's bytes and offsets
    } ld;

    // pinned, device-mapped query buffers (per-call ForklessCause, getters)
    lxi::MappedBuf<uint8_t> qp;
    // at least `bytes` of it (grown in steps of 64 KiB at least, after a wait for the stream)
    int ensure_qp(uint64_t bytes) {
        return hip(qp.grow(bytes, std::max<uint64_t>(bytes, 1u << 16), stream, true), "pinned query buffer");
    }
    bool fc_unchecked = false;             // a ForklessCause launch may have flagged status[1] since lx_sync looked
    // the resident single-row server (k_get_server, option get_server)
    // 0 off; 1 auto: only while this handle is the process's only one (the
    // server holds a hardware queue while resident, and GPU_MAX_HW_QUEUES = 4
    // lets more streams share queues: work queued behind the resident kernel
    // would wait up to its 250-us idle exit); 2 on whatever the handle count
    struct RowServer {
        int opt = 1;
        lxi::Stream stream;                // its own (high-priority) stream
        lxi::MappedBuf<uint64_t> host;     // [0] request word, [1] exited gen
        bool live = false;                 // launched and not known to have left
        uint32_t gen = 0;
        GetSrvArgs args{};                 // the live server's arguments (ticks, seen0, gen aside)
        uint64_t ticks_us = 0;             // wall clock ticks per microsecond
        uint64_t served = 0, launches = 0, fallbacks = 0;
        uint32_t get_tag = 0;              // completion tag of the last single-row getter
    } srv;
    uint32_t *q_sink = nullptr;            // status word the pinned FC path lets the kernel flag into
    bool get_host_check = true;            // option getter_host_check=0 (tests): device bound only

    // timing (HIP events on `stream`)
    lxi::Event ev[4];
    lx_stats stats{};
    bool stats_lazy = false;               // small path: ms_index from ev[1..2] on demand
    bool small_timing = false;             // option timing=1: time small-path launches (two event records)
    uint32_t cpw_hint = 0;                 // option cpw: walker columns per workgroup (0 = auto)
    bool pack16 = true;                    // option pack16=0: two slot units per event even for small seqs
    bool fold3 = true;                     // option fold3=0: the integer fold even when every seq <= kFold3MaxSeq
    bool seg_xmap_opt = false;             // option seg_xmap=1: 12-column walks keep each HB line's slices on one XCD
    bool crec_opt = false;                 // option crec=1: the 8- / 12-column walks stream the 32-B compact records
    bool prof = false;                     // LX_PROF=1 in make WPROF=1 builds: per-wave walker counters
    uint64_t last_npar = 0;                // parents in the current batch
    FcCache *fcc = nullptr;                // per-pair ForklessCause result cache (lx_fccache.cpp)
    uint32_t fcc_slots = 4096;             // option fc_cache: its working set (0 = no cache)
    bool fcc_slots_set = false;            // set by the option (else sized at lx_reset from V)
    // segmented walk (option segments, lx_segment.hip): scratch and timings of the last batch
    uint32_t segments = 0;
    bool fc_early = true;                  // option fc_early=0: k_fc always reads whole rows
    uint32_t fc_early_lanes = 32;          // option fc_early_lanes: k_fc_early's lanes per query (16 or 32)
    lxi::DevBuf<unsigned long long> d_clk;     // walk clock records (IndexArgs::clk)
    // column-shard early exit (lx_fc_shard_undecided_dev): flags, scan, scan scratch
    struct ShardEarly {
        lxi::DU32 flag, pos;
        lxi::DBytes tmp;
        size_t tmp_bytes = 0;              // of it, what the scan asks for
    } fcs;
    lxi::DevBuf<unsigned long long> d_fc_full;   // early exit counters (device): past round 1, past round 2, all
    bool fc_early_forks = false;           // option fc_early_forks=1: the early exit in fork epochs too (k_fc_fk_early)
    lxi::DevBuf<unsigned long long> d_fc_fke;    // ... its counters, same layout
    bool seg_auto = true;                  // option seg_auto=0: never split a batch on its own
    uint32_t n_cus = 256;                  // compute units of the device (auto segments)
    std::vector<lxi::Event> seg_ev;        // timing events of the segmented walks (seg_events)
    lx_seg_stats seg_stats{};
    // row-segment rank (options seg_rank / seg_count, lx_rowseg.cpp): one batch
    // per epoch, this rank walks and owns the rows of segment rs_rank
    uint32_t rs_rank = 0, rs_count = 0;
    int rs_state = 0;                      // 0 idle, 1 rows needed, 2 rows final, 3 LowestAfter sent, 4 ready
    uint32_t rs_lo = 0, rs_hi = 0, rs_npartial = 0, rs_nreq = 0;
    // the rank's own segment walked as rs_sub side-by-side sub-segments (option
    // seg_sub, 0: auto); rs_seg_lo then holds rs_count x rs_sub segments
    uint32_t rs_sub = 1, rs_sub_opt = 0;
    uint32_t rs_npart[kMaxSegments] = {};   // partial events per own sub-segment
    uint32_t rs_seg_lo[kMaxSegments + 1] = {};
    uint64_t rs_out_per = 0;               // triples per destination in rs_out
    uint64_t rs_nsend = 0;                 // triples packed in rs_send (lx_rowseg_la)
    uint32_t rs_gen = 0;                   // ForklessCause batch counter across ranks (lay.rs_stamp)
    uint32_t rsq_nlist = 0;                // distinct remote rows of the last lx_rowseg_fc_need
    bool rowseg() const { return rs_count >= 1; }   // seg_count = 1: one rank, the whole epoch

    // the epoch and the options as the walk plan sees them (lx_walk_plan.h)
    WalkEpoch walk_epoch() const {
        WalkEpoch e{};
        e.ncols = ncols;
        e.V = V;
        e.B = B;
        e.max_seq = max_seq;
        e.n_cus = n_cus;
        e.sharded = sharded();
        e.rowseg = rowseg();
        e.crec = b_crec_ok;
        e.cpw = cpw_hint;
        e.pack16 = pack16;
        e.fold3 = fold3;
        e.seg_xmap = seg_xmap_opt;
        e.seg_auto = seg_auto;
        e.segments = segments;
        return e;
    }

    int fail(int code, const char *fmt, ...) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        err = buf;
        return code;
    }
    int hip(hipError_t e, const char *what) {
        if (e == hipSuccess) return 0;
        return fail(e == hipErrorOutOfMemory ? LX_ERR_NOMEM : LX_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
    }
};

#define HIPCHK(h, expr)                                  \
    do {                                                 \
        int _rc = (h)->hip((expr), #expr);               \
        if (_rc) return _rc;                             \
    } while (0)


// Between lx_load_rows and lx_load_finish the branch table, B, the cheater
// tables and the branch lengths are not rebuilt yet: every entry point that
// reads or changes the epoch refuses (the load is finished or reset first).
#define NOT_LOADING(h)                                                                            \
    do {                                                                                          \
        if ((h)->loading) return (h)->fail(LX_ERR_STATE, "index is loading (lx_load_finish first)"); \
    } while (0)
// entry points that read whole rows of any event: not on a row-segment rank
#define WHOLE_INDEX(h)                                                                            \
    do {                                                                                          \
        if ((h)->rowseg()) return (h)->fail(LX_ERR_STATE, "needs a whole index (a row-segment rank holds its own rows)"); \
    } while (0)

// device scratch grown to `need` elements (contents not kept; waits for the stream before it frees)
template <typename T>
int grow_scratch(lx_index *h, lxi::DevBuf<T> &b, uint64_t need) {
    if (b.cap() >= need && b) return 0;
    if (b)
        if (int rc = h->hip(hipStreamSynchronize(h->stream), "grow_scratch sync")) return rc;
    return h->hip(b.renew(need), "grow_scratch");
}

// internal entry points shared by lx_index_*.cpp, lx_capi.cpp and lx_fccache.cpp
int lx_fc_args(lx_index *h, uint64_t n, const uint32_t *a, const uint32_t *b, uint8_t *out, uint32_t *partial,
               FcArgs *fa);                     // lx_index_fc.cpp
int flush_pending(lx_index *h);                 // launch the pending small-path run (lx_index_small.cpp)
// slots of the FC cache changed since its device mirror was written
struct Add1Delta {
    uint32_t n;
    uint32_t slot[kAdd1Delta], ev[kAdd1Delta];
    uint8_t tag[kAdd1Delta];
};
int flush_add1_row(lx_index *h, uint32_t a, uint32_t *evk_dev, uint32_t n_slots, uint8_t *tag_dev, uint8_t *out_dev,
                   uint32_t *psum_dev, const Add1Delta *delta);   // 1: not applicable
int rs_begin(lx_index *h, IndexArgs ia, hipStream_t s);   // lx_rowseg.cpp
int rs_planes(lx_index *h, uint32_t n);          // lx_rowseg.cpp: own rows of an n-event epoch
void srv_stop(lx_index *h);   // lx_index_get.cpp: the resident row server leaves
void fcc_destroy(lx_index *h);
void fcc_clear(lx_index *h);                    // Reset: a new epoch
void fcc_forget_from(lx_index *h, uint64_t n);  // DropNotFlushed: events >= n are gone

// between the sources of the handle only (not exported)
#pragma GCC visibility push(hidden)
// lx_index_layout.cpp
void free_all(lx_index *h);                     // a re-layout: every buffer of the old layout goes
int grow_events(lx_index *h, uint64_t need);
int grow_branches(lx_index *h, uint32_t need);
int grow_scap(lx_index *h, uint32_t need);
int grow_local(lx_index *h, uint32_t need);
int ensure_batch(lx_index *h, uint64_t n, uint64_t npar);
int rebuild_columns(lx_index *h);
int la_tail(lx_index *h, hipStream_t s);
int restart_tail(lx_index *h);                  // the LowestAfter tail table starts over
BatchArgs batch_args(lx_index *h, uint32_t n, const uint32_t *creator, const uint32_t *seq, const uint32_t *poff,
                     const uint32_t *par);
IndexArgs index_args(const lx_index *h, uint32_t n, const uint32_t *poff, const uint32_t *par);
UnfillArgs unfill_args(lx_index *h);
// lx_index_add.cpp
int add_batch_dev(lx_index *h, uint32_t n, const uint32_t *creator, const uint32_t *seq, const uint32_t *poff,
                  const uint32_t *par, uint32_t *err_index);
// lx_index_small.cpp
int hm_sync(lx_index *h);
// lx_index_shard.cpp
void shard_bounds(const lx_index *h, uint32_t r, uint32_t *lo, uint32_t *hi);

// Buffers that grow together, `guard` the one whose capacity the caller's check
// reads: emptied first and allocated last, so that a failure on the way leaves
// the check failing again
template <typename G, typename... R>
hipError_t renew_guarded(uint64_t cap, G &guard, R &...rest) {
    guard.reset();
    hipError_t e = hipSuccess;
    (void)((e = rest.renew(cap)) || ...);
    return e ? e : guard.renew(cap);
}

// the timing events of a segmented walk (lx_index_add.cpp, lx_rowseg.cpp)
inline int seg_events(lx_index *h, size_t n) {
    while (h->seg_ev.size() < n) {
        lxi::Event e;
        HIPCHK(h, hipEventCreate(&e.e));
        h->seg_ev.push_back(std::move(e));
    }
    return 0;
}
#pragma GCC visibility pop

// Host-time counters of the small Add path (make hprof: build_hprof/, read by
// lx_host_prof; absent from the default build)
#ifdef LX_HOST_PROF
#include <x86intrin.h>
extern uint64_t g_hprof[16];   // lx_index_small.cpp
#define HP_T(v) const uint64_t v = __rdtsc()
#define HP_ADD(k, t0) (g_hprof[k] += __rdtsc() - (t0))
#define HP_CNT(k, x) (g_hprof[k] += (x))
#else
#define HP_T(v)
#define HP_ADD(k, t0)
#define HP_CNT(k, x)
#endif
