// lx_capi.cpp -- host engine behind the C ABI (include/lachesis_hip.h).
//
// Mirrors the lifecycle of vecfc.Index / vecengine.Engine (Reset, Add, Flush,
// DropNotFlushed, ForklessCause, getters) on top of the device planes of
// lx_internal.h.  Host state is O(branches); all per-event work is on the GPU.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "lx_index.h"

using namespace lxi;

// index handles alive in this process (the row server's option get_server = 1)
static std::atomic<int> g_live_handles{0};

// what outlives every call goes with the handle: the row server, the work on
// its stream, the FC cache; then the members, the stream last (lx_index.h)
lx_index::~lx_index() {
    if (!stream) return;   // lx_create failed before anything could run
    (void)hipSetDevice(device);
    srv_stop(this);
    (void)hipStreamSynchronize(stream);   // (a row-segment rank's walk may still write its rows)
    fcc_destroy(this);
}

// =============================================================================== C ABI
extern "C" {

int lx_create(const lx_config *cfg, lx_index **out) {
    if (!out) return LX_ERR_ARG;
    auto h = std::make_unique<lx_index>();
    if (cfg) {
        h->device = cfg->device;
        h->cap_hint = cfg->event_capacity;
        h->reserve = cfg->branch_reserve;
        h->shard_rank = cfg->shard_rank;
        h->shard_count = cfg->shard_count ? cfg->shard_count : 1;
    }
    if (h->shard_rank >= h->shard_count) return LX_ERR_ARG;
    bool ok = hipSetDevice(h->device) == hipSuccess &&
              hipStreamCreateWithFlags(&h->stream.s, hipStreamNonBlocking) == hipSuccess &&
              h->status.renew(kStatusWords) == hipSuccess && hipMemset(h->status, 0, kStatusWords * 4) == hipSuccess;
    for (auto &e : h->ev) ok = ok && hipEventCreate(&e.e) == hipSuccess;
    for (auto &e : h->st.copied) ok = ok && hipEventCreateWithFlags(&e.e, hipEventDisableTiming) == hipSuccess;
    if (!ok) return LX_ERR_HIP;
#ifdef LX_WALKER_PROF
    if (const char *d = getenv("LX_PROF")) h->prof = (d[0] == '1');   // counters build only (make WPROF=1)
#endif
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device) == hipSuccess && cus > 0)
            h->n_cus = (uint32_t)cus;
    }
    g_live_handles.fetch_add(1, std::memory_order_relaxed);
    *out = h.release();
    return 0;
}

void lx_destroy(lx_index *h) {
    if (!h) return;
    g_live_handles.fetch_sub(1, std::memory_order_relaxed);
    delete h;
}

const char *lx_last_error(const lx_index *h) { return h ? h->err.c_str() : "null handle"; }

int lx_last_walk_clock(lx_index *h, float out[20]) {
    if (!h || !out) return LX_ERR_ARG;
    for (int i = 0; i < 20; i++) out[i] = 0.0f;
    if (!h->d_clk) return 0;
    HIPCHK(h, set_dev(h->device));
    std::vector<unsigned long long> v(1 + 3ull * kClkBlocks);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(v.data(), h->d_clk, v.size() * 8, hipMemcpyDeviceToHost));
    std::vector<float> mhz, ms, xm[8], xt[8];
    const uint64_t g = std::min<uint64_t>(v[0], kClkBlocks);
    for (uint64_t b = 0; b < g; b++) {
        const unsigned long long cyc = v[1 + 3 * b], tick = v[2 + 3 * b], xcc = v[3 + 3 * b];
        if (!tick || !cyc) continue;   // a workgroup without a walk (rounding, or none of the columns)
        const float f = (float)((double)cyc / (double)tick * 100.0), t = (float)((double)tick / 1e5);
        mhz.push_back(f);
        ms.push_back(t);
        if (xcc < 8) {
            xm[xcc].push_back(f);
            xt[xcc].push_back(t);
        }
    }
    if (mhz.empty()) return 0;
    auto med = [](std::vector<float> &x) {
        std::sort(x.begin(), x.end());
        return x.empty() ? 0.0f : x[x.size() / 2];
    };
    out[0] = med(mhz);
    out[1] = mhz.front();
    out[2] = mhz.back();
    out[3] = med(ms);
    for (int x = 0; x < 8; x++) {
        out[4 + x] = med(xm[x]);
        std::sort(xt[x].begin(), xt[x].end());
        out[12 + x] = xt[x].empty() ? 0.0f : xt[x].back();
    }
    return 0;
}

int lx_set_option(lx_index *h, const char *name, int64_t value) {
    if (!h || !name) return LX_ERR_ARG;
    const std::string k(name);
    if (k == "small_max") {
        if (value < 0) return h->fail(LX_ERR_ARG, "small_max < 0");
        h->small_max = (uint32_t)std::min<int64_t>(value, kSmallMaxN);
    } else if (k == "fc_fk") {
        h->fc_fk = value != 0;
    } else if (k == "fc_early") {
        h->fc_early = value != 0;
    } else if (k == "fc_early_forks") {
        if (value != 0 && value != 1) return h->fail(LX_ERR_ARG, "fc_early_forks must be 0 or 1");
        h->fc_early_forks = value != 0;
    } else if (k == "fc_early_lanes") {
        if (value != 16 && value != 32) return h->fail(LX_ERR_ARG, "fc_early_lanes must be 16 or 32");
        h->fc_early_lanes = (uint32_t)value;
    } else if (k == "cpw") {
        if (value != 0 && value != 1 && value != 2 && value != 4 && value != 8 && value != 12)
            return h->fail(LX_ERR_ARG, "cpw must be 0, 1, 2, 4, 8 or 12 (8, 12: fork-free epochs with seqs <= 0xFFFF)");
        h->cpw_hint = (uint32_t)value;
    } else if (k == "pack16") {
        h->pack16 = value != 0;
    } else if (k == "fold3") {
        h->fold3 = value != 0;
    } else if (k == "crec") {
        h->crec_opt = value != 0;
    } else if (k == "seg_xmap") {
        h->seg_xmap_opt = value != 0;
    } else if (k == "realloc_records") {
        // diagnostics (walk slow-mode probe): move the batch's record buffers
        // to a fresh allocation now (the new one taken before the old is freed)
        if (value) {
            HIPCHK(h, set_dev(h->device));
            HIPCHK(h, hipStreamSynchronize(h->stream));
            const uint64_t n = (h->lay.batch_cap + 63) / 64 * 64;
            auto move = [&](auto &b) -> int {
                if (!b) return 0;
                std::remove_reference_t<decltype(b)> nb;
                HIPCHK(h, nb.renew(n));
                b = std::move(nb);
                return 0;
            };
            if (int rc = move(h->lay.b_rec)) return rc;
            if (int rc = move(h->lay.b_crec)) return rc;
        }
    } else if (k == "dbl") {
        h->dbl = value != 0;
    } else if (k == "seg_auto") {
        h->seg_auto = value != 0;
    } else if (k == "la_memset") {
        if (h->have_epoch) return h->fail(LX_ERR_STATE, "la_memset must be set before lx_reset");
        h->la_tail = value == 0;
    } else if (k == "shard_wire") {
        if (value != 0 && value != 2 && value != 4) return h->fail(LX_ERR_ARG, "shard_wire must be 0, 2 or 4");
        h->wire_force = (uint32_t)value;
    } else if (k == "timing") {
        h->small_timing = value != 0;
    } else if (k == "seg_count" || k == "seg_rank") {
        if (h->have_epoch) return h->fail(LX_ERR_STATE, "%s must be set before lx_reset", name);
        if (h->sharded()) return h->fail(LX_ERR_STATE, "row segments on a column shard");
        if (value < 0 || value > (int64_t)kMaxSegments) return h->fail(LX_ERR_ARG, "%s must be 0..%u", name, kMaxSegments);
        (k == "seg_count" ? h->rs_count : h->rs_rank) = (uint32_t)value;
    } else if (k == "segments") {
        if (value < 0 || value > (int64_t)kMaxSegments) return h->fail(LX_ERR_ARG, "segments must be 0..%u", kMaxSegments);
        if (value > 1 && h->sharded()) return h->fail(LX_ERR_STATE, "segments on a column shard");
        h->segments = (uint32_t)value;
    } else if (k == "seg_sub") {
        // row-segment ranks: sub-segments each rank walks side by side (0: auto);
        // every rank of a job must use the same value
        if (value < 0 || value > (int64_t)kSegLaunchMax) return h->fail(LX_ERR_ARG, "seg_sub must be 0..%u", kSegLaunchMax);
        h->rs_sub_opt = (uint32_t)value;
    } else if (k == "get_server") {
        // single-row getters through the resident row server (default 1)
        if (value < 0 || value > 2) return h->fail(LX_ERR_ARG, "get_server must be 0, 1 (auto) or 2");
        h->srv.opt = (int)value;
        if (!h->srv.opt) srv_stop(h);
    } else if (k == "getter_host_check") {
        // 0 (tests only): getters skip the host's event check, so an unknown
        // event reaches the row kernel's / row server's own bound
        h->get_host_check = value != 0;
    } else if (k == "fc_cache") {
        if (value < 0 || value > 16384) return h->fail(LX_ERR_ARG, "fc_cache must be 0..16384");
        fcc_destroy(h);
        h->fcc_slots = value ? round_up((uint32_t)value, 64) : 0;
        h->fcc_slots_set = true;
    } else {
        return h->fail(LX_ERR_ARG, "unknown option %s", name);
    }
    return 0;
}

int lx_reset(lx_index *h, uint32_t nv, const uint32_t *w) {
    if (!h || (nv && !w)) return LX_ERR_ARG;
    if (nv == 0) return h->fail(LX_ERR_ARG, "empty validator set");
    uint64_t tot = 0;
    for (uint32_t i = 0; i < nv; i++) {
        if (w[i] == 0) return h->fail(LX_ERR_ARG, "zero weight at idx %u (builder drops such validators)", i);
        tot += w[i];
    }
    if (tot > 0x7FFFFFFFull) return h->fail(LX_ERR_ARG, "validators weight overflow");   // validators.go:101-110
    HIPCHK(h, set_dev(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->pend.n = 0;     // a pending run of the old epoch is simply forgotten
    h->wb.ready = false;
    h->V = nv;
    h->weights.assign(w, w + nv);
    h->quorum = (uint32_t)(tot * 2 / 3 + 1);
    shard_bounds(h, h->shard_rank, &h->own_lo, &h->own_hi);
    h->sc.events = ~0ull;
    h->sx.full = true;      // a new epoch: the next LowestAfter exchange is whole
    h->sx.active = false;
    uint32_t reserve = h->reserve ? h->reserve : std::max<uint32_t>(64, nv / 16);
    uint32_t want_stride = round_up(nv + reserve, 64);
    // a shard stores its own columns: originals + a share of the fork reserve
    const uint32_t norig = h->own_hi - h->own_lo;
    const uint32_t want_p = h->sharded() ? round_up(norig + std::max<uint32_t>(16, reserve / h->shard_count), 16)
                                         : want_stride;
    // (re)allocate when the layout changes; otherwise zero what the last epoch used
    if (want_stride > h->stride || (h->stride && want_stride * 2 < h->stride) || want_p > h->pstride ||
        (h->pstride && want_p * 2 < h->pstride)) {
        free_all(h);
        h->stride = 0;
        int rc;
        h->s_cap = 0;
        h->pstride = h->sharded() ? want_p : 0;
        if ((rc = grow_branches(h, want_stride))) return rc;
        if (h->sharded()) HIPCHK(h, h->lay.wloc.renew(h->pstride));
        uint32_t s0 = 1024;
        if (h->cap_hint) s0 = (uint32_t)std::min<uint64_t>(h->cap_hint / nv + 64, 0x7FFFFFFF);
        if ((rc = grow_scap(h, s0))) return rc;
        h->hwm = 0;
        if ((rc = grow_events(h, h->cap_hint ? h->cap_hint : 4096))) return rc;
    } else if (h->hwm && h->rowseg()) {
        // a row-segment rank: its own rows are rewritten (HB by the walk and the
        // fix-up, LA zeroed at the batch, rs_begin); only the metadata resets
        HIPCHK(h, lx::launch_fill_u32(h->lay.first_child, h->hwm, LX_NONE, h->stream));
        h->hwm = 0;
    } else if (h->hwm) {
        // HB: the walker rewrites the original columns of every new event's row
        // (the original branches always exist); only the fork-branch columns can
        // keep stale values for rows written before such a branch existed
        // (only columns some row may have written: a previous epoch's originals
        // or fork branches beyond this epoch's originals)
        const uint32_t no = h->sharded() ? norig : nv;
        const uint32_t used = std::min(h->pcols_used, h->pstride);
        if (used > no)
            HIPCHK(h, hipMemset2DAsync(h->lay.hb + no, (size_t)h->pstride * 4, 0, (size_t)(used - no) * 4, h->hwm,
                                       h->stream));
        // a shard's query plane is rewritten whole by the exchange (full blocks,
        // zeros included) before any ForklessCause: only its fill target needs zeroing
        if (h->lay.lap) {
            HIPCHK(h, hipMemsetAsync(h->lay.lap, 0, (uint64_t)h->pstride * h->s_cap * h->stride * 4, h->stream));
        } else if (h->la_tail) {
            // every entry (x, j < B) of a row is rewritten after its batch (fill or
            // tail, la_tail): only fork-branch columns of old rows need zeroing
            if (used > no)
                HIPCHK(h, hipMemset2DAsync(h->lay.la + no, (size_t)h->pstride * 4, 0, (size_t)(used - no) * 4, h->hwm,
                                           h->stream));
            if (int rc = restart_tail(h)) return rc;
        } else {
            HIPCHK(h, hipMemsetAsync(h->lay.la, 0, h->hwm * h->pstride * 4, h->stream));
        }
        HIPCHK(h, lx::launch_fill_u32(h->lay.first_child, h->hwm, LX_NONE, h->stream));
        h->hwm = 0;
    }
    if (h->sharded()) {
        h->h_cmap.assign(nv, LX_NONE);
        for (uint32_t c = h->own_lo; c < h->own_hi; c++) h->h_cmap[c] = c - h->own_lo;
        h->nloc = norig;
        std::vector<uint32_t> wl(h->pstride, 0);
        for (uint32_t c = h->own_lo; c < h->own_hi; c++) wl[c - h->own_lo] = w[c];
        HIPCHK(h, hipMemcpyAsync(h->lay.wloc, wl.data(), (uint64_t)h->pstride * 4, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, lx::launch_fill_u32(h->lay.cmap, h->lay.cmap.cap(), LX_NONE, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->lay.cmap, h->h_cmap.data(), nv * 4ull, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    HIPCHK(h, h->lay.first_root.renew(nv));
    HIPCHK(h, lx::launch_fill_u32(h->lay.first_root, nv, LX_NONE, h->stream));
    std::vector<uint32_t> ones(nv, 1), idx(nv), wp(h->stride, 0);
    for (uint32_t i = 0; i < nv; i++) idx[i] = i;
    for (uint32_t i = h->own_lo; i < h->own_hi; i++) wp[i] = w[i];
    HIPCHK(h, hipMemsetAsync(h->lay.branch_len, 0, (uint64_t)h->stride * 4, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->lay.branch_first, ones.data(), nv * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->lay.branch_creator, idx.data(), nv * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->lay.wpad, wp.data(), (uint64_t)h->stride * 4, hipMemcpyHostToDevice, h->stream));
    h->n_events = h->n_flushed = 0;
    h->rolled_epoch();
    h->rs_state = 0;
    h->pcols_used = h->sharded() ? norig : nv;
    h->B = h->B_flushed = nv;
    h->max_seq = 0;
    h->h_branch_creator = idx;
    h->h_branch_first = ones;
    h->by_creator.assign(nv, {});
    for (uint32_t i = 0; i < nv; i++) h->by_creator[i].push_back(i);
    h->hm.ok = true;
    h->hm.n = 0;
    for (auto *v : {&h->hm.creator, &h->hm.seq, &h->hm.branch, &h->hm.bbefore}) v->clear();
    h->hm.blen.assign(nv, 0);
    h->stats_lazy = false;
    h->loading = false;
    h->have_epoch = true;
    if (!h->fcc_slots_set) {
        // two frames of roots (C5, V = 1000: 2048 slots miss as often as 4032 and
        // fill rows half as long; profiles/r03/dropin)
        const uint32_t w = std::min<uint32_t>(8192, std::max<uint32_t>(512, round_up(2 * nv, 64)));
        if (w != h->fcc_slots) fcc_destroy(h);
        h->fcc_slots = w;
    }
    fcc_clear(h);
    h->ncols = 0;
    return rebuild_columns(h);
}

int lx_flush(lx_index *h) {
    if (!h) return LX_ERR_ARG;
    NOT_LOADING(h);
    h->wb.ready = false;
    h->n_flushed = h->n_events;
    h->B_flushed = h->B;
    return 0;
}

int lx_drop_not_flushed(lx_index *h) {
    if (!h) return LX_ERR_ARG;
    NOT_LOADING(h);
    WHOLE_INDEX(h);
    if (!h->have_epoch) return 0;
    HIPCHK(h, set_dev(h->device));
    h->wb.ready = false;
    if (h->n_events == h->n_flushed && h->B == h->B_flushed) return 0;
    h->rolled_back(h->n_flushed);
    if (h->pend.n && h->n_flushed >= h->pend.bs) {
        // every dropped event is still in the pending run: it never reached the
        // device, so the rollback is host-only (Build = Add + DropNotFlushed
        // costs no launch)
        const uint32_t keep = (uint32_t)(h->n_flushed - h->pend.bs);
        h->pend.old.resize(h->pend.ev[keep].q1.x);
        h->pend.pl.resize(4ull * h->pend.meta[keep].y);
        h->pend.ev.resize(keep);
        h->pend.lvl.resize(keep);
        h->pend.meta.resize(keep);
        h->pend.maxlvl = 0;
        h->pend.nh = 0;
        h->pend.npar = 0;
        for (uint32_t i = 0; i < keep; i++) {
            SmallEv &e = h->pend.ev[i];
            if (e.q2.z != LX_NONE && e.q2.z >= h->n_flushed) e.q2.z = LX_NONE;
            if (e.q2.w != LX_NONE) h->pend.nh = e.q2.w + 1;
            h->pend.npar += e.q0.w;
            h->pend.maxlvl = std::max(h->pend.maxlvl, h->pend.lvl[i]);
        }
        h->pend.n = keep;
    } else {
        int rc;
        if ((rc = flush_pending(h))) return rc;
        HIPCHK(h, lx::launch_unfill(unfill_args(h), h->stream));
        HIPCHK(h, lx::launch_zero_rows(h->lay.hb, h->lay.la, h->pstride, (uint32_t)h->n_flushed, (uint32_t)h->n_events,
                                       h->stream));
        // re-added events may land on rows this epoch has not used yet (stale from an
        // earlier epoch) with seqs the tail table already counts as done: start over
        if ((rc = restart_tail(h))) return rc;
    }
    // host mirror: the same rollback of the branch lengths (k_unclaim) and rows
    if (h->hm.ok) {
        for (uint64_t e = h->n_flushed; e < h->n_events; e++) {
            const uint32_t br = h->hm.branch[e];
            if (br < h->B_flushed) h->hm.blen[br] = std::min(h->hm.blen[br], h->hm.seq[e] - h->h_branch_first[br]);
        }
        h->hm.blen.resize(h->B_flushed);
        for (auto *v : {&h->hm.creator, &h->hm.seq, &h->hm.branch, &h->hm.bbefore}) v->resize(h->n_flushed);
    }
    h->hm.n = std::min(h->hm.n, h->n_flushed);
    h->n_events = h->n_flushed;
    fcc_forget_from(h, h->n_flushed);
    h->sx.full = true;      // receivers may hold entries of the dropped events
    h->sx.active = false;
    if (h->B != h->B_flushed) {
        h->B = h->B_flushed;
        h->h_branch_creator.resize(h->B);
        h->h_branch_first.resize(h->B);
        for (auto &l : h->by_creator)
            while (!l.empty() && l.back() >= h->B) l.pop_back();
        if (h->sharded()) {
            // dropped fork columns: their plane columns were zeroed with the rows
            // that used them (rows > n_flushed); older rows never saw them
            for (uint32_t b = h->B; b < h->h_cmap.size(); b++)
                if (h->h_cmap[b] != LX_NONE) h->nloc--;
            h->h_cmap.resize(h->B);
            HIPCHK(h, lx::launch_fill_u32(h->lay.cmap + h->B, h->lay.cmap.cap() - h->B, LX_NONE, h->stream));
        }
        return rebuild_columns(h);
    }
    return 0;
}

uint64_t lx_num_events(const lx_index *h) { return h ? h->n_events : 0; }
uint32_t lx_num_branches(const lx_index *h) { return h ? h->B : 0; }
int lx_at_least_one_fork(const lx_index *h) { return h && h->B > h->V; }
uint32_t lx_quorum(const lx_index *h) { return h ? h->quorum : 0; }

int lx_live_handles(void) { return g_live_handles.load(std::memory_order_relaxed); }

int lx_last_stats(const lx_index *h, lx_stats *out) {
    if (!h || !out) return LX_ERR_ARG;
    *out = h->stats;
    if (h->stats_lazy) {
        // small path: the launch is timed by ev[1..2]; wait for it only when asked
        float t = 0;
        if (hipEventSynchronize(h->ev[2]) == hipSuccess && hipEventElapsedTime(&t, h->ev[1], h->ev[2]) == hipSuccess)
            out->ms_index = t;
    }
    return 0;
}

int lx_device_planes(lx_index *h, void **hb, void **la, uint32_t *stride, void **stream) {
    if (!h) return LX_ERR_ARG;
    HIPCHK(h, set_dev(h->device));
    {
        const int rc = flush_pending(h);   // the caller reads the planes in stream order after this
        if (rc) return rc;
    }
    if (hb) *hb = h->lay.hb;
    if (la) *la = h->lay.la;
    if (stride) *stride = h->pstride;
    if (stream) *stream = (hipStream_t)h->stream;
    return 0;
}

int lx_device_bytes(const lx_index *h, uint64_t out[4]) {
    if (!h || !out) return LX_ERR_ARG;
    const Layout &l = h->lay;
    const uint64_t ps = h->pstride;
    uint64_t planes = h->rowseg() ? 2 * l.rs_mem_rows * ps * 4 : (l.hb ? 2 * h->n_cap * ps * 4 : 0);
    if (l.lap) planes += (uint64_t)h->pstride * h->s_cap * h->stride * 4;
    const uint64_t recv = 4 * (l.rs_rhb.cap() + l.rs_rla.cap());
    uint64_t per_ev = 6 * 4 * h->n_cap;   // creator, seq, branch, bbefore, sp, first_child
    for (const DU32 *b : {&l.seg_mf, &l.seg_plist, &l.seg_elist, &l.rs_need, &l.rs_hslot, &l.rs_lslot, &l.rs_stamp,
                          &l.wb_flag})
        per_ev += b->bytes();
    uint64_t other = 4 * ((uint64_t)h->stride * h->s_cap + 5ull * h->stride + l.tail_cap() * (uint64_t)l.tail_cap() * 2);
    other += 4 * (8 * l.batch_cap + l.b_par.cap() + 2 * l.q_a.cap()) + l.q_a.cap() + 16 * l.batch_cap;
    for (const DU32 *b : {&l.rs_req, &l.rs_ids, &l.rs_out, &l.rs_send, &l.rsq_scratch, &l.rsq_list}) other += b->bytes();
    other += l.rsq_tmp.bytes() + l.scan_tmp.bytes();
    out[0] = planes;
    out[1] = recv;
    out[2] = per_ev;
    out[3] = other;
    return 0;
}

int lx_last_segment_stats(const lx_index *h, lx_seg_stats *out) {
    if (!h || !out) return LX_ERR_ARG;
    *out = h->seg_stats;
    return 0;
}

int lx_sync(lx_index *h) {
    if (!h) return LX_ERR_ARG;
    HIPCHK(h, set_dev(h->device));
    {
        const int rc = flush_pending(h);
        if (rc) return rc;
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    // the unknown-event flag of asynchronous ForklessCause batches: read only
    // when one ran since the last check (a blocking 4-byte copy costs ~10 us,
    // the whole of an Add-and-sync otherwise)
    if (!h->fc_unchecked) return 0;
    h->fc_unchecked = false;
    uint32_t bad = 0;
    HIPCHK(h, hipMemcpy(&bad, h->status + 1, 4, hipMemcpyDeviceToHost));
    if (bad) {
        HIPCHK(h, hipMemset(h->status + 1, 0, 4));
        return h->fail(LX_ERR_ARG, "ForklessCause on an unknown event");
    }
    return 0;
}

}  // extern "C"

// view for the abft engine (lx_abft_engine.h); see lx_internal.h
int lx_index_view(lx_index *h, IndexView *o) {
    if (!h || !o) return LX_ERR_ARG;
    WHOLE_INDEX(h);
    if (!h->have_epoch) return h->fail(LX_ERR_STATE, "index has no epoch (lx_reset first)");
    {
        const int rc = flush_pending(h);   // abft and the emitter enqueue after the index's work
        if (rc) return rc;
    }
    return lx_index_peek(h, o);
}

uint64_t lx_index_kept_since(const lx_index *h, uint64_t gen) {
    if (gen < h->epoch_gen) return 0;
    uint64_t keep = ~0ull;
    for (uint64_t k = gen - h->epoch_gen; k < h->roll_keep.size(); k++) keep = std::min(keep, h->roll_keep[k]);
    return keep;
}

int lx_index_peek(lx_index *h, IndexView *o) {
    if (!h || !o) return LX_ERR_ARG;
    WHOLE_INDEX(h);
    if (!h->have_epoch) return h->fail(LX_ERR_STATE, "index has no epoch (lx_reset first)");
    o->stream = h->stream;
    o->device = h->device;
    o->hb = h->lay.hb;
    o->la = h->lay.la;
    o->stride = h->pstride;
    o->n_events = h->n_events;
    o->n_flushed = h->n_flushed;
    o->epoch_gen = h->epoch_gen;
    o->roll_gen = h->roll_gen;
    o->V = h->V;
    o->B = h->B;
    o->branch_gen = h->branch_gen;
    o->quorum = h->quorum;
    o->max_seq = h->max_seq;
    o->wpad = h->lay.wpad;
    o->ev_branch = h->lay.ev_branch;
    o->ev_seq = h->lay.ev_seq;
    o->ev_creator = h->lay.ev_creator;
    o->brow = h->lay.brow;
    o->branch_first = h->lay.branch_first;
    o->s_cap = h->s_cap;
    o->cheat_of = h->lay.cheat_of;
    o->cheat_off = h->lay.cheat_off;
    o->cheat_br = h->lay.cheat_br;
    o->cheat_creator = h->lay.cheat_creator;
    o->n_cheat = h->n_cheat;
    o->branch_len = h->lay.branch_len;
    o->weights = &h->weights;
    o->by_creator = &h->by_creator;
    o->shard_count = h->shard_count;
    o->loading = h->loading;
    return 0;
}

// the host mirror of the per-event metadata (hm_sync: waits for the stream only
// after batches the device assigned); see lx_internal.h
int lx_index_host_meta(lx_index *h, IndexHostMeta *o) {
    if (!h || !o) return LX_ERR_ARG;
    WHOLE_INDEX(h);
    if (!h->have_epoch) return h->fail(LX_ERR_STATE, "index has no epoch (lx_reset first)");
    HIPCHK(h, set_dev(h->device));
    const int rc = hm_sync(h);
    if (rc) return rc;
    o->ev_creator = h->hm.creator.data();
    o->ev_seq = h->hm.seq.data();
    o->ev_branch = h->hm.branch.data();
    o->branch_len = h->hm.blen.data();
    o->branch_first = h->h_branch_first.data();
    return 0;
}
