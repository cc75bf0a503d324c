// lx_abft_engine.h -- the state of the batched abft caller (include/lachesis_abft.h)
// and what its three sources share:
//   lx_abft.cpp           epoch start / clear, add and process passes, snapshot, restore, the C API
//   lx_abft_frames.cpp    uploads and readback, the frame-step launcher, frames of a batch,
//                         Build without Add and the progress rounds
//   lx_abft_election.cpp  votes, elections ahead and round by round, blocks, the confirm sweep
// Every device buffer, pinned buffer and event of the engine is owned by a type
// that frees it (lx_devbuf.h): nothing is freed by hand.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/lachesis_abft.h"
#include "lx_devbuf.h"
#include "lx_internal.h"

namespace lxa {

constexpr uint32_t NONE = LX_NONE;
constexpr uint32_t kSpecDepth = 4;      // self-children evaluated ahead per launch (LX_SPEC overrides)
constexpr uint32_t kBuildCap = 100;     // calcFrameIdx: selfParentFrame + 100 in Build
constexpr uint32_t kVoteWindow = 64;    // subjects voted on first (chooseAtropos walks idx order)
constexpr uint32_t kElectAhead = 2;     // rounds per election in run_elections_ahead (3: 72 vote launches, slower)

// Device buffers recycled within one abft handle.  Every device operation of
// the handle is enqueued on the index's stream, so a buffer handed back to the
// pool can be reused by later work on that stream without a host sync (frame
// arrays and vote tables come and go with every decided frame: allocating
// them with hipMalloc / hipFree cost ~6 ms per 50k-event epoch).
using BufPool = lxi::BlockPool<>;
template <typename T>
using DVec = lxi::PoolBuf<T>;

using lxi::Event;   // lx_devbuf.h

inline double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// LX_ABFT_TIMING=1: host wall time between the marks of the batched frame and
// election passes, one line per pass on stderr (diagnostics only)
struct PassTimer {
    const char *name;
    bool on;
    double t0, last;
    std::string out;
    explicit PassTimer(const char *n) : name(n), on(getenv("LX_ABFT_TIMING") != nullptr) {
        if (on) t0 = last = now_ms();
    }
    void mark(const char *what) {
        if (!on) return;
        const double t = now_ms();
        char b[64];
        snprintf(b, sizeof b, " %s=%.3f", what, t - last);
        out += b;
        last = t;
    }
    ~PassTimer() {
        if (on) fprintf(stderr, "abft_timing %s total=%.3f%s\n", name, now_ms() - t0, out.c_str());
    }
};

struct Frame {
    std::vector<uint32_t> ev, creator, dup, bm_len;
    std::vector<uint64_t> bm_off;
    std::vector<uint32_t> last_of;   // creator -> last slot index (for dup)
    uint32_t synced = 0;
    uint32_t voted = 0;              // slots with votes for the current election
    DVec<uint32_t> d_ev, d_creator, d_dup, d_bm_len, votes;
    DVec<uint64_t> d_bm_off;
};

// The host-to-device uploads of one step (frame metadata, candidates,
// cheater columns) go out together: data and descriptors are gathered on the
// host, copied into a pinned, device-mapped staging slot, and one k_scatter
// launch moves them (a hipMemcpyAsync from pageable memory per array cost
// ~10 us each, ~250 per epoch at C5).
struct Uploader {
    static constexpr int kSlots = 4;
    lxi::MappedBuf<uint8_t> pin[kSlots];
    Event done[kSlots];              // recorded behind the slot's k_scatter
    bool used[kSlots] = {};
    int next = 0;
    std::vector<uint8_t> data;
    std::vector<ScatterDesc> desc;
    uint64_t launches = 0;
    void add(void *dst, const void *src, uint64_t bytes) {
        if (!bytes) return;
        const uint64_t off = data.size();
        data.resize(off + (bytes + 15) / 16 * 16);
        memcpy(data.data() + off, src, bytes);
        desc.push_back(ScatterDesc{dst, off, bytes});
    }
    bool pending() const { return !desc.empty(); }
    // a pending upload writes into [p, p + bytes)
    bool targets(const void *p, uint64_t bytes) const {
        const uint8_t *lo = static_cast<const uint8_t *>(p), *hi = lo + bytes;
        for (const ScatterDesc &d : desc) {
            const uint8_t *x = static_cast<const uint8_t *>(d.dst);
            if (x >= lo && x < hi) return true;
        }
        return false;
    }
};

// blocks decided by the last lx_abft_process_batch (option block_log)
struct BlockLog {
    std::vector<uint32_t> frame, atropos, cheaters, cheat_off{0}, confirmed, conf_off{0};
    void clear() {
        frame.clear();
        atropos.clear();
        cheaters.clear();
        confirmed.clear();
        cheat_off.assign(1, 0);
        conf_off.assign(1, 0);
    }
};

}  // namespace lxa

struct lx_abft {
    template <typename T>
    using DVec = lxa::DVec<T>;

    lx_index *ix = nullptr;
    std::string err;
    lx_abft_callbacks cb{};
    bool booted = false;

    uint32_t epoch = 0, V = 0, quorum = 0;
    std::vector<uint32_t> weights;
    uint32_t last_decided = 0;
    uint64_t t_prev = 0;                // event whose processing decided the last frame

    // per event of the epoch (dense index)
    std::vector<uint32_t> ev_frame, ev_sp, ev_confirmed;
    std::vector<uint64_t> par_off{0};
    std::vector<uint32_t> par;

    // ahead of every DVec: members go in reverse order, the pool is drained last
    lxa::BufPool pool;                  // recycled device buffers (all DVecs below)
    lxa::Uploader up;                   // batched host-to-device uploads of a step
    // pinned and device-mapped: k_root_quorum answers; k_readback target
    // (decisions + error word, atropos HB rows)
    lxi::MappedBuf<uint8_t> q_pin;
    lxi::MappedBuf<uint32_t> rb_pin;
    std::vector<lxa::Event> fc_ev;      // pairs around k_root_fc launches (stats.ms_root_fc_gpu)
    uint32_t fc_ev_used = 0;
    std::vector<lxa::Frame> frames;     // [0] unused
    DVec<uint32_t> arena;               // bit rows (observed roots) of k_root_fc launches
    uint64_t arena_used = 0;

    // scratch
    DVec<uint32_t> d_cand, d_psum;
    DVec<unsigned long long> d_dec;
    DVec<uint32_t> d_err;
    DVec<uint32_t> d_kcol, d_kflag, d_kw;
    DVec<uint32_t> ea_votes, ea_err;      // elections decided ahead: vote tables, error words
    DVec<unsigned long long> ea_dec;      // ... decision words per election x subject
    DVec<VoteArgs> ea_args;               // ... launch args, grouped by round
    DVec<RootFcArgs> d_fcargs;            // merged frame steps: per-step args
    DVec<QuorumArgs> d_qargs;
    DVec<ProgressArgs> d_pgargs;          // lx_abft_build_progress / lx_abft_event_progress: per-step args
    // lx_abft_build_frames: the scratch plane of virtual rows, the per-candidate
    // tables, bit rows nobody reads, the NONE list k_root_quorum takes as events
    DVec<uint32_t> b_plane, b_tab, b_bits, b_none;
    DVec<BuildArgs> b_args;             // the tables' pointers as the OWN kernels read them
    uint64_t b_none_n = 0;              // entries of b_none written
    lx_abft_build_stats bstats{};
    // the progress calls: k_root_progress records and pair stakes of one round
    // (pinned, device-mapped), and the pair stakes kept for
    // lx_abft_last_progress_pairs -- rows in the order their candidates stopped
    lxi::MappedBuf<uint4> pg_pin;
    lxi::MappedBuf<uint32_t> pp_pin;
    struct PairEnt {
        uint64_t off;                   // into pp_keep
        uint32_t n, frame;              // slots of the frame asked
    };
    std::vector<PairEnt> pp_ent;        // per entry of the call
    std::vector<uint32_t> pp_keep;
    uint32_t n_k = 0;
    uint64_t k_gen = 0;                 // branch_gen the cheater columns were built for; 0 = stale
    bool dec_dirty = true;
    uint32_t vw = 0;                    // subject window [0, vw) of the current election
    uint32_t spec_depth = lxa::kSpecDepth;
    bool fc16 = true;                   // option fc16=0: k_root_fc (32-bit) even for 16-bit seqs
    bool claimed_batch = true;          // option claimed_batch=0: claimed batches take the Build path's steps
    uint32_t elect_ahead = lxa::kElectAhead;  // option elect_ahead: rounds per election decided ahead (0 = off)
    uint32_t block_log = 0;             // option block_log: without callbacks, log blocks (2: with confirmed events)
    lxa::BlockLog blog;
    std::vector<uint32_t> sweep_atropos, sweep_frame, sweep_label;   // confirmations queued for confirm_sweep

    lx_abft_stats stats{};

    // queued work may still use the buffers: wait before any member is freed
    ~lx_abft() { (void)hipDeviceSynchronize(); }

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
    int ixfail(int rc) {
        err = lx_last_error(ix);
        return rc;
    }
};

#define AHIP(a, expr)                               \
    do {                                            \
        int _rc = (a)->hip((expr), #expr);          \
        if (_rc) return _rc;                        \
    } while (0)
#define ARC(expr)                                   \
    do {                                            \
        int _rc = (expr);                           \
        if (_rc) return _rc;                        \
    } while (0)

namespace lxa {

// ---- lx_abft_frames.cpp
int flush_uploads(lx_abft *a, hipStream_t s);

// v holds n elements, its first `keep` kept; nothing waits (stream-ordered reuse)
template <typename T>
int reserve(lx_abft *a, DVec<T> &v, uint64_t n, uint64_t keep, hipStream_t s) {
    if (n <= v.cap()) return 0;
    if (v && a->up.targets(v, v.bytes())) ARC(flush_uploads(a, s));   // the buffer is about to move
    AHIP(a, v.regrow(a->pool, std::max<uint64_t>({n, v.cap() + v.cap() / 2, 256}), keep, s));
    return 0;
}

template <typename T>
int upload(lx_abft *a, DVec<T> &v, const std::vector<T> &h, uint64_t from, hipStream_t s) {
    ARC(reserve(a, v, h.size(), from, s));
    if (h.size() > from) a->up.add(v + from, h.data() + from, (h.size() - from) * sizeof(T));
    return 0;
}

int readback(lx_abft *a, hipStream_t s, const uint32_t *x, uint32_t na, const uint32_t *y, uint32_t nb,
             const uint32_t **out);
int readback_rows(lx_abft *a, const IndexView &iv, const std::vector<uint32_t> &rows, const uint32_t **out);
Frame &frame_at(lx_abft *a, uint32_t f);
void add_slot(lx_abft *a, uint32_t f, uint32_t e, uint32_t creator, uint64_t bm_off, uint32_t bm_len);
int sync_frame(lx_abft *a, Frame &fr, hipStream_t s);
int q_buffer(lx_abft *a, uint64_t n, hipStream_t s);
int collect_fc_times(lx_abft *a);

// One step of a root-FC launch: cand[0, n_cand) against the first n_roots
// slots of frame `frame`; bit rows (words each) at word row0 of the read-out's
// rows, q answers at q_pin + qoff.  n_cand and words are not 0.
struct FcStep {
    uint32_t frame;
    const uint32_t *cand;
    uint32_t n_cand, n_roots, words;
    uint64_t row0, qoff;
    uint64_t pair0 = 0;   // progress steps that keep the pair stakes: the step's first word
};

// What a set of steps reads, writes and is charged to (launch_fc_steps).
struct StepSet {
    // the candidates' rows: indexed events on the index's HB plane, or row
    // numbers of the scratch plane of lx_abft_build_frames (the OWN kernels)
    enum Rows { kIndex, kScratch } rows = kIndex;
    // the read-out: bit rows into the arena, bit rows into scratch nobody
    // reads, or progress records (k_root_progress in place of k_root_quorum)
    enum Out { kArena, kScratchBits, kProgress } out = kArena;
    // engine: the last batch's stats are charged and k_root_fc is timed; else
    // the build stats are, and nothing of the engine's state is written
    bool engine = true;
    bool by_value = false;           // one step, its kernel arguments by value: nothing uploaded but the candidates
    bool pairs = false;              // kProgress: the pair stakes are kept too (pp_pin)
    bool seq16 = true;               // kScratch: the candidates' own seqs fit 16 bits
    const BuildRowsArgs *first = nullptr;   // kScratch, first round: k_build_rows goes between the uploads and the steps
    PassTimer *pt = nullptr;
};
int launch_fc_steps(lx_abft *a, const IndexView &iv, const std::vector<FcStep> &st, const StepSet &set);

// a claimed batch takes the merged path (compute_frames_claimed, in bounded passes)
bool claimed_path(const lx_abft *a, uint32_t n, const uint32_t *claimed);
int compute_frames(lx_abft *a, uint64_t base, uint32_t n, const uint32_t *creator, const uint32_t *claimed);

// What a progress call wants beyond the frames (lx_abft_build_progress,
// lx_abft_event_progress).  Any out pointer may be NULL.
struct Progress {
    const uint32_t *events;   // lx_abft_event_progress: entry k is indexed event events[k]; NULL: candidates
    const uint32_t *at_frame; // per entry: LX_FRAME_BUILD or the frame to ask; NULL: LX_FRAME_BUILD
    bool pairs;               // LX_PROGRESS_PAIRS
    uint32_t *n_roots, *n_caused, *stake;
    uint64_t *root_stake;
};
int build_frames(lx_abft *a, uint32_t n, const uint32_t *creator, const uint32_t *seq, const uint64_t *poff,
                 const uint32_t *par, uint32_t *out_frame, uint8_t *out_is_root, uint32_t *err_index,
                 const Progress *pg = nullptr);
int event_progress(lx_abft *a, uint32_t n, const uint32_t *ev, uint32_t *out_frame, uint32_t *err_index,
                   const Progress *pg);

// ---- lx_abft_election.cpp
int run_elections(lx_abft *a, uint64_t *sealed_at, std::vector<uint32_t> *new_w);
void confirm_sweep(lx_abft *a);

}  // namespace lxa
