// strsim_capi.cpp -- the thin kernel ABI of include/strsim_amd.h: contexts, workspace, launch, timing.
//
// Host-side counterpart of the row loop in the reference's `parallel_apply`
// (reference src/expressions/strsim.rs:41-107): shape rule, literal broadcast, row partition.
// There is no CPU compute path in this library: without a HIP device every compute call fails.
#include <hip/hip_runtime.h>
#include <algorithm>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>

#include "strsim_amd.h"
#include "strsim_internal.h"
#include "strsim_kernels.h"
#define STRSIM_OSA_NO_KERNELS // (constants and sizes only: the kernels are compiled in strsim_kernels.hip)
#include "strsim_osa.h"
#include "strsim_distance.h"
#include "strsim_indel.h"
#include "strsim_qgram.h"
#include "strsim_damerau.h"
#include "strsim_common.h"
#include "strsim_partial.h"
#include "strsim_token.h"
#include "strsim_wratio.h"
#include "strsim_process.h"
#include "strsim_nearest.h"
#include "strsim_extract.h"
#include "strsim_cdist.h"
#include "strsim_join.h"
#include "strsim_match_join.h"
#include "strsim_qgram_join.h"
#include "strsim_distance_join.h"
#include "strsim_components.h"

namespace strsim {

static thread_local std::string g_last_error;

void set_error(const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
}

int hip_fail(hipError_t e, const char *what)
{
    set_error("HIP error in %s: %s (%d)", what, hipGetErrorString(e), (int)e);
    if (e == hipErrorOutOfMemory) return STRSIM_ERR_OOM;
    if (e == hipErrorNoDevice || e == hipErrorInvalidDevice) return STRSIM_ERR_NO_DEVICE;
    return STRSIM_ERR_HIP;
}

#define HIP_TRY(expr)                                          \
    do {                                                       \
        hipError_t e__ = (expr);                               \
        if (e__ != hipSuccess) return hip_fail(e__, #expr);    \
    } while (0)

} // namespace strsim

using namespace strsim;

// A grow-only device buffer: what a call needs is reserved before it is enqueued; a buffer that is too small is freed first and
// allocated again with an eighth to spare.  Freed with the context.
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0; // bytes
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    int reserve(size_t bytes)
    {
        if (bytes <= cap) return STRSIM_OK;
        if (p) { HIP_TRY(hipFree(p)); p = nullptr; cap = 0; }
        const size_t want = bytes + bytes / 8 + 256;
        HIP_TRY(hipMalloc(&p, want));
        cap = want;
        return STRSIM_OK;
    }
    template <class T> T *as() const { return static_cast<T *>(p); }
};

// The fields are grouped by the functions that own them; strsim_ctx_destroy releases them in this order (the DevBufs free
// themselves when the context is deleted).
struct strsim_ctx {
    int device = -1;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int num_cu = 0;

    // ---- ring of pending calls and their status blocks (slot_begin / slot_commit, ctx_retire_slot, ctx_drain) ----
    // per-call deferred state: a ring of status words + event triples, so calls can be enqueued
    // back to back without a host sync; the ring is drained by strsim_ctx_synchronize()
    static constexpr int RING = 32;
    int head = 0;
    bool slot_pending[RING] = {};
    // A call whose lane kernel is EXPECTED to leave nothing behind (the last retired call did not: short ASCII columns) is
    // ONE kernel launch: k_lane_stage's last workgroup publishes lane_left and the ticket itself.  If it did leave rows, the
    // slow-row kernels are launched when the call is retired (strsim_ctx_synchronize / strsim_ctx_retire_oldest) -- like
    // the long-string pass -- and the next calls enqueue the whole chain up front again.
    bool slot_deferred[RING] = {};
    bool slot_timed[RING] = {};
    LaunchArgs slot_args[RING] = {}; // what each pending call was launched with (for the long-string pass)
    int slot_measure[RING] = {};     // STRSIM_NUM_MEASURES = the fused all-measures call
    double *slot_outs[RING][5] = {};
    uint32_t slot_ticket[RING] = {}; // what the device writes into status_host[slot].ticket when the call's status block is out
    uint32_t ticket_seq = 0;
    DevStatus *status = nullptr;      // device, RING entries
    uint32_t *sched = nullptr;        // device, RING x 4 words: work-distribution counters of k_lane_stage (zero between launches)
    DevStatus *status_host = nullptr; // pinned, RING entries
    DevStatus *status_host_dev = nullptr; // the same memory as the device addresses it
    bool expect_slow = false;
    bool long_rows = false;        // ... and left more than 1/16 of its rows: frames of long strings (see k_lane_stage, TABLES)
    bool stream_ordered = true;    // strsim_ctx_set_stream_ordered(ctx, 0) opts in to one-launch calls
    uint64_t enqueued_ops = 0;     // kernels + copies this context has put on its stream for pair calls (strsim_ctx_enqueued_ops)
    uint64_t last_wave_rows = 0;
    uint64_t last_long_rows = 0;   // over the slots retired by the last synchronize
    uint64_t last_late_rows = 0;   // rows finished by a pass launched from synchronize / retire (deferred + long-string)
    uint64_t carry_late_rows = 0, carry_long_rows = 0; // the same of calls the library had to retire itself (the ring of status
                                   // slots wrapped): reported with the caller's next strsim_ctx_synchronize / _retire_oldest

    // ---- workspaces of the pairwise calls (pairs_device_impl, ctx_run_huge, strsim_pairs_host; all grow-only) ----
    // The "not finished yet" masks (+ backup + work list) of a call.  A call whose slow-row kernels may be
    // launched late (a one-launch call, above) needs its mask intact while younger calls run: it OWNS one of the first RING
    // buffers (the lowest free one; allocated on first use, so a caller that keeps k calls in flight touches k of them) until it is
    // retired.  Calls that enqueue all their kernels up front share the last buffer (they use it in stream order).  Nothing is ever
    // retired behind the caller's back to make room: a buffer is always free while a ring slot is.
    static constexpr int MASKBUFS = RING + 1;
    static constexpr int SHARED_MASKBUF = MASKBUFS - 1;
    DevBuf slowmask[MASKBUFS];
    int maskbuf_owner[MASKBUFS];     // ring slot of the pending one-launch call that owns the buffer, or -1 (set in strsim_ctx_create)
    DevBuf lev_ws;                   // scratch of k_wave_pairs<LEVENSHTEIN>: staged texts + non-ASCII fallback arrays
    DevBuf huge_ws;                  // workspace of the long-string pass
    double *qtab = nullptr;          // QTAB_N x QTAB_N quotients a / b (strsim_lane_core.h), filled at creation
    uint32_t *scan_ws = nullptr;     // block sums of strsim_offsets_from_lengths (SCAN_WS_WORDS, allocated on first use)
    DevBuf stage[5];                 // device copies of a *_host call's four input buffers and its outputs (ctx_stage)
    void *pin = nullptr;   // pinned staging of strsim_pairs_host's small calls (kernels work on it in place)
    void *pin_dev = nullptr;
    size_t pin_cap = 0;

    // ---- timing (strsim_ctx_timing_enable / _read) ----
    bool timing = false;
    double lane_ms = 0, wave_ms = 0;
    uint64_t lane_launches = 0, wave_launches = 0;
    hipEvent_t ev[RING][3] = {};
    hipEvent_t ev_late[2] = {};    // timing of a deferred slow pass

    // ---- environment knobs, read ONCE in strsim_ctx_create (not on the launch path: a small call is ~23 us, and a host that
    // calls setenv concurrently must not race a getenv of ours per call) ----
    int stage_wg_per_cu = 5;  // resident workgroups of k_lane_stage per CU; STRSIM_STAGE_WG_PER_CU overrides (tuning knob)
    int lev_waves_per_cu = 20; // five per SIMD (96 VGPRs, 7.6 KB of LDS = six 1 280-byte granules); STRSIM_LEV_WAVES_PER_CU overrides (tuning knob)
    bool no_literal_path = false;      // STRSIM_NO_LITERAL_PATH (tuning / A-B knob)
    int wide_cap_per_cu = 192;         // STRSIM_WIDE_WG_PER_CU (tuning knob)
    int huge_waves_per_cu = 16;        // STRSIM_HUGE_WAVES_PER_CU (tuning knob); 8 KB of LDS per Levenshtein wave
    uint64_t host_direct_rows = 65536; // STRSIM_HOST_DIRECT_ROWS=0 switches strsim_pairs_host's in-place path off (tests do)
    // fault injection (tests only): the k-th slot retirement of this context fails with STRSIM_ERR_INTERNAL -- the one way to see
    // STRSIM_ERR_EARLIER_CALL and the "a slot is retired whatever fails" rule without breaking the device
    uint64_t fault_retire_at = 0;      // STRSIM_FAULT_RETIRE_AT (0 = never)
    uint64_t retired = 0;

    // ---- search calls (search_pack / slow_walk / search_fallback_merge; strsim_best_match_device, strsim_nearest_device) ----
    // packed strings + slow lists + partial lists (nearest: also the length order and the merged scores), the fallback's score
    // (nearest: and distance) batches, and a pinned word pair for the two slow counts
    DevBuf match_ws, match_scratch;
    DevBuf nearest_ws, nearest_scratch;
    uint32_t *match_counts_host = nullptr;
    // strsim_extract_device: its workspace and fallback batches, the device copy of the rank table (extract_table) and, for
    // STRSIM_TOKEN_SORT_RATIO, the normalised columns -- buffers of its own, so that the pairwise calls of the fallback (which
    // may use any scratch of the pairwise flows) can neither reuse nor grow over them
    DevBuf extract_ws, extract_scratch, extract_tab;
    bool extract_tab_ready = false;
    DevBuf extract_off[2], extract_val[2];
    // strsim_cdist_device: the packed strings and slow lists, the fallback's score columns and the device copy of the Indel score
    // table (strsim_cdist.h) -- buffers of its own, for the same reason; scorer 14 normalises into extract_off / extract_val,
    // which no flow inside a cdist call uses
    DevBuf cdist_ws, cdist_scratch, cdist_tab;
    bool cdist_tab_ready = false;
    // strsim_join_device: the packed strings, slow lists, length order, counts and cursors, and the fallback's score columns --
    // buffers of its own, for the same reason; it reads extract_tab (the rank table, never rewritten) and scorer 14 normalises into
    // extract_off / extract_val, which no flow inside a join call uses
    DevBuf join_ws, join_scratch;
    // strsim_qgram_join_device in set mode: one word per candidate in length order (its first occurrences, strsim_qgram_join.h)
    DevBuf qgram_join_first;
    // strsim_distance_join_device: the hits' f64 values -(double)d until the finishing kernel has written the caller's uint32 column,
    // and one uint32 column of the fallback's pairwise distances (strsim_distance_join.h)
    DevBuf distance_join_score, distance_join_col;
    // strsim_components_device: parent[], the root flags and their scan, and the status words {count, indices out of range} with
    // their pinned read-back; strsim_cluster_device: the CSR of its self-join, which never reaches the host -- buffers of their own,
    // for the same reason (the join inside a cluster call uses every buffer above freely)
    DevBuf components_ws, cluster_pairs;
    uint64_t *components_host = nullptr;

    // ---- two-pass measures (two_pass: pairs_osa, distance_device_impl, partial_device_impl) ----
    DevBuf osa_list;                 // the work list of the wave kernel (one word per row)
    DevBuf osa_scratch;              // its scratch for patterns too long for LDS
    // bounded distances and the alignment: the status block of the lane kernel and its pinned read-back (a pairwise call uses
    // its ring slot's)
    DevStatus *dist_status = nullptr;
    DevStatus *dist_status_host = nullptr;

    // ---- token transforms (token_bounds, token_sort_column, token_set_columns; strsim_token.h) ----
    DevBuf tok_off[2], tok_val[2];   // the normalised columns (sort form: of a and b; set form: ab and ba)
    DevBuf tok_list[2];              // work lists of the wave kernels (one word per row)
    DevBuf tok_desc;                 // their token descriptors beyond LDS
    DevBuf tok_sums;                 // block sums of the offset scan
    DevBuf tok_rec;                  // set form: one record a row, then the uint32 distances
    TokenStatus *tok_status = nullptr;      // device
    TokenStatus *tok_status_host = nullptr; // pinned: bounds before the transform, the work-list counts behind it

    // ---- token_ratio, the partial token ratios and WRatio (pairs_weighted; strsim_wratio.h) ----
    // buffers of their own: the flows a call composes (two_pass, the token transforms) use every buffer above freely
    DevBuf wr_score;                 // sub-scores: one f64 a row (ids 18, 24); WRatio: near | far x 2 | one more of the longer list
    DevBuf wr_cls, wr_pos;           // WRatio: a row's class (a byte) and its position on its list
    DevBuf wr_list[2];               // the near and the far list (one word per row)
    DevBuf wr_off[2], wr_val[2];     // the gathered sub-frame (near first, then far, in stream order)
    WratioStatus *wr_status = nullptr;      // device
    WratioStatus *wr_status_host = nullptr; // pinned: the list counts, read behind the wait of token_bounds
    uint64_t last_wratio_rows[2] = {};      // strsim_ctx_last_wratio_rows

    // ---- default_process and processed scoring (process_measure, process_write; strsim_process.h) ----
    // buffers of their own: the pairwise flow that runs behind the transform uses every buffer above freely
    DevBuf proc_off[2], proc_val[2]; // the processed columns of strsim_pairs_processed_device
    DevBuf proc_list[2];             // work lists of the wave kernel (one word per row)
    DevBuf proc_sums;                // block sums of the offset scan
    DevBuf proc_table;               // the table of strsim_process_table.h (PROCESS_TABLE_BYTES), uploaded on first use
    bool proc_table_ready = false;
    TokenStatus *proc_status = nullptr;      // device: wave_rows, max_len, begin, end of each side
    TokenStatus *proc_status_host = nullptr; // pinned: the same, and in pad[side] the processed bytes of each side
};

static int ctx_set_device(strsim_ctx *c) { HIP_TRY(hipSetDevice(c->device)); return STRSIM_OK; }

// strsim_pairs_host computes calls up to this size in place on pinned host memory (see there).  Measured through ctypes
// (bench_support/bench_small_host_calls.py), in place vs copies: 37 vs 70 us at 1..100 rows, 57 vs 95 us at 10 000,
// 92 vs 117 us at 32 768, 150 vs 171 us at 70 000, 246 vs 207 us at 100 000 -- hence the limit.
static constexpr size_t HOST_DIRECT_BYTES = (size_t)2 << 20;

// Rows with a string longer than STRSIM_WAVE_PATH_MAX_BYTES: rerun them with the scratch arrays in global memory.
static int ctx_run_huge(strsim_ctx *c, int slot, const DevStatus &st)
{
    const uint32_t cap = (st.max_len + 63u) & ~63u;
    const size_t per_wave = (size_t)HUGE_WS_WORDS(cap) * sizeof(uint32_t);
    const size_t max_waves = (size_t)c->num_cu * (size_t)c->huge_waves_per_cu;
    size_t waves = st.huge_rows < max_waves ? st.huge_rows : max_waves;
    const size_t budget = (size_t)4 << 30; // keep the workspace under 4 GiB
    if (waves * per_wave > budget) waves = budget / per_wave ? budget / per_wave : 1;
    int rc = c->huge_ws.reserve(waves * per_wave);
    if (rc) return rc;
    LaunchArgs a = c->slot_args[slot];
    a.ev_lane0 = a.ev_lane1 = a.ev_wave1 = nullptr;
    if (c->slot_measure[slot] == STRSIM_NUM_MEASURES) {
        for (int m = 0; m < STRSIM_NUM_MEASURES; ++m) {
            a.out = c->slot_outs[slot][m];
            hipError_t e = launch_huge(m, a, c->huge_ws.as<uint32_t>(), cap, (int)waves);
            if (e != hipSuccess) return hip_fail(e, "long-string kernel launch");
        }
    } else {
        hipError_t e = launch_huge(c->slot_measure[slot], a, c->huge_ws.as<uint32_t>(), cap, (int)waves);
        if (e != hipSuccess) return hip_fail(e, "long-string kernel launch");
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return STRSIM_OK;
}

// Retire one pending slot whose kernels have completed: timing, counters, the long-string pass.  A slot is retired whatever
// fails on the way (a slot left pending would be re-run by a later synchronize with buffers its caller may have freed).
// Has the device published the status block of the call in slot s?  (The ticket is the last word the publisher writes, with
// release semantics at system scope; the acquire fence pairs with it.)
static bool ctx_slot_published(const strsim_ctx *c, int s)
{
    const uint32_t seen = *reinterpret_cast<const volatile uint32_t *>(&c->status_host[s].ticket);
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    return seen == c->slot_ticket[s];
}

static constexpr uint32_t LANE_LEFT_UNKNOWN = 0xFFFFFFFFu; // the call's first kernel has not reported yet

// The slow-row kernels of a call that was enqueued as its lane kernel alone and left rows behind: launched now, behind
// whatever the stream holds, and waited for.
static int ctx_run_deferred(strsim_ctx *c, int s)
{
    LaunchArgs a = c->slot_args[s];
    a.ev_lane0 = a.ev_lane1 = a.ev_wave1 = nullptr;
    a.publish_host = nullptr;
    a.publish_ticket = 0u;
    const bool timed = c->slot_timed[s];
    if (timed) {
        for (int i = 0; i < 2; ++i)
            if (!c->ev_late[i]) HIP_TRY(hipEventCreateWithFlags(&c->ev_late[i], hipEventDisableSystemFence));
        HIP_TRY(hipEventRecord(c->ev_late[0], c->stream));
    }
    hipError_t e;
    if (c->slot_measure[s] == STRSIM_NUM_MEASURES) {
        const uint64_t nchunks = (a.n + 63u) >> 6;
        e = launch_slow_all_only(a, c->slot_outs[s], a.slowmask + nchunks);
    } else {
        e = launch_slow_only(c->slot_measure[s], a);
    }
    if (e != hipSuccess) return hip_fail(e, "kernel launch (slow rows of a retired call)");
    c->enqueued_ops += (c->slot_measure[s] == STRSIM_NUM_MEASURES ? 20u : 3u) + 1u; // + the status copy
    if (timed) HIP_TRY(hipEventRecord(c->ev_late[1], c->stream));
    if (++c->ticket_seq == 0u) c->ticket_seq = 1u;
    c->slot_ticket[s] = c->ticket_seq;
    c->status_host[s].ticket = 0u;
    HIP_TRY(launch_publish_status(c->status + s, c->status_host_dev + s, c->slot_ticket[s], c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (timed) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, c->ev_late[0], c->ev_late[1]));
        c->wave_ms += ms;
        c->wave_launches++;
    }
    return STRSIM_OK;
}

static void release_maskbufs(strsim_ctx *c, int s)
{
    for (int b = 0; b < strsim_ctx::MASKBUFS; ++b) if (c->maskbuf_owner[b] == s) c->maskbuf_owner[b] = -1;
}

static bool two_pass_measure(int measure) { return measure == STRSIM_OSA || measure == STRSIM_INDEL || measure == STRSIM_PARTIAL_RATIO; }

static int ctx_retire_slot(strsim_ctx *c, int s)
{
    int rc = STRSIM_OK;
    c->slot_pending[s] = false;
    struct Release { // the slot's mask buffer is free again whichever way this function is left
        strsim_ctx *c; int s;
        ~Release() { release_maskbufs(c, s); }
    } release{c, s};
    if (!ctx_slot_published(c, s)) { // (cannot happen behind a stream synchronise; strsim_ctx_retire_oldest checks before it gets here)
        c->slot_timed[s] = c->slot_deferred[s] = false;
        set_error("internal: the status block of a completed call was not published (slot %d)", s);
        return STRSIM_ERR_INTERNAL;
    }
    if (c->fault_retire_at && ++c->retired == c->fault_retire_at) { // (tests only: STRSIM_FAULT_RETIRE_AT)
        c->slot_timed[s] = c->slot_deferred[s] = false;
        set_error("fault injected at retirement %llu of this context (STRSIM_FAULT_RETIRE_AT)", (unsigned long long)c->retired);
        return STRSIM_ERR_INTERNAL;
    }
    // (a two-pass call has no lane_left: it says nothing about what the next call of the other measures leaves behind)
    const uint32_t left = two_pass_measure(c->slot_measure[s]) ? LANE_LEFT_UNKNOWN
                                                               : *reinterpret_cast<const volatile uint32_t *>(&c->status_host[s].lane_left);
    if (left != LANE_LEFT_UNKNOWN) { // what the next call on this context is enqueued for
        c->expect_slow = left != 0u;
        c->long_rows = (uint64_t)left * 16u > c->slot_args[s].n;
    }
    if (c->slot_timed[s]) {
        float a = 0, b = 0;
        // (the ticket says the kernels are done; the event right behind them may be a moment later)
        hipError_t e = hipEventSynchronize(c->ev[s][c->slot_deferred[s] ? 1 : 2]);
        if (e == hipSuccess) e = hipEventElapsedTime(&a, c->ev[s][0], c->ev[s][1]);
        if (e == hipSuccess && !c->slot_deferred[s]) e = hipEventElapsedTime(&b, c->ev[s][1], c->ev[s][2]);
        if (e == hipSuccess) {
            c->lane_ms += a; c->wave_ms += b;
            c->lane_launches++;
            if (!c->slot_deferred[s]) c->wave_launches++; // (a deferred call's slow-row kernels: counted where they are launched)
        } else {
            rc = hip_fail(e, "hipEventElapsedTime");
        }
    }
    if (c->slot_deferred[s] && left != 0u && rc == STRSIM_OK) {
        rc = ctx_run_deferred(c, s);
        if (rc == STRSIM_OK && !ctx_slot_published(c, s)) {
            set_error("internal: the status block of a deferred pass was not published (slot %d)", s);
            rc = STRSIM_ERR_INTERNAL;
        }
        c->last_late_rows += left;
    }
    c->slot_timed[s] = c->slot_deferred[s] = false;
    if (rc != STRSIM_OK) return rc;
    const DevStatus &st = c->status_host[s];
    c->last_wave_rows = st.wave_rows;
    c->last_long_rows += st.huge_rows;
    c->last_late_rows += st.huge_rows;
    if (st.huge_rows != 0) rc = ctx_run_huge(c, s, st);
    return rc;
}

// Retire every pending slot (the stream must already be synchronised); the first error is what the caller gets.
static int ctx_drain(strsim_ctx *c)
{
    int rc = STRSIM_OK;
    c->last_long_rows = 0;
    c->last_late_rows = 0;
    for (int k = 0; k < strsim_ctx::RING; ++k) {
        const int s = (c->head + k) % strsim_ctx::RING; // oldest first
        if (!c->slot_pending[s]) continue;
        if (rc == STRSIM_OK) {
            rc = ctx_retire_slot(c, s);
        } else {
            c->slot_pending[s] = c->slot_timed[s] = c->slot_deferred[s] = false;
            release_maskbufs(c, s);
        }
    }
    return rc;
}

extern "C" {

uint32_t strsim_abi_version(void) { return STRSIM_ABI_VERSION; }

uint32_t strsim_measure_supported(int measure, int entry_point) { return measure_accepted(measure, entry_point) ? 1u : 0u; }

const char *strsim_last_error_message(void) { return g_last_error.c_str(); }

int strsim_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n < 0 ? 0 : n;
}

int strsim_ctx_create(int device, void *hip_stream, strsim_ctx_t **out_ctx)
{
    if (!out_ctx) { set_error("strsim_ctx_create: out_ctx is NULL"); return STRSIM_ERR_ARG; }
    *out_ctx = nullptr;
    const int ndev = strsim_device_count();
    if (ndev == 0) {
        set_error("no HIP device is available; polars-strsim_amd has no CPU fallback");
        return STRSIM_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= ndev) {
        set_error("strsim_ctx_create: device %d out of range (0..%d)", device, ndev - 1);
        return STRSIM_ERR_ARG;
    }
    strsim_ctx *c = new (std::nothrow) strsim_ctx();
    if (!c) { set_error("out of host memory"); return STRSIM_ERR_OOM; }
    c->device = device;
    for (int b = 0; b < strsim_ctx::MASKBUFS; ++b) c->maskbuf_owner[b] = -1;
    int rc = ctx_set_device(c);
    if (rc) { delete c; return rc; }
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) { delete c; return hip_fail(e, "hipGetDeviceProperties"); }
    c->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (const char *env = getenv("STRSIM_STAGE_WG_PER_CU")) {
        const int v = atoi(env);
        if (v >= 1 && v <= 64) c->stage_wg_per_cu = v;
    }
    {
        const int resident = strsim::wave_lev_resident_per_cu(); // never more than fit: the grid is persistent
        if (resident >= 1 && resident < c->lev_waves_per_cu) c->lev_waves_per_cu = resident;
    }
    if (const char *env = getenv("STRSIM_LEV_WAVES_PER_CU")) {
        const int v = atoi(env);
        if (v >= 1 && v <= 256) c->lev_waves_per_cu = v;
    }
    c->no_literal_path = getenv("STRSIM_NO_LITERAL_PATH") != nullptr;
    if (const char *env = getenv("STRSIM_WIDE_WG_PER_CU")) {
        const int v = atoi(env);
        if (v >= 1 && v <= 4096) c->wide_cap_per_cu = v;
    }
    if (const char *env = getenv("STRSIM_HUGE_WAVES_PER_CU")) {
        const int v = atoi(env);
        if (v >= 1 && v <= 32) c->huge_waves_per_cu = v;
    }
    if (const char *env = getenv("STRSIM_HOST_DIRECT_ROWS")) c->host_direct_rows = (uint64_t)strtoull(env, nullptr, 10);
    if (const char *env = getenv("STRSIM_FAULT_RETIRE_AT")) c->fault_retire_at = (uint64_t)strtoull(env, nullptr, 10);
    if (hip_stream) {
        c->stream = (hipStream_t)hip_stream;
    } else {
        e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
        if (e != hipSuccess) { delete c; return hip_fail(e, "hipStreamCreateWithFlags"); }
        c->own_stream = true;
    }
    e = hipMalloc((void **)&c->status, sizeof(DevStatus) * strsim_ctx::RING);
    if (e == hipSuccess) e = hipMalloc((void **)&c->sched, sizeof(uint32_t) * 4 * strsim_ctx::RING);
    // (cleared on the context's own stream: a memset on the null stream would bring the legacy default stream into a process
    //  that may initialise torch's runtime later, tests/test_hip_runtime_sharing.py)
    if (e == hipSuccess) e = hipMemsetAsync(c->sched, 0, sizeof(uint32_t) * 4 * strsim_ctx::RING, c->stream);
    if (e == hipSuccess)
        e = hipHostMalloc((void **)&c->status_host, sizeof(DevStatus) * strsim_ctx::RING, hipHostMallocDefault);
    if (e != hipSuccess) { strsim_ctx_destroy(c); return hip_fail(e, "status allocation"); }
    memset(c->status_host, 0, sizeof(DevStatus) * strsim_ctx::RING);
    e = hipHostGetDevicePointer((void **)&c->status_host_dev, c->status_host, 0);
    if (e != hipSuccess) { strsim_ctx_destroy(c); return hip_fail(e, "hipHostGetDevicePointer"); }
    {   // integer quotients for the epilogues of the one-pair-per-lane kernels: the host's IEEE division is the device's
        static double q[QTAB_N * QTAB_N];
        for (int a = 0; a < QTAB_N; ++a)
            for (int b = 0; b < QTAB_N; ++b) q[a * QTAB_N + b] = b ? (double)a / (double)b : 0.0;
        e = hipMalloc((void **)&c->qtab, sizeof(q));
        if (e == hipSuccess) e = hipMemcpy(c->qtab, q, sizeof(q), hipMemcpyHostToDevice);
        if (e != hipSuccess) { strsim_ctx_destroy(c); return hip_fail(e, "quotient table"); }
    }
    *out_ctx = c;
    return STRSIM_OK;
}

void strsim_ctx_destroy(strsim_ctx_t *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    // in the order of the declaration (the grow-only buffers are freed by `delete`)
    if (c->status) (void)hipFree(c->status);
    if (c->sched) (void)hipFree(c->sched);
    if (c->status_host) (void)hipHostFree(c->status_host);
    if (c->qtab) (void)hipFree(c->qtab);
    if (c->scan_ws) (void)hipFree(c->scan_ws);
    if (c->pin) (void)hipHostFree(c->pin);
    for (int s = 0; s < strsim_ctx::RING; ++s)
        for (int i = 0; i < 3; ++i)
            if (c->ev[s][i]) (void)hipEventDestroy(c->ev[s][i]);
    for (int i = 0; i < 2; ++i) if (c->ev_late[i]) (void)hipEventDestroy(c->ev_late[i]);
    if (c->match_counts_host) (void)hipHostFree(c->match_counts_host);
    if (c->components_host) (void)hipHostFree(c->components_host);
    if (c->dist_status) (void)hipFree(c->dist_status);
    if (c->dist_status_host) (void)hipHostFree(c->dist_status_host);
    if (c->tok_status) (void)hipFree(c->tok_status);
    if (c->tok_status_host) (void)hipHostFree(c->tok_status_host);
    if (c->wr_status) (void)hipFree(c->wr_status);
    if (c->wr_status_host) (void)hipHostFree(c->wr_status_host);
    if (c->proc_status) (void)hipFree(c->proc_status);
    if (c->proc_status_host) (void)hipHostFree(c->proc_status_host);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

void *strsim_ctx_stream(strsim_ctx_t *c) { return c ? (void *)c->stream : nullptr; }

void strsim_split_offsets(uint64_t len, uint64_t n, uint64_t *out)
{
    // reference split_offsets, strsim.rs:21-39: len/n rows each, the remainder goes to the last part
    if (n == 0 || !out) return;
    if (n == 1) { out[0] = 0; out[1] = len; return; }
    const uint64_t chunk = len / n;
    for (uint64_t p = 0; p < n; ++p) {
        out[2 * p] = p * chunk;
        out[2 * p + 1] = (p == n - 1) ? len - p * chunk : chunk;
    }
}

} // extern "C"

// ---- columns, argument checks and staging shared by the entry points ----

// A string column as every function below the entry points takes it: rows + 1 Arrow offsets, the values they index, the rows.
struct Col {
    const uint32_t *off; const uint8_t *val; uint64_t rows;
};
// Row i of a column as a column of its own: the literal of a pairwise or distance call.
static Col literal(const Col &col, uint32_t i) { return Col{col.off + i, col.val, 1}; }

// Shape rule of parallel_apply, strsim.rs:48-52: the rows a call of two columns produces.
static int shape_rows(uint64_t a_rows, uint64_t b_rows, uint64_t *n)
{
    if (a_rows != b_rows && a_rows != 1 && b_rows != 1) {
        set_error("Inputs must have the same length, or one of them must be a Utf8 literal.");
        return STRSIM_ERR_SHAPE;
    }
    *n = (a_rows == 1) ? b_rows : a_rows;
    return STRSIM_OK;
}

// ... which must be what the caller's output holds, and fit the kernels: row and chunk indices are 32-bit inside them (as are
// the offsets themselves).
static int check_rows(const char *who, uint64_t a_rows, uint64_t b_rows, uint64_t out_rows, uint64_t *n)
{
    int rc = shape_rows(a_rows, b_rows, n);
    if (rc) return rc;
    if (out_rows != *n) {
        set_error("%s: out_rows=%llu but the inputs produce %llu rows", who, (unsigned long long)out_rows, (unsigned long long)*n);
        return STRSIM_ERR_ARG;
    }
    if (*n > 0xFFFFFFFFull) {
        set_error("%s: %llu rows in one call; split the column (at most 2^32 - 1 rows per call)", who, (unsigned long long)*n);
        return STRSIM_ERR_ARG;
    }
    return STRSIM_OK;
}

// The checks of the distance and alignment entry points behind their measure test (buffers: every input and output pointer is set).
static int elementwise_check(const char *who, strsim_ctx *c, uint64_t a_rows, uint64_t b_rows, uint64_t out_rows, bool buffers)
{
    uint64_t n;
    int rc = check_rows(who, a_rows, b_rows, out_rows, &n);
    if (rc) return rc;
    if (n && !buffers) { set_error("%s: NULL buffer", who); return STRSIM_ERR_ARG; }
    if (!c) { set_error("%s: ctx is NULL", who); return STRSIM_ERR_ARG; }
    return STRSIM_OK;
}

// What the searches and cdist check alike: the row limits of the two sides and the NULL test of the candidate side.  Each family
// keeps its own tests of the query side and the outputs, which it words and places differently.
static int search_rows_check(const char *who, const Col &q, const Col &cnd)
{
    if (q.rows > 0xFFFFFFFFull) { set_error("%s: %llu queries (at most 2^32 - 1)", who, (unsigned long long)q.rows); return STRSIM_ERR_ARG; }
    if (cnd.rows > 0xFFFFFFFEull) { set_error("%s: %llu candidates (at most 2^32 - 2)", who, (unsigned long long)cnd.rows); return STRSIM_ERR_ARG; }
    return STRSIM_OK;
}
static int candidate_buffers_check(const char *who, const Col &cnd)
{
    if (cnd.rows && (!cnd.off || !cnd.val)) { set_error("%s: NULL candidate buffer", who); return STRSIM_ERR_ARG; }
    return STRSIM_OK;
}

// The checks of the search families behind their measure test (best match: min_score may not be NaN; nearest passes 0; extract
// tests its score_cutoff itself).
static int search_check(const char *who, strsim_ctx *c, const Col &q, const Col &cnd, uint32_t k, uint32_t max_k, double min_score,
                        const void *out_a, const void *out_b)
{
    if (k < 1u || k > max_k) { set_error("%s: k=%u is outside 1..%u", who, k, max_k); return STRSIM_ERR_ARG; }
    if (min_score != min_score) { set_error("%s: min_score is NaN", who); return STRSIM_ERR_ARG; }
    int rc = search_rows_check(who, q, cnd);
    if (rc) return rc;
    if (q.rows && (!q.off || !q.val || !out_a || !out_b)) { set_error("%s: NULL query or output buffer", who); return STRSIM_ERR_ARG; }
    rc = candidate_buffers_check(who, cnd);
    if (rc) return rc;
    if (!c) { set_error("%s: ctx is NULL", who); return STRSIM_ERR_ARG; }
    return STRSIM_OK;
}

// The copy path of the *_host entry points: device copies of two host columns in stage[0..3] (uploads on the context's stream)
// and out_bytes of stage[4] for the results.  The caller's offset base is kept and the values go up from byte 0 of the caller's
// buffer, so every offset the kernels can form, 0 included, is inside the device copy.  The second column may have no rows.
struct Staged {
    Col a, b;
    uint8_t *out;
};
static Col dev_col(const DevBuf &off, const DevBuf &val, uint64_t rows) { return Col{off.as<uint32_t>(), val.as<uint8_t>(), rows}; }
static const Col NO_COL{nullptr, nullptr, 0};

static int ctx_stage(strsim_ctx *c, const Col &a, const Col &b, size_t out_bytes, Staged *s)
{
    const size_t a_bytes = a.off[a.rows], b_bytes = b.rows ? b.off[b.rows] : 0;
    const size_t need[5] = {(a.rows + 1) * 4, a_bytes + 1, (b.rows + 1) * 4, b_bytes + 1, out_bytes};
    for (int i = 0; i < 5; ++i) {
        int rc = c->stage[i].reserve(need[i]);
        if (rc) return rc;
    }
    HIP_TRY(hipMemcpyAsync(c->stage[0].p, a.off, need[0], hipMemcpyHostToDevice, c->stream));
    if (a_bytes) HIP_TRY(hipMemcpyAsync(c->stage[1].p, a.val, a_bytes, hipMemcpyHostToDevice, c->stream));
    if (b.rows) {
        HIP_TRY(hipMemcpyAsync(c->stage[2].p, b.off, need[2], hipMemcpyHostToDevice, c->stream));
        if (b_bytes) HIP_TRY(hipMemcpyAsync(c->stage[3].p, b.val, b_bytes, hipMemcpyHostToDevice, c->stream));
    }
    *s = Staged{dev_col(c->stage[0], c->stage[1], a.rows), dev_col(c->stage[2], c->stage[3], b.rows), c->stage[4].as<uint8_t>()};
    return STRSIM_OK;
}

static size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// The *_host entry point of an element-wise family behind its check (`checked`: what the check returned; n: the rows of the call):
// both columns staged, the device implementation on the staged columns with its output a (a_bytes) and, where the family has one, its
// output b (b_bytes, at a 256-byte boundary behind a) in stage[4], the copies back and the wait for them.  settle() runs between the
// device implementation and the copies: a pairwise family retires its call there (strsim_ctx_synchronize -- the long-string pass
// writes into the staged output from it), a distance family has nothing to do.
template <class Device, class Settle>
static int elementwise_host(strsim_ctx *c, int checked, const Col &a, const Col &b, uint64_t n, void *out_a, size_t a_bytes, void *out_b,
                            size_t b_bytes, Device device, Settle settle)
{
    if (checked || n == 0) return checked;
    int rc = ctx_set_device(c);
    if (rc) return rc;
    Staged s;
    rc = ctx_stage(c, a, b, b_bytes ? up256(a_bytes) + b_bytes : a_bytes, &s);
    if (rc) return rc;
    uint8_t *const d_a = s.out, *const d_b = s.out + up256(a_bytes);
    rc = device(s, d_a, d_b);
    if (rc == STRSIM_OK) rc = settle();
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(out_a, d_a, a_bytes, hipMemcpyDeviceToHost, c->stream));
    if (b_bytes) HIP_TRY(hipMemcpyAsync(out_b, d_b, b_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return STRSIM_OK;
}
static int nothing_to_settle() { return STRSIM_OK; }

// Take a ticket for the call in `slot` and clear the host copy of its status block.
static void slot_begin(strsim_ctx *c, int slot)
{
    if (++c->ticket_seq == 0u) c->ticket_seq = 1u;
    c->slot_ticket[slot] = c->ticket_seq;
    memset(&c->status_host[slot], 0, sizeof(DevStatus)); // (the slot is not pending: nothing on the device writes this block now)
}

// Record the call in its ring slot: it is pending from here on.  outs: the five outputs of a fused call, else nullptr.
static void slot_commit(strsim_ctx *c, int slot, const LaunchArgs &la, int measure, bool timed, bool deferred, double *const *outs)
{
    c->slot_timed[slot] = timed;
    c->slot_deferred[slot] = deferred;
    c->slot_args[slot] = la;
    c->slot_measure[slot] = measure;
    for (int q = 0; q < STRSIM_NUM_MEASURES; ++q) c->slot_outs[slot][q] = outs ? outs[q] : nullptr;
    c->slot_pending[slot] = true;
    c->head = (slot + 1) % strsim_ctx::RING;
}

// The two ways a status block reaches the host: published into the ring slot's host-mapped block with the slot's ticket (pairwise
// calls), or copied from dist_status (distance and alignment calls).
static int publish_slot(strsim_ctx *c, int slot)
{
    HIP_TRY(launch_publish_status(c->status + slot, c->status_host_dev + slot, c->slot_ticket[slot], c->stream));
    return STRSIM_OK;
}
static int dist_report(strsim_ctx *c)
{
    HIP_TRY(hipMemcpyAsync(c->dist_status_host, c->dist_status, sizeof(DevStatus), hipMemcpyDeviceToHost, c->stream));
    return STRSIM_OK;
}

// ---- two-pass measures: optimal string alignment, Indel, partial ratio, and the bounded distances ----
//
// One-pair-per-lane kernel over every row, a read-back of what it left for the wave kernel (how many rows, how long their patterns
// can be), then the wave kernel sized for that.  Every row is complete in stream order.

static constexpr size_t OSA_SCRATCH_BUDGET = (size_t)1 << 30; // the wave kernel runs fewer waves rather than use more scratch

// Which pair of kernels a call runs, and what they take beside the LaunchArgs.
enum TwoPassKind { TP_DIST, TP_INDEL, TP_PARTIAL, TP_QGRAM, TP_DAMERAU, TP_COMMON };
struct TwoPassCall {
    TwoPassKind kind;
    int measure;     // TP_DIST: STRSIM_LEVENSHTEIN or STRSIM_OSA; TP_QGRAM: the kind (STRSIM_QGRAM_*); TP_COMMON: STRSIM_COMMON_*
    uint32_t k;      // TP_DIST, TP_INDEL, TP_DAMERAU, TP_COMMON: the cutoff (DIST_UNBOUNDED: none)
    uint32_t *out32; // TP_DIST, TP_INDEL, TP_DAMERAU: the distances, or nullptr for the similarity in la.out (TP_DIST: of STRSIM_OSA)
    uint32_t *span;  // TP_PARTIAL: the alignment, or nullptr for the score alone
    uint32_t q = 0u;     // TP_QGRAM: 1..3
    uint32_t flags = 0u; // TP_QGRAM: STRSIM_QGRAM_SET
    int mode = 0;        // TP_COMMON: what `out` holds (a CommonOut of strsim_common.h)
    void *out = nullptr; // TP_COMMON: the f64 similarities, the uint32 distances or the uint32 counts
};
static const char *const TWO_PASS_LANE[] = {"kernel launch (k_dist_lane)", "kernel launch (k_indel_lane)",
                                            "kernel launch (k_partial_lane)", "kernel launch (k_qgram_lane)",
                                            "kernel launch (k_dl_lane)", "kernel launch (k_common_lane)"};
static const char *const TWO_PASS_WAVE[] = {"kernel launch (k_dist_wave)", "kernel launch (k_indel_wave)",
                                            "kernel launch (k_partial_wave)", "kernel launch (k_qgram_wave)",
                                            "kernel launch (k_dl_wave)", "kernel launch (k_common_wave)"};

static hipError_t two_pass_lane(const TwoPassCall &t, const LaunchArgs &la, uint32_t *list)
{
    switch (t.kind) {
    case TP_DIST: return launch_dist_lane(t.measure, la, t.k, t.out32, list);
    case TP_INDEL: return launch_indel_lane(la, t.k, t.out32, list);
    case TP_QGRAM: return launch_qgram_lane(la, t.measure, t.q, (t.flags & STRSIM_QGRAM_SET) != 0u, list);
    case TP_DAMERAU: return launch_dl_lane(la, t.k, t.out32, list);
    case TP_COMMON: return launch_common_lane(la, t.measure, t.mode, t.k, t.out, list);
    default: return launch_partial_lane(la, t.span, list);
    }
}

// a bound of the grams of a pair on a q-gram call's work list: max_len / pad1[0] bound its shorter and its longer string (bytes)
static uint64_t qgram_grams_bound(const DevStatus &st) { return (uint64_t)st.max_len + st.pad1[0]; }

static hipError_t two_pass_wave(const TwoPassCall &t, const LaunchArgs &la, const DevStatus &st, const uint32_t *list, int grid, uint32_t *scratch,
                                uint64_t words)
{
    switch (t.kind) {
    case TP_DIST: return launch_dist_wave(t.measure, la, t.k, t.out32, list, grid, scratch, words);
    case TP_INDEL: return launch_indel_wave(la, t.k, t.out32, list, grid, scratch, words);
    case TP_QGRAM: return launch_qgram_wave(la, t.measure, t.q, (t.flags & STRSIM_QGRAM_SET) != 0u, qgram_grams_bound(st), list, grid, scratch, words);
    case TP_DAMERAU: return launch_dl_wave(la, t.k, t.out32, st.max_len, list, grid, scratch, words);
    case TP_COMMON: return launch_common_wave(la, t.measure, t.mode, t.k, t.out, list, grid, scratch, words);
    default: return launch_partial_wave(la, t.span, list, grid, scratch, words);
    }
}

// Words of global scratch one wave needs for the work list `st` describes; 0 when LDS holds its tables.
static uint64_t two_pass_slot_words(TwoPassKind kind, const DevStatus &st, int measure = 0)
{
    if (kind == TP_COMMON) // (only LCSseq's wave kernel holds a pattern: Indel's)
        return measure == STRSIM_COMMON_LCSSEQ && st.max_len > OSA_WAVE_LDS_CPS ? indel_wave_slot_words(st.max_len) : 0u;
    if (kind == TP_PARTIAL) { // max_len / pad1[0] bound the needles and haystacks (bytes, hence scalar values)
        // (partial_wave_words grows with both arguments: the larger of the two forms at the bounds covers every pair)
        const uint64_t w = std::max(partial_wave_words(64u, st.pad1[0]), partial_wave_words(std::max(st.max_len, 65u), st.pad1[0]));
        return w > PARTIAL_WAVE_LDS_WORDS ? (w + 1u) & ~(uint64_t)1 : 0u; // (64-bit words inside a slot)
    }
    if (kind == TP_QGRAM) { // the table of both strings' grams and the values of one string
        const uint64_t grams = qgram_grams_bound(st);
        return grams > QGRAM_WAVE_LDS_GRAMS ? qgram_wave_slot_words(grams, st.pad1[0]) : 0u;
    }
    if (kind == TP_DAMERAU) // the columns and the boundary row of the shorter string (max_len: bytes, hence scalar values)
        return st.max_len > DL_WAVE_LDS_COLS ? dl_wave_slot_words(st.max_len) : 0u;
    if (st.max_len <= OSA_WAVE_LDS_CPS) return 0u; // (max_len bounds the pattern in scalar values: it is a byte length)
    return kind == TP_DIST ? dist_wave_slot_words(st.max_len) : indel_wave_slot_words(st.max_len);
}

// The shared flow.  la.status is the device status block the lane kernel counts into.  slot >= 0: a pairwise call, whose status
// is published into that ring slot; slot < 0: a distance or alignment call, whose status is copied.  c->osa_list holds la.n words.
static int two_pass(strsim_ctx *c, const LaunchArgs &la, const TwoPassCall &t, int slot)
{
    uint32_t *const list = c->osa_list.as<uint32_t>();
    HIP_TRY(hipMemsetAsync(la.status, 0, sizeof(DevStatus), c->stream));
    hipError_t e = two_pass_lane(t, la, list);
    if (e != hipSuccess) return hip_fail(e, TWO_PASS_LANE[t.kind]);
    int rc = slot >= 0 ? publish_slot(c, slot) : dist_report(c);
    if (rc) return rc;
    c->enqueued_ops += 3u;
    HIP_TRY(hipStreamSynchronize(c->stream));
    const DevStatus &st = slot >= 0 ? c->status_host[slot] : *c->dist_status_host;
    const uint32_t rows = st.wave_rows;
    if (rows == 0u) return STRSIM_OK;
    int grid = c->num_cu * 16;
    if ((uint64_t)grid > rows) grid = (int)rows;
    uint32_t *scratch = nullptr;
    const uint64_t words = two_pass_slot_words(t.kind, st, t.measure);
    if (words) {
        const size_t per = (size_t)words * sizeof(uint32_t);
        if ((size_t)grid * per > OSA_SCRATCH_BUDGET) grid = (int)std::max<size_t>(1, OSA_SCRATCH_BUDGET / per);
        rc = c->osa_scratch.reserve((size_t)grid * per);
        if (rc) return rc;
        scratch = c->osa_scratch.as<uint32_t>();
    }
    e = two_pass_wave(t, la, st, list, grid, scratch, words);
    if (e != hipSuccess) return hip_fail(e, TWO_PASS_WAVE[t.kind]);
    c->enqueued_ops += 1u;
    return STRSIM_OK;
}

// The one place that copies columns into a LaunchArgs; everything else is zero.
static LaunchArgs two_pass_args(strsim_ctx *c, const Col &a, const Col &b, double *out, uint64_t n, DevStatus *status)
{
    LaunchArgs la{};
    la.offA = a.off; la.valA = a.val; la.rowsA = a.rows;
    la.offB = b.off; la.valB = b.val; la.rowsB = b.rows;
    la.out = out; la.n = n;
    la.status = status; la.stream = c->stream;
    return la;
}

// The two columns of a pairwise call and the rows it produces.
struct PairCols {
    Col a, b;
    uint64_t n;
};

// A pairwise call of a two-pass measure (OSA: strsim_osa.h, Indel: strsim_indel.h, partial ratio: strsim_partial.h).  It occupies
// a ring slot like any other (its status block carries the ticket and the work-list count) and has nothing to do at retirement.
static int pairs_osa(strsim_ctx *c, int slot, int measure, const PairCols &p, double *out)
{
    int rc = c->osa_list.reserve(p.n * sizeof(uint32_t));
    if (rc) return rc;
    slot_begin(c, slot);
    const LaunchArgs la = two_pass_args(c, p.a, p.b, out, p.n, c->status + slot);
    const TwoPassKind kind = measure == STRSIM_PARTIAL_RATIO ? TP_PARTIAL : measure == STRSIM_INDEL ? TP_INDEL : TP_DIST;
    rc = two_pass(c, la, TwoPassCall{kind, measure, DIST_UNBOUNDED, nullptr, nullptr}, slot);
    if (rc) return rc;
    slot_commit(c, slot, la, measure, false, false, nullptr);
    return STRSIM_OK;
}

// ---- token transforms (strsim_token.h): token_sort_ratio, token_set_ratio, strsim_token_sort_* ----
//
// A call first reads the bounds of its columns (k_token_bounds: longest row, first and last offset) and waits for them: they size
// the scratch columns (a normalised string is never longer than its input) and the descriptor slots of the wave kernels.  That is
// the one host wait a token call makes beyond two_pass's; everything behind it is enqueued without another.  The work-list counts
// are copied to the pinned block behind the transform: strsim_ctx_last_token_wave_rows reads them once the stream has got there.

static constexpr size_t TOKEN_PAD = 64; // bytes behind a scratch value column
static int dist_prepare(strsim_ctx *c, uint64_t n);

static int token_prepare(strsim_ctx *c)
{
    int rc = ctx_set_device(c);
    if (rc) return rc;
    if (!c->tok_status) HIP_TRY(hipMalloc((void **)&c->tok_status, sizeof(TokenStatus)));
    if (!c->tok_status_host) HIP_TRY(hipHostMalloc((void **)&c->tok_status_host, sizeof(TokenStatus), hipHostMallocDefault));
    return STRSIM_OK;
}

// The bounds of one or two columns into c->tok_status_host (b == nullptr: one column); waits for the stream.
static int token_bounds(strsim_ctx *c, const Col &a, const Col *b)
{
    HIP_TRY(hipMemsetAsync(c->tok_status, 0, sizeof(TokenStatus), c->stream));
    HIP_TRY(launch_token_bounds(a.off, a.rows, c->tok_status, 0, c->stream));
    if (b) HIP_TRY(launch_token_bounds(b->off, b->rows, c->tok_status, 1, c->stream));
    HIP_TRY(hipMemcpyAsync(c->tok_status_host, c->tok_status, sizeof(TokenStatus), hipMemcpyDeviceToHost, c->stream));
    c->enqueued_ops += b ? 4u : 3u;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return STRSIM_OK;
}

// The grid of a wave kernel and its descriptor scratch for rows that hold up to max_tokens tokens.
static int token_wave_scratch(strsim_ctx *c, uint64_t max_tokens, int *grid, uint32_t **scratch, uint64_t *slot_words)
{
    *grid = c->num_cu * 8;
    *scratch = nullptr;
    *slot_words = 0;
    if (max_tokens <= TOKEN_WAVE_LDS_TOKENS) return STRSIM_OK;
    *slot_words = 2u * max_tokens + 2u;
    const size_t per = (size_t)*slot_words * sizeof(uint32_t);
    if ((size_t)*grid * per > OSA_SCRATCH_BUDGET) *grid = (int)std::max<size_t>(1, OSA_SCRATCH_BUDGET / per);
    int rc = c->tok_desc.reserve((size_t)*grid * per);
    if (rc) return rc;
    *scratch = c->tok_desc.as<uint32_t>();
    return STRSIM_OK;
}

static int token_copy_counts(strsim_ctx *c)
{
    HIP_TRY(hipMemcpyAsync(c->tok_status_host->wave_rows, c->tok_status->wave_rows, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    c->enqueued_ops += 1u;
    return STRSIM_OK;
}

// The sort form of one column into (out_off, out_val): out_off holds rows + 1 words, out_val the column's byte size.  max_len: the
// column's longest row (token_bounds).  side: which work list and counter (zeroed by token_bounds) the column uses.
static int token_sort_column(strsim_ctx *c, int side, const Col &col, uint32_t max_len, uint32_t *out_off, uint8_t *out_val)
{
    const uint64_t rows = col.rows;
    int rc = c->tok_list[side].reserve(rows * sizeof(uint32_t));
    if (rc) return rc;
    rc = c->tok_sums.reserve(((rows + 4095u) / 4096u) * sizeof(uint32_t));
    if (rc) return rc;
    int grid;
    uint32_t *scratch;
    uint64_t slot_words;
    rc = token_wave_scratch(c, token_max_tokens(max_len), &grid, &scratch, &slot_words);
    if (rc) return rc;
    uint32_t *const list = c->tok_list[side].as<uint32_t>(), *const count = &c->tok_status->wave_rows[side];
    hipError_t e = launch_token_sort(false, col.off, col.val, rows, out_off, out_val, list, count, grid, scratch, slot_words, c->stream);
    if (e != hipSuccess) return hip_fail(e, "kernel launch (k_token_sort_lane / _wave, measuring)");
    e = launch_token_scan(out_off, rows, c->tok_sums.as<uint32_t>(), c->stream);
    if (e != hipSuccess) return hip_fail(e, "kernel launch (k_token_scan)");
    e = launch_token_sort(true, col.off, col.val, rows, out_off, out_val, list, count, grid, scratch, slot_words, c->stream);
    if (e != hipSuccess) return hip_fail(e, "kernel launch (k_token_sort_lane / _wave, writing)");
    c->enqueued_ops += 7u;
    return STRSIM_OK;
}

// What sizes the scratch of a pair of columns: upper bounds of each column's bytes and longest row (token_bounds of the columns
// themselves, or of the columns a sub-frame was gathered from).
struct ColBounds {
    uint64_t bytes[2];
    uint32_t max_len[2];
};

static ColBounds token_col_bounds(const strsim_ctx *c)
{
    const TokenStatus st = *c->tok_status_host;
    return ColBounds{{(uint64_t)st.end[0] - st.begin[0], (uint64_t)st.end[1] - st.begin[1]}, {st.max_len[0], st.max_len[1]}};
}

// The sort form of two columns with the bounds bd into (off[s], val[s]), which *a and *b name afterwards (a literal stays one row; a
// side without rows -- the candidates of a search that has none -- is left as it is).  The work-list counters are zero on entry.
static int token_sort_columns(strsim_ctx *c, Col *a, Col *b, const ColBounds &bd, DevBuf (&off)[2], DevBuf (&val)[2])
{
    Col *const side[2] = {a, b};
    for (int s = 0; s < 2; ++s) {
        if (!side[s]->rows) continue;
        int rc = off[s].reserve((side[s]->rows + 1) * sizeof(uint32_t));
        if (rc == STRSIM_OK) rc = val[s].reserve(bd.bytes[s] + TOKEN_PAD);
        if (rc == STRSIM_OK) rc = token_sort_column(c, s, *side[s], bd.max_len[s], off[s].as<uint32_t>(), val[s].as<uint8_t>());
        if (rc) return rc;
        *side[s] = dev_col(off[s], val[s], side[s]->rows);
    }
    return token_copy_counts(c);
}

// The same for the two sides of a search or of cdist: their bounds are read here (the call's one wait beyond the search's),
// and the columns are the context's extract_off / extract_val.
static int token_sort_search_columns(strsim_ctx *c, Col *q, Col *cnd)
{
    int rc = token_prepare(c);
    if (rc == STRSIM_OK) rc = token_bounds(c, *q, cnd->rows ? cnd : nullptr);
    if (rc) return rc;
    return token_sort_columns(c, q, cnd, token_col_bounds(c), c->extract_off, c->extract_val);
}

// The set form of p.n pairs: ab and ba into c->tok_off / c->tok_val at full length, the records into *rec, and room for the uint32
// distances behind them (*d32).  The work-list counters are zero on entry.
static int token_set_columns(strsim_ctx *c, const PairCols &p, const ColBounds &bd, TokenSetRec **rec_out, uint32_t **d32_out)
{
    const uint64_t n = p.n;
    // a difference is never longer than its string; a literal's is materialised for every row
    const uint64_t cap[2] = {p.a.rows == 1 ? n * bd.bytes[0] : bd.bytes[0], p.b.rows == 1 ? n * bd.bytes[1] : bd.bytes[1]};
    if (cap[0] > 0xFFFFFFFFull || cap[1] > 0xFFFFFFFFull) {
        set_error("strsim_pairs_device: token_set_ratio with a literal of %llu bytes against %llu rows exceeds 32-bit offsets; split the column",
                  (unsigned long long)(p.a.rows == 1 ? bd.bytes[0] : bd.bytes[1]), (unsigned long long)n);
        return STRSIM_ERR_ARG;
    }
    int rc = STRSIM_OK;
    for (int s = 0; s < 2; ++s) {
        rc = c->tok_off[s].reserve((n + 1) * sizeof(uint32_t));
        if (rc == STRSIM_OK) rc = c->tok_val[s].reserve(cap[s] + TOKEN_PAD);
        if (rc) return rc;
    }
    const size_t d32_at = up256(n * sizeof(TokenSetRec));
    rc = c->tok_rec.reserve(d32_at + n * sizeof(uint32_t));
    if (rc == STRSIM_OK) rc = c->tok_list[0].reserve(n * sizeof(uint32_t));
    if (rc == STRSIM_OK) rc = c->tok_sums.reserve(((n + 4095u) / 4096u) * sizeof(uint32_t));
    if (rc) return rc;
    int grid;
    uint32_t *scratch;
    uint64_t slot_words;
    rc = token_wave_scratch(c, token_max_tokens(bd.max_len[0]) + token_max_tokens(bd.max_len[1]), &grid, &scratch, &slot_words);
    if (rc) return rc;
    uint32_t *const off_ab = c->tok_off[0].as<uint32_t>(), *const off_ba = c->tok_off[1].as<uint32_t>();
    uint8_t *const val_ab = c->tok_val[0].as<uint8_t>(), *const val_ba = c->tok_val[1].as<uint8_t>();
    TokenSetRec *const rec = c->tok_rec.as<TokenSetRec>();
    uint32_t *const list = c->tok_list[0].as<uint32_t>(), *const count = &c->tok_status->wave_rows[0];
    LaunchArgs in = two_pass_args(c, p.a, p.b, nullptr, n, nullptr);
    hipError_t e = launch_token_set(false, in, off_ab, val_ab, off_ba, val_ba, rec, list, count, grid, scratch, slot_words);
    if (e != hipSuccess) return hip_fail(e, "kernel launch (k_token_set_lane / _wave, measuring)");
    e = launch_token_scan(off_ab, n, c->tok_sums.as<uint32_t>(), c->stream);
    if (e == hipSuccess) e = launch_token_scan(off_ba, n, c->tok_sums.as<uint32_t>(), c->stream);
    if (e != hipSuccess) return hip_fail(e, "kernel launch (k_token_scan)");
    e = launch_token_set(true, in, off_ab, val_ab, off_ba, val_ba, rec, list, count, grid, scratch, slot_words);
    if (e != hipSuccess) return hip_fail(e, "kernel launch (k_token_set_lane / _wave, writing)");
    c->enqueued_ops += 10u;
    *rec_out = rec;
    *d32_out = reinterpret_cast<uint32_t *>(c->tok_rec.as<uint8_t>() + d32_at);
    return token_copy_counts(c);
}

// token_set_ratio of p.n pairs into out: the set columns, the Indel flow with the unbounded integer distance, the epilogue.
static int token_set_scores(strsim_ctx *c, const PairCols &p, const ColBounds &bd, double *out)
{
    TokenSetRec *rec;
    uint32_t *d32;
    int rc = token_set_columns(c, p, bd, &rec, &d32);
    if (rc) return rc;
    rc = dist_prepare(c, p.n);
    if (rc) return rc;
    const LaunchArgs la = two_pass_args(c, dev_col(c->tok_off[0], c->tok_val[0], p.n), dev_col(c->tok_off[1], c->tok_val[1], p.n), nullptr, p.n, c->dist_status);
    rc = two_pass(c, la, TwoPassCall{TP_INDEL, STRSIM_INDEL, DIST_UNBOUNDED, d32, nullptr}, -1);
    if (rc) return rc;
    const hipError_t e = launch_token_set_epilogue(rec, d32, out, p.n, c->stream);
    if (e != hipSuccess) return hip_fail(e, "kernel launch (k_token_set_epilogue)");
    c->enqueued_ops += 1u;
    return STRSIM_OK;
}

// A pairwise call of a token measure.  Sort form: both columns normalised into scratch (a literal stays one row), then the Indel
// flow into the caller's out, in this call's ring slot.  Set form: ab and ba into scratch at full length, the Indel flow with the
// unbounded integer distance, then the epilogue; it takes no ring slot (nothing is left to do at retirement).
static int pairs_token(strsim_ctx *c, int slot, int measure, const PairCols &p, double *out)
{
    int rc = token_prepare(c);
    if (rc) return rc;
    rc = token_bounds(c, p.a, &p.b);
    if (rc) return rc;
    const ColBounds bd = token_col_bounds(c);
    if (measure == STRSIM_TOKEN_SET_RATIO) return token_set_scores(c, p, bd, out);
    PairCols t = p;
    rc = token_sort_columns(c, &t.a, &t.b, bd, c->tok_off, c->tok_val);
    if (rc) return rc;
    return pairs_osa(c, slot, STRSIM_INDEL, t, out);
}

// ---- token_ratio, the partial token ratios and WRatio (strsim_wratio.h) ----
//
// Compositions of the flows above.  None takes a ring slot: every two_pass below reports through dist_status, and nothing is left
// to do at retirement.  A composition reads the bounds of its raw columns once (token_bounds, one wait); the sub-frames of WRatio are
// sized by the bounds of the columns they were gathered from.

// The work-list counters of the token transforms, which token_bounds zeroes for the first transform of a call only.
static int token_zero_counts(strsim_ctx *c)
{
    HIP_TRY(hipMemsetAsync(c->tok_status->wave_rows, 0, 2 * sizeof(uint32_t), c->stream));
    c->enqueued_ops += 1u;
    return STRSIM_OK;
}

// Indel similarity (TP_INDEL) or partial ratio (TP_PARTIAL) of p.n pairs into out.
static int two_pass_scores(strsim_ctx *c, const PairCols &p, TwoPassKind kind, double *out)
{
    int rc = dist_prepare(c, p.n);
    if (rc) return rc;
    const LaunchArgs la = two_pass_args(c, p.a, p.b, out, p.n, c->dist_status);
    if (kind == TP_PARTIAL) return two_pass(c, la, TwoPassCall{TP_PARTIAL, STRSIM_PARTIAL_RATIO, 0u, nullptr, nullptr}, -1);
    return two_pass(c, la, TwoPassCall{TP_INDEL, STRSIM_INDEL, DIST_UNBOUNDED, nullptr, nullptr}, -1);
}

// token_sort_ratio (TP_INDEL) or partial_token_sort_ratio (TP_PARTIAL) into out
static int token_sort_scores(strsim_ctx *c, const PairCols &p, const ColBounds &bd, TwoPassKind kind, double *out)
{
    PairCols t = p;
    int rc = token_zero_counts(c);
    if (rc == STRSIM_OK) rc = token_sort_columns(c, &t.a, &t.b, bd, c->tok_off, c->tok_val);
    if (rc) return rc;
    return two_pass_scores(c, t, kind, out);
}

// partial_token_set_ratio into out: the set columns, partial ratio of ab and ba into out, the rule over the records in place
static int partial_token_set_scores(strsim_ctx *c, const PairCols &p, const ColBounds &bd, double *out)
{
    TokenSetRec *rec;
    uint32_t *d32;
    int rc = token_zero_counts(c);
    if (rc == STRSIM_OK) rc = token_set_columns(c, p, bd, &rec, &d32);
    if (rc) return rc;
    const PairCols t{dev_col(c->tok_off[0], c->tok_val[0], p.n), dev_col(c->tok_off[1], c->tok_val[1], p.n), p.n};
    rc = two_pass_scores(c, t, TP_PARTIAL, out);
    if (rc) return rc;
    const hipError_t e = launch_partial_token_set_epilogue(rec, out, out, p.n, c->stream);
    if (e != hipSuccess) return hip_fail(e, "kernel launch (k_partial_token_set_epilogue)");
    c->enqueued_ops += 1u;
    return STRSIM_OK;
}

// token_ratio (partial = false) or partial_token_ratio (partial = true) into out; tmp: p.n more f64
static int token_max_scores(strsim_ctx *c, const PairCols &p, const ColBounds &bd, bool partial, double *out, double *tmp)
{
    int rc = token_sort_scores(c, p, bd, partial ? TP_PARTIAL : TP_INDEL, out);
    if (rc) return rc;
    if (partial) rc = partial_token_set_scores(c, p, bd, tmp);
    else {
        rc = token_zero_counts(c);
        if (rc == STRSIM_OK) rc = token_set_scores(c, p, bd, tmp);
    }
    if (rc) return rc;
    const hipError_t e = launch_max_f64(out, tmp, out, p.n, c->stream);
    if (e != hipSuccess) return hip_fail(e, "kernel launch (k_max_f64)");
    c->enqueued_ops += 1u;
    return STRSIM_OK;
}

static int wratio_prepare(strsim_ctx *c)
{
    if (!c->wr_status) HIP_TRY(hipMalloc((void **)&c->wr_status, sizeof(WratioStatus)));
    if (!c->wr_status_host) HIP_TRY(hipHostMalloc((void **)&c->wr_status_host, sizeof(WratioStatus), hipHostMallocDefault));
    return STRSIM_OK;
}

// WRatio of p.n pairs into out: Indel over every row, the classes and the two lists, then each family over the gather of its rows.
static int pairs_wratio(strsim_ctx *c, const PairCols &p, double *out)
{
    const uint64_t n = p.n;
    int rc = wratio_prepare(c);
    if (rc == STRSIM_OK) rc = c->wr_cls.reserve(n);
    if (rc == STRSIM_OK) rc = c->wr_pos.reserve(n * sizeof(uint32_t));
    for (int f = 0; f < 2 && rc == STRSIM_OK; ++f) rc = c->wr_list[f].reserve(n * sizeof(uint32_t));
    if (rc) return rc;
    rc = two_pass_scores(c, p, TP_INDEL, out);
    if (rc) return rc;
    uint8_t *const cls = c->wr_cls.as<uint8_t>();
    uint32_t *const pos = c->wr_pos.as<uint32_t>();
    uint32_t *const list[2] = {c->wr_list[0].as<uint32_t>(), c->wr_list[1].as<uint32_t>()};
    const LaunchArgs la = two_pass_args(c, p.a, p.b, out, n, nullptr);
    HIP_TRY(hipMemsetAsync(c->wr_status, 0, sizeof(WratioStatus), c->stream));
    hipError_t e = launch_wratio_classify(la, cls, pos, list[0], list[1], c->wr_status);
    if (e != hipSuccess) return hip_fail(e, "kernel launch (k_wratio_classify)");
    HIP_TRY(hipMemcpyAsync(c->wr_status_host, c->wr_status, sizeof(WratioStatus), hipMemcpyDeviceToHost, c->stream));
    c->enqueued_ops += 3u;
    rc = token_bounds(c, p.a, &p.b); // (the list counts ride on this wait)
    if (rc) return rc;
    const ColBounds bd = token_col_bounds(c);
    const uint64_t m[2] = {c->wr_status_host->rows[0], c->wr_status_host->rows[1]};
    const uint64_t longer = std::max(m[0], m[1]);
    // sub-scores: token_ratio of the near rows | partial_ratio, partial_token_ratio of the far rows | one column of the longer list
    rc = c->wr_score.reserve((m[0] + 2u * m[1] + longer) * sizeof(double));
    if (rc == STRSIM_OK) rc = c->tok_sums.reserve(((longer + 4095u) / 4096u) * sizeof(uint32_t));
    const Col *const side[2] = {&p.a, &p.b};
    for (int s = 0; s < 2 && rc == STRSIM_OK; ++s) {
        if (side[s]->rows == 1) continue; // a literal is not gathered
        rc = c->wr_off[s].reserve((longer + 1) * sizeof(uint32_t));
        if (rc == STRSIM_OK) rc = c->wr_val[s].reserve(bd.bytes[s] + TOKEN_PAD);
    }
    if (rc) return rc;
    double *const s_near = c->wr_score.as<double>(), *const s_far0 = s_near + m[0], *const s_far1 = s_far0 + m[1], *const tmp = s_far1 + m[1];
    for (int f = 0; f < 2; ++f) {
        if (m[f] == 0) continue; // a family without rows launches nothing
        PairCols sub{p.a, p.b, m[f]};
        Col *const sub_side[2] = {&sub.a, &sub.b};
        for (int s = 0; s < 2; ++s) {
            if (side[s]->rows == 1) continue;
            e = launch_take(side[s]->off, side[s]->val, list[f], (uint32_t)m[f], c->wr_off[s].as<uint32_t>(), c->wr_val[s].as<uint8_t>(),
                            c->tok_sums.as<uint32_t>(), c->stream);
            if (e != hipSuccess) return hip_fail(e, "kernel launch (k_take_measure / k_token_scan / k_take_write)");
            c->enqueued_ops += 5u;
            *sub_side[s] = dev_col(c->wr_off[s], c->wr_val[s], m[f]);
        }
        if (f == 0) rc = token_max_scores(c, sub, bd, false, s_near, tmp);
        else {
            rc = two_pass_scores(c, sub, TP_PARTIAL, s_far0);
            if (rc == STRSIM_OK) rc = token_max_scores(c, sub, bd, true, s_far1, tmp);
        }
        if (rc) return rc;
    }
    e = launch_wratio_combine(la, cls, pos, s_near, s_far0, s_far1);
    if (e != hipSuccess) return hip_fail(e, "kernel launch (k_wratio_combine)");
    c->enqueued_ops += 1u;
    c->last_wratio_rows[0] = m[0];
    c->last_wratio_rows[1] = m[1];
    return STRSIM_OK;
}

// A pairwise call of one of the five: ids 18 .. 24 over the whole frame, WRatio routed.
static int pairs_weighted(strsim_ctx *c, int measure, const PairCols &p, double *out)
{
    int rc = token_prepare(c);
    if (rc) return rc;
    if (measure == STRSIM_WRATIO) return pairs_wratio(c, p, out);
    rc = token_bounds(c, p.a, &p.b);
    if (rc) return rc;
    const ColBounds bd = token_col_bounds(c);
    if (measure == STRSIM_PARTIAL_TOKEN_SORT_RATIO) return token_sort_scores(c, p, bd, TP_PARTIAL, out);
    if (measure == STRSIM_PARTIAL_TOKEN_SET_RATIO) return partial_token_set_scores(c, p, bd, out);
    rc = c->wr_score.reserve(p.n * sizeof(double));
    if (rc) return rc;
    return token_max_scores(c, p, bd, measure == STRSIM_PARTIAL_TOKEN_RATIO, out, c->wr_score.as<double>());
}

static int pairs_device_impl(strsim_ctx_t *c, int measure, const Col &a, const Col &b, double *const *outs, uint64_t out_rows, bool eager = false)
{
    const bool all = measure == STRSIM_NUM_MEASURES;
    if (!c) { set_error("strsim_pairs_device: ctx is NULL"); return STRSIM_ERR_ARG; }
    if (!all && !measure_accepted(measure, STRSIM_ENTRY_PAIRWISE)) {
        set_error("strsim_pairs_device: unknown measure %d", measure);
        return STRSIM_ERR_ARG;
    }
    uint64_t n;
    int rc = check_rows("strsim_pairs_device", a.rows, b.rows, out_rows, &n);
    if (rc || n == 0) return rc;
    if (!a.off || !b.off || !outs) { set_error("strsim_pairs_device: NULL buffer"); return STRSIM_ERR_ARG; }
    for (int q = 0; q < (all ? STRSIM_NUM_MEASURES : 1); ++q)
        if (!outs[q]) { set_error("strsim_pairs_device: NULL output buffer"); return STRSIM_ERR_ARG; }
    rc = ctx_set_device(c);
    if (rc) return rc;
    // the ring slot about to be reused must have been retired
    const int slot = c->head;
    if (c->slot_pending[slot]) {
        // the ring of status slots has wrapped (RING calls in flight without a retire): everything pending is retired here, and
        // what those calls finished late is kept for the caller's next strsim_ctx_synchronize / strsim_ctx_retire_oldest
        HIP_TRY(hipStreamSynchronize(c->stream));
        rc = ctx_drain(c);
        c->carry_late_rows += c->last_late_rows;
        c->carry_long_rows += c->last_long_rows;
        if (rc) { //  the failure belongs to an earlier call: say so, with a code of its own -- this call was not enqueued
            const std::string why = strsim_last_error_message();
            set_error("strsim_pairs_device: retiring earlier pending calls at the wrap of the ring failed (this call was not enqueued): %s", why.c_str());
            return STRSIM_ERR_EARLIER_CALL;
        }
    }
    const PairCols p{a, b, n};
    if (two_pass_measure(measure)) return pairs_osa(c, slot, measure, p, outs[0]);
    if (measure == STRSIM_TOKEN_SORT_RATIO || measure == STRSIM_TOKEN_SET_RATIO) return pairs_token(c, slot, measure, p, outs[0]);
    if (weighted_measure(measure)) return pairs_weighted(c, measure, p, outs[0]);
    const uint64_t nchunks = (n + 63) >> 6;
    // One launch (the lane kernel alone, the rest at retirement if it turns out to be needed) when the caller has opted in and the
    // context's last retired call left nothing behind its lane kernel.  Such a call owns a mask buffer until it is retired (there
    // is always a free one: as many as ring slots).
    bool defer = !eager && !c->expect_slow && !c->stream_ordered;
    int mb = strsim_ctx::SHARED_MASKBUF;
    if (defer) {
        defer = false;
        for (int b = 0; b < strsim_ctx::SHARED_MASKBUF; ++b)
            if (c->maskbuf_owner[b] < 0) { mb = b; defer = true; break; }
    }
    // mask + backup (five-measure call) + the work list of k_lane_utf8 (one u32 per chunk)
    rc = c->slowmask[mb].reserve(2 * nchunks * sizeof(unsigned long long) + nchunks * sizeof(uint32_t));
    if (rc) return rc;
    unsigned long long *const mask = c->slowmask[mb].as<unsigned long long>();
    // (the status block of the slot is cleared by the first kernel of the call)
    slot_begin(c, slot);
    c->status_host[slot].lane_left = LANE_LEFT_UNKNOWN;

    LaunchArgs la = two_pass_args(c, a, b, outs[0], n, c->status + slot);
    la.slowmask = mask;
    la.sched = c->sched + 4 * slot;
    la.worklist = reinterpret_cast<uint32_t *>(mask + 2 * nchunks);
    la.qtab = c->qtab;
    la.stage_grid = c->num_cu * c->stage_wg_per_cu;
    la.no_literal_path = c->no_literal_path;
    la.long_rows = c->long_rows;
    la.wide_grid = c->num_cu * 3; // resident (LDS)
    la.wide_grid_cap = c->num_cu * c->wide_cap_per_cu;
    la.wave_grid = c->num_cu * 16;                       // k_wave_pairs, other measures: 4 waves per SIMD
    la.wave_grid_lev = c->num_cu * c->lev_waves_per_cu;
    {   // per-wave global scratch of k_wave_pairs (scalar-value arrays; Levenshtein: text arenas as well)
        const size_t waves = (size_t)std::max(la.wave_grid, la.wave_grid_lev);
        rc = c->lev_ws.reserve(waves * LEV_WS_WORDS * sizeof(uint32_t));
        if (rc) return rc;
        la.lev_ws = c->lev_ws.as<uint32_t>();
    }
    la.ev_lane0 = la.ev_lane1 = la.ev_wave1 = nullptr;
    if (c->timing) {
        for (int i = 0; i < 3; ++i)
            // timing only: no system-scope fence when the event completes (a default event costs ~5 us of GPU time
            // between two kernels, three of them were 1/3 of a 1 M-row call)
            if (!c->ev[slot][i]) HIP_TRY(hipEventCreateWithFlags(&c->ev[slot][i], hipEventDisableSystemFence));
        la.ev_lane0 = c->ev[slot][0]; la.ev_lane1 = c->ev[slot][1]; la.ev_wave1 = c->ev[slot][2];
    }
    if (eager && !all && !c->timing) {
        // Small call the caller is going to wait for anyway: launch the one-pair-per-lane kernel alone, let its last
        // workgroup report how many rows it left (host-mapped status word) and wait for it.  Usually that is none --
        // short ASCII strings -- and the call is done after ONE kernel launch instead of five (the three slow-row kernels
        // and the status copy cost ~4 us each even when they find nothing to do).
        la.publish_host = c->status_host_dev + slot;
        hipError_t e0 = launch_lane_only(measure, la);
        if (e0 != hipSuccess) return hip_fail(e0, "kernel launch");
        c->enqueued_ops += (uint64_t)lane_kernel_launches(measure, la);
        HIP_TRY(hipStreamSynchronize(c->stream));
        const uint32_t left = *reinterpret_cast<volatile uint32_t *>(&c->status_host[slot].lane_left);
        if (left == 0u) {
            // nothing pending FOR THIS CALL: strsim_ctx_synchronize() has nothing to retire for it.  The last_* counters describe
            // the last retirement; they are only reset when no other call of this context is still pending (a caller
            // with one-launch calls in flight that copied results out early still has to see their late rows)
            bool others = false;
            for (int s2 = 0; s2 < strsim_ctx::RING; ++s2) others = others || c->slot_pending[s2];
            if (!others) {
                c->last_wave_rows = 0;
                c->last_long_rows = 0;
                c->last_late_rows = 0;
            }
            return STRSIM_OK;
        }
        la.publish_host = nullptr;
        e0 = launch_slow_only(measure, la);
        if (e0 != hipSuccess) return hip_fail(e0, "kernel launch");
        c->enqueued_ops += 4u;
        rc = publish_slot(c, slot);
        if (rc) return rc;
        slot_commit(c, slot, la, measure, false, false, nullptr);
        return STRSIM_OK;
    }
    la.publish_host = c->status_host_dev + slot; // lane_left reaches the host either way: it sets expect_slow
    hipError_t e;
    if (defer) {
        la.publish_ticket = c->slot_ticket[slot];
        e = all ? launch_lane_all_only(la, outs) : launch_lane_only(measure, la);
    } else {
        e = all ? launch_pairs_all(la, outs, mask + nchunks) : launch_pairs(measure, la);
    }
    if (e != hipSuccess) return hip_fail(e, "kernel launch");
    // lane kernel (+ k_publish_lit behind k_lane_lit) | + three slow-row kernels (x 5, + 5 mask copies) + status copy
    c->enqueued_ops += (uint64_t)lane_kernel_launches(measure, la) + (defer ? 0u : (all ? 21u : 4u));
    if (defer) c->maskbuf_owner[mb] = slot;
    else if ((rc = publish_slot(c, slot)) != STRSIM_OK) return rc;
    slot_commit(c, slot, la, measure, c->timing, defer, all ? outs : nullptr);
    return STRSIM_OK;
}

// strsim_pairs_device (eager: strsim_pairs_device_small), which the flows below call with a literal or with columns of their own.
static int pairs_device(strsim_ctx *c, int measure, const Col &a, const Col &b, double *out, uint64_t out_rows, bool eager = false)
{
    if (measure == STRSIM_NUM_MEASURES) {
        set_error("%s: unknown measure %d", eager ? "strsim_pairs_device_small" : "strsim_pairs_device", measure);
        return STRSIM_ERR_ARG;
    }
    double *outs[1] = {out};
    return pairs_device_impl(c, measure, a, b, out ? outs : nullptr, out_rows, eager);
}

extern "C" {

int strsim_pairs_device(strsim_ctx_t *c, int measure, const uint32_t *a_off, const uint8_t *a_val, uint64_t a_rows,
                        const uint32_t *b_off, const uint8_t *b_val, uint64_t b_rows, double *out, uint64_t out_rows)
{
    return pairs_device(c, measure, Col{a_off, a_val, a_rows}, Col{b_off, b_val, b_rows}, out, out_rows);
}

int strsim_pairs_device_small(strsim_ctx_t *c, int measure, const uint32_t *a_off, const uint8_t *a_val, uint64_t a_rows,
                              const uint32_t *b_off, const uint8_t *b_val, uint64_t b_rows, double *out, uint64_t out_rows)
{
    return pairs_device(c, measure, Col{a_off, a_val, a_rows}, Col{b_off, b_val, b_rows}, out, out_rows, true);
}

int strsim_pairs_device_all(strsim_ctx_t *c, const uint32_t *a_off, const uint8_t *a_val, uint64_t a_rows,
                            const uint32_t *b_off, const uint8_t *b_val, uint64_t b_rows, double *const outs[5],
                            uint64_t out_rows)
{
    return pairs_device_impl(c, STRSIM_NUM_MEASURES, Col{a_off, a_val, a_rows}, Col{b_off, b_val, b_rows}, outs, out_rows);
}

int strsim_ctx_synchronize(strsim_ctx_t *c)
{
    if (!c) { set_error("strsim_ctx_synchronize: ctx is NULL"); return STRSIM_ERR_ARG; }
    int rc = ctx_set_device(c);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    rc = ctx_drain(c);
    c->last_late_rows += c->carry_late_rows;
    c->last_long_rows += c->carry_long_rows;
    c->carry_late_rows = c->carry_long_rows = 0;
    return rc;
}

int strsim_internal_ctx_device(strsim_ctx *c) { return c ? c->device : 0; }

int strsim_internal_scan_workspace(strsim_ctx *c, uint32_t **p)
{
    int rc = ctx_set_device(c);
    if (rc) return rc;
    if (!c->scan_ws) HIP_TRY(hipMalloc((void **)&c->scan_ws, strsim::SCAN_WS_WORDS * sizeof(uint32_t)));
    *p = c->scan_ws;
    return STRSIM_OK;
}

int strsim_ctx_retire_oldest(strsim_ctx_t *c)
{
    if (!c) { set_error("strsim_ctx_retire_oldest: ctx is NULL"); return STRSIM_ERR_ARG; }
    int rc = ctx_set_device(c);
    if (rc) return rc;
    auto report_carry = [c] { // what calls retired by the library itself finished late goes out with this retirement
        c->last_long_rows = c->carry_long_rows;
        c->last_late_rows = c->carry_late_rows;
        c->carry_late_rows = c->carry_long_rows = 0;
    };
    for (int k = 0; k < strsim_ctx::RING; ++k) {
        const int s = (c->head + k) % strsim_ctx::RING; // oldest first
        if (!c->slot_pending[s]) continue;
        if (!ctx_slot_published(c, s)) {
            // the caller's promise does not hold (e.g. its event was recorded on another stream than strsim_ctx_stream()):
            // say so instead of reading a status block the device has not written; the call stays pending
            set_error("strsim_ctx_retire_oldest: the oldest call has not completed (wait on an event recorded on "
                      "strsim_ctx_stream() behind it, or call strsim_ctx_synchronize())");
            return STRSIM_ERR_ARG;
        }
        report_carry();
        return ctx_retire_slot(c, s);
    }
    report_carry();
    return STRSIM_OK; // nothing pending (e.g. a small call that completed inside strsim_pairs_device_small)
}

int strsim_pairs_host(strsim_ctx_t *c, int measure, const uint32_t *a_off, const uint8_t *a_val, uint64_t a_rows,
                      const uint32_t *b_off, const uint8_t *b_val, uint64_t b_rows, double *out, uint64_t out_rows)
{
    if (!c) { set_error("strsim_pairs_host: ctx is NULL"); return STRSIM_ERR_ARG; }
    const Col a{a_off, a_val, a_rows}, b{b_off, b_val, b_rows};
    uint64_t n;
    int rc = shape_rows(a_rows, b_rows, &n);
    if (rc) return rc;
    if (out_rows != n) { set_error("strsim_pairs_host: out_rows mismatch"); return STRSIM_ERR_ARG; }
    if (n == 0) return STRSIM_OK;
    if (!a_off || !b_off || !out) { set_error("strsim_pairs_host: NULL buffer"); return STRSIM_ERR_ARG; }
    const size_t abytes = (size_t)a_off[a_rows] - a_off[0], bbytes = (size_t)b_off[b_rows] - b_off[0];
    if (n <= c->host_direct_rows && abytes <= HOST_DIRECT_BYTES && bbytes <= HOST_DIRECT_BYTES) {
        rc = ctx_set_device(c);
        if (rc) return rc;
        // Small call: gather the five buffers in one pinned block and let the kernels work on it in place through the
        // device's mapping of host memory -- no copy engine, whose hand-overs (four H2D, one D2H) are most of a small call.
        const size_t o_aoff = 0, o_aval = o_aoff + up256((a_rows + 1) * 4), o_boff = o_aval + up256(abytes + 64),
                     o_bval = o_boff + up256((b_rows + 1) * 4), o_out = o_bval + up256(bbytes + 64), total = o_out + up256(n * 8);
        if (total > c->pin_cap) {
            if (c->pin) { HIP_TRY(hipHostFree(c->pin)); c->pin = nullptr; c->pin_cap = 0; }
            const size_t want = total + total / 4 + 4096;
            HIP_TRY(hipHostMalloc(&c->pin, want, hipHostMallocDefault));
            HIP_TRY(hipHostGetDevicePointer(&c->pin_dev, c->pin, 0));
            c->pin_cap = want;
        }
        uint8_t *h = static_cast<uint8_t *>(c->pin);
        const uint8_t *d = static_cast<const uint8_t *>(c->pin_dev);
        // the offsets are rebased to 0 on the way in, so that the kernels get the value blocks' real addresses (with the
        // caller's base kept and a pointer moved back by it, any kernel access at "offset 0" -- skipped rows of a block,
        // alignment of a staging copy -- would land a_off[0] bytes in front of the pinned block: a slice of a big column)
        {
            uint32_t *ha = reinterpret_cast<uint32_t *>(h + o_aoff), *hb = reinterpret_cast<uint32_t *>(h + o_boff);
            const uint32_t a0 = a_off[0], b0 = b_off[0];
            for (uint64_t i = 0; i <= a_rows; ++i) ha[i] = a_off[i] - a0;
            for (uint64_t i = 0; i <= b_rows; ++i) hb[i] = b_off[i] - b0;
        }
        if (abytes) memcpy(h + o_aval, a_val + a_off[0], abytes);
        if (bbytes) memcpy(h + o_bval, b_val + b_off[0], bbytes);
        rc = strsim_pairs_device_small(c, measure, (const uint32_t *)(d + o_aoff), d + o_aval, a_rows,
                                       (const uint32_t *)(d + o_boff), d + o_bval, b_rows,
                                       (double *)(const_cast<uint8_t *>(d) + o_out), n);
        if (rc) return rc;
        rc = strsim_ctx_synchronize(c); // also runs the long-string pass, which writes into the same block
        if (rc) return rc;
        memcpy(out, h + o_out, n * 8);
        return STRSIM_OK;
    }
    return elementwise_host(
        c, STRSIM_OK, a, b, n, out, n * 8, nullptr, 0,
        [&](const Staged &s, uint8_t *d_out, uint8_t *) { return pairs_device(c, measure, s.a, s.b, (double *)d_out, n); },
        [&] { return strsim_ctx_synchronize(c); });
}

int strsim_ctx_timing_enable(strsim_ctx_t *c, int enable)
{
    if (!c) { set_error("strsim_ctx_timing_enable: ctx is NULL"); return STRSIM_ERR_ARG; }
    int rc = strsim_ctx_synchronize(c);
    if (rc) return rc;
    c->timing = enable != 0;
    return STRSIM_OK;
}

int strsim_ctx_timing_read(strsim_ctx_t *c, double *lane_ms, uint64_t *lane_launches, double *wave_ms,
                           uint64_t *wave_launches)
{
    if (!c) { set_error("strsim_ctx_timing_read: ctx is NULL"); return STRSIM_ERR_ARG; }
    int rc = strsim_ctx_synchronize(c);
    if (rc) return rc;
    if (lane_ms) *lane_ms = c->lane_ms;
    if (lane_launches) *lane_launches = c->lane_launches;
    if (wave_ms) *wave_ms = c->wave_ms;
    if (wave_launches) *wave_launches = c->wave_launches;
    c->lane_ms = c->wave_ms = 0;
    c->lane_launches = c->wave_launches = 0;
    return STRSIM_OK;
}

uint64_t strsim_ctx_last_wave_rows(strsim_ctx_t *c) { return c ? c->last_wave_rows : 0; }
uint64_t strsim_ctx_last_long_rows(strsim_ctx_t *c) { return c ? c->last_long_rows : 0; }
uint64_t strsim_ctx_last_late_rows(strsim_ctx_t *c) { return c ? c->last_late_rows : 0; }
uint64_t strsim_ctx_enqueued_ops(strsim_ctx_t *c) { return c ? c->enqueued_ops : 0; }

int strsim_ctx_set_stream_ordered(strsim_ctx_t *c, int enable)
{
    if (!c) { set_error("strsim_ctx_set_stream_ordered: ctx is NULL"); return STRSIM_ERR_ARG; }
    c->stream_ordered = enable != 0;
    return STRSIM_OK;
}

int strsim_ctx_get_stream_ordered(strsim_ctx_t *c) { return c ? (c->stream_ordered ? 1 : 0) : 1; }

} // extern "C"

// ---- best match (strsim_match.h) ----

// Candidate splits of k_match_lane for nq queries x nc candidates: about eight workgroups of four waves per CU in all (a
// frame of few queries spreads its candidates over more workgroups), at least MATCH_MIN_PER_SPLIT candidates per split (a
// split writes a partial list per query that the merge reads back), and the partial lists within MATCH_MAX_PARTIAL entries.
static constexpr uint64_t MATCH_MIN_PER_SPLIT = 512;
static constexpr uint64_t MATCH_MAX_PARTIAL = (uint64_t)1 << 24;
static uint32_t match_splits(uint64_t nq, uint64_t nc, uint32_t kp, int num_cu)
{
    const uint64_t qblocks = (nq + 255) / 256;
    const uint64_t target = 8u * (uint64_t)(num_cu > 0 ? num_cu : 256);
    uint64_t s = (target + qblocks - 1) / qblocks;
    const uint64_t by_m = (nc + MATCH_MIN_PER_SPLIT - 1) / MATCH_MIN_PER_SPLIT;
    if (s > by_m) s = by_m;
    const uint64_t by_mem = MATCH_MAX_PARTIAL / (nq * kp);
    if (s > by_mem) s = by_mem;
    if (s > 65535u) s = 65535u;
    return s ? (uint32_t)s : 1u;
}

// fallback: scores of up to MATCH_FALLBACK_CALLS literal calls per batch, at most MATCH_FALLBACK_SCORES doubles
static constexpr uint64_t MATCH_FALLBACK_CALLS = 16;
static constexpr uint64_t MATCH_FALLBACK_SCORES = (uint64_t)1 << 24;

// The part of a search call's workspace that both families lay out alike: both sides packed by k_match_pack (32-byte words +
// meta) and their slow lists; `tail` is the family's own, and starts with the two slow counts.
struct SearchPack {
    Col q, c;        // the call's columns
    uint32_t nq, nc; // their rows
    uint32_t *qw, *qm, *cw, *cm, *qs, *cs;
    uint8_t *tail;
    uint32_t q_slow, c_slow; // strings k_match_pack could not pack
};

// Reserve `ws` for the common part + tail_bytes, zero the first zero_bytes of the tail, pack both sides and read the two slow
// counts back: they decide what runs (the only wait of a call without slow strings).
static int search_pack(strsim_ctx *c, DevBuf &ws, size_t tail_bytes, size_t zero_bytes, const Col &q, const Col &cnd, SearchPack *p)
{
    const uint32_t nq = (uint32_t)q.rows, nc = (uint32_t)cnd.rows;
    const size_t o_qw = 0, o_qm = o_qw + up256((size_t)nq * 32), o_cw = o_qm + up256((size_t)nq * 4), o_cm = o_cw + up256((size_t)nc * 32),
                 o_qs = o_cm + up256((size_t)nc * 4), o_cs = o_qs + up256((size_t)nq * 4), o_tail = o_cs + up256((size_t)nc * 4);
    int rc = ws.reserve(o_tail + tail_bytes);
    if (rc) return rc;
    if (!c->match_counts_host) HIP_TRY(hipHostMalloc((void **)&c->match_counts_host, 64, hipHostMallocDefault));
    uint8_t *const b = ws.as<uint8_t>();
    p->q = q; p->c = cnd; p->nq = nq; p->nc = nc;
    p->qw = (uint32_t *)(b + o_qw); p->qm = (uint32_t *)(b + o_qm); p->cw = (uint32_t *)(b + o_cw); p->cm = (uint32_t *)(b + o_cm);
    p->qs = (uint32_t *)(b + o_qs); p->cs = (uint32_t *)(b + o_cs); p->tail = b + o_tail;
    uint32_t *const cnt = (uint32_t *)p->tail;
    hipStream_t st = c->stream;
    HIP_TRY(hipMemsetAsync(cnt, 0, zero_bytes, st));
    HIP_TRY(launch_match_pack(q.off, q.val, nq, p->qw, p->qm, p->qs, cnt, st));
    HIP_TRY(launch_match_pack(cnd.off, cnd.val, nc, p->cw, p->cm, p->cs, cnt + 1, st));
    HIP_TRY(hipMemcpyAsync(c->match_counts_host, cnt, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    p->q_slow = c->match_counts_host[0];
    p->c_slow = c->match_counts_host[1];
    return STRSIM_OK;
}

static uint64_t fallback_calls(uint32_t nq, uint32_t nc)
{
    const uint64_t calls = MATCH_FALLBACK_SCORES / std::max(nq, nc);
    return std::min(std::max<uint64_t>(calls, 1), MATCH_FALLBACK_CALLS);
}

// Every pair with a slow side: that side as the literal of a call against the other column, `calls` of them per batch -- the slow
// queries against every candidate, then the slow candidates against every query.  score(side, literal, column, b) enqueues literal b
// of a batch; done(side, b0, nb) ends the batch of the slow strings b0 .. b0 + nb - 1 of side 0 (p.qs) or 1 (p.cs).
template <class Score, class Done>
static int slow_walk(strsim_ctx *c, const char *who, const SearchPack &p, uint64_t calls, Score score, Done done)
{
    hipStream_t st = c->stream;
    const uint32_t slow[2] = {p.q_slow, p.c_slow};
    const std::unique_ptr<uint32_t[]> host_list(new (std::nothrow) uint32_t[(size_t)slow[0] + slow[1] + 1]);
    if (!host_list) { set_error("%s: out of host memory", who); return STRSIM_ERR_OOM; }
    if (slow[0]) HIP_TRY(hipMemcpyAsync(host_list.get(), p.qs, (size_t)slow[0] * 4, hipMemcpyDeviceToHost, st));
    if (slow[1]) HIP_TRY(hipMemcpyAsync(host_list.get() + slow[0], p.cs, (size_t)slow[1] * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const Col *const col[2] = {&p.q, &p.c};
    for (int side = 0; side < 2; ++side) {
        const uint32_t *const list = host_list.get() + (side ? slow[0] : 0u);
        for (uint32_t b0 = 0; b0 < slow[side]; b0 += (uint32_t)calls) {
            const uint32_t nb = (uint32_t)(slow[side] - b0 < calls ? slow[side] - b0 : calls);
            for (uint32_t b = 0; b < nb; ++b) {
                int r = score(side, literal(*col[side], list[b0 + b]), *col[1 - side], b);
                if (r) return r;
            }
            int r = done(side, b0, nb);
            if (r) return r;
        }
    }
    return STRSIM_OK;
}

// The end of every search call: when `fallback` and a side has slow strings, every pair with a slow side goes through slow_walk,
// its batches in `scratch` (pair_bytes per pair, the f64 scores first), folded into list `used` (the fast ones of a slow candidate's
// queries are kept); then the lists are merged.  finish(scores) leaves a batch's `scores` scores, row b at b * rows, at the front of
// `scratch` for the fold; score / finish read their batch pointers from `scratch` when they run: it is reserved only here.
template <class Score, class Finish>
static int search_fallback_merge(strsim_ctx *c, const char *who, const SearchPack &p, uint32_t k, double min_score, bool fallback,
                                 DevBuf &scratch, size_t pair_bytes, uint32_t used, double *lscore, uint32_t *lidx, uint32_t *out_index,
                                 double *out_score, Score score, Finish finish)
{
    const uint32_t kp = (uint32_t)match_lane_k(k);
    hipStream_t st = c->stream;
    if (fallback && p.nc && (p.q_slow || p.c_slow)) {
        const uint64_t calls = fallback_calls(p.nq, p.nc);
        int rc = scratch.reserve((size_t)(calls * std::max(p.nq, p.nc) * pair_bytes));
        if (rc) return rc;
        const double *const batch = scratch.as<double>();
        double *const fs = lscore + (size_t)used * p.nq * kp;
        uint32_t *const fi = lidx + (size_t)used * p.nq * kp;
        HIP_TRY(launch_match_clear(fs, fi, (uint64_t)p.nq * kp, st));
        rc = slow_walk(c, who, p, calls, score, [&](int side, uint32_t b0, uint32_t nb) -> int {
            int r = finish((uint64_t)nb * (side ? p.nq : p.nc));
            if (r) return r;
            if (side == 0) HIP_TRY(launch_match_fold_cols(k, batch, p.qs + b0, nb, p.nc, min_score, fs, fi, st));
            else HIP_TRY(launch_match_fold_rows(k, batch, p.cs + b0, nb, p.qm, p.nq, min_score, fs, fi, st));
            return STRSIM_OK;
        });
        if (rc) return rc;
        ++used;
    }
    HIP_TRY(launch_match_merge(k, lscore, lidx, used, p.nq, out_index, out_score, st));
    return STRSIM_OK;
}

// A length-ordered search (nearest, extract) up to its lane launch.  The tail of its workspace: the small block (slow counts,
// histograms, bucket starts, cursors), the query permutation, the candidates in length order, (splits + 1) lists of kp per query
// (the last: the fallback) and extra_bytes of the family's own.
struct OrderedSearch {
    SearchPack p;
    SweepLaneArgs lane; // what the family's lane launch takes; lane.pscore / lane.pidx are the lists
    uint8_t *extra;
    bool fast;          // the length order is in place and the lane kernel has work: lists 0 .. splits - 1 are its
};
// `sweep`: the family admits a sweep at all (extract under a cutoff above 1.0 does not).
static int ordered_search_pack(strsim_ctx *c, DevBuf &ws, size_t extra_bytes, bool sweep, const Col &q, const Col &cnd, uint32_t k, OrderedSearch *o)
{
    const uint32_t nq = (uint32_t)q.rows, nc = (uint32_t)cnd.rows;
    const uint32_t kp = (uint32_t)match_lane_k(k);
    const uint32_t splits = nc ? match_splits(nq, nc, kp, c->num_cu) : 0u;
    const size_t lists = ((size_t)splits + 1) * nq * kp;
    const size_t o_qp = 1024, o_sw = o_qp + up256((size_t)nq * 4), o_sm = o_sw + up256((size_t)nc * 32), o_si = o_sm + up256((size_t)nc * 4),
                 o_ls = o_si + up256((size_t)nc * 4), o_li = o_ls + up256(lists * 8), o_ex = o_li + up256(lists * 4);
    SearchPack &p = o->p;
    // (of the small block, the counts and histograms are zeroed)
    int rc = search_pack(c, ws, o_ex + extra_bytes, 4 * 88, q, cnd, &p);
    if (rc) return rc;
    uint32_t *const small = (uint32_t *)p.tail;
    uint32_t *const qhist = small + 8, *const chist = qhist + 40, *const qstart = chist + 40, *const cstart = qstart + 40,
                   *const qcur = cstart + 40, *const ccur = qcur + 40;
    uint32_t *const qperm = (uint32_t *)(p.tail + o_qp), *const sw = (uint32_t *)(p.tail + o_sw), *const sm = (uint32_t *)(p.tail + o_sm),
                   *const si = (uint32_t *)(p.tail + o_si);
    o->lane = SweepLaneArgs{p.qw, p.qm, qperm, qstart, nq, sw, sm, si, cstart, splits, k, (double *)(p.tail + o_ls), (uint32_t *)(p.tail + o_li),
                            c->stream};
    o->extra = p.tail + o_ex;
    // fast x fast: length order on the device
    o->fast = sweep && splits && p.q_slow < nq && p.c_slow < nc;
    if (o->fast) {
        NearestOrderArgs oa{p.qm, nq, p.cw, p.cm, nc, qhist, chist, qstart, cstart, qcur, ccur, qperm, sw, sm, si, c->stream};
        HIP_TRY(launch_nearest_order(oa));
    }
    return STRSIM_OK;
}

// The *_host entry point of a search family behind its check (`checked`: what the check returned): both columns staged, the
// device entry point on the staged columns with outputs a then b in stage[4], the two copies back and the family's wait.
template <class A, class B, class Device, class Wait>
static int search_host(strsim_ctx *c, int checked, const Col &q, const Col &cnd, uint32_t k, A *out_a, B *out_b, Device device, Wait wait)
{
    if (checked || q.rows == 0) return checked;
    int rc = ctx_set_device(c);
    if (rc) return rc;
    const size_t ob = q.rows * (size_t)k;
    Staged s;
    rc = ctx_stage(c, q, cnd, ob * (sizeof(A) + sizeof(B)) + 256, &s);
    if (rc) return rc;
    A *const d_a = reinterpret_cast<A *>(s.out);
    B *const d_b = reinterpret_cast<B *>(s.out + up256(ob * sizeof(A)));
    rc = device(s, d_a, d_b);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(out_a, d_a, ob * sizeof(A), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(out_b, d_b, ob * sizeof(B), hipMemcpyDeviceToHost, c->stream));
    return wait();
}

static int best_match_check(const char *who, strsim_ctx_t *c, int measure, const Col &q, const Col &cnd, uint32_t k, double min_score,
                            const void *out_index, const void *out_score)
{
    if (!measure_accepted(measure, STRSIM_ENTRY_BEST_MATCH)) { set_error("%s: unknown measure %d", who, measure); return STRSIM_ERR_ARG; }
    return search_check(who, c, q, cnd, k, STRSIM_BEST_MATCH_MAX_K, min_score, out_index, out_score);
}

extern "C" {

int strsim_best_match_device(strsim_ctx_t *c, int measure, const uint32_t *q_off, const uint8_t *q_val, uint64_t q_rows,
                             const uint32_t *c_off, const uint8_t *c_val, uint64_t c_rows, uint32_t k, double min_score,
                             uint32_t *out_index, double *out_score)
{
    const Col q{q_off, q_val, q_rows}, cnd{c_off, c_val, c_rows};
    int rc = best_match_check("strsim_best_match_device", c, measure, q, cnd, k, min_score, out_index, out_score);
    if (rc || q_rows == 0) return rc;
    rc = ctx_set_device(c);
    if (rc) return rc;
    const uint32_t nq = (uint32_t)q_rows, nc = (uint32_t)c_rows, kp = (uint32_t)match_lane_k(k);
    const uint32_t splits = nc ? match_splits(nq, nc, kp, c->num_cu) : 0u;
    const uint32_t per = splits ? (uint32_t)(((uint64_t)nc + splits - 1) / splits) : 0u;
    const uint32_t nsplit = splits ? (uint32_t)(((uint64_t)nc + per - 1) / per) : 0u;
    // the tail of the workspace: the slow counts, then (nsplit + 1) lists of kp per query (the last: fallback)
    const size_t lists = ((size_t)nsplit + 1) * nq * kp;
    const size_t o_ls = 256, o_li = o_ls + up256(lists * 8);
    SearchPack p;
    rc = search_pack(c, c->match_ws, o_li + up256(lists * 4), 8, q, cnd, &p);
    if (rc) return rc;
    double *const lscore = (double *)(p.tail + o_ls);
    uint32_t *const lidx = (uint32_t *)(p.tail + o_li);
    hipStream_t st = c->stream;
    // fast x fast: lists 0 .. nsplit - 1
    uint32_t used = 0;
    if (nsplit && p.q_slow < nq && p.c_slow < nc) {
        MatchLaneArgs a{p.qw, p.qm, nq, p.cw, p.cm, nc, nsplit, per, k, c->qtab, min_score, lscore, lidx, st};
        HIP_TRY(launch_match_lane(measure, a));
        used = nsplit;
    }
    // every pair with a slow side: strsim_pairs_device with that side as the literal, batch by batch, folded into list `used`
    return search_fallback_merge(
        c, "strsim_best_match_device", p, k, min_score, true, c->match_scratch, 8, used, lscore, lidx, out_index, out_score,
        [&](int, const Col &lit, const Col &col, uint32_t b) {
            return pairs_device(c, measure, lit, col, c->match_scratch.as<double>() + (size_t)b * col.rows, col.rows);
        },
        [&](uint64_t) { return strsim_ctx_synchronize(c); });
}

int strsim_best_match_host(strsim_ctx_t *c, int measure, const uint32_t *q_off, const uint8_t *q_val, uint64_t q_rows,
                           const uint32_t *c_off, const uint8_t *c_val, uint64_t c_rows, uint32_t k, double min_score,
                           uint32_t *out_index, double *out_score)
{
    const Col q{q_off, q_val, q_rows}, cnd{c_off, c_val, c_rows};
    return search_host(
        c, best_match_check("strsim_best_match_host", c, measure, q, cnd, k, min_score, out_index, out_score), q, cnd, k, out_score, out_index,
        [&](const Staged &s, double *d_score, uint32_t *d_index) {
            return strsim_best_match_device(c, measure, s.a.off, s.a.val, q_rows, s.b.off, s.b.val, c_rows, k, min_score, d_index, d_score);
        },
        [&] { return strsim_ctx_synchronize(c); });
}

} // extern "C"

// ---- bounded distances (strsim_distance.h) ----

static int distance_check(const char *who, strsim_ctx_t *c, int measure, const Col &a, const Col &b, const uint32_t *out, uint64_t out_rows)
{
    if (measure != STRSIM_LEVENSHTEIN && measure != STRSIM_OSA && measure != STRSIM_INDEL) {
        set_error("%s: measure %d has no distance (STRSIM_LEVENSHTEIN, STRSIM_OSA or STRSIM_INDEL)", who, measure);
        return STRSIM_ERR_ARG;
    }
    return elementwise_check(who, c, a.rows, b.rows, out_rows, a.off && a.val && b.off && b.val && out);
}

// The status block of a distance or alignment call and its pinned read-back, and the work list for n rows.
static int dist_prepare(strsim_ctx *c, uint64_t n)
{
    int rc = ctx_set_device(c);
    if (rc) return rc;
    rc = c->osa_list.reserve(n * sizeof(uint32_t));
    if (rc) return rc;
    if (!c->dist_status) HIP_TRY(hipMalloc((void **)&c->dist_status, sizeof(DevStatus)));
    if (!c->dist_status_host) HIP_TRY(hipHostMalloc((void **)&c->dist_status_host, sizeof(DevStatus), hipHostMallocDefault));
    return STRSIM_OK;
}

// k_dist_lane, then k_dist_wave (Indel: k_indel_lane / k_indel_wave with the uint32 output, strsim_indel.h).
static int distance_device_impl(strsim_ctx_t *c, int measure, const Col &a, const Col &b, uint32_t k, uint32_t *out, uint64_t n)
{
    int rc = dist_prepare(c, n);
    if (rc) return rc;
    const LaunchArgs la = two_pass_args(c, a, b, nullptr, n, c->dist_status);
    return two_pass(c, la, TwoPassCall{measure == STRSIM_INDEL ? TP_INDEL : TP_DIST, measure, k, out, nullptr}, -1);
}

// strsim_distance_device, which the fallback of the nearest search calls with a literal.
static int distance_device(strsim_ctx *c, int measure, const Col &a, const Col &b, uint32_t max_distance, uint32_t *out, uint64_t out_rows)
{
    int rc = distance_check("strsim_distance_device", c, measure, a, b, out, out_rows);
    if (rc || out_rows == 0) return rc;
    return distance_device_impl(c, measure, a, b, max_distance, out, out_rows);
}

extern "C" {

int strsim_distance_device(strsim_ctx_t *c, int measure, const uint32_t *a_off, const uint8_t *a_val, uint64_t a_rows,
                           const uint32_t *b_off, const uint8_t *b_val, uint64_t b_rows, uint32_t max_distance, uint32_t *out,
                           uint64_t out_rows)
{
    return distance_device(c, measure, Col{a_off, a_val, a_rows}, Col{b_off, b_val, b_rows}, max_distance, out, out_rows);
}

int strsim_distance_host(strsim_ctx_t *c, int measure, const uint32_t *a_off, const uint8_t *a_val, uint64_t a_rows,
                         const uint32_t *b_off, const uint8_t *b_val, uint64_t b_rows, uint32_t max_distance, uint32_t *out,
                         uint64_t out_rows)
{
    const Col a{a_off, a_val, a_rows}, b{b_off, b_val, b_rows};
    return elementwise_host(
        c, distance_check("strsim_distance_host", c, measure, a, b, out, out_rows), a, b, out_rows, out, out_rows * 4, nullptr, 0,
        [&](const Staged &s, uint8_t *d_out, uint8_t *) { return distance_device_impl(c, measure, s.a, s.b, max_distance, (uint32_t *)d_out, out_rows); },
        nothing_to_settle);
}

} // extern "C"

// ---- q-gram similarity (strsim_qgram.h) ----

// kind, q and the mode flags of every q-gram entry point
static int qgram_kind_check(const char *who, int kind, uint32_t q, uint32_t flags)
{
    if (kind < STRSIM_QGRAM_JACCARD || kind > STRSIM_QGRAM_COSINE) {
        set_error("%s: unknown kind %d (STRSIM_QGRAM_JACCARD, _SORENSEN_DICE, _OVERLAP or _COSINE: 0..3)", who, kind);
        return STRSIM_ERR_ARG;
    }
    if (q < 1u || q > QGRAM_MAX_Q) { set_error("%s: q=%u is outside 1..%u", who, q, QGRAM_MAX_Q); return STRSIM_ERR_ARG; }
    if (flags & ~STRSIM_QGRAM_SET) {
        set_error("%s: unknown flag bits 0x%x (STRSIM_QGRAM_SET is the only flag)", who, flags & ~STRSIM_QGRAM_SET);
        return STRSIM_ERR_ARG;
    }
    return STRSIM_OK;
}

static int qgram_check(const char *who, strsim_ctx_t *c, int kind, uint32_t q, uint32_t flags, const Col &a, const Col &b, const double *out,
                       uint64_t out_rows)
{
    const int rc = qgram_kind_check(who, kind, q, flags);
    if (rc) return rc;
    return elementwise_check(who, c, a.rows, b.rows, out_rows, a.off && a.val && b.off && b.val && out);
}

// k_qgram_lane, then k_qgram_wave.  The size of the work list is what strsim_ctx_last_wave_rows reports (two_pass has waited for it).
static int qgram_device_impl(strsim_ctx_t *c, int kind, uint32_t q, uint32_t flags, const Col &a, const Col &b, double *out, uint64_t n)
{
    int rc = dist_prepare(c, n);
    if (rc) return rc;
    const LaunchArgs la = two_pass_args(c, a, b, out, n, c->dist_status);
    rc = two_pass(c, la, TwoPassCall{TP_QGRAM, kind, 0u, nullptr, nullptr, q, flags}, -1);
    if (rc) return rc;
    c->last_wave_rows = c->dist_status_host->wave_rows;
    return STRSIM_OK;
}

extern "C" {

int strsim_qgram_device(strsim_ctx_t *c, int kind, uint32_t q, uint32_t flags, const uint32_t *a_off, const uint8_t *a_val, uint64_t a_rows,
                        const uint32_t *b_off, const uint8_t *b_val, uint64_t b_rows, double *out, uint64_t out_rows)
{
    const Col a{a_off, a_val, a_rows}, b{b_off, b_val, b_rows};
    int rc = qgram_check("strsim_qgram_device", c, kind, q, flags, a, b, out, out_rows);
    if (rc || out_rows == 0) return rc;
    return qgram_device_impl(c, kind, q, flags, a, b, out, out_rows);
}

int strsim_qgram_host(strsim_ctx_t *c, int kind, uint32_t q, uint32_t flags, const uint32_t *a_off, const uint8_t *a_val, uint64_t a_rows,
                      const uint32_t *b_off, const uint8_t *b_val, uint64_t b_rows, double *out, uint64_t out_rows)
{
    const Col a{a_off, a_val, a_rows}, b{b_off, b_val, b_rows};
    return elementwise_host(
        c, qgram_check("strsim_qgram_host", c, kind, q, flags, a, b, out, out_rows), a, b, out_rows, out, out_rows * 8, nullptr, 0,
        [&](const Staged &s, uint8_t *d_out, uint8_t *) { return qgram_device_impl(c, kind, q, flags, s.a, s.b, (double *)d_out, out_rows); },
        nothing_to_settle);
}

} // extern "C"

// ---- unrestricted Damerau-Levenshtein similarity and distance (strsim_damerau.h) ----

// k_dl_lane, then k_dl_wave: the distances under the cutoff k into out32, or with out32 == nullptr the similarity into out.  The
// size of the work list is what strsim_ctx_last_wave_rows reports (two_pass has waited for it).
static int damerau_device_impl(strsim_ctx_t *c, const Col &a, const Col &b, uint32_t k, double *out, uint32_t *out32, uint64_t n)
{
    int rc = dist_prepare(c, n);
    if (rc) return rc;
    const LaunchArgs la = two_pass_args(c, a, b, out, n, c->dist_status);
    rc = two_pass(c, la, TwoPassCall{TP_DAMERAU, 0, k, out32, nullptr}, -1);
    if (rc) return rc;
    c->last_wave_rows = c->dist_status_host->wave_rows;
    return STRSIM_OK;
}

static int damerau_check(const char *who, strsim_ctx_t *c, const Col &a, const Col &b, const void *out, uint64_t out_rows)
{
    return elementwise_check(who, c, a.rows, b.rows, out_rows, a.off && a.val && b.off && b.val && out);
}

extern "C" {

int strsim_damerau_device(strsim_ctx_t *c, const uint32_t *a_off, const uint8_t *a_val, uint64_t a_rows, const uint32_t *b_off,
                          const uint8_t *b_val, uint64_t b_rows, double *out, uint64_t out_rows)
{
    const Col a{a_off, a_val, a_rows}, b{b_off, b_val, b_rows};
    int rc = damerau_check("strsim_damerau_device", c, a, b, out, out_rows);
    if (rc || out_rows == 0) return rc;
    return damerau_device_impl(c, a, b, DIST_UNBOUNDED, out, nullptr, out_rows);
}

int strsim_damerau_host(strsim_ctx_t *c, const uint32_t *a_off, const uint8_t *a_val, uint64_t a_rows, const uint32_t *b_off,
                        const uint8_t *b_val, uint64_t b_rows, double *out, uint64_t out_rows)
{
    const Col a{a_off, a_val, a_rows}, b{b_off, b_val, b_rows};
    return elementwise_host(
        c, damerau_check("strsim_damerau_host", c, a, b, out, out_rows), a, b, out_rows, out, out_rows * 8, nullptr, 0,
        [&](const Staged &s, uint8_t *d_out, uint8_t *) { return damerau_device_impl(c, s.a, s.b, DIST_UNBOUNDED, (double *)d_out, nullptr, out_rows); },
        nothing_to_settle);
}

int strsim_damerau_distance_device(strsim_ctx_t *c, const uint32_t *a_off, const uint8_t *a_val, uint64_t a_rows, const uint32_t *b_off,
                                   const uint8_t *b_val, uint64_t b_rows, uint32_t max_distance, uint32_t *out, uint64_t out_rows)
{
    const Col a{a_off, a_val, a_rows}, b{b_off, b_val, b_rows};
    int rc = damerau_check("strsim_damerau_distance_device", c, a, b, out, out_rows);
    if (rc || out_rows == 0) return rc;
    return damerau_device_impl(c, a, b, max_distance, nullptr, out, out_rows);
}

int strsim_damerau_distance_host(strsim_ctx_t *c, const uint32_t *a_off, const uint8_t *a_val, uint64_t a_rows, const uint32_t *b_off,
                                 const uint8_t *b_val, uint64_t b_rows, uint32_t max_distance, uint32_t *out, uint64_t out_rows)
{
    const Col a{a_off, a_val, a_rows}, b{b_off, b_val, b_rows};
    return elementwise_host(
        c, damerau_check("strsim_damerau_distance_host", c, a, b, out, out_rows), a, b, out_rows, out, out_rows * 4, nullptr, 0,
        [&](const Staged &s, uint8_t *d_out, uint8_t *) { return damerau_device_impl(c, s.a, s.b, max_distance, nullptr, (uint32_t *)d_out, out_rows); },
        nothing_to_settle);
}

} // extern "C"

// ---- Hamming, prefix, postfix and LCSseq (strsim_common.h) ----

static int common_check(const char *who, strsim_ctx_t *c, int kind, const Col &a, const Col &b, const void *out, uint64_t out_rows)
{
    if (kind < STRSIM_COMMON_HAMMING || kind > STRSIM_COMMON_LCSSEQ) {
        set_error("%s: unknown kind %d (STRSIM_COMMON_HAMMING, _PREFIX, _POSTFIX or _LCSSEQ: 0..3)", who, kind);
        return STRSIM_ERR_ARG;
    }
    return elementwise_check(who, c, a.rows, b.rows, out_rows, a.off && a.val && b.off && b.val && out);
}

// k_common_lane, then k_common_wave (LCSseq: k_common_lcs_lane / _wave): `out` holds what mode says (a CommonOut).  The size of the
// work list is what strsim_ctx_last_wave_rows reports (two_pass has waited for it).
static int common_device_impl(strsim_ctx_t *c, int kind, int mode, const Col &a, const Col &b, uint32_t k, void *out, uint64_t n)
{
    int rc = dist_prepare(c, n);
    if (rc) return rc;
    const LaunchArgs la = two_pass_args(c, a, b, nullptr, n, c->dist_status);
    TwoPassCall t{TP_COMMON, kind, k, nullptr, nullptr};
    t.mode = mode;
    t.out = out;
    rc = two_pass(c, la, t, -1);
    if (rc) return rc;
    c->last_wave_rows = c->dist_status_host->wave_rows;
    return STRSIM_OK;
}

static int common_device(const char *who, strsim_ctx_t *c, int kind, int mode, const Col &a, const Col &b, uint32_t k, void *out,
                         uint64_t out_rows)
{
    int rc = common_check(who, c, kind, a, b, out, out_rows);
    if (rc || out_rows == 0) return rc;
    return common_device_impl(c, kind, mode, a, b, k, out, out_rows);
}

static int common_host(const char *who, strsim_ctx_t *c, int kind, int mode, const Col &a, const Col &b, uint32_t k, void *out,
                       uint64_t out_rows)
{
    return elementwise_host(
        c, common_check(who, c, kind, a, b, out, out_rows), a, b, out_rows, out, out_rows * (mode == COMMON_OUT_SIM ? 8u : 4u), nullptr, 0,
        [&](const Staged &s, uint8_t *d_out, uint8_t *) { return common_device_impl(c, kind, mode, s.a, s.b, k, d_out, out_rows); },
        nothing_to_settle);
}

extern "C" {

int strsim_common_device(strsim_ctx_t *c, int kind, const uint32_t *a_off, const uint8_t *a_val, uint64_t a_rows, const uint32_t *b_off,
                         const uint8_t *b_val, uint64_t b_rows, double *out, uint64_t out_rows)
{
    return common_device("strsim_common_device", c, kind, COMMON_OUT_SIM, Col{a_off, a_val, a_rows}, Col{b_off, b_val, b_rows}, DIST_UNBOUNDED,
                         out, out_rows);
}

int strsim_common_host(strsim_ctx_t *c, int kind, const uint32_t *a_off, const uint8_t *a_val, uint64_t a_rows, const uint32_t *b_off,
                       const uint8_t *b_val, uint64_t b_rows, double *out, uint64_t out_rows)
{
    return common_host("strsim_common_host", c, kind, COMMON_OUT_SIM, Col{a_off, a_val, a_rows}, Col{b_off, b_val, b_rows}, DIST_UNBOUNDED, out,
                       out_rows);
}

int strsim_common_distance_device(strsim_ctx_t *c, int kind, const uint32_t *a_off, const uint8_t *a_val, uint64_t a_rows,
                                  const uint32_t *b_off, const uint8_t *b_val, uint64_t b_rows, uint32_t max_distance, uint32_t *out,
                                  uint64_t out_rows)
{
    return common_device("strsim_common_distance_device", c, kind, COMMON_OUT_DIST, Col{a_off, a_val, a_rows}, Col{b_off, b_val, b_rows},
                         max_distance, out, out_rows);
}

int strsim_common_distance_host(strsim_ctx_t *c, int kind, const uint32_t *a_off, const uint8_t *a_val, uint64_t a_rows,
                                const uint32_t *b_off, const uint8_t *b_val, uint64_t b_rows, uint32_t max_distance, uint32_t *out,
                                uint64_t out_rows)
{
    return common_host("strsim_common_distance_host", c, kind, COMMON_OUT_DIST, Col{a_off, a_val, a_rows}, Col{b_off, b_val, b_rows},
                       max_distance, out, out_rows);
}

int strsim_common_count_device(strsim_ctx_t *c, int kind, const uint32_t *a_off, const uint8_t *a_val, uint64_t a_rows,
                               const uint32_t *b_off, const uint8_t *b_val, uint64_t b_rows, uint32_t *out, uint64_t out_rows)
{
    return common_device("strsim_common_count_device", c, kind, COMMON_OUT_COUNT, Col{a_off, a_val, a_rows}, Col{b_off, b_val, b_rows},
                         DIST_UNBOUNDED, out, out_rows);
}

int strsim_common_count_host(strsim_ctx_t *c, int kind, const uint32_t *a_off, const uint8_t *a_val, uint64_t a_rows, const uint32_t *b_off,
                             const uint8_t *b_val, uint64_t b_rows, uint32_t *out, uint64_t out_rows)
{
    return common_host("strsim_common_count_host", c, kind, COMMON_OUT_COUNT, Col{a_off, a_val, a_rows}, Col{b_off, b_val, b_rows},
                       DIST_UNBOUNDED, out, out_rows);
}

} // extern "C"

// ---- partial ratio with its alignment (strsim_partial.h) ----

// k_partial_lane<ALIGN>, then k_partial_wave<ALIGN>.
static int partial_device_impl(strsim_ctx_t *c, const Col &a, const Col &b, double *out_score, uint32_t *out_span, uint64_t n)
{
    int rc = dist_prepare(c, n);
    if (rc) return rc;
    const LaunchArgs la = two_pass_args(c, a, b, out_score, n, c->dist_status);
    return two_pass(c, la, TwoPassCall{TP_PARTIAL, STRSIM_PARTIAL_RATIO, 0u, nullptr, out_span}, -1);
}

extern "C" {

int strsim_partial_alignment_device(strsim_ctx_t *c, const uint32_t *a_off, const uint8_t *a_val, uint64_t a_rows, const uint32_t *b_off,
                                    const uint8_t *b_val, uint64_t b_rows, double *out_score, uint32_t *out_span, uint64_t out_rows)
{
    int rc = elementwise_check("strsim_partial_alignment_device", c, a_rows, b_rows, out_rows, a_off && a_val && b_off && b_val && out_score && out_span);
    if (rc || out_rows == 0) return rc;
    return partial_device_impl(c, Col{a_off, a_val, a_rows}, Col{b_off, b_val, b_rows}, out_score, out_span, out_rows);
}

int strsim_partial_alignment_host(strsim_ctx_t *c, const uint32_t *a_off, const uint8_t *a_val, uint64_t a_rows, const uint32_t *b_off,
                                  const uint8_t *b_val, uint64_t b_rows, double *out_score, uint32_t *out_span, uint64_t out_rows)
{
    const int checked = elementwise_check("strsim_partial_alignment_host", c, a_rows, b_rows, out_rows, a_off && a_val && b_off && b_val && out_score && out_span);
    return elementwise_host(
        c, checked, Col{a_off, a_val, a_rows}, Col{b_off, b_val, b_rows}, out_rows, out_score, out_rows * 8, out_span, out_rows * 16,
        [&](const Staged &s, uint8_t *d_score, uint8_t *d_span) { return partial_device_impl(c, s.a, s.b, (double *)d_score, (uint32_t *)d_span, out_rows); },
        nothing_to_settle);
}

} // extern "C"

// ---- the token_sort transform itself (strsim_token.h) ----

// The checks of the two column transforms (token_sort here, default_process below).
static int transform_check(const char *who, strsim_ctx_t *c, const Col &col, const uint32_t *out_off, const uint8_t *out_val)
{
    if (col.rows > 0xFFFFFFFFull) {
        set_error("%s: %llu rows in one call; split the column (at most 2^32 - 1 rows per call)", who, (unsigned long long)col.rows);
        return STRSIM_ERR_ARG;
    }
    if (!col.off || !out_off || (col.rows && (!col.val || !out_val))) { set_error("%s: NULL buffer", who); return STRSIM_ERR_ARG; }
    if (!c) { set_error("%s: ctx is NULL", who); return STRSIM_ERR_ARG; }
    return STRSIM_OK;
}

// The *_host entry point of a transform behind its checks: the column staged (stage[0..1]), rows + 1 new offsets in stage[2] and room
// for `room` bytes of new values in stage[3], transform(column, offsets, values, &total) on them, the new column copied back.  A
// transform that learns the new column's byte size sets *total; otherwise it is read from the offsets once they are back.
static constexpr uint64_t TOTAL_UNKNOWN = ~(uint64_t)0;
template <class Transform>
static int transform_host(strsim_ctx *c, const Col &col, uint64_t room, uint32_t *out_off, uint8_t *out_val, Transform transform)
{
    if (col.rows == 0) { out_off[0] = 0u; return STRSIM_OK; }
    int rc = ctx_set_device(c);
    if (rc) return rc;
    Staged s;
    rc = ctx_stage(c, col, NO_COL, 0, &s);
    if (rc == STRSIM_OK) rc = c->stage[2].reserve((col.rows + 1) * sizeof(uint32_t));
    if (rc == STRSIM_OK) rc = c->stage[3].reserve(room + TOKEN_PAD);
    if (rc) return rc;
    uint32_t *const d_off = c->stage[2].as<uint32_t>();
    uint8_t *const d_val = c->stage[3].as<uint8_t>();
    uint64_t total = TOTAL_UNKNOWN;
    rc = transform(s.a, d_off, d_val, &total);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(out_off, d_off, (col.rows + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (total == TOTAL_UNKNOWN) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        total = out_off[col.rows];
    }
    if (total) HIP_TRY(hipMemcpyAsync(out_val, d_val, total, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return STRSIM_OK;
}

extern "C" {

int strsim_token_sort_device(strsim_ctx_t *c, const uint32_t *off, const uint8_t *val, uint64_t rows, uint32_t *out_off, uint8_t *out_val,
                             uint64_t out_capacity)
{
    const Col col{off, val, rows};
    int rc = transform_check("strsim_token_sort_device", c, col, out_off, out_val);
    if (rc) return rc;
    rc = token_prepare(c);
    if (rc) return rc;
    if (rows == 0) {
        HIP_TRY(hipMemsetAsync(out_off, 0, sizeof(uint32_t), c->stream));
        return STRSIM_OK;
    }
    rc = token_bounds(c, col, nullptr);
    if (rc) return rc;
    const ColBounds bd = token_col_bounds(c);
    if (out_capacity < bd.bytes[0]) {
        set_error("strsim_token_sort_device: out_capacity=%llu but the column holds %llu bytes (its byte size always suffices)",
                  (unsigned long long)out_capacity, (unsigned long long)bd.bytes[0]);
        return STRSIM_ERR_ARG;
    }
    rc = token_sort_column(c, 0, col, bd.max_len[0], out_off, out_val);
    if (rc) return rc;
    return token_copy_counts(c);
}

int strsim_token_sort_host(strsim_ctx_t *c, const uint32_t *off, const uint8_t *val, uint64_t rows, uint32_t *out_off, uint8_t *out_val,
                           uint64_t out_capacity)
{
    const Col col{off, val, rows};
    int rc = transform_check("strsim_token_sort_host", c, col, out_off, out_val);
    if (rc) return rc;
    const uint64_t bytes = (uint64_t)off[rows] - off[0];
    if (out_capacity < bytes) {
        set_error("strsim_token_sort_host: out_capacity=%llu but the column holds %llu bytes (its byte size always suffices)",
                  (unsigned long long)out_capacity, (unsigned long long)bytes);
        return STRSIM_ERR_ARG;
    }
    return transform_host(c, col, bytes, out_off, out_val, [&](const Col &d, uint32_t *d_off, uint8_t *d_val, uint64_t *) {
        return strsim_token_sort_device(c, d.off, d.val, rows, d_off, d_val, bytes);
    });
}

uint64_t strsim_ctx_last_token_wave_rows(strsim_ctx_t *c)
{
    if (!c || !c->tok_status_host) return 0;
    const volatile uint32_t *w = c->tok_status_host->wave_rows;
    return (uint64_t)w[0] + w[1];
}

int strsim_ctx_last_wratio_rows(strsim_ctx_t *c, uint64_t *near_rows, uint64_t *far_rows)
{
    if (near_rows) *near_rows = c ? c->last_wratio_rows[0] : 0;
    if (far_rows) *far_rows = c ? c->last_wratio_rows[1] : 0;
    if (!c) { set_error("strsim_ctx_last_wratio_rows: ctx is NULL"); return STRSIM_ERR_ARG; }
    return STRSIM_OK;
}

} // extern "C"

// ---- default_process and processed scoring (strsim_process.h) ----
//
// The transform of a column is the measuring pass, the offset scan and the writing pass.  Between the scan and the writing pass the
// host learns how many bytes the processed column holds (the last offset) -- a processed row can be longer than its input, so only
// that figure sizes the values exactly -- together with the column's bounds and the work-list count: one wait for the stream, for
// both sides of a processed-scoring call.

static ProcessTable process_host_table() { return ProcessTable{PROCESS_BLOCK, PROCESS_CLASS, PROCESS_DELTA}; }

static int process_prepare(strsim_ctx *c, ProcessTable *t)
{
    int rc = ctx_set_device(c);
    if (rc) return rc;
    if (!c->proc_status) HIP_TRY(hipMalloc((void **)&c->proc_status, sizeof(TokenStatus)));
    if (!c->proc_status_host) HIP_TRY(hipHostMalloc((void **)&c->proc_status_host, sizeof(TokenStatus), hipHostMallocDefault));
    if (!c->proc_table_ready) {
        rc = c->proc_table.reserve(PROCESS_TABLE_BYTES);
        if (rc) return rc;
        uint8_t *d = c->proc_table.as<uint8_t>();
        // (static tables: pageable copies, complete for the host when the calls return)
        HIP_TRY(hipMemcpy(d, PROCESS_BLOCK, sizeof(PROCESS_BLOCK), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d + PROCESS_TABLE_CLASS_AT, PROCESS_CLASS, sizeof(PROCESS_CLASS), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d + PROCESS_TABLE_DELTA_AT, PROCESS_DELTA, sizeof(PROCESS_DELTA), hipMemcpyHostToDevice));
        c->proc_table_ready = true;
    }
    const uint8_t *d = c->proc_table.as<uint8_t>();
    *t = ProcessTable{d, d + PROCESS_TABLE_CLASS_AT, reinterpret_cast<const int32_t *>(d + PROCESS_TABLE_DELTA_AT)};
    // strsim_ctx_last_process_wave_rows describes THIS call from here on: one without rows, or one that fails before its wait,
    // reports 0 (nothing on the stream writes this block now: every call that copies into it has waited for the copy)
    c->proc_status_host->wave_rows[0] = c->proc_status_host->wave_rows[1] = 0u;
    return STRSIM_OK;
}

// The pairwise call of an earlier strsim_pairs_processed_device may still be pending (a ring measure is retired by the caller, and
// its long-string or deferred pass reads its input columns again then): those columns are proc_off / proc_val, which the next call
// overwrites and may reallocate.  So every pending call is retired before they are touched -- a wait for the stream and the
// retirement passes, exactly what the wrap of the ring does; what they finished late is kept for the caller's next
// strsim_ctx_synchronize / strsim_ctx_retire_oldest.
static int process_retire_pending(strsim_ctx *c, const char *who)
{
    bool pending = false;
    for (int s = 0; s < strsim_ctx::RING; ++s) pending = pending || c->slot_pending[s];
    if (!pending) return STRSIM_OK;
    HIP_TRY(hipStreamSynchronize(c->stream));
    const int rc = ctx_drain(c);
    c->carry_late_rows += c->last_late_rows;
    c->carry_long_rows += c->last_long_rows;
    if (rc) {
        const std::string why = strsim_last_error_message();
        set_error("%s: retiring earlier pending calls failed (this call was not enqueued): %s", who, why.c_str());
        return STRSIM_ERR_EARLIER_CALL;
    }
    return STRSIM_OK;
}

static int process_wave_grid(const strsim_ctx *c) { return c->num_cu * 8; }

// Bounds, measuring pass and scan of one column (side 0 or 1 of c->proc_status, zeroed by the caller): out_off becomes the
// processed column's offsets, and its last word is on its way to c->proc_status_host->pad[side].
static int process_measure(strsim_ctx *c, int side, const ProcessTable &t, const Col &col, uint32_t *out_off)
{
    const uint64_t rows = col.rows;
    int rc = c->proc_list[side].reserve(rows * sizeof(uint32_t));
    if (rc) return rc;
    rc = c->proc_sums.reserve(((rows + 4095u) / 4096u) * sizeof(uint32_t));
    if (rc) return rc;
    HIP_TRY(launch_token_bounds(col.off, rows, c->proc_status, side, c->stream));
    hipError_t e = launch_process(false, col.off, col.val, rows, out_off, nullptr, c->proc_list[side].as<uint32_t>(), &c->proc_status->wave_rows[side],
                                  process_wave_grid(c), t, c->stream);
    if (e != hipSuccess) return hip_fail(e, "kernel launch (k_process_lane / _wave, measuring)");
    e = launch_token_scan(out_off, rows, c->proc_sums.as<uint32_t>(), c->stream);
    if (e != hipSuccess) return hip_fail(e, "kernel launch (k_token_scan)");
    HIP_TRY(hipMemcpyAsync(&c->proc_status_host->pad[side], out_off + rows, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    c->enqueued_ops += 7u;
    return STRSIM_OK;
}

// The wait of a call: the status words of both sides (not the pad words, which the copies above fill) reach the host.
static int process_wait(strsim_ctx *c)
{
    HIP_TRY(hipMemcpyAsync(c->proc_status_host, c->proc_status, offsetof(TokenStatus, pad), hipMemcpyDeviceToHost, c->stream));
    c->enqueued_ops += 1u;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return STRSIM_OK;
}

// A column whose processed form might not fit 32-bit offsets is refused (the scan would have wrapped).
static int process_check_size(const char *who, const strsim_ctx *c, int side)
{
    const TokenStatus &st = *c->proc_status_host;
    const uint64_t bytes = (uint64_t)st.end[side] - st.begin[side];
    if (STRSIM_DEFAULT_PROCESS_CAPACITY(bytes) > 0xFFFFFFFFull) {
        set_error("%s: a column of %llu bytes may not fit 32-bit offsets once processed; split the column (bytes + bytes / 2 <= 2^32 - 1)",
                  who, (unsigned long long)bytes);
        return STRSIM_ERR_ARG;
    }
    return STRSIM_OK;
}

static int process_write(strsim_ctx *c, int side, const ProcessTable &t, const Col &col, uint32_t *out_off, uint8_t *out_val)
{
    hipError_t e = launch_process(true, col.off, col.val, col.rows, out_off, out_val, c->proc_list[side].as<uint32_t>(), &c->proc_status->wave_rows[side],
                                  process_wave_grid(c), t, c->stream);
    if (e != hipSuccess) return hip_fail(e, "kernel launch (k_process_lane / _wave, writing)");
    c->enqueued_ops += 2u;
    return STRSIM_OK;
}

static int process_capacity_error(const char *who, uint64_t capacity, uint64_t total)
{
    set_error("%s: out_capacity=%llu but the processed column holds %llu bytes (bytes + bytes / 2 of the input always suffices)", who,
              (unsigned long long)capacity, (unsigned long long)total);
    return STRSIM_ERR_ARG;
}

static int pairs_processed_check(const char *who, strsim_ctx_t *c, int measure, int processor, const Col &a, const Col &b, const double *out,
                                 uint64_t out_rows, uint64_t *n)
{
    if (processor != STRSIM_PROCESS_DEFAULT) {
        set_error("%s: unknown processor %d (STRSIM_PROCESS_DEFAULT = 1 is the only one)", who, processor);
        return STRSIM_ERR_ARG;
    }
    if (!measure_accepted(measure, STRSIM_ENTRY_PAIRWISE)) { set_error("%s: unknown measure %d", who, measure); return STRSIM_ERR_ARG; }
    int rc = check_rows(who, a.rows, b.rows, out_rows, n);
    if (rc) return rc;
    if (*n && (!a.off || !a.val || !b.off || !b.val || !out)) { set_error("%s: NULL buffer", who); return STRSIM_ERR_ARG; }
    if (!c) { set_error("%s: ctx is NULL", who); return STRSIM_ERR_ARG; }
    return STRSIM_OK;
}

extern "C" {

uint32_t strsim_default_process_char(uint32_t cp) { return process_map(cp, process_host_table()); }

const char *strsim_default_process_unicode_version(void) { return STRSIM_PROCESS_UNICODE_VERSION; }

int strsim_default_process_device(strsim_ctx_t *c, const uint32_t *off, const uint8_t *val, uint64_t rows, uint32_t *out_off, uint8_t *out_val,
                                  uint64_t out_capacity)
{
    const char *const who = "strsim_default_process_device";
    const Col col{off, val, rows};
    int rc = transform_check(who, c, col, out_off, out_val);
    if (rc) return rc;
    ProcessTable t;
    rc = process_prepare(c, &t);
    if (rc) return rc;
    if (rows == 0) {
        HIP_TRY(hipMemsetAsync(out_off, 0, sizeof(uint32_t), c->stream));
        return STRSIM_OK;
    }
    HIP_TRY(hipMemsetAsync(c->proc_status, 0, sizeof(TokenStatus), c->stream));
    c->enqueued_ops += 1u;
    rc = process_measure(c, 0, t, col, out_off);
    if (rc == STRSIM_OK) rc = process_wait(c);
    if (rc == STRSIM_OK) rc = process_check_size(who, c, 0);
    if (rc) return rc;
    const uint64_t total = c->proc_status_host->pad[0];
    if (out_capacity < total) return process_capacity_error(who, out_capacity, total);
    return process_write(c, 0, t, col, out_off, out_val);
}

int strsim_default_process_host(strsim_ctx_t *c, const uint32_t *off, const uint8_t *val, uint64_t rows, uint32_t *out_off, uint8_t *out_val,
                                uint64_t out_capacity)
{
    const char *const who = "strsim_default_process_host";
    const Col col{off, val, rows};
    int rc = transform_check(who, c, col, out_off, out_val);
    if (rc) return rc;
    const uint64_t room = STRSIM_DEFAULT_PROCESS_CAPACITY((uint64_t)off[rows] - off[0]);
    return transform_host(c, col, room, out_off, out_val, [&](const Col &d, uint32_t *d_off, uint8_t *d_val, uint64_t *total) {
        const int r = strsim_default_process_device(c, d.off, d.val, rows, d_off, d_val, room);
        if (r) return r;
        *total = c->proc_status_host->pad[0]; // (the device call has waited for it)
        return out_capacity < *total ? process_capacity_error(who, out_capacity, *total) : STRSIM_OK;
    });
}

int strsim_pairs_processed_device(strsim_ctx_t *c, int measure, int processor, const uint32_t *a_off, const uint8_t *a_val, uint64_t a_rows,
                                  const uint32_t *b_off, const uint8_t *b_val, uint64_t b_rows, double *out, uint64_t out_rows)
{
    const char *const who = "strsim_pairs_processed_device";
    const Col a{a_off, a_val, a_rows}, b{b_off, b_val, b_rows};
    uint64_t n;
    int rc = pairs_processed_check(who, c, measure, processor, a, b, out, out_rows, &n);
    if (rc || n == 0) return rc;
    ProcessTable t;
    rc = process_prepare(c, &t);
    if (rc == STRSIM_OK) rc = process_retire_pending(c, who);
    if (rc) return rc;
    const Col *const side[2] = {&a, &b};
    for (int s = 0; s < 2; ++s) {
        rc = c->proc_off[s].reserve((side[s]->rows + 1) * sizeof(uint32_t));
        if (rc) return rc;
    }
    HIP_TRY(hipMemsetAsync(c->proc_status, 0, sizeof(TokenStatus), c->stream));
    c->enqueued_ops += 1u;
    for (int s = 0; s < 2; ++s) {
        rc = process_measure(c, s, t, *side[s], c->proc_off[s].as<uint32_t>());
        if (rc) return rc;
    }
    rc = process_wait(c); // the one wait of the transform: both sides' totals
    for (int s = 0; s < 2 && rc == STRSIM_OK; ++s) rc = process_check_size(who, c, s);
    for (int s = 0; s < 2 && rc == STRSIM_OK; ++s) rc = c->proc_val[s].reserve((size_t)c->proc_status_host->pad[s] + TOKEN_PAD);
    for (int s = 0; s < 2 && rc == STRSIM_OK; ++s)
        rc = process_write(c, s, t, *side[s], c->proc_off[s].as<uint32_t>(), c->proc_val[s].as<uint8_t>());
    if (rc) return rc;
    return pairs_device(c, measure, dev_col(c->proc_off[0], c->proc_val[0], a_rows), dev_col(c->proc_off[1], c->proc_val[1], b_rows), out, out_rows);
}

int strsim_pairs_processed_host(strsim_ctx_t *c, int measure, int processor, const uint32_t *a_off, const uint8_t *a_val, uint64_t a_rows,
                                const uint32_t *b_off, const uint8_t *b_val, uint64_t b_rows, double *out, uint64_t out_rows)
{
    const Col a{a_off, a_val, a_rows}, b{b_off, b_val, b_rows};
    uint64_t n = 0;
    const int checked = pairs_processed_check("strsim_pairs_processed_host", c, measure, processor, a, b, out, out_rows, &n);
    return elementwise_host(
        c, checked, a, b, n, out, n * 8, nullptr, 0,
        [&](const Staged &s, uint8_t *d_out, uint8_t *) {
            return strsim_pairs_processed_device(c, measure, processor, s.a.off, s.a.val, a_rows, s.b.off, s.b.val, b_rows, (double *)d_out, n);
        },
        [&] { return strsim_ctx_synchronize(c); });
}

uint64_t strsim_ctx_last_process_wave_rows(strsim_ctx_t *c)
{
    if (!c || !c->proc_status_host) return 0;
    const volatile uint32_t *w = c->proc_status_host->wave_rows;
    return (uint64_t)w[0] + w[1];
}

} // extern "C"

// ---- nearest match (strsim_nearest.h, strsim_nearest_kernels.h) ----

static int nearest_check(const char *who, strsim_ctx_t *c, int measure, const Col &q, const Col &cnd, uint32_t k, const void *out_index,
                         const void *out_distance)
{
    if (measure != STRSIM_LEVENSHTEIN && measure != STRSIM_OSA) {
        set_error("%s: measure %d has no distance (STRSIM_LEVENSHTEIN or STRSIM_OSA)", who, measure);
        return STRSIM_ERR_ARG;
    }
    return search_check(who, c, q, cnd, k, STRSIM_NEAREST_MAX_K, 0.0, out_index, out_distance);
}

extern "C" {

int strsim_nearest_device(strsim_ctx_t *c, int measure, const uint32_t *q_off, const uint8_t *q_val, uint64_t q_rows,
                          const uint32_t *c_off, const uint8_t *c_val, uint64_t c_rows, uint32_t k, uint32_t max_distance,
                          uint32_t *out_index, uint32_t *out_distance)
{
    const Col q{q_off, q_val, q_rows}, cnd{c_off, c_val, c_rows};
    int rc = nearest_check("strsim_nearest_device", c, measure, q, cnd, k, out_index, out_distance);
    if (rc || q_rows == 0) return rc;
    rc = ctx_set_device(c);
    if (rc) return rc;
    const uint32_t nq = (uint32_t)q_rows, nc = (uint32_t)c_rows;
    const size_t ob = (size_t)nq * k;
    OrderedSearch o; // (extra: the merged scores)
    rc = ordered_search_pack(c, c->nearest_ws, up256(ob * 8), true, q, cnd, k, &o);
    if (rc) return rc;
    if (o.fast) HIP_TRY(launch_nearest_lane(measure, NearestLaneArgs{o.lane, max_distance}));
    // every pair with a slow side: strsim_distance_device with that side as the literal (its length prefilter and block cutoff
    // apply), batch by batch, folded into list `used` as the scores -(double)d; a batch's distances lie behind its scores
    hipStream_t st = c->stream;
    double *const mscore = (double *)o.extra;
    const uint64_t pairs = fallback_calls(nq, nc) * std::max(nq, nc);
    auto dist = [&] { return reinterpret_cast<uint32_t *>(c->nearest_scratch.as<double>() + pairs); };
    rc = search_fallback_merge(
        c, "strsim_nearest_device", o.p, k, -(double)max_distance /* a cut pair comes back as max_distance + 1 */, true, c->nearest_scratch, 12,
        o.fast ? o.lane.splits : 0u, o.lane.pscore, o.lane.pidx, out_index, mscore,
        [&](int, const Col &lit, const Col &col, uint32_t b) {
            return distance_device(c, measure, lit, col, max_distance, dist() + (size_t)b * col.rows, col.rows);
        },
        [&](uint64_t count) -> int { HIP_TRY(launch_nearest_scores(dist(), count, c->nearest_scratch.as<double>(), st)); return STRSIM_OK; });
    if (rc) return rc;
    HIP_TRY(launch_nearest_finish(mscore, out_index, ob, out_distance, st));
    return STRSIM_OK;
}

int strsim_nearest_host(strsim_ctx_t *c, int measure, const uint32_t *q_off, const uint8_t *q_val, uint64_t q_rows,
                        const uint32_t *c_off, const uint8_t *c_val, uint64_t c_rows, uint32_t k, uint32_t max_distance,
                        uint32_t *out_index, uint32_t *out_distance)
{
    const Col q{q_off, q_val, q_rows}, cnd{c_off, c_val, c_rows};
    return search_host(
        c, nearest_check("strsim_nearest_host", c, measure, q, cnd, k, out_index, out_distance), q, cnd, k, out_index, out_distance,
        [&](const Staged &s, uint32_t *d_index, uint32_t *d_dist) {
            return strsim_nearest_device(c, measure, s.a.off, s.a.val, q_rows, s.b.off, s.b.val, c_rows, k, max_distance, d_index, d_dist);
        },
        [&]() -> int { HIP_TRY(hipStreamSynchronize(c->stream)); return STRSIM_OK; });
}

} // extern "C"

// ---- extract: top-k by Indel similarity with a score cutoff (strsim_extract.h, strsim_extract_kernels.h) ----

static int extract_check(const char *who, strsim_ctx_t *c, int scorer, const Col &q, const Col &cnd, uint32_t k, double score_cutoff,
                         const void *out_index, const void *out_score)
{
    if (scorer != STRSIM_INDEL && scorer != STRSIM_TOKEN_SORT_RATIO) {
        set_error("%s: scorer %d is not a scorer of extract (STRSIM_INDEL = 8 or STRSIM_TOKEN_SORT_RATIO = 14)", who, scorer);
        return STRSIM_ERR_ARG;
    }
    if (score_cutoff != score_cutoff) { set_error("%s: score_cutoff is NaN", who); return STRSIM_ERR_ARG; }
    return search_check(who, c, q, cnd, k, STRSIM_EXTRACT_MAX_K, score_cutoff, out_index, out_score);
}

// The rank table of strsim_extract.h, built once per process.
static const ExtractTable &extract_table()
{
    static const ExtractTable *const t = [] {
        ExtractTable *n = new ExtractTable;
        extract_build_table(*n);
        return n;
    }();
    return *t;
}

// The search over two columns of Indel scores (for STRSIM_TOKEN_SORT_RATIO: the normalised ones).
static int extract_search(strsim_ctx *c, const Col &q, const Col &cnd, uint32_t k, double score_cutoff, uint32_t *out_index, double *out_score)
{
    const ExtractTable &tab = extract_table();
    hipStream_t st = c->stream;
    if (!c->extract_tab_ready) {
        int rc = c->extract_tab.reserve(sizeof(ExtractTable));
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(c->extract_tab.p, &tab, sizeof(ExtractTable), hipMemcpyHostToDevice, st));
        c->extract_tab_ready = true;
    }
    const uint32_t rlimit = extract_rank_limit(tab, score_cutoff); // 0: the cutoff is above 1.0 and nothing is reported
    OrderedSearch o;
    int rc = ordered_search_pack(c, c->extract_ws, 0, rlimit != 0u, q, cnd, k, &o);
    if (rc) return rc;
    if (o.fast) HIP_TRY(launch_extract_lane(ExtractLaneArgs{o.lane, c->extract_tab.as<ExtractTable>(), rlimit}));
    // every pair with a slow side: strsim_pairs_device(STRSIM_INDEL) with that side as the literal, batch by batch, folded into
    // list `used` with score_cutoff as the least score
    return search_fallback_merge(
        c, "strsim_extract_device", o.p, k, score_cutoff, rlimit != 0u, c->extract_scratch, 8, o.fast ? o.lane.splits : 0u, o.lane.pscore,
        o.lane.pidx, out_index, out_score,
        [&](int, const Col &lit, const Col &col, uint32_t b) {
            return pairs_device(c, STRSIM_INDEL, lit, col, c->extract_scratch.as<double>() + (size_t)b * col.rows, col.rows);
        },
        [&](uint64_t) { return strsim_ctx_synchronize(c); });
}

extern "C" {

int strsim_extract_device(strsim_ctx_t *c, int scorer, const uint32_t *q_off, const uint8_t *q_val, uint64_t q_rows,
                          const uint32_t *c_off, const uint8_t *c_val, uint64_t c_rows, uint32_t k, double score_cutoff,
                          uint32_t *out_index, double *out_score)
{
    Col q{q_off, q_val, q_rows}, cnd{c_off, c_val, c_rows};
    int rc = extract_check("strsim_extract_device", c, scorer, q, cnd, k, score_cutoff, out_index, out_score);
    if (rc || q_rows == 0) return rc;
    rc = ctx_set_device(c);
    if (rc) return rc;
    // token_sort_ratio: both sides through the token_sort transform into the context's own columns, on the device
    if (scorer == STRSIM_TOKEN_SORT_RATIO && (rc = token_sort_search_columns(c, &q, &cnd)) != STRSIM_OK) return rc;
    return extract_search(c, q, cnd, k, score_cutoff, out_index, out_score);
}

int strsim_extract_host(strsim_ctx_t *c, int scorer, const uint32_t *q_off, const uint8_t *q_val, uint64_t q_rows,
                        const uint32_t *c_off, const uint8_t *c_val, uint64_t c_rows, uint32_t k, double score_cutoff,
                        uint32_t *out_index, double *out_score)
{
    const Col q{q_off, q_val, q_rows}, cnd{c_off, c_val, c_rows};
    return search_host(
        c, extract_check("strsim_extract_host", c, scorer, q, cnd, k, score_cutoff, out_index, out_score), q, cnd, k, out_score, out_index,
        [&](const Staged &s, double *d_score, uint32_t *d_index) {
            return strsim_extract_device(c, scorer, s.a.off, s.a.val, q_rows, s.b.off, s.b.val, c_rows, k, score_cutoff, d_index, d_score);
        },
        [&] { return strsim_ctx_synchronize(c); });
}

} // extern "C"

// ---- cdist: the full score matrix (strsim_cdist.h, strsim_cdist_kernels.h) ----

static bool cdist_measure(int m) { return (m >= STRSIM_LEVENSHTEIN && m <= STRSIM_SORENSEN_DICE) || m == STRSIM_INDEL || m == STRSIM_TOKEN_SORT_RATIO; }

static int cdist_check(const char *who, strsim_ctx_t *c, int measure, const Col &q, const Col &cnd, double score_cutoff, const double *out,
                       uint64_t out_ld)
{
    if (!cdist_measure(measure)) {
        set_error("%s: measure %d is not a measure of cdist (the reference measures 0 .. 4, STRSIM_INDEL = 8 or STRSIM_TOKEN_SORT_RATIO = 14)", who,
                  measure);
        return STRSIM_ERR_ARG;
    }
    if (score_cutoff != score_cutoff) { set_error("%s: score_cutoff is NaN", who); return STRSIM_ERR_ARG; }
    int rc = search_rows_check(who, q, cnd);
    if (rc) return rc;
    if (out_ld < cnd.rows) {
        set_error("%s: out_ld=%llu is less than the %llu candidates of a row", who, (unsigned long long)out_ld, (unsigned long long)cnd.rows);
        return STRSIM_ERR_ARG;
    }
    if (q.rows && (!q.off || !q.val)) { set_error("%s: NULL query buffer", who); return STRSIM_ERR_ARG; }
    rc = candidate_buffers_check(who, cnd);
    if (rc) return rc;
    if (q.rows && cnd.rows && !out) { set_error("%s: NULL output buffer", who); return STRSIM_ERR_ARG; }
    if (!c) { set_error("%s: ctx is NULL", who); return STRSIM_ERR_ARG; }
    return STRSIM_OK;
}

// The Indel score table of strsim_cdist.h, built once per process.
static const double *cdist_indel_table()
{
    static const double *const t = [] {
        double *n = new double[CDIST_TAB_N];
        cdist_build_indel_table(n);
        return n;
    }();
    return t;
}

// The matrix of one pairwise measure (0 .. 4 or STRSIM_INDEL) over two columns (for STRSIM_TOKEN_SORT_RATIO: the normalised ones).
static int cdist_matrix(strsim_ctx *c, int measure, const Col &q, const Col &cnd, double cutoff, double *out, uint64_t ld)
{
    hipStream_t st = c->stream;
    const uint32_t nq = (uint32_t)q.rows, nc = (uint32_t)cnd.rows;
    const double *tab = c->qtab;
    if (measure == STRSIM_INDEL) {
        if (!c->cdist_tab_ready) {
            int rc = c->cdist_tab.reserve(CDIST_TAB_N * sizeof(double));
            if (rc) return rc;
            HIP_TRY(hipMemcpyAsync(c->cdist_tab.p, cdist_indel_table(), CDIST_TAB_N * sizeof(double), hipMemcpyHostToDevice, st));
            c->cdist_tab_ready = true;
        }
        tab = c->cdist_tab.as<double>();
    }
    SearchPack p; // (tail: the two slow counts)
    int rc = search_pack(c, c->cdist_ws, 256, 8, q, cnd, &p);
    if (rc) return rc;
    c->enqueued_ops += 4u;
    // fast x fast; a pair with a slow side is written as 0.0 here and by the fallback below, which is enqueued behind this grid
    if (p.q_slow < nq && p.c_slow < nc) {
        const uint32_t splits = cdist_splits(nq, nc, c->num_cu);
        const uint32_t per = (uint32_t)(((uint64_t)nc + splits - 1) / splits);
        const uint32_t nsplit = (uint32_t)(((uint64_t)nc + per - 1) / per);
        HIP_TRY(launch_cdist_lane(measure, CdistLaneArgs{p.qw, p.qm, nq, p.cw, p.cm, nc, nsplit, per, tab, cutoff, out, ld, st}));
        c->enqueued_ops += 1u;
    }
    if (!p.q_slow && !p.c_slow) return STRSIM_OK;

    // every pair with a slow side: strsim_pairs_device with that side as the literal, batch by batch (slow_walk) -- a slow query straight
    // into its row, a slow candidate into a scratch column and from there into its column; a batch is waited for (the long-string
    // pass of a pairwise call writes from strsim_ctx_synchronize)
    const uint64_t calls = fallback_calls(nq, nc);
    if (p.c_slow) {
        rc = c->cdist_scratch.reserve((size_t)calls * nq * sizeof(double));
        if (rc) return rc;
    }
    double *const col = c->cdist_scratch.as<double>();
    return slow_walk(
        c, "strsim_cdist_device", p, calls,
        [&](int side, const Col &lit, const Col &other, uint32_t b) { // (a literal's row: where its offsets start in its column)
            double *const to = side == 0 ? out + cdist_index((uint32_t)(lit.off - q.off), ld, 0) : col + (size_t)b * nq;
            return pairs_device(c, measure, lit, other, to, other.rows);
        },
        [&](int side, uint32_t b0, uint32_t nb) -> int {
            const int r = strsim_ctx_synchronize(c);
            if (r) return r;
            if (side == 1) HIP_TRY(launch_cdist_put_col(col, p.cs + b0, nb, p.qm, nq, cutoff, out, ld, st));
            else if (cutoff > 0.0) HIP_TRY(launch_cdist_cutoff(out, p.qs + b0, nb, nc, ld, cutoff, st));
            return STRSIM_OK;
        });
}

extern "C" {

int strsim_cdist_device(strsim_ctx_t *c, int measure, const uint32_t *q_off, const uint8_t *q_val, uint64_t q_rows, const uint32_t *c_off,
                        const uint8_t *c_val, uint64_t c_rows, double score_cutoff, double *out, uint64_t out_ld)
{
    Col q{q_off, q_val, q_rows}, cnd{c_off, c_val, c_rows};
    int rc = cdist_check("strsim_cdist_device", c, measure, q, cnd, score_cutoff, out, out_ld);
    if (rc || q_rows == 0 || c_rows == 0) return rc;
    rc = ctx_set_device(c);
    if (rc) return rc;
    if (measure == STRSIM_TOKEN_SORT_RATIO) { // both sides through the token_sort transform, as in strsim_extract_device; then their Indel scores
        rc = token_sort_search_columns(c, &q, &cnd);
        if (rc) return rc;
        measure = STRSIM_INDEL;
    }
    return cdist_matrix(c, measure, q, cnd, score_cutoff, out, out_ld);
}

int strsim_cdist_host(strsim_ctx_t *c, int measure, const uint32_t *q_off, const uint8_t *q_val, uint64_t q_rows, const uint32_t *c_off,
                      const uint8_t *c_val, uint64_t c_rows, double score_cutoff, double *out, uint64_t out_ld)
{
    const Col q{q_off, q_val, q_rows}, cnd{c_off, c_val, c_rows};
    int rc = cdist_check("strsim_cdist_host", c, measure, q, cnd, score_cutoff, out, out_ld);
    if (rc || q_rows == 0 || c_rows == 0) return rc;
    rc = ctx_set_device(c);
    if (rc) return rc;
    const size_t row_bytes = (size_t)c_rows * sizeof(double);
    Staged s;
    rc = ctx_stage(c, q, cnd, (size_t)q_rows * row_bytes + 16, &s);
    if (rc) return rc;
    double *const d_out = reinterpret_cast<double *>(s.out);
    rc = strsim_cdist_device(c, measure, s.a.off, s.a.val, q_rows, s.b.off, s.b.val, c_rows, score_cutoff, d_out, c_rows);
    if (rc) return rc;
    HIP_TRY(hipMemcpy2DAsync(out, (size_t)out_ld * sizeof(double), d_out, row_bytes, row_bytes, (size_t)q_rows, hipMemcpyDeviceToHost, c->stream));
    return strsim_ctx_synchronize(c);
}

} // extern "C"

// ---- threshold join: every pair at or above a score cutoff, as CSR (strsim_join.h, strsim_join_kernels.h) ----

// What the two families of entry points word differently: which ids they take, the sentence that refuses another (one %s, one %d)
// and the name of the cutoff.
struct JoinWords {
    bool (*accepts)(int);
    const char *refusal, *cutoff;
};
static const JoinWords JOIN_WORDS = {[](int id) { return id == STRSIM_INDEL || id == STRSIM_TOKEN_SORT_RATIO; },
                                     "%s: scorer %d is not a scorer of join (STRSIM_INDEL = 8 or STRSIM_TOKEN_SORT_RATIO = 14)", "score_cutoff"};
static const JoinWords MATCH_JOIN_WORDS = {[](int id) { return id >= STRSIM_LEVENSHTEIN && id <= STRSIM_SORENSEN_DICE; },
                                           "%s: measure %d is not a measure of match_join (the reference measures 0 .. 4)", "min_score"};

// What every join entry point checks behind its scorer (or kind, q and flags), the context last; `cutoff`: the name of the cutoff.
static int join_rest_check(const char *cutoff, const char *who, strsim_ctx_t *c, const Col &q, const Col &cnd, double score_cutoff, uint32_t flags,
                           uint64_t capacity, const uint64_t *out_indptr, const uint32_t *out_index, const double *out_score, const uint64_t *out_nnz)
{
    if (score_cutoff != score_cutoff) { set_error("%s: %s is NaN", who, cutoff); return STRSIM_ERR_ARG; }
    if (flags & ~STRSIM_JOIN_UPPER) { set_error("%s: unknown flags 0x%x (STRSIM_JOIN_UPPER = 1)", who, flags); return STRSIM_ERR_ARG; }
    int rc = search_rows_check(who, q, cnd);
    if (rc) return rc;
    if (q.rows && (!q.off || !q.val)) { set_error("%s: NULL query buffer", who); return STRSIM_ERR_ARG; }
    rc = candidate_buffers_check(who, cnd);
    if (rc) return rc;
    if (!out_nnz) { set_error("%s: out_nnz is NULL", who); return STRSIM_ERR_ARG; }
    if (!out_indptr) { set_error("%s: out_indptr is NULL", who); return STRSIM_ERR_ARG; }
    if (capacity && (!out_index || !out_score)) {
        set_error("%s: capacity=%llu with a NULL output buffer", who, (unsigned long long)capacity);
        return STRSIM_ERR_ARG;
    }
    if (!c) { set_error("%s: ctx is NULL", who); return STRSIM_ERR_ARG; }
    return STRSIM_OK;
}

static int join_check(const JoinWords &words, const char *who, strsim_ctx_t *c, int scorer, const Col &q, const Col &cnd, double score_cutoff,
                      uint32_t flags, uint64_t capacity, const uint64_t *out_indptr, const uint32_t *out_index, const double *out_score,
                      const uint64_t *out_nnz)
{
    if (!words.accepts(scorer)) {
        set_error(words.refusal, who, scorer);
        return STRSIM_ERR_ARG;
    }
    return join_rest_check(words.cutoff, who, c, q, cnd, score_cutoff, flags, capacity, out_indptr, out_index, out_score, out_nnz);
}

// The join over two columns, q.rows >= 1, by the scores of one pairwise measure.  What a family of entry points brings: `who` (for
// the fallback's errors), `nothing` (the cutoff is above every score: no sweep), ready() (the sweep's table on the device; called
// only when there is a sweep to come), sweep(fill, args) (the launcher of its lane sweep) and slow_score(lit, other, to) (the
// fallback's pairwise call: the scores of the literal `lit` against the column `other` into `to`, complete in stream order).
// strsim_join_*: Indel ranks (for STRSIM_TOKEN_SORT_RATIO over the normalised columns); strsim_match_join_*: the f64 score of a
// reference measure, both with strsim_pairs_device behind slow_score; strsim_qgram_join_*: the f64 q-gram score, with
// strsim_qgram_device's flow behind it.  Waits for the stream: once for the slow counts (search_pack), once
// for nnz; the fallback waits for every batch of its pairwise calls (in the count pass, and again in the fill when their scores
// were too many to keep).
template <class Ready, class Sweep, class SlowScore>
static int join_pairs(strsim_ctx *c, const char *who, const Col &q, const Col &cnd, double cutoff, uint32_t flags, uint64_t capacity,
                      uint64_t *out_indptr, uint32_t *out_index, double *out_score, uint64_t *out_nnz, bool nothing, Ready ready, Sweep sweep,
                      SlowScore slow_score)
{
    hipStream_t st = c->stream;
    const uint32_t nq = (uint32_t)q.rows, nc = (uint32_t)cnd.rows;
    const uint32_t upper = flags & STRSIM_JOIN_UPPER;
    *out_nnz = 0;
    if (nothing || nc == 0u) { // no hit anywhere: no sweep
        HIP_TRY(hipMemsetAsync(out_indptr, 0, ((size_t)nq + 1) * sizeof(uint64_t), st));
        c->enqueued_ops += 1u;
        return STRSIM_OK;
    }
    {
        const int rc = ready();
        if (rc) return rc;
    }
    // the tail of the workspace: the small block of ordered_search_pack (slow counts, histograms, bucket starts, cursors; its last
    // two words: nnz), the query permutation, the candidates in length order, (splits + 1) counts and one cursor per query, the
    // block sums of the scan and the hit map of the sweeps
    const uint32_t splits = join_splits(nq, nc, c->num_cu);
    const size_t o_qp = 1024, o_sw = o_qp + up256((size_t)nq * 4), o_sm = o_sw + up256((size_t)nc * 32), o_si = o_sm + up256((size_t)nc * 4),
                 o_cnt = o_si + up256((size_t)nc * 4), o_cur = o_cnt + up256(((size_t)splits + 1) * nq * 4), o_sums = o_cur + up256((size_t)nq * 4),
                 o_map = o_sums + up256((size_t)join_scan_blocks(nq) * 8);
    const uint32_t map_shift = join_map_shift(nq, nc, splits);
    const uint64_t map_words = join_map_words(nc, splits, map_shift);
    const size_t o_end = o_map + up256((size_t)(((uint64_t)nq + 63u) / 64u * map_words * 4u));
    SearchPack p;
    int rc = search_pack(c, c->join_ws, o_end, 4 * 88, q, cnd, &p);
    if (rc) return rc;
    c->enqueued_ops += 4u;
    uint32_t *const small = (uint32_t *)p.tail;
    uint32_t *const qhist = small + 8, *const chist = qhist + 40, *const qstart = chist + 40, *const cstart = qstart + 40,
                   *const qcur = cstart + 40, *const ccur = qcur + 40;
    uint32_t *const qperm = (uint32_t *)(p.tail + o_qp), *const sw = (uint32_t *)(p.tail + o_sw), *const sm = (uint32_t *)(p.tail + o_sm),
                   *const si = (uint32_t *)(p.tail + o_si), *const cnt = (uint32_t *)(p.tail + o_cnt), *const cur = (uint32_t *)(p.tail + o_cur);
    uint64_t *const sums = (uint64_t *)(p.tail + o_sums);
    const bool fast = p.q_slow < nq && p.c_slow < nc;
    const bool slow = p.q_slow || p.c_slow;
    const uint32_t ns = fast ? splits : 0u; // lists of the sweep; list ns is the fallback's
    uint32_t *const fb = cnt + (size_t)ns * nq;
    JoinLaneArgs la{p.qw, p.qm, qperm, qstart, nq, sw, sm, si, cstart, splits, upper, cnt,
                    (uint32_t *)(p.tail + o_map), map_words, map_shift, out_indptr, out_index, out_score, st};
    JoinSlowArgs sa{c->join_scratch.as<double>(), nullptr, 0u, p.qm, nq, nc, cutoff, upper, fb, cur, out_indptr, out_index, out_score, st};
    const uint64_t calls = fallback_calls(nq, nc);
    // every pair with a slow side: slow_score with that side as the literal, batch by batch (slow_walk), a batch
    // waited for and then counted into the fallback's list.  The columns of scores are kept for the fill when they fit
    // JOIN_KEEP_SCORES doubles (the slow queries' columns first, then the slow candidates'); otherwise a batch reuses the scratch and
    // the fill walks, scores and waits again.
    const uint64_t slow_scores = (uint64_t)p.q_slow * nc + (uint64_t)p.c_slow * nq;
    const bool keep = slow_scores <= JOIN_KEEP_SCORES;
    auto kept_column = [&](int side, uint64_t b) { // column b of a side's kept scores
        return c->join_scratch.as<double>() + (side ? (size_t)p.q_slow * nc : (size_t)0) + (size_t)b * (side ? nq : nc);
    };
    uint64_t walked[2] = {0, 0}; // slow strings of each side whose batch is done
    auto slow_pass = [&](bool fill) -> int {
        if (fill && keep) { // no pairwise call, no wait: the kept columns, at most 32 768 per launch (grid.y)
            for (int side = 0; side < 2; ++side) {
                const uint32_t n = side ? p.c_slow : p.q_slow;
                for (uint32_t b0 = 0; b0 < n; b0 += 32768u) {
                    sa.scores = kept_column(side, b0);
                    sa.list = (side ? p.cs : p.qs) + b0;
                    sa.nb = n - b0 < 32768u ? n - b0 : 32768u;
                    HIP_TRY(launch_join_slow(side, true, sa));
                    c->enqueued_ops += 1u;
                }
            }
            return STRSIM_OK;
        }
        return slow_walk(
            c, who, p, calls,
            [&](int side, const Col &lit, const Col &other, uint32_t b) {
                double *const to = keep ? kept_column(side, walked[side] + b) : c->join_scratch.as<double>() + (size_t)b * other.rows;
                return slow_score(lit, other, to);
            },
            [&](int side, uint32_t b0, uint32_t nb) -> int {
                const int r = strsim_ctx_synchronize(c);
                if (r) return r;
                sa.scores = keep ? kept_column(side, b0) : c->join_scratch.as<double>();
                sa.list = (side ? p.cs : p.qs) + b0;
                sa.nb = nb;
                HIP_TRY(launch_join_slow(side, fill, sa));
                c->enqueued_ops += 1u;
                walked[side] = (uint64_t)b0 + nb;
                return STRSIM_OK;
            });
    };

    // count
    HIP_TRY(hipMemsetAsync(fb, 0, (size_t)nq * 4, st));
    c->enqueued_ops += 1u;
    if (fast) {
        NearestOrderArgs oa{p.qm, nq, p.cw, p.cm, nc, qhist, chist, qstart, cstart, qcur, ccur, qperm, sw, sm, si, st};
        HIP_TRY(launch_nearest_order(oa));
        HIP_TRY(sweep(false, la));
        c->enqueued_ops += 6u;
    }
    if (slow) {
        rc = c->join_scratch.reserve((size_t)(keep ? slow_scores : calls * std::max(nq, nc)) * sizeof(double));
        if (rc) return rc;
        rc = slow_pass(false);
        if (rc) return rc;
    }
    // counts -> indptr, and nnz back: the call's second wait
    HIP_TRY(launch_join_indptr(cnt, nq, ns + 1u, out_indptr, sums, st));
    uint64_t *const nnz_host = reinterpret_cast<uint64_t *>(c->match_counts_host) + 1; // (search_pack's pinned block: 64 bytes)
    HIP_TRY(hipMemcpyAsync(nnz_host, out_indptr + nq, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    c->enqueued_ops += 5u;
    const uint64_t nnz = *nnz_host;
    *out_nnz = nnz;
    if (nnz == 0u || nnz > capacity) return STRSIM_OK; // count only: not one element of out_index / out_score is touched

    // fill: the same sweep over the same order, then the fallback again, then every row by candidate index
    if (fast) {
        HIP_TRY(sweep(true, la));
        c->enqueued_ops += 1u;
    }
    if (slow) {
        HIP_TRY(hipMemsetAsync(cur, 0, (size_t)nq * 4, st));
        c->enqueued_ops += 1u;
        rc = slow_pass(true);
        if (rc) return rc;
    }
    HIP_TRY(launch_join_sort_rows(out_indptr, nq, nc, out_index, out_score, st));
    c->enqueued_ops += nc < 2u ? 0u : nc > JOIN_SORT_WAVE_MAX ? 2u : 1u;
    return STRSIM_OK;
}

// The host-resident form of a join entry point behind its check (`checked`: what the check returned): the columns staged,
// device_call(queries, candidates, indptr, index, score) -- the family's *_device entry point on the staged columns with the
// caller's cutoff, flags, capacity and out_nnz --, the results copied back.
typedef int (*JoinDeviceFn)(strsim_ctx_t *, int, const uint32_t *, const uint8_t *, uint64_t, const uint32_t *, const uint8_t *, uint64_t, double, uint32_t,
                            uint64_t, uint64_t *, uint32_t *, double *, uint64_t *);
template <class DeviceCall>
static int join_host(int checked, DeviceCall device_call, strsim_ctx_t *c, const Col &q, const Col &cnd, uint64_t capacity, uint64_t *out_indptr,
                     uint32_t *out_index, double *out_score, uint64_t *out_nnz)
{
    int rc = checked;
    if (rc) return rc;
    *out_nnz = 0;
    out_indptr[0] = 0;
    if (q.rows == 0) return STRSIM_OK;
    rc = ctx_set_device(c);
    if (rc) return rc;
    const size_t ptr_bytes = up256(((size_t)q.rows + 1) * sizeof(uint64_t)), idx_bytes = up256((size_t)capacity * sizeof(uint32_t));
    Staged s;
    rc = ctx_stage(c, q, cnd, ptr_bytes + idx_bytes + (size_t)capacity * sizeof(double) + 256, &s);
    if (rc) return rc;
    uint64_t *const d_ptr = reinterpret_cast<uint64_t *>(s.out);
    uint32_t *const d_idx = capacity ? reinterpret_cast<uint32_t *>(s.out + ptr_bytes) : nullptr;
    double *const d_score = capacity ? reinterpret_cast<double *>(s.out + ptr_bytes + idx_bytes) : nullptr;
    rc = device_call(Col{s.a.off, s.a.val, q.rows}, Col{s.b.off, s.b.val, cnd.rows}, d_ptr, d_idx, d_score);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(out_indptr, d_ptr, ((size_t)q.rows + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    if (*out_nnz && *out_nnz <= capacity) {
        HIP_TRY(hipMemcpyAsync(out_index, d_idx, (size_t)*out_nnz * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(out_score, d_score, (size_t)*out_nnz * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    }
    return strsim_ctx_synchronize(c);
}

extern "C" {

int strsim_join_device(strsim_ctx_t *c, int scorer, const uint32_t *q_off, const uint8_t *q_val, uint64_t q_rows, const uint32_t *c_off,
                       const uint8_t *c_val, uint64_t c_rows, double score_cutoff, uint32_t flags, uint64_t capacity, uint64_t *out_indptr,
                       uint32_t *out_index, double *out_score, uint64_t *out_nnz)
{
    Col q{q_off, q_val, q_rows}, cnd{c_off, c_val, c_rows};
    int rc = join_check(JOIN_WORDS, "strsim_join_device", c, scorer, q, cnd, score_cutoff, flags, capacity, out_indptr, out_index, out_score, out_nnz);
    if (rc) return rc;
    rc = ctx_set_device(c);
    if (rc) return rc;
    if (q_rows == 0) {
        *out_nnz = 0;
        HIP_TRY(hipMemsetAsync(out_indptr, 0, sizeof(uint64_t), c->stream));
        return STRSIM_OK;
    }
    // token_sort_ratio: both sides through the token_sort transform, as in strsim_extract_device (its bounds wait); then their Indel scores
    if (scorer == STRSIM_TOKEN_SORT_RATIO && c_rows && (rc = token_sort_search_columns(c, &q, &cnd)) != STRSIM_OK) return rc;
    const ExtractTable &tab = extract_table();
    const uint32_t rlimit = extract_rank_limit(tab, score_cutoff); // 0: the cutoff is above 1.0 and nothing is reported
    return join_pairs(
        c, "strsim_join_device", q, cnd, score_cutoff, flags, capacity, out_indptr, out_index, out_score, out_nnz, rlimit == 0u,
        [&]() -> int {
            if (c->extract_tab_ready) return STRSIM_OK;
            const int r = c->extract_tab.reserve(sizeof(ExtractTable));
            if (r) return r;
            HIP_TRY(hipMemcpyAsync(c->extract_tab.p, &tab, sizeof(ExtractTable), hipMemcpyHostToDevice, c->stream));
            c->extract_tab_ready = true;
            return STRSIM_OK;
        },
        [&](bool fill, const JoinLaneArgs &a) { return launch_join_lane(fill, a, c->extract_tab.as<ExtractTable>(), rlimit); },
        [&](const Col &lit, const Col &other, double *to) { return pairs_device(c, STRSIM_INDEL, lit, other, to, other.rows); });
}

int strsim_join_host(strsim_ctx_t *c, int scorer, const uint32_t *q_off, const uint8_t *q_val, uint64_t q_rows, const uint32_t *c_off,
                     const uint8_t *c_val, uint64_t c_rows, double score_cutoff, uint32_t flags, uint64_t capacity, uint64_t *out_indptr,
                     uint32_t *out_index, double *out_score, uint64_t *out_nnz)
{
    const Col q{q_off, q_val, q_rows}, cnd{c_off, c_val, c_rows};
    return join_host(
        join_check(JOIN_WORDS, "strsim_join_host", c, scorer, q, cnd, score_cutoff, flags, capacity, out_indptr, out_index, out_score, out_nnz),
        [&](const Col &dq, const Col &dc, uint64_t *d_ptr, uint32_t *d_idx, double *d_score) {
            return strsim_join_device(c, scorer, dq.off, dq.val, dq.rows, dc.off, dc.val, dc.rows, score_cutoff, flags, capacity, d_ptr, d_idx, d_score,
                                      out_nnz);
        },
        c, q, cnd, capacity, out_indptr, out_index, out_score, out_nnz);
}

// ---- threshold join by the five reference measures (strsim_match_join.h, strsim_match_join_kernels.h): join_pairs with another sweep ----

int strsim_match_join_device(strsim_ctx_t *c, int measure, const uint32_t *q_off, const uint8_t *q_val, uint64_t q_rows, const uint32_t *c_off,
                             const uint8_t *c_val, uint64_t c_rows, double min_score, uint32_t flags, uint64_t capacity, uint64_t *out_indptr,
                             uint32_t *out_index, double *out_score, uint64_t *out_nnz)
{
    const Col q{q_off, q_val, q_rows}, cnd{c_off, c_val, c_rows};
    int rc = join_check(MATCH_JOIN_WORDS, "strsim_match_join_device", c, measure, q, cnd, min_score, flags, capacity, out_indptr, out_index, out_score,
                        out_nnz);
    if (rc) return rc;
    rc = ctx_set_device(c);
    if (rc) return rc;
    if (q_rows == 0) {
        *out_nnz = 0;
        HIP_TRY(hipMemsetAsync(out_indptr, 0, sizeof(uint64_t), c->stream));
        return STRSIM_OK;
    }
    MatchJoinNeed need; // which candidate lengths a query of each length visits: 33 words, a kernel argument
    const bool some = match_join_need_mask(measure, min_score, need);
    return join_pairs(
        c, "strsim_match_join_device", q, cnd, min_score, flags, capacity, out_indptr, out_index, out_score, out_nnz, !some,
        []() -> int { return STRSIM_OK; }, // (the quotient table is the context's, on the device since the context was made)
        [&](bool fill, const JoinLaneArgs &a) { return launch_match_join_lane(measure, fill, a, c->qtab, need, min_score); },
        [&](const Col &lit, const Col &other, double *to) { return pairs_device(c, measure, lit, other, to, other.rows); });
}

int strsim_match_join_host(strsim_ctx_t *c, int measure, const uint32_t *q_off, const uint8_t *q_val, uint64_t q_rows, const uint32_t *c_off,
                           const uint8_t *c_val, uint64_t c_rows, double min_score, uint32_t flags, uint64_t capacity, uint64_t *out_indptr,
                           uint32_t *out_index, double *out_score, uint64_t *out_nnz)
{
    const Col q{q_off, q_val, q_rows}, cnd{c_off, c_val, c_rows};
    return join_host(
        join_check(MATCH_JOIN_WORDS, "strsim_match_join_host", c, measure, q, cnd, min_score, flags, capacity, out_indptr, out_index, out_score, out_nnz),
        [&](const Col &dq, const Col &dc, uint64_t *d_ptr, uint32_t *d_idx, double *d_score) {
            return strsim_match_join_device(c, measure, dq.off, dq.val, dq.rows, dc.off, dc.val, dc.rows, min_score, flags, capacity, d_ptr, d_idx,
                                            d_score, out_nnz);
        },
        c, q, cnd, capacity, out_indptr, out_index, out_score, out_nnz);
}

} // extern "C"

// ---- connected components of a CSR graph and the fused cluster call (strsim_components.h, strsim_components_kernels.h) ----

static int components_check(const char *who, strsim_ctx_t *c, uint64_t rows, const uint64_t *indptr, const uint32_t *index, uint64_t nnz,
                            const uint32_t *out_root, const uint64_t *out_count)
{
    if (rows > 0xFFFFFFFFull) { set_error("%s: %llu rows (at most 2^32 - 1)", who, (unsigned long long)rows); return STRSIM_ERR_ARG; }
    if (!indptr) { set_error("%s: indptr is NULL", who); return STRSIM_ERR_ARG; }
    if (nnz && !index) { set_error("%s: index is NULL with nnz=%llu", who, (unsigned long long)nnz); return STRSIM_ERR_ARG; }
    if (rows && !out_root) { set_error("%s: out_root is NULL", who); return STRSIM_ERR_ARG; }
    if (!out_count) { set_error("%s: out_count is NULL", who); return STRSIM_ERR_ARG; }
    if (!c) { set_error("%s: ctx is NULL", who); return STRSIM_ERR_ARG; }
    return STRSIM_OK;
}

// The labels of a device-resident CSR graph, rows >= 1, behind the check.  nnz == 0: one launch, no wait.  Otherwise
// COMPONENTS_LAUNCHES launches and one copy whatever the graph holds, and the call's one wait: the count and the number of
// indices out of range come back together.
static int components_labels(strsim_ctx *c, const char *who, uint32_t rows, const uint64_t *indptr, const uint32_t *index, uint64_t nnz,
                             uint32_t *out_root, uint32_t *out_cluster, uint64_t *out_count)
{
    hipStream_t st = c->stream;
    if (nnz == 0u) {
        HIP_TRY(launch_components_identity(rows, out_root, out_cluster, st));
        c->enqueued_ops += 1u;
        *out_count = rows;
        return STRSIM_OK;
    }
    const size_t o_parent = 256, o_scan = o_parent + up256((size_t)rows * 4), o_sums = o_scan + up256((size_t)rows * 8),
                 o_end = o_sums + up256((size_t)join_scan_blocks(rows) * 8);
    int rc = c->components_ws.reserve(o_end);
    if (rc) return rc;
    if (!c->components_host) HIP_TRY(hipHostMalloc((void **)&c->components_host, 64, hipHostMallocDefault));
    uint8_t *const b = c->components_ws.as<uint8_t>();
    uint64_t *const status = (uint64_t *)b;
    ComponentsArgs a{indptr, index, rows, nnz, (uint32_t *)(b + o_parent), (uint64_t *)(b + o_scan), (uint64_t *)(b + o_sums), status,
                     out_root, out_cluster, st};
    HIP_TRY(launch_components(a));
    HIP_TRY(hipMemcpyAsync(c->components_host, status, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    c->enqueued_ops += COMPONENTS_LAUNCHES + 1u;
    *out_count = c->components_host[0];
    if (c->components_host[1]) {
        set_error("%s: index out of range (%llu of %llu edges name a row >= rows=%u; they were skipped)", who,
                  (unsigned long long)c->components_host[1], (unsigned long long)nnz, rows);
        return STRSIM_ERR_ARG;
    }
    return STRSIM_OK;
}

// Which join flow a measure of cluster runs: 0 .. 4 strsim_match_join_device, 8 and 14 strsim_join_device; nullptr: refused.
static JoinDeviceFn cluster_join(int measure)
{
    if (MATCH_JOIN_WORDS.accepts(measure)) return strsim_match_join_device;
    if (JOIN_WORDS.accepts(measure)) return strsim_join_device;
    return nullptr;
}

// The self-join of strsim_cluster_*: the join flow of `measure` over one column under STRSIM_JOIN_UPPER.
static auto cluster_self_join(strsim_ctx *c, int measure)
{
    const JoinDeviceFn join = cluster_join(measure);
    return [=](const Col &col, double min_score, uint64_t cap, uint64_t *indptr, uint32_t *index, double *score, uint64_t *nnz) {
        return join(c, measure, col.off, col.val, col.rows, col.off, col.val, col.rows, min_score, STRSIM_JOIN_UPPER, cap, indptr, index, score, nnz);
    };
}

// What every cluster entry point checks behind its measure (or kind, q and flags), the context last.
static int cluster_rest_check(const char *who, strsim_ctx_t *c, const Col &col, double min_score, const uint32_t *out_root, const uint64_t *out_count)
{
    if (min_score != min_score) { set_error("%s: min_score is NaN", who); return STRSIM_ERR_ARG; }
    if (col.rows > 0xFFFFFFFEull) { set_error("%s: %llu rows (at most 2^32 - 2)", who, (unsigned long long)col.rows); return STRSIM_ERR_ARG; }
    if (col.rows && (!col.off || !col.val)) { set_error("%s: NULL column buffer", who); return STRSIM_ERR_ARG; }
    if (col.rows && !out_root) { set_error("%s: out_root is NULL", who); return STRSIM_ERR_ARG; }
    if (!out_count) { set_error("%s: out_count is NULL", who); return STRSIM_ERR_ARG; }
    if (!c) { set_error("%s: ctx is NULL", who); return STRSIM_ERR_ARG; }
    return STRSIM_OK;
}

static int cluster_check(const char *who, strsim_ctx_t *c, int measure, const Col &col, double min_score, const uint32_t *out_root,
                         const uint64_t *out_count)
{
    if (!cluster_join(measure)) {
        set_error("%s: measure %d is not a measure of cluster (the reference measures 0 .. 4, STRSIM_INDEL = 8 or STRSIM_TOKEN_SORT_RATIO = 14)",
                  who, measure);
        return STRSIM_ERR_ARG;
    }
    return cluster_rest_check(who, c, col, min_score, out_root, out_count);
}

// The STRSIM_JOIN_UPPER self-join of a device-resident column, rows >= 1, into the context's cluster_pairs under the capacity
// protocol (4 * rows + 1024 slots, or what the buffer already holds; when the hits do not fit, exactly nnz and one more call), then
// the components of its CSR.  join(col, min_score, capacity, indptr, index, score, &nnz): the self-join of a family of entry points.
template <class Join>
static int cluster_labels(strsim_ctx *c, const char *who, Join join, const Col &col, double min_score, uint32_t *out_root,
                          uint32_t *out_cluster, uint64_t *out_count, uint64_t *out_nnz)
{
    const size_t ptr_bytes = up256(((size_t)col.rows + 1) * sizeof(uint64_t));
    uint64_t cap = 4u * col.rows + 1024u, nnz = 0;
    if (c->cluster_pairs.cap > ptr_bytes + 256) { // the buffer only grows: what an earlier call left is the first capacity when it is more
        const uint64_t have = (c->cluster_pairs.cap - ptr_bytes - 256) / (sizeof(uint32_t) + sizeof(double));
        if (have > cap) cap = have;
    }
    uint64_t *d_ptr = nullptr;
    uint32_t *d_idx = nullptr;
    for (int call = 0;; ++call) {
        const size_t idx_bytes = up256((size_t)cap * sizeof(uint32_t));
        int rc = c->cluster_pairs.reserve(ptr_bytes + idx_bytes + (size_t)cap * sizeof(double));
        if (rc) return rc;
        uint8_t *const b = c->cluster_pairs.as<uint8_t>();
        d_ptr = reinterpret_cast<uint64_t *>(b);
        d_idx = reinterpret_cast<uint32_t *>(b + ptr_bytes);
        rc = join(col, min_score, cap, d_ptr, d_idx, reinterpret_cast<double *>(b + ptr_bytes + idx_bytes), &nnz);
        if (rc) return rc;
        if (nnz <= cap) break;
        if (call) {
            set_error("%s: nnz changed between two joins of the same column (%llu > %llu)", who, (unsigned long long)nnz, (unsigned long long)cap);
            return STRSIM_ERR_INTERNAL;
        }
        cap = nnz;
    }
    if (out_nnz) *out_nnz = nnz;
    return components_labels(c, who, (uint32_t)col.rows, d_ptr, d_idx, nnz, out_root, out_cluster, out_count);
}

// The labels of a *_host entry point back from stage[4]: root, then cluster at a 256-byte boundary behind it.
static int labels_to_host(strsim_ctx *c, uint64_t rows, const uint8_t *d_out, uint32_t *out_root, uint32_t *out_cluster)
{
    HIP_TRY(hipMemcpyAsync(out_root, d_out, (size_t)rows * 4, hipMemcpyDeviceToHost, c->stream));
    if (out_cluster) HIP_TRY(hipMemcpyAsync(out_cluster, d_out + up256((size_t)rows * 4), (size_t)rows * 4, hipMemcpyDeviceToHost, c->stream));
    return strsim_ctx_synchronize(c);
}

extern "C" {

int strsim_components_device(strsim_ctx_t *c, uint64_t rows, const uint64_t *indptr, const uint32_t *index, uint64_t nnz, uint32_t *out_root,
                             uint32_t *out_cluster, uint64_t *out_count)
{
    int rc = components_check("strsim_components_device", c, rows, indptr, index, nnz, out_root, out_count);
    if (rc) return rc;
    *out_count = 0;
    if (rows == 0) return STRSIM_OK;
    rc = ctx_set_device(c);
    if (rc) return rc;
    return components_labels(c, "strsim_components_device", (uint32_t)rows, indptr, index, nnz, out_root, out_cluster, out_count);
}

int strsim_components_host(strsim_ctx_t *c, uint64_t rows, const uint64_t *indptr, const uint32_t *index, uint64_t nnz, uint32_t *out_root,
                           uint32_t *out_cluster, uint64_t *out_count)
{
    int rc = components_check("strsim_components_host", c, rows, indptr, index, nnz, out_root, out_count);
    if (rc) return rc;
    *out_count = 0;
    if (rows == 0) return STRSIM_OK;
    rc = ctx_set_device(c);
    if (rc) return rc;
    const size_t ptr_bytes = ((size_t)rows + 1) * sizeof(uint64_t), idx_bytes = (size_t)nnz * sizeof(uint32_t), lab_bytes = up256((size_t)rows * 4);
    rc = c->stage[0].reserve(ptr_bytes);
    if (rc == STRSIM_OK) rc = c->stage[1].reserve(idx_bytes + 4);
    if (rc == STRSIM_OK) rc = c->stage[4].reserve(2 * lab_bytes);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(c->stage[0].p, indptr, ptr_bytes, hipMemcpyHostToDevice, c->stream));
    if (nnz) HIP_TRY(hipMemcpyAsync(c->stage[1].p, index, idx_bytes, hipMemcpyHostToDevice, c->stream));
    uint8_t *const d_out = c->stage[4].as<uint8_t>();
    rc = components_labels(c, "strsim_components_host", (uint32_t)rows, c->stage[0].as<uint64_t>(), c->stage[1].as<uint32_t>(), nnz,
                           reinterpret_cast<uint32_t *>(d_out), out_cluster ? reinterpret_cast<uint32_t *>(d_out + lab_bytes) : nullptr, out_count);
    if (rc) return rc;
    return labels_to_host(c, rows, d_out, out_root, out_cluster);
}

int strsim_cluster_device(strsim_ctx_t *c, int measure, const uint32_t *offsets, const uint8_t *values, uint64_t rows, double min_score,
                          uint32_t *out_root, uint32_t *out_cluster, uint64_t *out_count, uint64_t *out_nnz)
{
    const Col col{offsets, values, rows};
    int rc = cluster_check("strsim_cluster_device", c, measure, col, min_score, out_root, out_count);
    if (rc) return rc;
    *out_count = 0;
    if (out_nnz) *out_nnz = 0;
    if (rows == 0) return STRSIM_OK;
    rc = ctx_set_device(c);
    if (rc) return rc;
    return cluster_labels(c, "strsim_cluster_device", cluster_self_join(c, measure), col, min_score, out_root, out_cluster, out_count, out_nnz);
}

int strsim_cluster_host(strsim_ctx_t *c, int measure, const uint32_t *offsets, const uint8_t *values, uint64_t rows, double min_score,
                        uint32_t *out_root, uint32_t *out_cluster, uint64_t *out_count, uint64_t *out_nnz)
{
    const Col col{offsets, values, rows};
    int rc = cluster_check("strsim_cluster_host", c, measure, col, min_score, out_root, out_count);
    if (rc) return rc;
    *out_count = 0;
    if (out_nnz) *out_nnz = 0;
    if (rows == 0) return STRSIM_OK;
    rc = ctx_set_device(c);
    if (rc) return rc;
    Staged s;
    rc = ctx_stage(c, col, NO_COL, 2 * up256((size_t)rows * 4), &s);
    if (rc) return rc;
    rc = cluster_labels(c, "strsim_cluster_host", cluster_self_join(c, measure), s.a, min_score, reinterpret_cast<uint32_t *>(s.out),
                        out_cluster ? reinterpret_cast<uint32_t *>(s.out + up256((size_t)rows * 4)) : nullptr, out_count, out_nnz);
    if (rc) return rc;
    return labels_to_host(c, rows, s.out, out_root, out_cluster);
}

} // extern "C"

// ---- threshold join and cluster by q-gram similarity (strsim_qgram_join.h, strsim_qgram_join_kernels.h): join_pairs with a third sweep ----

static int qgram_join_check(const char *who, strsim_ctx_t *c, int kind, uint32_t q, uint32_t qflags, const Col &qc, const Col &cnd, double min_score,
                            uint32_t flags, uint64_t capacity, const uint64_t *out_indptr, const uint32_t *out_index, const double *out_score,
                            const uint64_t *out_nnz)
{
    const int rc = qgram_kind_check(who, kind, q, qflags);
    if (rc) return rc;
    return join_rest_check("min_score", who, c, qc, cnd, min_score, flags, capacity, out_indptr, out_index, out_score, out_nnz);
}

// strsim_qgram_join_device behind its check.  Multiset mode enqueues what strsim_match_join_device enqueues; set mode one kernel
// more, behind the length order: the candidates' first occurrences.
static int qgram_join_device_impl(strsim_ctx_t *c, const char *who, int kind, uint32_t q, uint32_t qflags, const Col &qc, const Col &cnd,
                                  double min_score, uint32_t flags, uint64_t capacity, uint64_t *out_indptr, uint32_t *out_index, double *out_score,
                                  uint64_t *out_nnz)
{
    int rc = ctx_set_device(c);
    if (rc) return rc;
    if (qc.rows == 0) {
        *out_nnz = 0;
        HIP_TRY(hipMemsetAsync(out_indptr, 0, sizeof(uint64_t), c->stream));
        return STRSIM_OK;
    }
    const bool set = (qflags & STRSIM_QGRAM_SET) != 0u;
    MatchJoinNeed need; // which candidate lengths a query of each length visits: 33 words, a kernel argument
    const bool some = qgram_join_need_mask(kind, q, set, min_score, need);
    return join_pairs(
        c, who, qc, cnd, min_score, flags, capacity, out_indptr, out_index, out_score, out_nnz, !some,
        [&]() -> int { return set ? c->qgram_join_first.reserve((size_t)cnd.rows * sizeof(uint32_t)) : STRSIM_OK; },
        [&](bool fill, const JoinLaneArgs &a) -> hipError_t {
            uint32_t *const first = set ? c->qgram_join_first.as<uint32_t>() : nullptr;
            if (set && !fill) { // (the fill reads what the count's launch left)
                const hipError_t e = launch_qgram_join_first(q, a, (uint32_t)cnd.rows, first);
                if (e != hipSuccess) return e;
                c->enqueued_ops += 1u;
            }
            return launch_qgram_join_lane(kind, q, set, fill, a, first, need, min_score);
        },
        [&](const Col &lit, const Col &other, double *to) {
            // (strsim_ctx_last_wave_rows describes the caller's last pairwise q-gram or distance call: a fallback batch leaves it alone)
            const uint64_t wave_rows = c->last_wave_rows;
            const int r = qgram_device_impl(c, kind, q, qflags, lit, other, to, other.rows);
            c->last_wave_rows = wave_rows;
            return r;
        });
}

extern "C" {

int strsim_qgram_join_device(strsim_ctx_t *c, int kind, uint32_t q, uint32_t qflags, const uint32_t *q_off, const uint8_t *q_val, uint64_t q_rows,
                             const uint32_t *c_off, const uint8_t *c_val, uint64_t c_rows, double min_score, uint32_t flags, uint64_t capacity,
                             uint64_t *out_indptr, uint32_t *out_index, double *out_score, uint64_t *out_nnz)
{
    const Col qc{q_off, q_val, q_rows}, cnd{c_off, c_val, c_rows};
    const int rc = qgram_join_check("strsim_qgram_join_device", c, kind, q, qflags, qc, cnd, min_score, flags, capacity, out_indptr, out_index,
                                    out_score, out_nnz);
    if (rc) return rc;
    return qgram_join_device_impl(c, "strsim_qgram_join_device", kind, q, qflags, qc, cnd, min_score, flags, capacity, out_indptr, out_index,
                                  out_score, out_nnz);
}

int strsim_qgram_join_host(strsim_ctx_t *c, int kind, uint32_t q, uint32_t qflags, const uint32_t *q_off, const uint8_t *q_val, uint64_t q_rows,
                           const uint32_t *c_off, const uint8_t *c_val, uint64_t c_rows, double min_score, uint32_t flags, uint64_t capacity,
                           uint64_t *out_indptr, uint32_t *out_index, double *out_score, uint64_t *out_nnz)
{
    const Col qc{q_off, q_val, q_rows}, cnd{c_off, c_val, c_rows};
    return join_host(
        qgram_join_check("strsim_qgram_join_host", c, kind, q, qflags, qc, cnd, min_score, flags, capacity, out_indptr, out_index, out_score, out_nnz),
        [&](const Col &dq, const Col &dc, uint64_t *d_ptr, uint32_t *d_idx, double *d_score) {
            return qgram_join_device_impl(c, "strsim_qgram_join_host", kind, q, qflags, dq, dc, min_score, flags, capacity, d_ptr, d_idx, d_score,
                                          out_nnz);
        },
        c, qc, cnd, capacity, out_indptr, out_index, out_score, out_nnz);
}

} // extern "C"

static int qgram_cluster_check(const char *who, strsim_ctx_t *c, int kind, uint32_t q, uint32_t qflags, const Col &col, double min_score,
                               const uint32_t *out_root, const uint64_t *out_count)
{
    const int rc = qgram_kind_check(who, kind, q, qflags);
    if (rc) return rc;
    return cluster_rest_check(who, c, col, min_score, out_root, out_count);
}

// The self-join of strsim_qgram_cluster_*: the q-gram join of one column under STRSIM_JOIN_UPPER, kind, q and the mode bound.
static auto qgram_cluster_self_join(strsim_ctx *c, const char *who, int kind, uint32_t q, uint32_t qflags)
{
    return [=](const Col &col, double min_score, uint64_t cap, uint64_t *indptr, uint32_t *index, double *score, uint64_t *nnz) {
        return qgram_join_device_impl(c, who, kind, q, qflags, col, col, min_score, STRSIM_JOIN_UPPER, cap, indptr, index, score, nnz);
    };
}

extern "C" {

int strsim_qgram_cluster_device(strsim_ctx_t *c, int kind, uint32_t q, uint32_t qflags, const uint32_t *offsets, const uint8_t *values, uint64_t rows,
                                double min_score, uint32_t *out_root, uint32_t *out_cluster, uint64_t *out_count, uint64_t *out_nnz)
{
    const Col col{offsets, values, rows};
    int rc = qgram_cluster_check("strsim_qgram_cluster_device", c, kind, q, qflags, col, min_score, out_root, out_count);
    if (rc) return rc;
    *out_count = 0;
    if (out_nnz) *out_nnz = 0;
    if (rows == 0) return STRSIM_OK;
    rc = ctx_set_device(c);
    if (rc) return rc;
    return cluster_labels(c, "strsim_qgram_cluster_device", qgram_cluster_self_join(c, "strsim_qgram_cluster_device", kind, q, qflags), col, min_score,
                          out_root, out_cluster, out_count, out_nnz);
}

int strsim_qgram_cluster_host(strsim_ctx_t *c, int kind, uint32_t q, uint32_t qflags, const uint32_t *offsets, const uint8_t *values, uint64_t rows,
                              double min_score, uint32_t *out_root, uint32_t *out_cluster, uint64_t *out_count, uint64_t *out_nnz)
{
    const Col col{offsets, values, rows};
    int rc = qgram_cluster_check("strsim_qgram_cluster_host", c, kind, q, qflags, col, min_score, out_root, out_count);
    if (rc) return rc;
    *out_count = 0;
    if (out_nnz) *out_nnz = 0;
    if (rows == 0) return STRSIM_OK;
    rc = ctx_set_device(c);
    if (rc) return rc;
    Staged s;
    rc = ctx_stage(c, col, NO_COL, 2 * up256((size_t)rows * 4), &s);
    if (rc) return rc;
    rc = cluster_labels(c, "strsim_qgram_cluster_host", qgram_cluster_self_join(c, "strsim_qgram_cluster_host", kind, q, qflags), s.a, min_score,
                        reinterpret_cast<uint32_t *>(s.out), out_cluster ? reinterpret_cast<uint32_t *>(s.out + up256((size_t)rows * 4)) : nullptr,
                        out_count, out_nnz);
    if (rc) return rc;
    return labels_to_host(c, rows, s.out, out_root, out_cluster);
}

} // extern "C"

// ---- join and cluster by integer edit distance (strsim_distance_join.h, strsim_distance_join_kernels.h): join_pairs with a fourth sweep ----

static int edit_kind_check(const char *who, int kind)
{
    if (kind < STRSIM_EDIT_LEVENSHTEIN || kind > STRSIM_EDIT_DAMERAU) {
        set_error("%s: unknown kind %d (STRSIM_EDIT_LEVENSHTEIN, _OSA or _DAMERAU: 0..2)", who, kind);
        return STRSIM_ERR_ARG;
    }
    return STRSIM_OK;
}

static int distance_join_check(const char *who, strsim_ctx_t *c, int kind, const Col &qc, const Col &cnd, uint32_t flags, uint64_t capacity,
                               const uint64_t *out_indptr, const uint32_t *out_index, const uint32_t *out_distance, const uint64_t *out_nnz)
{
    const int rc = edit_kind_check(who, kind);
    if (rc) return rc;
    // (an integer cutoff is never NaN; the distances stand where the scores stand, looked at for NULL only)
    return join_rest_check("max_distance", who, c, qc, cnd, 0.0, flags, capacity, out_indptr, out_index,
                           reinterpret_cast<const double *>(out_distance), out_nnz);
}

// The join by edit distance in the join's own terms, qc.rows >= 1: the hits carry -(double)d in out_score.  It enqueues what
// strsim_match_join_device enqueues, and in the fallback one conversion behind every pairwise call.
static int distance_join_scores(strsim_ctx *c, const char *who, int kind, const Col &qc, const Col &cnd, uint32_t k, uint32_t flags,
                                uint64_t capacity, uint64_t *out_indptr, uint32_t *out_index, double *out_score, uint64_t *out_nnz)
{
    MatchJoinNeed need; // which candidate lengths a query of each length visits: 33 words, a kernel argument
    distance_join_need_mask(k, need);
    return join_pairs(
        c, who, qc, cnd, distance_join_cutoff(k), flags, capacity, out_indptr, out_index, out_score, out_nnz, false,
        [&]() -> int { return c->distance_join_col.reserve((size_t)std::max(qc.rows, cnd.rows) * sizeof(uint32_t)); },
        [&](bool fill, const JoinLaneArgs &a) { return launch_distance_join_lane(kind, fill, a, need, k); },
        [&](const Col &lit, const Col &other, double *to) -> int {
            // the pairwise call under the cutoff (its length prefilter applies; k + 1 stands for every longer distance and is no
            // hit), then the column as k_join_slow reads it.  One uint32 column serves every call: they run in stream order.
            // (strsim_ctx_last_wave_rows describes the caller's last pairwise call: a fallback batch leaves it alone)
            uint32_t *const d32 = c->distance_join_col.as<uint32_t>();
            const uint64_t wave_rows = c->last_wave_rows;
            const int r = kind == STRSIM_EDIT_DAMERAU
                              ? damerau_device_impl(c, lit, other, k, nullptr, d32, other.rows)
                              : distance_device_impl(c, kind == STRSIM_EDIT_OSA ? STRSIM_OSA : STRSIM_LEVENSHTEIN, lit, other, k, d32, other.rows);
            c->last_wave_rows = wave_rows;
            if (r) return r;
            HIP_TRY(launch_nearest_scores(d32, other.rows, to, c->stream));
            c->enqueued_ops += 1u;
            return STRSIM_OK;
        });
}

// strsim_distance_join_device behind its check: the join into the context's f64 column, then the distances of the hits that were
// stored.
static int distance_join_device_impl(strsim_ctx_t *c, const char *who, int kind, const Col &qc, const Col &cnd, uint32_t k, uint32_t flags,
                                     uint64_t capacity, uint64_t *out_indptr, uint32_t *out_index, uint32_t *out_distance, uint64_t *out_nnz)
{
    int rc = ctx_set_device(c);
    if (rc) return rc;
    if (qc.rows == 0) {
        *out_nnz = 0;
        HIP_TRY(hipMemsetAsync(out_indptr, 0, sizeof(uint64_t), c->stream));
        return STRSIM_OK;
    }
    // (a hit is stored only when all of them fit, and there are at most q_rows * c_rows)
    const uint64_t slots = std::min(capacity, qc.rows * cnd.rows);
    rc = c->distance_join_score.reserve((size_t)slots * sizeof(double));
    if (rc) return rc;
    double *const score = slots ? c->distance_join_score.as<double>() : nullptr;
    rc = distance_join_scores(c, who, kind, qc, cnd, k, flags, capacity, out_indptr, out_index, score, out_nnz);
    if (rc) return rc;
    if (*out_nnz && *out_nnz <= capacity) {
        HIP_TRY(launch_distance_join_finish(score, *out_nnz, out_distance, c->stream));
        c->enqueued_ops += 1u;
    }
    return STRSIM_OK;
}

extern "C" {

int strsim_distance_join_device(strsim_ctx_t *c, int kind, const uint32_t *q_off, const uint8_t *q_val, uint64_t q_rows, const uint32_t *c_off,
                                const uint8_t *c_val, uint64_t c_rows, uint32_t max_distance, uint32_t flags, uint64_t capacity,
                                uint64_t *out_indptr, uint32_t *out_index, uint32_t *out_distance, uint64_t *out_nnz)
{
    const Col qc{q_off, q_val, q_rows}, cnd{c_off, c_val, c_rows};
    const int rc = distance_join_check("strsim_distance_join_device", c, kind, qc, cnd, flags, capacity, out_indptr, out_index, out_distance, out_nnz);
    if (rc) return rc;
    return distance_join_device_impl(c, "strsim_distance_join_device", kind, qc, cnd, max_distance, flags, capacity, out_indptr, out_index,
                                     out_distance, out_nnz);
}

// (join_host with a uint32 column where its f64 column stands)
int strsim_distance_join_host(strsim_ctx_t *c, int kind, const uint32_t *q_off, const uint8_t *q_val, uint64_t q_rows, const uint32_t *c_off,
                              const uint8_t *c_val, uint64_t c_rows, uint32_t max_distance, uint32_t flags, uint64_t capacity,
                              uint64_t *out_indptr, uint32_t *out_index, uint32_t *out_distance, uint64_t *out_nnz)
{
    const Col qc{q_off, q_val, q_rows}, cnd{c_off, c_val, c_rows};
    int rc = distance_join_check("strsim_distance_join_host", c, kind, qc, cnd, flags, capacity, out_indptr, out_index, out_distance, out_nnz);
    if (rc) return rc;
    *out_nnz = 0;
    out_indptr[0] = 0;
    if (q_rows == 0) return STRSIM_OK;
    rc = ctx_set_device(c);
    if (rc) return rc;
    const size_t ptr_bytes = up256(((size_t)q_rows + 1) * sizeof(uint64_t)), idx_bytes = up256((size_t)capacity * sizeof(uint32_t));
    Staged s;
    rc = ctx_stage(c, qc, cnd, ptr_bytes + 2 * idx_bytes + 256, &s);
    if (rc) return rc;
    uint64_t *const d_ptr = reinterpret_cast<uint64_t *>(s.out);
    uint32_t *const d_idx = capacity ? reinterpret_cast<uint32_t *>(s.out + ptr_bytes) : nullptr;
    uint32_t *const d_dist = capacity ? reinterpret_cast<uint32_t *>(s.out + ptr_bytes + idx_bytes) : nullptr;
    rc = distance_join_device_impl(c, "strsim_distance_join_host", kind, Col{s.a.off, s.a.val, q_rows}, Col{s.b.off, s.b.val, c_rows}, max_distance,
                                   flags, capacity, d_ptr, d_idx, d_dist, out_nnz);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(out_indptr, d_ptr, ((size_t)q_rows + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    if (*out_nnz && *out_nnz <= capacity) {
        HIP_TRY(hipMemcpyAsync(out_index, d_idx, (size_t)*out_nnz * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(out_distance, d_dist, (size_t)*out_nnz * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    }
    return strsim_ctx_synchronize(c);
}

} // extern "C"

static int distance_cluster_check(const char *who, strsim_ctx_t *c, int kind, const Col &col, const uint32_t *out_root, const uint64_t *out_count)
{
    const int rc = edit_kind_check(who, kind);
    if (rc) return rc;
    return cluster_rest_check(who, c, col, 0.0, out_root, out_count);
}

// The self-join of strsim_distance_cluster_*: the join by edit distance of one column under STRSIM_JOIN_UPPER, kind and cutoff
// bound.  cluster_labels reads the CSR alone, so the f64 column of its buffer is never turned into distances.
static auto distance_cluster_self_join(strsim_ctx *c, const char *who, int kind, uint32_t k)
{
    return [=](const Col &col, double, uint64_t cap, uint64_t *indptr, uint32_t *index, double *score, uint64_t *nnz) {
        return distance_join_scores(c, who, kind, col, col, k, STRSIM_JOIN_UPPER, cap, indptr, index, score, nnz);
    };
}

extern "C" {

int strsim_distance_cluster_device(strsim_ctx_t *c, int kind, const uint32_t *offsets, const uint8_t *values, uint64_t rows, uint32_t max_distance,
                                   uint32_t *out_root, uint32_t *out_cluster, uint64_t *out_count, uint64_t *out_nnz)
{
    const Col col{offsets, values, rows};
    int rc = distance_cluster_check("strsim_distance_cluster_device", c, kind, col, out_root, out_count);
    if (rc) return rc;
    *out_count = 0;
    if (out_nnz) *out_nnz = 0;
    if (rows == 0) return STRSIM_OK;
    rc = ctx_set_device(c);
    if (rc) return rc;
    return cluster_labels(c, "strsim_distance_cluster_device", distance_cluster_self_join(c, "strsim_distance_cluster_device", kind, max_distance),
                          col, distance_join_cutoff(max_distance), out_root, out_cluster, out_count, out_nnz);
}

int strsim_distance_cluster_host(strsim_ctx_t *c, int kind, const uint32_t *offsets, const uint8_t *values, uint64_t rows, uint32_t max_distance,
                                 uint32_t *out_root, uint32_t *out_cluster, uint64_t *out_count, uint64_t *out_nnz)
{
    const Col col{offsets, values, rows};
    int rc = distance_cluster_check("strsim_distance_cluster_host", c, kind, col, out_root, out_count);
    if (rc) return rc;
    *out_count = 0;
    if (out_nnz) *out_nnz = 0;
    if (rows == 0) return STRSIM_OK;
    rc = ctx_set_device(c);
    if (rc) return rc;
    Staged s;
    rc = ctx_stage(c, col, NO_COL, 2 * up256((size_t)rows * 4), &s);
    if (rc) return rc;
    rc = cluster_labels(c, "strsim_distance_cluster_host", distance_cluster_self_join(c, "strsim_distance_cluster_host", kind, max_distance), s.a,
                        distance_join_cutoff(max_distance), reinterpret_cast<uint32_t *>(s.out),
                        out_cluster ? reinterpret_cast<uint32_t *>(s.out + up256((size_t)rows * 4)) : nullptr, out_count, out_nnz);
    if (rc) return rc;
    return labels_to_host(c, rows, s.out, out_root, out_cluster);
}

} // extern "C"
