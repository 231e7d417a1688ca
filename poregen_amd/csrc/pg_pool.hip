// pg_pool.hip -- `poregen model --pool` / `poregen offsets`: median and sstdev of POOLS of dump files, several files read as one.
//
// Replaces `cat F1 F2 ... | tr ';,' '\n' | tail -n +2 | datamash median 1` and `... sstdev 1` (scripts/poregen.sh:73-74 over a
// concatenation), for every group of every labeling at once. Per batch: the parse kernels of pg_dumptext.hip (pg_launch_dump_parse), the
// per-file reduction of pg_model.hip with the first value kept, and a copy of the batch's parsed units behind the arena. At finish the
// files' moments are combined on the host (pg_pool.h, exact) and the two middle values of every group are selected on the device:
//   k_pool_hist   one pass per 8-bit digit, most significant first, each one streaming read of the arena. A workgroup takes
//                 PG_POOL_TILE values; the file of its first value comes from one binary search over the files' value offsets, the
//                 next ones from a walk. For the part of a file inside the tile it keeps, per labeling, one 256-bin LDS histogram for
//                 each of the group's two targets and adds the non-zero bins to the group's global bins when the tile leaves the file
//                 (vector atomicAdd, device scope: one flush per file and tile, not one atomic per value). A part of at most
//                 PG_POOL_DIRECT values skips the LDS and adds value by value.
//   k_pool_pick   one thread per group walks the 256 bins to the bin of each target's rank: the prefix of the next pass and the rank
//                 inside it. The two targets, ranks (n - 1) / 2 and n / 2, share their bins until they part.
// The value `tail -n +2` drops is skipped by its arena index in k_pool_hist. Nothing is handed from workgroup to workgroup in a launch.
#include "../../include/pgmove.h"
#include <hip/hip_runtime.h>
#include "pg_hip_host.h"
#include "pg_internal.h"
#include "pg_model.h"
#include "pg_dumptext.h"
#include "pg_pool.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace {

constexpr int kThreads = PG_POOL_THREADS;
constexpr uint32_t kTile = PG_POOL_TILE;
constexpr uint32_t kDirect = PG_POOL_DIRECT;
constexpr uint32_t kNoGroup = PG_POOL_NO_GROUP;
constexpr uint64_t kNoIndex = ~0ull;
constexpr int64_t kBias = PG_POOL_KEY_BIAS;          // key = units + kBias in (0, 2^56): the sign of the units is the key's first digit's top bit
constexpr uint64_t kMaxBatchBytes = 1ull << 31;
constexpr uint32_t kMaxBatchFiles = 1u << 24;
static_assert(kTile % (2 * kThreads) == 0 && kDirect <= (uint32_t)kThreads, "a thread loads pairs of values; a direct part is one value per thread");

enum { SEL_ACTIVE = 1, SEL_PARTED = 2, SEL_LOST = 4 };
struct PoolSel { // one group's selection between the passes
    uint64_t prefix_lo, prefix_hi; // the digits found so far of the two targets
    uint64_t drop;                 // arena index of the value that does not count, or kNoIndex
    uint32_t rank_lo, rank_hi;     // ranks among the values that share the prefix
    uint32_t state, pad;
};

struct PoolPass {
    const int64_t *arena; uint64_t n_values;
    const uint64_t *fval_off; uint32_t n_files; // the files that have values: file f holds arena [fval_off[f], fval_off[f + 1])
    const uint32_t *gid;                        // [n_files][L] index of the file's group among all groups, or kNoGroup
    uint32_t L;
    const PoolSel *sel;
    uint32_t *hist;                             // [groups][2][256]
    uint32_t shift;                             // of this pass's digit
};

__device__ __forceinline__ uint32_t pool_file_of(const uint64_t *__restrict__ off, uint32_t n_files, uint64_t pos) {
    uint32_t lo = 0, hi = n_files;
    while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (off[mid] <= pos) lo = mid; else hi = mid; }
    return lo;
}

__global__ __launch_bounds__(kThreads) void k_pool_hist(PoolPass a) {
    extern __shared__ uint32_t bins[];               // [L][2][256]
    __shared__ uint64_t s_lo[PG_POOL_MAX_LABELINGS], s_hi[PG_POOL_MAX_LABELINGS], s_drop[PG_POOL_MAX_LABELINGS];
    __shared__ uint32_t s_g[PG_POOL_MAX_LABELINGS], s_parted[PG_POOL_MAX_LABELINGS];
    const uint32_t tid = threadIdx.x;
    const uint64_t tile_base = (uint64_t)blockIdx.x * kTile, tile_end = min(tile_base + kTile, a.n_values);
    if (tile_base >= tile_end) return;
    const uint32_t up = a.shift + 8;
    uint32_t f = pool_file_of(a.fval_off, a.n_files, tile_base);
    for (uint64_t lo = tile_base; lo < tile_end && f < a.n_files; f++) {
        const uint64_t hi = min(a.fval_off[f + 1], tile_end);
        if (tid < a.L) {
            uint32_t g = a.gid[(uint64_t)f * a.L + tid], parted = 0;
            if (g != kNoGroup) {
                const PoolSel s = a.sel[g];
                if (s.state & SEL_ACTIVE) { s_lo[tid] = s.prefix_lo; s_hi[tid] = s.prefix_hi; s_drop[tid] = s.drop; parted = s.state & SEL_PARTED; }
                else g = kNoGroup;
            }
            s_g[tid] = g; s_parted[tid] = parted;
        }
        const bool direct = hi - lo <= kDirect;
        if (!direct) for (uint32_t i = tid; i < a.L * 512; i += kThreads) bins[i] = 0;
        __syncthreads();
        auto count = [&](uint64_t idx, int64_t units) {
            const uint64_t key = (uint64_t)(units + kBias);
            const uint64_t top = key >> up;
            const uint32_t digit = (uint32_t)(key >> a.shift) & 255u;
            for (uint32_t l = 0; l < a.L; l++) {
                const uint32_t g = s_g[l];
                if (g == kNoGroup || idx == s_drop[l]) continue;
                const bool parted = s_parted[l];
                if (top == s_lo[l]) { if (direct) atomicAdd(&a.hist[(uint64_t)g * 512 + digit], 1u); else atomicAdd(&bins[l * 512 + digit], 1u); }
                else if (parted && top == s_hi[l]) { if (direct) atomicAdd(&a.hist[(uint64_t)g * 512 + 256 + digit], 1u); else atomicAdd(&bins[l * 512 + 256 + digit], 1u); }
            }
        };
        if (direct) {
            if (tid < hi - lo) count(lo + tid, a.arena[lo + tid]);
        } else {
            // pairs of values at even indices: 16-byte loads (the arena is 16-byte aligned and has room for one value behind n_values)
            for (uint64_t i = (lo & ~1ull) + 2 * tid; i < hi; i += 2 * kThreads) {
                const longlong2 v = *reinterpret_cast<const longlong2 *>(a.arena + i);
                if (i >= lo) count(i, v.x);
                if (i + 1 < hi) count(i + 1, v.y);
            }
            __syncthreads();
            for (uint32_t l = 0; l < a.L; l++) {
                const uint32_t g = s_g[l];
                if (g == kNoGroup) continue;
                const uint32_t c0 = bins[l * 512 + tid];
                if (c0) atomicAdd(&a.hist[(uint64_t)g * 512 + tid], c0);
                if (s_parted[l]) { const uint32_t c1 = bins[l * 512 + 256 + tid]; if (c1) atomicAdd(&a.hist[(uint64_t)g * 512 + 256 + tid], c1); }
            }
        }
        __syncthreads(); // the labelings' entries and the bins are the next file's from here
        lo = hi;
    }
}

// the bin that holds rank r of the 256 bins at h; r becomes the rank inside it. false: the bins hold fewer than r + 1 values
__device__ __forceinline__ bool pool_walk(const uint32_t *__restrict__ h, uint32_t &r, uint32_t &bin) {
    uint64_t cum = 0;
    for (uint32_t b = 0; b < 256; b++) {
        const uint32_t c = h[b];
        if (cum + c > r) { bin = b; r -= (uint32_t)cum; return true; }
        cum += c;
    }
    bin = 255;
    return false;
}

__global__ __launch_bounds__(kThreads) void k_pool_pick(PoolSel *sel, const uint32_t *hist, uint32_t n_groups) {
    const uint32_t g = blockIdx.x * kThreads + threadIdx.x;
    if (g >= n_groups) return;
    PoolSel s = sel[g];
    if (!(s.state & SEL_ACTIVE)) return;
    const uint32_t *h = hist + (uint64_t)g * 512;
    uint32_t b_lo, b_hi;
    bool ok = pool_walk(h, s.rank_lo, b_lo);
    ok &= pool_walk((s.state & SEL_PARTED) ? h + 256 : h, s.rank_hi, b_hi);
    if (!(s.state & SEL_PARTED) && b_lo != b_hi) s.state |= SEL_PARTED;
    if (!ok) s.state |= SEL_LOST;
    s.prefix_lo = (s.prefix_lo << 8) | b_lo; s.prefix_hi = (s.prefix_hi << 8) | b_hi;
    sel[g] = s;
}

// out[i] = arena[idx[i]] (0 for kNoIndex): the value behind the dropped one of every group
__global__ __launch_bounds__(kThreads) void k_pool_gather(const int64_t *arena, uint64_t n_values, const uint64_t *idx, int64_t *out, uint32_t n) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const uint64_t at = idx[i];
    out[i] = at < n_values ? arena[at] : 0;
}

enum { F_MEMBER_BAD = 1, F_NEGZERO = 2 };
struct FileRec { uint64_t n, count, arena_off; int64_t origin, s1; unsigned __int128 s2; uint32_t flags; const char *why; };

} // namespace

struct pg_pool {
    int device = 0;
    uint32_t flags = 0;
    uint32_t L = 0, n_groups_total = 0;
    std::vector<uint32_t> n_groups, base;
    uint64_t max_values = 0;
    PgStream st;
    PgEvent e0, e1;
    // the batch in flight
    PgDev<uint8_t> d_bytes;
    PgDev<> d_file_off, d_tile, d_fflags, d_fstart, d_val_base, d_ev_off, d_units, d_samp_off, d_ev_len, d_out, d_dwell, d_scratch;
    PgPinned<> dl_model, dl_dwell, dl_flags, dl_base, up_off;
    // everything since the last finish
    PgDev<int64_t> arena;
    uint64_t arena_n = 0;
    std::vector<FileRec> files;
    std::vector<uint32_t> file_gid; // [files][L], index among all groups or PG_POOL_NO_GROUP
    uint64_t n_bytes = 0; uint32_t n_batches = 0;
    // finish
    PgDev<> d_foff, d_gid, d_sel, d_hist, d_idx, d_second;
    bool finished = false;
    std::vector<uint64_t> r_n, r_s2lo, r_s2hi, r_dn, r_files;
    std::vector<int64_t> r_lo, r_hi, r_origin, r_s1, r_refused;
    std::vector<double> r_med, r_sd, r_dmed;
    std::vector<uint32_t> r_status;
    std::vector<unsigned __int128> r_num;
    std::vector<std::string> r_why;
    pg_pool_result result{};
    std::string err;
};

namespace {

void pool_clear(pg_pool *h) {
    h->arena_n = 0; h->files.clear(); h->file_gid.clear(); h->n_bytes = 0; h->n_batches = 0;
    h->finished = false;
    h->result = pg_pool_result{};
}

template <class B> bool too_small(const B &b, size_t bytes) { return bytes > b.cap; }

// room for `values` in the arena: doubled (at most max_values) and copied over when it has to grow; one value of slack for the pair loads
pg_status pool_reserve(pg_pool *h, uint64_t values) {
    const uint64_t have = h->arena.cap / 8;
    if (values + 2 <= have) return PG_OK;
    const uint64_t want = std::min<uint64_t>(std::max<uint64_t>(values, 2 * h->arena_n), std::max<uint64_t>(h->max_values, values));
    PgDev<int64_t> bigger;
    PG_HIP_TRY(h, bigger.ensure((want + 2) * 8));
    if (h->arena_n) PG_HIP_TRY(h, hipMemcpyAsync(bigger.p, h->arena.p, h->arena_n * 8, hipMemcpyDeviceToDevice, h->st));
    PG_HIP_TRY(h, hipStreamSynchronize(h->st));
    h->arena = std::move(bigger);
    return PG_OK;
}

} // namespace

extern "C" {

const char *pg_pool_last_error(const pg_pool *h) { return h ? h->err.c_str() : pg_create_error<pg_pool>().c_str(); }

pg_status pg_pool_create(int32_t device, uint32_t n_labelings, const uint32_t *n_groups, uint64_t max_values, uint32_t flags, pg_pool **out) {
    if (!out) return pg_fail<pg_pool>(nullptr, PG_ERR_INVALID_ARG, "pg_pool_create: null argument");
    *out = nullptr;
    if (flags & ~(uint32_t)PG_MODEL_KEEP_FIRST) return pg_fail<pg_pool>(nullptr, PG_ERR_INVALID_ARG, "pg_pool_create: unknown flags 0x%x", flags);
    if (n_labelings < 1 || n_labelings > PG_POOL_MAX_LABELINGS || !n_groups)
        return pg_fail<pg_pool>(nullptr, PG_ERR_INVALID_ARG, "pg_pool_create: 1 to %u labelings and their group counts are needed", PG_POOL_MAX_LABELINGS);
    uint64_t total = 0;
    for (uint32_t l = 0; l < n_labelings; l++) total += n_groups[l];
    if (total == 0 || total > (1u << 24)) return pg_fail<pg_pool>(nullptr, PG_ERR_INVALID_ARG, "pg_pool_create: 1 to 2^24 groups in all, not %llu", (unsigned long long)total);
    if (pg_status st = pg_select_device<pg_pool>(device)) return st;
    pg_pool *h = new pg_pool();
    h->device = device; h->flags = flags; h->L = n_labelings; h->n_groups_total = (uint32_t)total;
    h->n_groups.assign(n_groups, n_groups + n_labelings);
    h->base.assign(n_labelings + 1, 0);
    for (uint32_t l = 0; l < n_labelings; l++) h->base[l + 1] = h->base[l] + n_groups[l];
    auto init = [&]() -> pg_status {
        PG_HIP_TRY(h, hipStreamCreateWithFlags(&h->st.h, hipStreamNonBlocking));
        PG_HIP_TRY(h, hipEventCreate(&h->e0.h)); PG_HIP_TRY(h, hipEventCreate(&h->e1.h));
        if (max_values == 0) { // half of what is free now: the doubling arena holds old and new for a moment, 3/4 of it at the most
            size_t free_b = 0, total_b = 0;
            PG_HIP_TRY(h, hipMemGetInfo(&free_b, &total_b));
            max_values = std::max<uint64_t>(free_b / 2 / 8, 1);
        }
        h->max_values = max_values;
        return PG_OK;
    };
    if (pg_status st = init()) return pg_create_failed(h, st, pg_pool_destroy);
    *out = h;
    return PG_OK;
}

void pg_pool_destroy(pg_pool *h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->st) (void)hipStreamSynchronize(h->st);
    delete h;
}

pg_status pg_pool_submit(pg_pool *h, const void *bytes, const uint64_t *file_off, uint32_t n_files, const uint32_t *group, int32_t location) {
    if (!h) return pg_fail<pg_pool>(nullptr, PG_ERR_INVALID_ARG, "pg_pool_submit: null handle");
    if (location != PG_LOC_HOST && location != PG_LOC_DEVICE) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_pool_submit: location must be PG_LOC_HOST or PG_LOC_DEVICE");
    if (h->finished) pool_clear(h);
    if (!n_files) return PG_OK;
    if (!file_off || !group) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_pool_submit: null file_off or group");
    if (n_files > kMaxBatchFiles) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_pool_submit: more than %u files in one call", kMaxBatchFiles);
    if (file_off[0] != 0) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_pool_submit: file_off[0] must be 0");
    for (uint32_t i = 0; i < n_files; i++)
        if (file_off[i + 1] < file_off[i]) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_pool_submit: file_off decreases at file %u", i);
    const uint64_t n = file_off[n_files];
    if (n > kMaxBatchBytes) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_pool_submit: more than 2^31 bytes in one call");
    if (n && !bytes) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_pool_submit: null bytes");
    if (h->files.size() + (uint64_t)n_files > 0xffffffffull) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_pool_submit: more than 2^32 files since the last finish");
    for (uint32_t l = 0; l < h->L; l++)
        for (uint32_t i = 0; i < n_files; i++) {
            const uint32_t g = group[(size_t)l * n_files + i];
            if (g != kNoGroup && g >= h->n_groups[l]) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_pool_submit: file %u has group %u in labeling %u, which has %u groups", i, g, l, h->n_groups[l]);
        }
    PG_HIP_TRY(h, hipSetDevice(h->device));
    if (location == PG_LOC_DEVICE && n && pg_ptr_kind(bytes, h->device) != PG_PTR_DEVICE)
        return pg_fail(h, PG_ERR_INVALID_ARG, "pg_pool_submit: PG_LOC_DEVICE bytes are not device memory of device %d", h->device);

    const uint32_t n_tiles = (uint32_t)((n + PG_DT_TILE - 1) / PG_DT_TILE);
    const uint64_t cap_values = n / PG_DT_MIN_FIELD + 1;
    const size_t nf1 = (size_t)n_files + 1;
    const size_t scratch = pg_slot_model_scratch_bytes(n_files);
    auto room = [](size_t b) { return b + b / 4 + 256; };
    // (every call is settled before it returns: no batch is in flight when a buffer is replaced)
    PG_HIP_TRY(h, h->d_bytes.ensure(n + 64, room(n + 64))); PG_HIP_TRY(h, h->d_file_off.ensure(nf1 * 8, room(nf1 * 8)));
    PG_HIP_TRY(h, h->d_tile.ensure(((size_t)n_tiles + 1) * 8, room(((size_t)n_tiles + 1) * 8))); PG_HIP_TRY(h, h->d_fflags.ensure(nf1 * 4, room(nf1 * 4)));
    PG_HIP_TRY(h, h->d_fstart.ensure(nf1 * 8, room(nf1 * 8))); PG_HIP_TRY(h, h->d_val_base.ensure(nf1 * 8, room(nf1 * 8)));
    PG_HIP_TRY(h, h->d_ev_off.ensure(nf1 * 8, room(nf1 * 8))); PG_HIP_TRY(h, h->d_units.ensure(cap_values * 8, room(cap_values * 8)));
    PG_HIP_TRY(h, h->d_samp_off.ensure((cap_values + 1) * 8, room((cap_values + 1) * 8))); PG_HIP_TRY(h, h->d_ev_len.ensure(cap_values * 4, room(cap_values * 4)));
    PG_HIP_TRY(h, h->d_out.ensure(nf1 * sizeof(PgSlotModel), room(nf1 * sizeof(PgSlotModel)))); PG_HIP_TRY(h, h->d_dwell.ensure(nf1 * sizeof(PgSlotDwell), room(nf1 * sizeof(PgSlotDwell))));
    PG_HIP_TRY(h, h->d_scratch.ensure(scratch, room(scratch)));
    PG_HIP_TRY(h, h->up_off.ensure(nf1 * 8, room(nf1 * 8))); PG_HIP_TRY(h, h->dl_base.ensure(nf1 * 8, room(nf1 * 8)));
    PG_HIP_TRY(h, h->dl_model.ensure(nf1 * sizeof(PgSlotModel), room(nf1 * sizeof(PgSlotModel)))); PG_HIP_TRY(h, h->dl_dwell.ensure(nf1 * sizeof(PgSlotDwell), room(nf1 * sizeof(PgSlotDwell))));
    PG_HIP_TRY(h, h->dl_flags.ensure(nf1 * 4, room(nf1 * 4)));

    memcpy(h->up_off.p, file_off, nf1 * 8);
    const uint8_t *p = h->d_bytes.p;
    if (location == PG_LOC_DEVICE) { if (n) p = static_cast<const uint8_t *>(bytes); }
    else if (n) PG_HIP_TRY(h, hipMemcpyAsync(h->d_bytes.p, bytes, n, hipMemcpyHostToDevice, h->st));
    PG_HIP_TRY(h, hipMemcpyAsync(h->d_file_off.p, h->up_off.p, nf1 * 8, hipMemcpyHostToDevice, h->st));
    PG_HIP_TRY(h, hipMemsetAsync(h->d_fflags.p, 0, nf1 * 4, h->st));

    PgDtBatch b{};
    b.p = p; b.n = n; b.file_off = h->d_file_off.as<uint64_t>(); b.n_files = n_files; b.n_tiles = n_tiles;
    b.tile_pre = h->d_tile.as<uint2>(); b.fflags = h->d_fflags.as<uint32_t>(); b.fstart = h->d_fstart.as<uint2>();
    b.val_base = h->d_val_base.as<uint64_t>(); b.ev_off = h->d_ev_off.as<uint64_t>();
    b.units = h->d_units.as<int64_t>(); b.samp_off = h->d_samp_off.as<uint64_t>(); b.ev_len = h->d_ev_len.as<uint32_t>();
    b.cap_values = cap_values;
    PG_HIP_TRY(h, pg_launch_dump_parse(h->st, b));
    // the reduction of every file with its first value kept: the pool drops one value, and only finish knows whose
    const int all_kinds[PG_MODEL_KINDS] = {1 << 20, 1 << 20, 1 << 20, 1 << 20};
    PG_HIP_TRY(h, pg_launch_slot_model_units(h->st, n_files, all_kinds, b.ev_off, b.samp_off, b.ev_len, b.units, 0u, h->d_out.as<PgSlotModel>(),
                                             h->d_dwell.as<PgSlotDwell>(), h->d_scratch.p));
    PG_HIP_TRY(h, hipMemcpyAsync(h->dl_model.p, h->d_out.p, (size_t)n_files * sizeof(PgSlotModel), hipMemcpyDeviceToHost, h->st));
    PG_HIP_TRY(h, hipMemcpyAsync(h->dl_dwell.p, h->d_dwell.p, (size_t)n_files * sizeof(PgSlotDwell), hipMemcpyDeviceToHost, h->st));
    PG_HIP_TRY(h, hipMemcpyAsync(h->dl_flags.p, h->d_fflags.p, (size_t)n_files * 4, hipMemcpyDeviceToHost, h->st));
    PG_HIP_TRY(h, hipMemcpyAsync(h->dl_base.p, b.val_base, nf1 * 8, hipMemcpyDeviceToHost, h->st));
    PG_HIP_TRY(h, hipStreamSynchronize(h->st));

    const uint64_t *vb = h->dl_base.as<uint64_t>();
    const uint64_t total = vb[n_files];
    if (total > cap_values) return pg_fail(h, PG_ERR_HIP, "pg_pool_submit: internal: %llu values parsed out of %llu bytes", (unsigned long long)total, (unsigned long long)n);
    if (h->arena_n + total > h->max_values)
        return pg_fail(h, PG_ERR_UNSUPPORTED, "pg_pool_submit: %llu values behind %llu pass the arena's cap of %llu values (max_values); nothing of this batch is counted",
                       (unsigned long long)total, (unsigned long long)h->arena_n, (unsigned long long)h->max_values);
    if (pg_status st = pool_reserve(h, h->arena_n + total)) return st;
    if (total) {
        PG_HIP_TRY(h, hipMemcpyAsync(h->arena.p + h->arena_n, b.units, total * 8, hipMemcpyDeviceToDevice, h->st));
        PG_HIP_TRY(h, hipStreamSynchronize(h->st));
    }
    const PgSlotModel *mo = h->dl_model.as<PgSlotModel>();
    const PgSlotDwell *dw = h->dl_dwell.as<PgSlotDwell>();
    const uint32_t *fl = h->dl_flags.as<uint32_t>();
    for (uint32_t i = 0; i < n_files; i++) {
        FileRec r{};
        r.count = vb[i + 1] - vb[i]; r.arena_off = h->arena_n + vb[i];
        if (fl[i] & DT_BAD) { r.flags |= F_MEMBER_BAD; r.why = "is outside the strict grammar (-?D{1,8}.DDDDDDDD[,;])* with a last ';'"; }
        else if (dw[i].flags & PG_MODEL_BAD_COUNT) { r.flags |= F_MEMBER_BAD; r.why = "holds more than 2^23 values"; }
        else if (dw[i].flags & PG_MODEL_BAD_SPREAD) { r.flags |= F_MEMBER_BAD; r.why = "holds a value further than 2^40 units from its first"; }
        else if (dw[i].flags & PG_MODEL_BAD_VALUE) { r.flags |= F_MEMBER_BAD; r.why = "holds a value the fixed-point view declines"; }
        else {
            r.n = mo[i].n; r.origin = mo[i].origin; r.s1 = mo[i].s1;
            r.s2 = ((unsigned __int128)mo[i].s2_hh << 40) + ((unsigned __int128)mo[i].s2_hl << 21) + mo[i].s2_ll;
            if (r.n != r.count) { r.flags |= F_MEMBER_BAD; r.why = "was reduced to another number of values than were parsed (internal)"; }
        }
        if (fl[i] & DT_NEGZERO) r.flags |= F_NEGZERO;
        h->files.push_back(r);
        for (uint32_t l = 0; l < h->L; l++) {
            const uint32_t g = group[(size_t)l * n_files + i];
            h->file_gid.push_back(g == kNoGroup ? kNoGroup : h->base[l] + g);
        }
    }
    h->arena_n += total; h->n_bytes += n; h->n_batches++;
    return PG_OK;
}

pg_status pg_pool_sync(pg_pool *h) {
    if (!h) return pg_fail<pg_pool>(nullptr, PG_ERR_INVALID_ARG, "pg_pool_sync: null handle");
    PG_HIP_TRY(h, hipSetDevice(h->device));
    PG_HIP_TRY(h, hipStreamSynchronize(h->st));
    return PG_OK;
}

pg_status pg_pool_finish(pg_pool *h, pg_pool_result *out) {
    if (!h) return pg_fail<pg_pool>(nullptr, PG_ERR_INVALID_ARG, "pg_pool_finish: null handle");
    if (!out) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_pool_finish: null argument");
    if (h->finished) pool_clear(h);
    PG_HIP_TRY(h, hipSetDevice(h->device));
    const uint32_t G = h->n_groups_total, L = h->L;
    const size_t F = h->files.size();
    const bool drop = !(h->flags & PG_MODEL_KEEP_FIRST);

    // the groups' members, in submission order
    std::vector<uint64_t> g_off(G + 1, 0);
    for (size_t i = 0; i < F * L; i++) if (h->file_gid[i] != kNoGroup) g_off[h->file_gid[i] + 1]++;
    for (uint32_t g = 0; g < G; g++) g_off[g + 1] += g_off[g];
    std::vector<uint32_t> g_mem(g_off[G]);
    { std::vector<uint64_t> at(g_off.begin(), g_off.end() - 1);
      for (size_t f = 0; f < F; f++) for (uint32_t l = 0; l < L; l++) { const uint32_t g = h->file_gid[f * L + l]; if (g != kNoGroup) g_mem[at[g]++] = (uint32_t)f; } }

    h->r_status.assign(G, PG_POOL_GROUP_EMPTY); h->r_refused.assign(G, -1); h->r_files.assign(G, 0); h->r_why.assign(G, std::string());
    for (auto *v : {&h->r_n, &h->r_s2lo, &h->r_s2hi, &h->r_dn}) v->assign(G, 0);
    for (auto *v : {&h->r_lo, &h->r_hi, &h->r_origin, &h->r_s1}) v->assign(G, 0);
    for (auto *v : {&h->r_med, &h->r_sd, &h->r_dmed}) v->assign(G, NAN);
    h->r_num.assign(G, 0);
    auto refuse = [&](uint32_t g, int64_t file, const std::string &why) { h->r_status[g] = PG_POOL_GROUP_REFUSED; h->r_refused[g] = file; h->r_why[g] = why; h->r_n[g] = 0; };

    // per group: a member the device path declines refuses it; else the dropped value's arena index and that of the value behind it
    std::vector<uint64_t> drop_idx(G, kNoIndex), second_idx(G, kNoIndex);
    std::vector<int64_t> first_mem(G, -1);
    for (uint32_t g = 0; g < G; g++) {
        h->r_files[g] = g_off[g + 1] - g_off[g];
        for (uint64_t k = g_off[g]; k < g_off[g + 1]; k++) {
            const FileRec &r = h->files[g_mem[k]];
            if (r.flags & F_MEMBER_BAD) { refuse(g, g_mem[k], std::string("file ") + std::to_string(g_mem[k]) + " " + r.why + "; pools have no host path"); break; }
        }
        if (h->r_status[g] == PG_POOL_GROUP_REFUSED) continue;
        for (uint64_t k = g_off[g]; k < g_off[g + 1]; k++) {
            const FileRec &r = h->files[g_mem[k]];
            if (!r.n) continue;
            if (first_mem[g] < 0) { first_mem[g] = (int64_t)k; if (!drop) break; drop_idx[g] = r.arena_off; if (r.n >= 2) { second_idx[g] = r.arena_off + 1; break; } }
            else { second_idx[g] = r.arena_off; break; }
        }
    }
    std::vector<int64_t> second(G, 0);
    if (drop && h->arena_n) {
        PG_HIP_TRY(h, h->d_idx.ensure((size_t)G * 8)); PG_HIP_TRY(h, h->d_second.ensure((size_t)G * 8));
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_idx.p, second_idx.data(), (size_t)G * 8, hipMemcpyHostToDevice, h->st));
        hipLaunchKernelGGL(k_pool_gather, dim3((G + kThreads - 1) / kThreads), dim3(kThreads), 0, h->st, h->arena.p, h->arena_n, h->d_idx.as<uint64_t>(), h->d_second.as<int64_t>(), G);
        PG_HIP_TRY(h, hipGetLastError());
        PG_HIP_TRY(h, hipMemcpyAsync(second.data(), h->d_second.p, (size_t)G * 8, hipMemcpyDeviceToHost, h->st));
        PG_HIP_TRY(h, hipStreamSynchronize(h->st));
    }

    // moments, exact, on the host
    std::vector<PoolSel> sel(G, PoolSel{});
    std::vector<PgPoolMember> mem;
    bool any = false;
    for (uint32_t g = 0; g < G; g++) {
        if (h->r_status[g] == PG_POOL_GROUP_REFUSED) continue;
        mem.clear();
        for (uint64_t k = g_off[g]; k < g_off[g + 1]; k++) { const FileRec &r = h->files[g_mem[k]]; mem.push_back(PgPoolMember{r.n, r.origin, r.s1, r.s2}); }
        PgPoolMoments pm;
        pg_pool_combine(mem.data(), mem.size(), drop, second[g], pm);
        if (pm.status == PG_POOL_ST_EMPTY) continue;
        if (pm.status == PG_POOL_ST_REFUSED) {
            refuse(g, first_mem[g] >= 0 ? (int64_t)g_mem[first_mem[g]] : (int64_t)g_mem[g_off[g]],
                   pm.why == PG_POOL_WHY_COUNT ? "the pool holds more than 2^32 - 1 values" : "the pool's exact moments do not fit 128 bits (values too far apart for their number)");
            continue;
        }
        h->r_status[g] = PG_POOL_GROUP_OK;
        h->r_n[g] = pm.n; h->r_origin[g] = pm.origin; h->r_s1[g] = pm.s1; h->r_s2lo[g] = (uint64_t)pm.s2; h->r_s2hi[g] = (uint64_t)(pm.s2 >> 64); h->r_num[g] = pm.num;
        PoolSel &s = sel[g];
        s.drop = drop ? drop_idx[g] : kNoIndex; s.rank_lo = (uint32_t)((pm.n - 1) / 2); s.rank_hi = (uint32_t)(pm.n / 2); s.state = SEL_ACTIVE;
        any = true;
    }

    // medians, on the device
    float ms = 0;
    if (any) {
        std::vector<uint64_t> foff; std::vector<uint32_t> gid;
        for (size_t f = 0; f < F; f++) {
            const FileRec &r = h->files[f];
            if (!r.count) continue;
            foff.push_back(r.arena_off);
            for (uint32_t l = 0; l < L; l++) { const uint32_t g = h->file_gid[f * L + l]; gid.push_back(g != kNoGroup && (sel[g].state & SEL_ACTIVE) ? g : kNoGroup); }
        }
        foff.push_back(h->arena_n);
        const uint32_t nf = (uint32_t)(foff.size() - 1);
        const size_t hist_bytes = (size_t)G * 512 * 4;
        PG_HIP_TRY(h, h->d_foff.ensure(foff.size() * 8)); PG_HIP_TRY(h, h->d_gid.ensure(gid.size() * 4 + 4));
        PG_HIP_TRY(h, h->d_sel.ensure((size_t)G * sizeof(PoolSel))); PG_HIP_TRY(h, h->d_hist.ensure(hist_bytes));
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_foff.p, foff.data(), foff.size() * 8, hipMemcpyHostToDevice, h->st));
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_gid.p, gid.data(), gid.size() * 4, hipMemcpyHostToDevice, h->st));
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_sel.p, sel.data(), (size_t)G * sizeof(PoolSel), hipMemcpyHostToDevice, h->st));
        PoolPass a{};
        a.arena = h->arena.p; a.n_values = h->arena_n; a.fval_off = h->d_foff.as<uint64_t>(); a.n_files = nf; a.gid = h->d_gid.as<uint32_t>(); a.L = L;
        a.sel = h->d_sel.as<PoolSel>(); a.hist = h->d_hist.as<uint32_t>();
        const uint32_t tiles = (uint32_t)((h->arena_n + kTile - 1) / kTile);
        PG_HIP_TRY(h, hipEventRecord(h->e0, h->st));
        for (int pass = 0; pass < PG_POOL_DIGITS; pass++) {
            a.shift = 8u * (uint32_t)(PG_POOL_DIGITS - 1 - pass);
            PG_HIP_TRY(h, hipMemsetAsync(h->d_hist.p, 0, hist_bytes, h->st));
            hipLaunchKernelGGL(k_pool_hist, dim3(tiles), dim3(kThreads), (size_t)L * 512 * 4, h->st, a);
            hipLaunchKernelGGL(k_pool_pick, dim3((G + kThreads - 1) / kThreads), dim3(kThreads), 0, h->st, h->d_sel.as<PoolSel>(), h->d_hist.as<uint32_t>(), G);
            PG_HIP_TRY(h, hipGetLastError());
        }
        PG_HIP_TRY(h, hipEventRecord(h->e1, h->st));
        PG_HIP_TRY(h, hipMemcpyAsync(sel.data(), h->d_sel.p, (size_t)G * sizeof(PoolSel), hipMemcpyDeviceToHost, h->st));
        PG_HIP_TRY(h, hipStreamSynchronize(h->st));
        PG_HIP_TRY(h, hipEventElapsedTime(&ms, h->e0, h->e1));
    }
    for (uint32_t g = 0; g < G; g++) {
        if (h->r_status[g] != PG_POOL_GROUP_OK) continue;
        const PoolSel &s = sel[g];
        if (s.state & SEL_LOST) { pool_clear(h); return pg_fail(h, PG_ERR_HIP, "pg_pool_finish: internal: the selection of group %u ran out of values", g); }
        h->r_lo[g] = (int64_t)s.prefix_lo - kBias; h->r_hi[g] = (int64_t)s.prefix_hi - kBias;
        if (h->r_lo[g] == 0 && h->r_hi[g] == 0) // datamash would print the sign of a negative zero in the middle: the existing "-0" rule
            for (uint64_t k = g_off[g]; k < g_off[g + 1]; k++)
                if (h->files[g_mem[k]].flags & F_NEGZERO) { refuse(g, g_mem[k], std::string("file ") + std::to_string(g_mem[k]) + " holds a negative zero and the pool's median is 0; pools have no host path"); break; }
        if (h->r_status[g] != PG_POOL_GROUP_OK) { h->r_lo[g] = h->r_hi[g] = h->r_origin[g] = h->r_s1[g] = 0; h->r_s2lo[g] = h->r_s2hi[g] = 0; continue; }
        PgSlotModel m{}; m.n = h->r_n[g]; m.mid_lo = h->r_lo[g]; m.mid_hi = h->r_hi[g];
        h->r_med[g] = (double)pg_model_median(m);
        if (m.n >= 2) h->r_sd[g] = (double)(sqrtl((long double)h->r_num[g] / ((long double)m.n * (long double)(m.n - 1))) / 1e8L);
    }
    pg_pool_result &r = h->result;
    r = pg_pool_result{};
    r.model.n_slots = G; r.model.flags = h->flags & PG_MODEL_KEEP_FIRST;
    r.model.n_values = h->r_n.data(); r.model.median = h->r_med.data(); r.model.sstdev = h->r_sd.data(); r.model.mid_lo = h->r_lo.data(); r.model.mid_hi = h->r_hi.data();
    r.model.origin = h->r_origin.data(); r.model.sum1 = h->r_s1.data(); r.model.sum2_lo = h->r_s2lo.data(); r.model.sum2_hi = h->r_s2hi.data();
    r.model.dwell_n = h->r_dn.data(); r.model.dwell_median = h->r_dmed.data();
    r.n_groups = G; r.n_batches = h->n_batches; r.status = h->r_status.data(); r.refused_file = h->r_refused.data(); r.n_files = h->r_files.data();
    r.n_files_total = F; r.n_bytes = h->n_bytes; r.n_values = h->arena_n; r.select_ms = ms;
    *out = r;
    h->finished = true;
    return PG_OK;
}

size_t pg_pool_format(const pg_pool *h, uint32_t group, int32_t which, char *buf, size_t cap) {
    if (!h || !h->finished || !buf || cap == 0 || group >= h->result.n_groups) return 0;
    buf[0] = 0;
    if (h->r_status[group] != PG_POOL_GROUP_OK) return 0;
    int w;
    if (which == PG_MODEL_TEXT_MEDIAN) { PgSlotModel m{}; m.mid_lo = h->r_lo[group]; m.mid_hi = h->r_hi[group]; w = snprintf(buf, cap, "%.14Lg", pg_model_median(m)); }
    else if (which == PG_MODEL_TEXT_SSTDEV) w = h->r_n[group] < 2 ? snprintf(buf, cap, "nan") : pg_model_sstdev_text(h->r_n[group], h->r_num[group], buf, cap);
    else return 0;
    return (w < 0 || (size_t)w >= cap) ? 0 : (size_t)w;
}

const char *pg_pool_refusal(const pg_pool *h, uint32_t group) {
    return (h && h->finished && group < h->r_why.size()) ? h->r_why[group].c_str() : "";
}

} // extern "C"
