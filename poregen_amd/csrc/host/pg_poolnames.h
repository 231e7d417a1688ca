// pg_poolnames.h -- what `poregen model --pool` and `poregen offsets` share (host only): the checks on the dump files' names, made before a
// device is asked for, and the run of a DumpSet through pg_pool_* (include/pgmove.h) -- batches of whole logical files, batch i + 1 read on
// -t threads while batch i is on the device, as `poregen model` does.
#pragma once
#include "../../../include/pgmove.h"
#include "pg_dumpdir.h"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <future>
#include <string>
#include <vector>

namespace pgh {

struct PoolNames { size_t k = 0; char alphabet[5] = "ACGT"; };

// one length, and all over ACGT or all over ACGU (gmove --rna writes U). err names the first offender.
inline bool check_pool_names(const std::vector<std::string> &names, PoolNames &out, std::string &err) {
    out = PoolNames();
    if (names.empty()) { err = "no dump files to pool"; return false; }
    out.k = names[0].size();
    for (const std::string &n : names)
        if (n.size() != out.k) { err = n + ": the names have more than one length (" + std::to_string(n.size()) + " against " + std::to_string(out.k) + ")"; return false; }
    char tu = 0;
    for (const std::string &n : names)
        for (char c : n) {
            if (c != 'A' && c != 'C' && c != 'G' && c != 'T' && c != 'U') { err = n + ": a name that is no k-mer over ACGT or ACGU"; return false; }
            if (c == 'T' || c == 'U') { if (!tu) tu = c; else if (tu != c) { err = n + ": the names mix T and U"; return false; } }
        }
    if (tu) out.alphabet[3] = tu;
    return true;
}

inline uint32_t pool_base_code(char c) { return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : 3u; }

struct PoolTimes { double create = 0, read = 0, wait = 0, submit = 0, finish = 0; };

// Every logical file of ds through a new handle; groups_of(file, gid[n_labelings]) names its groups. On success *out_h holds the finished
// handle (the caller destroys it) and res its result. A refused group fails the run: err names the group's index and the file.
inline bool run_pool(const DumpSet &ds, int n_threads, bool keep_first, const std::vector<uint32_t> &n_groups,
                     const std::function<void(size_t, uint32_t *)> &groups_of, pg_pool **out_h, pg_pool_result &res, PoolTimes &tm, std::string &err) {
    using clk = std::chrono::steady_clock;
    auto secs = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); };
    *out_h = nullptr;
    uint64_t cap = 64ull << 20;
    if (const char *s = getenv("POREGEN_MODEL_BATCH")) { const long long v = atoll(s); if (v >= 1) cap = (uint64_t)v; }
    cap = std::min<uint64_t>(cap, 1ull << 31);
    std::vector<std::pair<size_t, size_t>> batches;
    for (size_t i = 0; i < ds.names.size();) {
        if (ds.size[i] > (1ull << 31)) { err = ds.names[i] + " is larger than 2^31 bytes"; return false; }
        size_t j = i; uint64_t b = 0;
        while (j < ds.names.size() && j - i < (1u << 22) && (j == i || b + ds.size[j] <= cap)) b += ds.size[j++];
        batches.emplace_back(i, j - i);
        i = j;
    }
    struct Batch { size_t first = 0, n = 0; std::vector<uint8_t> bytes; std::vector<uint64_t> file_off; std::string err; bool ok = true; double secs = 0; };
    auto read_batch = [&](size_t k) {
        Batch b; b.first = batches[k].first; b.n = batches[k].second;
        const clk::time_point t0 = clk::now();
        b.ok = read_dump_files(ds, b.first, b.n, n_threads, b.bytes, b.file_off, b.err);
        b.secs = secs(t0, clk::now());
        return b;
    };
    std::future<Batch> next;
    if (!batches.empty()) next = std::async(std::launch::async, read_batch, (size_t)0);
    const clk::time_point c0 = clk::now();
    pg_pool *h = nullptr;
    if (pg_pool_create(0, (uint32_t)n_groups.size(), n_groups.data(), 0, keep_first ? PG_MODEL_KEEP_FIRST : 0u, &h) != PG_OK) {
        if (next.valid()) next.wait();
        err = pg_pool_last_error(nullptr); return false;
    }
    tm.create = secs(c0, clk::now());
    const size_t L = n_groups.size();
    std::vector<uint32_t> gid, one(L);
    for (size_t k = 0; k < batches.size(); k++) {
        const clk::time_point w0 = clk::now();
        Batch b = next.get();
        tm.wait += secs(w0, clk::now()); tm.read += b.secs;
        if (k + 1 < batches.size()) next = std::async(std::launch::async, read_batch, k + 1);
        bool ok = b.ok;
        if (!ok) err = b.err;
        else {
            gid.assign(L * b.n, PG_POOL_NO_GROUP);
            for (size_t i = 0; i < b.n; i++) { groups_of(b.first + i, one.data()); for (size_t l = 0; l < L; l++) gid[l * b.n + i] = one[l]; }
            const clk::time_point s0 = clk::now();
            ok = pg_pool_submit(h, b.bytes.data(), b.file_off.data(), (uint32_t)b.n, gid.data(), PG_LOC_HOST) == PG_OK;
            tm.submit += secs(s0, clk::now());
            if (!ok) err = pg_pool_last_error(h);
        }
        if (!ok) { if (next.valid()) next.wait(); pg_pool_destroy(h); return false; }
    }
    const clk::time_point f0 = clk::now();
    if (pg_pool_finish(h, &res) != PG_OK) { err = pg_pool_last_error(h); pg_pool_destroy(h); return false; }
    tm.finish = secs(f0, clk::now());
    if (res.n_files_total != ds.names.size()) { err = "internal: " + std::to_string(res.n_files_total) + " files came back"; pg_pool_destroy(h); return false; }
    *out_h = h;
    return true;
}

// the first refused group, if any: its index and "<file name>: <message>"
inline bool pool_refused(const DumpSet &ds, const pg_pool *h, const pg_pool_result &res, uint32_t &group, std::string &what) {
    for (uint32_t g = 0; g < res.n_groups; g++)
        if (res.status[g] == PG_POOL_GROUP_REFUSED) {
            group = g;
            const int64_t f = res.refused_file[g];
            what = (f >= 0 && (size_t)f < ds.names.size() ? ds.names[(size_t)f] : std::string("?")) + ": " + pg_pool_refusal(h, g);
            return true;
        }
    return false;
}

inline void pool_summary(const char *tag, const pg_pool_result &res, const PoolTimes &tm, double t_list, double t_print, int n_threads) {
    uint64_t pooled = 0; // values that count in some group (a file counts once per labeling it is in)
    for (uint32_t g = 0; g < res.n_groups; g++) pooled += res.model.n_values[g];
    fprintf(stderr, "[%s] n_files: %llu n_bytes: %llu n_values: %llu n_batches: %u n_groups: %u n_pooled_values: %llu select_ms: %.3f\n", tag,
            (unsigned long long)res.n_files_total, (unsigned long long)res.n_bytes, (unsigned long long)res.n_values, res.n_batches, res.n_groups,
            (unsigned long long)pooled, res.select_ms);
    fprintf(stderr, "[%s] time: listing %.3f s, device context %.3f s, reading files %.3f s on %d threads (waited for: %.3f s), submit %.3f s, finish %.3f s, printing %.3f s\n",
            tag, t_list, tm.create, tm.read, n_threads, tm.wait, tm.submit, tm.finish, t_print);
}

} // namespace pgh
