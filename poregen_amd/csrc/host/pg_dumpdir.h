// pg_dumpdir.h -- the files of dump directories as `poregen model` sees them (host only; shared by host/model_cli.cpp and the CPU test shim).
// Per directory: what the shell glob DIR/* of scripts/poregen.sh:62 yields that can be read as a file -- names sorted by strcmp, names that
// begin with '.' skipped, anything that is not a regular file skipped. Several directories: the logical file of a name is the byte
// concatenation of that name's files in argument order (`cat a/K b/K`); the names are the sorted union.
#pragma once
#include <dirent.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <thread>
#include <vector>

namespace pgh {

struct DumpPart { uint32_t dir; uint64_t size; };
struct DumpSet {
    std::vector<std::string> dirs;
    std::vector<std::string> names;            // sorted union
    std::vector<std::vector<DumpPart>> parts;  // per name: its files, in argument order
    std::vector<uint64_t> size;                // per name: bytes of the logical file
};

// fn(i) for i in [0, n) on up to n_threads threads
template <class Fn> inline void dump_parallel_for(size_t n, int n_threads, Fn fn) {
    if (n_threads <= 1 || n < 2) { for (size_t i = 0; i < n; i++) fn(i); return; }
    std::atomic<size_t> next{0};
    auto work = [&]() { for (;;) { const size_t i0 = next.fetch_add(64); if (i0 >= n) return; for (size_t i = i0; i < std::min(n, i0 + 64); i++) fn(i); } };
    std::vector<std::thread> pool;
    for (int t = 1; t < n_threads; t++) pool.emplace_back(work);
    work();
    for (auto &t : pool) t.join();
}

inline bool list_dump_dirs(const std::vector<std::string> &dirs, int n_threads, DumpSet &out, std::string &err) {
    out = DumpSet();
    out.dirs = dirs;
    std::map<std::string, std::vector<DumpPart>> all;
    for (uint32_t d = 0; d < dirs.size(); d++) {
        DIR *dp = opendir(dirs[d].c_str());
        if (!dp) { err = "Could not open directory " + dirs[d] + ": " + strerror(errno); return false; }
        std::vector<std::string> names;
        while (struct dirent *de = readdir(dp)) if (de->d_name[0] != '.') names.emplace_back(de->d_name);
        closedir(dp);
        std::vector<int64_t> size(names.size(), -1); // -1: not a regular file
        dump_parallel_for(names.size(), n_threads, [&](size_t i) {
            struct stat sb;
            if (stat((dirs[d] + "/" + names[i]).c_str(), &sb) == 0 && S_ISREG(sb.st_mode)) size[i] = (int64_t)sb.st_size;
        });
        for (size_t i = 0; i < names.size(); i++) if (size[i] >= 0) all[names[i]].push_back({d, (uint64_t)size[i]});
    }
    for (auto &kv : all) { // (std::map<std::string>: byte order, strcmp's for names without NUL)
        uint64_t total = 0;
        for (const DumpPart &p : kv.second) total += p.size;
        out.names.push_back(kv.first); out.size.push_back(total); out.parts.push_back(std::move(kv.second));
    }
    return true;
}

// the logical files [first, first + n) back to back into bytes (file_off[n + 1], file_off[0] = 0), read on n_threads threads
inline bool read_dump_files(const DumpSet &ds, size_t first, size_t n, int n_threads, std::vector<uint8_t> &bytes, std::vector<uint64_t> &file_off, std::string &err) {
    file_off.assign(n + 1, 0);
    for (size_t i = 0; i < n; i++) file_off[i + 1] = file_off[i] + ds.size[first + i];
    bytes.resize(file_off[n] ? file_off[n] : 1);
    std::atomic<bool> failed{false};
    std::string first_err;
    std::atomic_flag err_lock = ATOMIC_FLAG_INIT;
    dump_parallel_for(n, n_threads, [&](size_t i) {
        uint64_t at = file_off[i];
        for (const DumpPart &p : ds.parts[first + i]) {
            if (!p.size) continue;
            const std::string path = ds.dirs[p.dir] + "/" + ds.names[first + i];
            std::string e;
            const int fd = open(path.c_str(), O_RDONLY);
            if (fd < 0) e = "Could not open " + path + ": " + strerror(errno);
            else {
                uint64_t got = 0;
                while (got < p.size) {
                    const ssize_t r = pread(fd, bytes.data() + at + got, p.size - got, (off_t)got);
                    if (r < 0 && errno == EINTR) continue;
                    if (r <= 0) { e = "Could not read " + path + (r < 0 ? std::string(": ") + strerror(errno) : std::string(": the file changed while it was read")); break; }
                    got += (uint64_t)r;
                }
                char extra;
                if (e.empty() && pread(fd, &extra, 1, (off_t)p.size) > 0) e = "Could not read " + path + ": the file changed while it was read";
                close(fd);
            }
            if (!e.empty()) { failed = true; while (err_lock.test_and_set()) {} if (first_err.empty()) first_err = e; err_lock.clear(); return; }
            at += p.size;
        }
    });
    if (failed) { err = first_err; return false; }
    return true;
}

} // namespace pgh
