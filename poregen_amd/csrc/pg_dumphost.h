// pg_dumphost.h -- one dump file as the pipeline's text tools read it, on the host (no device code; shared by pg_dumptext.hip and the
// CPU test shim). The device path of `poregen model` handles the files gmove writes without -d; every other file -- and every file the
// device reduction declines -- is finished here, by the rules of scripts/poregen.sh:54-85 and :33-52 as oracle/model_oracle.c states them:
//   stats: tr ';,' '\n' cuts the bytes at ';' ',' '\n' into lines (a last line without a terminator still counts, an empty one is a
//          line too); tail -n +2 drops the first; datamash parses every line with strtold into long double and stops at a line that is
//          not wholly a number (both fields then stay empty); median = middle value or the mean of the two middle ones; sstdev = sqrtl of
//          sum((x - mean)^2) / (n - 1) with both sums left to right in long double; "%.14Lg"; one value: "nan"; no value: nothing.
//   dwell: awk splits the '\n' records (empty ones have no fields) at ';' and prints the number of ',' per field; datamash median.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

struct PgDumpHostStats {
    uint64_t n = 0;              // values that reached datamash
    bool stopped = false;        // datamash met a line that is no number
    std::string median, sstdev;  // as printed (sstdev before the --stdv_limit cap)
    long double median_ld = NAN, sstdev_ld = NAN;
};
struct PgDumpHostDwell { uint64_t n = 0; uint64_t mid_lo = 0, mid_hi = 0; };

static inline int pg_dump_cmp_ld(const void *a, const void *b) {
    const long double x = *(const long double *)a, y = *(const long double *)b;
    return (x > y) - (x < y);
}

inline void pg_dump_host_stats(const char *b, size_t len, bool keep_first, PgDumpHostStats &o) {
    o = PgDumpHostStats();
    std::vector<long double> v;
    std::string field;
    size_t line_no = 0;
    bool ok = true;
    for (size_t i = 0; i < len;) {
        size_t j = i;
        while (j < len && b[j] != ';' && b[j] != ',' && b[j] != '\n') j++;
        line_no++;
        if (line_no >= 2 || keep_first) {
            field.assign(b + i, j - i);
            char *end;
            const long double x = strtold(field.c_str(), &end);
            if (end == field.c_str() || *end != 0) ok = false;
            v.push_back(x);
        }
        i = j + 1;
    }
    o.n = v.size();
    o.stopped = !ok;
    if (!ok || v.empty()) return;
    char t[64];
    {
        std::vector<long double> w(v);
        qsort(w.data(), w.size(), sizeof(long double), pg_dump_cmp_ld); // (the oracle's sort: the order of equal keys, -0 and 0, is its order)
        const size_t n = w.size();
        o.median_ld = (n & 1) ? w[n / 2] : (w[n / 2 - 1] + w[n / 2]) / 2.0L;
        snprintf(t, sizeof t, "%.14Lg", o.median_ld);
        o.median = t;
    }
    const size_t n = v.size();
    long double sum = 0;
    for (size_t i = 0; i < n; i++) sum += v[i];
    const long double mean = sum / n;
    sum = 0;
    for (size_t i = 0; i < n; i++) sum += (v[i] - mean) * (v[i] - mean);
    if (n < 2) { o.sstdev = "nan"; return; }
    o.sstdev_ld = sqrtl(sum / (n - 1));
    snprintf(t, sizeof t, "%.14Lg", o.sstdev_ld);
    o.sstdev = t;
}

inline void pg_dump_host_dwell(const char *b, size_t len, PgDumpHostDwell &o) {
    std::vector<uint64_t> v;
    for (size_t i = 0; i < len;) {
        size_t e = i;
        while (e < len && b[e] != '\n') e++;
        if (e > i) {
            uint64_t commas = 0;
            for (size_t j = i; j <= e; j++) {
                if (j == e || b[j] == ';') { v.push_back(commas); commas = 0; }
                else if (b[j] == ',') commas++;
            }
        }
        i = e + 1;
    }
    o = PgDumpHostDwell();
    o.n = v.size();
    if (v.empty()) return;
    std::sort(v.begin(), v.end());
    o.mid_lo = v[(v.size() - 1) / 2]; o.mid_hi = v[v.size() / 2];
}

// the stddev column behind the cap: bc -l "$stddev > $limit" on the two texts ("nan" and the empty string do not exceed it)
inline bool pg_dump_sd_capped(const char *sd, const char *limit) {
    return sd[0] && strcmp(sd, "nan") != 0 && strtold(sd, nullptr) > strtold(limit, nullptr);
}
