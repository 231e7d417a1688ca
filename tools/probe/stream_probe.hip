// stream_probe.hip -- how fast can one MI355X READ a 400 MB int16 buffer with the access shapes k_read_stats could use? (lines W: how fast can it
// WRITE one; PROBE_ONLY_WRITE=1 stops behind them)
// build: hipcc --offload-arch=gfx950 -O3 -o stream_probe stream_probe.hip ; run: ./stream_probe
#include <hip/hip_runtime.h>
#ifdef PROBE_REAL_KERNEL
#include "../../poregen_amd/csrc/pg_kernels.hip" // the product kernel on the probe's data (hipcc -DPROBE_REAL_KERNEL -I../../include -I../../poregen_amd/csrc)
#endif
#include <cstdio>
#include <cstdint>
#include <vector>
#include <cstdlib>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)

__device__ __forceinline__ uint32_t fold(const int4 &q) { return (uint32_t)(q.x ^ q.y ^ q.z ^ q.w); }

// A: plain grid-stride 16-byte reads, 256-thread blocks
__global__ __launch_bounds__(256) void k_plain(const int4 *__restrict__ v, size_t n, uint32_t *out) {
    uint32_t acc = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) acc ^= fold(v[i]);
    if (acc == 0x12345678u) out[0] = acc;
}
// W: plain grid-stride 16-byte WRITES, 256-thread blocks (what a generator such as k_sim_emit can hope for; run before the buffer is read)
__global__ __launch_bounds__(256) void k_write(int4 *__restrict__ v, size_t n, int x) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) v[i] = make_int4(x, (int)i, x, (int)i);
}
// B: one wave (64-thread block) per 8 KB chunk, all 8 loads issued, then consumed
__global__ __launch_bounds__(64) void k_chunk(const int4 *__restrict__ v, size_t n, uint32_t *out) {
    const size_t base = (size_t)blockIdx.x * 512 + threadIdx.x;
    int4 q[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) q[u] = v[base + u * 64];
    uint32_t acc = 0;
#pragma unroll
    for (int u = 0; u < 8; ++u) acc ^= fold(q[u]);
    if (acc == 0x12345678u) out[0] = acc;
}
// C: persistent waves, chunk c of wave w = w + c*G, rolling refill of 8 slots (DEPTH rows in flight)
template <int WORK> __global__ __launch_bounds__(64) void k_roll(const int4 *__restrict__ v, size_t n_chunks, uint32_t *out) {
    const size_t G = gridDim.x;
    size_t c = blockIdx.x;
    int4 q[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) q[u] = v[c * 512 + u * 64 + threadIdx.x];
    uint32_t acc = 0;
    for (; c < n_chunks; c += G) {
        const size_t nc = c + G < n_chunks ? c + G : c;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            uint32_t f = fold(q[u]);
#pragma unroll
            for (int k = 0; k < WORK; ++k) f = f * 1664525u + 1013904223u; // stand-in for the binning ALU work
            acc ^= f;
            q[u] = v[nc * 512 + u * 64 + threadIdx.x];
        }
    }
    if (acc == 0x12345678u) out[0] = acc;
}
// D: like B but each block handles R consecutive chunks one after the other (no prefetch)
__global__ __launch_bounds__(64) void k_chunk_seq(const int4 *__restrict__ v, size_t n_chunks, int R, uint32_t *out) {
    uint32_t acc = 0;
    for (int k = 0; k < R; ++k) {
        const size_t c = (size_t)blockIdx.x + (size_t)k * gridDim.x;
        if (c >= n_chunks) break;
        int4 q[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) q[u] = v[c * 512 + u * 64 + threadIdx.x];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc ^= fold(q[u]);
    }
    if (acc == 0x12345678u) out[0] = acc;
}


typedef unsigned short us2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void bin8(uint32_t *hist, const int4 &q, uint32_t c2, uint32_t cap2) {
    const us2 cv = __builtin_bit_cast(us2, c2), capv = __builtin_bit_cast(us2, cap2);
    const int w[4] = {q.x, q.y, q.z, q.w};
    us2 d[4], t[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) d[i] = __builtin_bit_cast(us2, w[i]) - cv;
#pragma unroll
    for (int i = 0; i < 4; ++i) d[i] = __builtin_elementwise_min(d[i], capv);
#pragma unroll
    for (int i = 0; i < 4; ++i) t[i] = d[i] >> (unsigned short)4;
#pragma unroll
    for (int i = 0; i < 4; ++i) d[i] = d[i] + t[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) d[i] = d[i] << (unsigned short)2;
    char *hb = reinterpret_cast<char *>(hist);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t aw = __builtin_bit_cast(uint32_t, d[i]);
        atomicAdd(reinterpret_cast<uint32_t *>(hb + (aw & 0xffffu)), 1u);
        atomicAdd(reinterpret_cast<uint32_t *>(hb + (aw >> 16)), 1u);
    }
}
#define HWORDS (1024 + 64 + 32 + 4)
// E: wave per chunk; MODE bit0: chunk offset comes from a table (dependent scalar load); bit1: zero an LDS histogram;
// bit2: bin all samples into it with LDS atomics
template <int MODE> __global__ __launch_bounds__(64) void k_chunk_x(const int4 *__restrict__ v, const uint64_t *__restrict__ tab, uint32_t *out) {
    __shared__ __attribute__((aligned(16))) uint32_t hist[HWORDS];
    const int lane = threadIdx.x;
    if (MODE & 2) { uint4 *h4 = (uint4 *)hist; for (int i = lane; i < HWORDS / 4; i += 64) h4[i] = make_uint4(0, 0, 0, 0); }
    const size_t base = ((MODE & 1) ? tab[blockIdx.x] : (size_t)blockIdx.x * 512) + lane;
    int4 q[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) q[u] = v[base + u * 64];
    uint32_t acc = 0;
    const uint32_t cap = 1024u + (lane & 31u);
#pragma unroll
    for (int u = 0; u < 8; ++u) { if (MODE & 4) bin8(hist, q[u], 0x00640064u, cap | (cap << 16)); else acc ^= fold(q[u]); }
    if (MODE & 2) { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); acc ^= hist[lane * 17]; }
    if (acc == 0x12345678u) out[0] = acc;
}
// F: rolling persistent + LDS binning
__global__ __launch_bounds__(64) void k_roll_bin(const int4 *__restrict__ v, size_t n_chunks, uint32_t *out) {
    __shared__ __attribute__((aligned(16))) uint32_t hist[HWORDS];
    const int lane = threadIdx.x;
    { uint4 *h4 = (uint4 *)hist; for (int i = lane; i < HWORDS / 4; i += 64) h4[i] = make_uint4(0, 0, 0, 0); }
    const size_t G = gridDim.x;
    size_t c = blockIdx.x;
    int4 q[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) q[u] = v[c * 512 + u * 64 + lane];
    const uint32_t cap = 1024u + (lane & 31u);
    uint32_t acc = 0;
    for (; c < n_chunks; c += G) {
        const size_t nc = c + G < n_chunks ? c + G : c;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            bin8(hist, q[u], 0x00640064u, cap | (cap << 16));
            q[u] = v[nc * 512 + u * 64 + lane];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        acc ^= hist[lane * 17];
        { uint4 *h4 = (uint4 *)hist; for (int i = lane; i < HWORDS / 4; i += 64) h4[i] = make_uint4(0, 0, 0, 0); }
    }
    if (acc == 0x12345678u) out[0] = acc;
}
// signal-like content: codes 100 + level(event) + noise, events of ~10-30 samples
__global__ void k_fill(int16_t *s, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        uint32_t ev = (uint32_t)(i / 30), h = ev * 2654435761u; h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
        uint32_t g = (uint32_t)i * 2246822519u; g ^= g >> 15; g *= 3266489917u; g ^= g >> 16;
        // level 70..130 pA at 0.18 pA per code, noise ~ N(0, 17 codes) as the sum of four uniforms (bench.py's signal)
        int noise = (int)(g & 31) + (int)((g >> 5) & 31) + (int)((g >> 10) & 31) + (int)((g >> 15) & 31) - 62;
        s[i] = (int16_t)(100 + 390 + (h % 333) + noise);
    }
}

// G: as E7 but reads of 500 vectors (8000 bytes, so every other read starts in the middle of a 128-byte line), the
// last row partial: lanes past the end re-read the last vector and do not bin (the shape of bench.py's reads)
__global__ __launch_bounds__(64) void k_chunk_500(const int4 *__restrict__ v, const uint64_t *__restrict__ tab, uint32_t *out) {
    __shared__ __attribute__((aligned(16))) uint32_t hist[HWORDS];
    const int lane = threadIdx.x;
    { uint4 *h4 = (uint4 *)hist; for (int i = lane; i < HWORDS / 4; i += 64) h4[i] = make_uint4(0, 0, 0, 0); }
    const int4 *vp = v + tab[blockIdx.x];
    int4 q[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) q[u] = vp[min(u * 64 + lane, 499)];
    const uint32_t cap = 1024u + (lane & 31u);
#pragma unroll
    for (int u = 0; u < 8; ++u) if (u * 64 + lane <= 499) bin8(hist, q[u], 0x00640064u, cap | (cap << 16));
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    uint32_t acc = hist[lane * 17];
    if (acc == 0x12345678u) out[0] = acc;
}

struct Rec { uint64_t beg, end; int32_t c_lo, span, z0, mode; double offset, scale, inv; uint32_t sym, pad; };
struct BigArgs { uint32_t n; uint64_t n_ops; const int16_t *sig; const uint64_t *a1; const double *a2, *a3, *a4; const int32_t *a5, *a6, *a7; const uint8_t *a8; const uint64_t *a9; const uint32_t *a10; const uint8_t *a11; const uint64_t *a12; };
// H: G + everything of the read comes from a 64-byte record (one scalar load), kernel arguments as k_read_stats, a
// generic pass loop, the edge test
__global__ __launch_bounds__(64) void k_chunk_rec(BigArgs B, const Rec *__restrict__ rec, double *__restrict__ med, uint32_t *out) {
    __shared__ __attribute__((aligned(16))) uint32_t hist[HWORDS];
    const int lane = threadIdx.x;
    const uint32_t r = blockIdx.x;
    const Rec m = rec[r];
    if (m.mode != 0) { if (lane == 0) med[r] = 0.0; return; }
    if (m.span > 1024) return;
    { uint4 *h4 = (uint4 *)hist; for (int i = lane; i < HWORDS / 4; i += 64) h4[i] = make_uint4(0, 0, 0, 0); }
    const uint32_t c16 = (uint32_t)m.c_lo & 0xffffu, c2 = c16 | (c16 << 16);
    const uint32_t cap = 1024u + (lane & 31u), cap2 = cap | (cap << 16);
    const uint64_t beg = m.beg, end = m.end, va = (beg + 7) >> 3, vb = end >> 3;
    if (va < vb) {
        const uint64_t n_vec = vb - va;
        for (uint64_t p = 0; p < n_vec; p += 512) {
            const int4 *__restrict__ vp = reinterpret_cast<const int4 *>(B.sig) + (va + p);
            const uint32_t last = n_vec - p > 512 ? 511 : (uint32_t)(n_vec - p) - 1;
            int4 q[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) q[u] = vp[min((uint32_t)(u * 64 + lane), last)];
#pragma unroll
            for (int u = 0; u < 8; ++u) if ((uint32_t)(u * 64 + lane) <= last) bin8(hist, q[u], c2, cap2);
        }
        if ((va << 3) != beg || (vb << 3) != end) out[1] = 1;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    uint32_t acc = hist[lane * 17];
    if (acc == 0x12345678u) out[0] = acc;
}

int main(int argc, char **argv) {
    const size_t mb = argc > 1 ? (size_t)atoll(argv[1]) : 400; // buffer size in MiB (256 MiB of Infinity Cache: try 1600)
    const size_t bytes = mb << 20, n = bytes / 16, n_chunks = n / 512;
    int4 *d; uint32_t *o;
    CK(hipMalloc(&d, bytes)); CK(hipMalloc(&o, 64)); CK(hipMemset(d, 1, bytes)); hipLaunchKernelGGL(k_fill, dim3(4096), dim3(256), 0, 0, (int16_t *)d, bytes / 2); CK(hipDeviceSynchronize());
    uint64_t *tab; CK(hipMalloc(&tab, n_chunks * 8)); { std::vector<uint64_t> h(n_chunks); for (size_t i = 0; i < n_chunks; ++i) h[i] = i * 512; CK(hipMemcpy(tab, h.data(), n_chunks * 8, hipMemcpyHostToDevice)); }
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    auto time = [&](const char *name, auto launch) {
        for (int i = 0; i < 3; ++i) launch();
        hipEventRecord(e0); for (int i = 0; i < 20; ++i) launch(); hipEventRecord(e1); hipEventSynchronize(e1);
        float ms; hipEventElapsedTime(&ms, e0, e1); ms /= 20;
        printf("%-50s %8.1f us  %6.2f TB/s\n", name, ms * 1e3, bytes / (ms * 1e-3) / 1e12); fflush(stdout);
    };
    const bool only_real = getenv("PROBE_ONLY_REAL") != nullptr;
    if (!only_real) {
    int4 *wbuf; CK(hipMalloc(&wbuf, bytes)); // a buffer of its own: the reads below keep their data
    time("W plain 16-byte writes, 2048 blocks x256", [&] { hipLaunchKernelGGL(k_write, dim3(2048), dim3(256), 0, 0, wbuf, n, 1); });
    time("W plain 16-byte writes, 8192 blocks x256", [&] { hipLaunchKernelGGL(k_write, dim3(8192), dim3(256), 0, 0, wbuf, n, 1); });
    time("W plain, one 16B write per thread (n/256 blocks)", [&] { hipLaunchKernelGGL(k_write, dim3((unsigned)(n / 256)), dim3(256), 0, 0, wbuf, n, 1); });
    CK(hipFree(wbuf));
    if (getenv("PROBE_ONLY_WRITE")) return 0;
    time("A plain grid-stride, 2048 blocks x256", [&] { hipLaunchKernelGGL(k_plain, dim3(2048), dim3(256), 0, 0, d, n, o); });
    time("A plain grid-stride, 8192 blocks x256", [&] { hipLaunchKernelGGL(k_plain, dim3(8192), dim3(256), 0, 0, d, n, o); });
    time("A plain, one 16B per thread (n/256 blocks)", [&] { hipLaunchKernelGGL(k_plain, dim3((unsigned)(n / 256)), dim3(256), 0, 0, d, n, o); });
    time("B wave per 8KB chunk (51200 blocks x64)", [&] { hipLaunchKernelGGL(k_chunk, dim3((unsigned)n_chunks), dim3(64), 0, 0, d, n, o); });
    for (int g : {2048, 4096, 6144, 8192}) {
        char nm[96]; snprintf(nm, sizeof nm, "C rolling persistent, %d waves, work 0", g);
        time(nm, [&] { hipLaunchKernelGGL(k_roll<0>, dim3(g), dim3(64), 0, 0, d, n_chunks, o); });
    }
    for (int g : {4096, 6144, 8192}) {
        char nm[96]; snprintf(nm, sizeof nm, "C rolling persistent, %d waves, work 8", g);
        time(nm, [&] { hipLaunchKernelGGL(k_roll<8>, dim3(g), dim3(64), 0, 0, d, n_chunks, o); });
    }
    for (int g : {4096, 6144, 8192}) {
        char nm[96]; snprintf(nm, sizeof nm, "C rolling persistent, %d waves, work 32", g);
        time(nm, [&] { hipLaunchKernelGGL(k_roll<32>, dim3(g), dim3(64), 0, 0, d, n_chunks, o); });
    }
    for (int R : {2, 4, 8}) {
        char nm[96]; snprintf(nm, sizeof nm, "D wave per chunk, %d chunks per block in turn", R);
        time(nm, [&] { hipLaunchKernelGGL(k_chunk_seq, dim3((unsigned)((n_chunks + R - 1) / R)), dim3(64), 0, 0, d, n_chunks, R, o); });
    }
    time("E0 wave per chunk (as B)", [&] { hipLaunchKernelGGL(k_chunk_x<0>, dim3((unsigned)n_chunks), dim3(64), 0, 0, d, tab, o); });
    time("E1 + chunk offset from a table", [&] { hipLaunchKernelGGL(k_chunk_x<1>, dim3((unsigned)n_chunks), dim3(64), 0, 0, d, tab, o); });
    time("E3 + table + zeroed LDS histogram", [&] { hipLaunchKernelGGL(k_chunk_x<3>, dim3((unsigned)n_chunks), dim3(64), 0, 0, d, tab, o); });
    time("E7 + table + zero + LDS-atomic binning", [&] { hipLaunchKernelGGL(k_chunk_x<7>, dim3((unsigned)n_chunks), dim3(64), 0, 0, d, tab, o); });
    time("E6 zero + binning, no table", [&] { hipLaunchKernelGGL(k_chunk_x<6>, dim3((unsigned)n_chunks), dim3(64), 0, 0, d, tab, o); });
    for (int g : {4096, 6144, 8192}) {
        char nm[96]; snprintf(nm, sizeof nm, "F rolling persistent + binning, %d waves", g);
        time(nm, [&] { hipLaunchKernelGGL(k_roll_bin, dim3(g), dim3(64), 0, 0, d, n_chunks, o); });
    }
    }
    { std::vector<uint64_t> h(n_chunks); for (size_t i = 0; i < n_chunks; ++i) h[i] = i * 500; CK(hipMemcpy(tab, h.data(), n_chunks * 8, hipMemcpyHostToDevice)); }
    time("G 500-vector reads at an 8000-byte stride", [&] { hipLaunchKernelGGL(k_chunk_500, dim3((unsigned)n_chunks), dim3(64), 0, 0, d, tab, o); });
    Rec *rec; CK(hipMalloc(&rec, n_chunks * sizeof(Rec))); double *medb; CK(hipMalloc(&medb, n_chunks * 8));
    { std::vector<Rec> h(n_chunks); for (size_t i = 0; i < n_chunks; ++i) { Rec x{}; x.beg = i * 4000; x.end = x.beg + 4000; x.c_lo = 100; x.span = 800; x.z0 = 0; x.mode = 0; x.offset = 1; x.scale = 0.2; x.inv = 5.0; x.sym = 1; h[i] = x; }
      CK(hipMemcpy(rec, h.data(), n_chunks * sizeof(Rec), hipMemcpyHostToDevice)); }
    BigArgs ba{}; ba.n = (uint32_t)n_chunks; ba.sig = (const int16_t *)d;
    { // the same kernel timed the way bench.py times k_read_stats: ONE launch between two events, other work in front
        float tot = 0; const int reps = 10;
        for (int i = 0; i < reps + 2; ++i) {
            hipLaunchKernelGGL(k_plain, dim3(2048), dim3(256), 0, 0, d, n / 4, o); // something else ran before
            hipEventRecord(e0); hipLaunchKernelGGL(k_chunk_rec, dim3((unsigned)n_chunks), dim3(64), 0, 0, ba, rec, medb, o); hipEventRecord(e1);
            hipEventSynchronize(e1); float ms; hipEventElapsedTime(&ms, e0, e1); if (i >= 2) tot += ms;
        }
        printf("%-50s %8.1f us  %6.2f TB/s\n", "H timed as ONE launch between two events", tot / reps * 1e3, bytes / (tot / reps * 1e-3) / 1e12);
    }
#ifdef PROBE_REAL_KERNEL
    {
        PgDevBatch PB{}; PB.n_reads = (uint32_t)n_chunks; PB.sig = (const int16_t *)d;
        double *madb; CK(hipMalloc(&madb, n_chunks * 8)); int32_t *stb; CK(hipMalloc(&stb, n_chunks * 4 + 64)); CK(hipMemset(stb, 0, n_chunks * 4 + 64));
        static_assert(sizeof(PgStatRec) == sizeof(Rec), "same record");
        for (int ro : {1, 0}) {
            char nm[96]; snprintf(nm, sizeof nm, "k_read_stats (product kernel), range_only=%d", ro);
            time(nm, [&] { hipLaunchKernelGGL(k_read_stats, dim3((unsigned)n_chunks), dim3(64), 0, 0, PB, (const PgStatRec *)rec, medb, madb, stb, stb + n_chunks, 15, (uint8_t *)nullptr, ro, (uint32_t *)nullptr, stb + n_chunks + 4, 0u, (double *)nullptr); });
        }
        { // ... and timed the way bench.py times it: ONE launch between two events, another kernel in front
            float tot = 0; const int reps = 10;
            for (int i = 0; i < reps + 2; ++i) {
                hipLaunchKernelGGL(k_plain, dim3(2048), dim3(256), 0, 0, d, n / 4, o);
                hipEventRecord(e0);
                hipLaunchKernelGGL(k_read_stats, dim3((unsigned)n_chunks), dim3(64), 0, 0, PB, (const PgStatRec *)rec, medb, madb, stb, stb + n_chunks, 15, (uint8_t *)nullptr, 0, (uint32_t *)nullptr, stb + n_chunks + 4);
                hipEventRecord(e1); hipEventSynchronize(e1); float ms; hipEventElapsedTime(&ms, e0, e1); if (i >= 2) tot += ms;
            }
            printf("%-50s %8.1f us  %6.2f TB/s\n", "k_read_stats as ONE launch between two events", tot / reps * 1e3, bytes / (tot / reps * 1e-3) / 1e12);
        }
    }
#endif
    time("H as G + 64-byte record, big kernarg, pass loop", [&] { hipLaunchKernelGGL(k_chunk_rec, dim3((unsigned)n_chunks), dim3(64), 0, 0, ba, rec, medb, o); });
    return 0;
}
