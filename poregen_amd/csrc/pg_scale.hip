// pg_scale.hip -- pg_params.scaling == PG_SCALING_PER_READ (include/pgmove.h: pg_set_read_scaling): the caller's per-read center, spread
// and use flag written into what the collector's kernels already read.
//
// The gathers compute (x - md) / ma from a 32-byte record per read, {offset, range / digitisation, md, ma} (gcal; pg_dev.h: gather_load),
// which the statistics kernels write for med-MAD. Here nobody computes statistics (pg_stats_plan.h: PG_STATS_NONE): k_scale_records writes
// the records from the caller's arrays, and the gathers run unchanged. A read without a scaling goes the way a read with an out-of-range
// sample goes under PG_FLAG_SKIP_OUT_OF_RANGE: oor[r] = 1, which k_apply_oor turns into PGR_SKIPPED in front of the walk.
//
// The dense gathers divide through a reciprocal whose proof wants a divisor >= 1 (pg_select.h: pg_div_by_recip); a spread is any positive
// number, so the kernel raises the batch's "divide with the instruction" flag (stat_err[3]), and every form of the gather gives the one
// correctly rounded quotient.
#include <hip/hip_runtime.h>
#include "pg_internal.h"
#include "pg_dev.h"

namespace {

// one lane per read, queued behind k_batch_init, the only other writer of div_flag's array in a scaling-2 context (it resets the flags
// where the batch's plan says so); the flag is set in every batch, so it holds whether or not anybody reset it. bad: lowest read with use set and a spread that is not a
// finite non-zero number or a center that is not finite (0xffffffff: none), by atomicMin as k_rl_starts reports its read.
__global__ __launch_bounds__(256) void k_scale_records(uint32_t n_reads, const double *__restrict__ dig, const double *__restrict__ off, const double *__restrict__ range,
                                                       const double *__restrict__ center, const double *__restrict__ spread, const uint8_t *__restrict__ use,
                                                       double *__restrict__ gcal, double *__restrict__ med, double *__restrict__ mad, uint8_t *__restrict__ oor,
                                                       int32_t *__restrict__ div_flag, uint32_t *__restrict__ bad) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r == 0) *div_flag = 1;
    if (r >= n_reads) return;
    const bool u = use[r] != 0;
    // a read that is not used still gets a record no gather can trip over (none reads it: the read has no event)
    const double c = u ? center[r] : 0.0, s = u ? spread[r] : 1.0;
    const bool finite_c = c - c == 0.0, finite_s = s - s == 0.0;
    if (u && (!finite_c || !finite_s || s == 0.0)) atomicMin(bad, r);
    const double o = off[r];
    reinterpret_cast<double4 *>(gcal)[r] = make_double4(o, range[r] / dig[r], c, s); // (range / digitisation: the expression PgStatRec::scale uses)
    med[r] = c; mad[r] = s;
    oor[r] = u ? 0 : 1;
}

} // namespace

hipError_t pg_launch_scale_records(hipStream_t st, const PgDevBatch &B, const double *center, const double *spread, const uint8_t *use, double *gcal, double *med, double *mad,
                                   uint8_t *oor, int32_t *div_flag, uint32_t *bad) {
    hipError_t e = hipMemsetAsync(bad, 0xff, sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_scale_records, dim3(B.n_reads ? (B.n_reads + 255u) / 256u : 1u), dim3(256), 0, st, B.n_reads, B.dig, B.off, B.range, center, spread, use, gcal, med, mad, oor,
                       div_flag, bad);
    return hipGetLastError();
}
