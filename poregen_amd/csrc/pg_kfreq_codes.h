// pg_kfreq_codes.h -- the 4-bit base codes of a BAM record's sequence field, shared by the kernel that counts packed reads
// (pg_kfreq.hip), the SAM front-end that packs column 10 (host/kfreq_reads.cpp) and the host test shim.
//   code  0 1 2 3 4 5 6 7 8 9 10 11 12 13 14 15
//   letter = A C M G R S V T W Y  H  K  D  B  N          (SAM specification 4.2.3; htslib's seq_nt16_str)
// A code is a set of bases (bit 0 = A, 1 = C, 2 = G, 3 = T), so the complement of a code is its four bits in reverse order.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PG_KF_HD __host__ __device__ __forceinline__
#else
#define PG_KF_HD static inline
#endif

// the letter of a code, as `samtools fastq` prints it
PG_KF_HD uint32_t pg_kf_letter(uint32_t code) {
    const uint64_t lo = 0x565352474d43413dull, hi = 0x4e42444b48595754ull; // "=ACMGRSV", "TWYHKDBN", first letter in the low byte
    return (uint32_t)((code & 8 ? hi : lo) >> (8 * (code & 7))) & 0xff;
}

// the code of the complementary base set: A<->T, C<->G, M<->K, R<->Y, V<->B, H<->D; '=', S, W, N stay
PG_KF_HD uint32_t pg_kf_complement(uint32_t code) {
    return (code & 1) << 3 | (code & 2) << 1 | (code & 4) >> 1 | (code & 8) >> 3;
}

// the code htslib packs for a byte of a SAM record's SEQ column (seq_nt16_table): the letters above in either case, any other byte N
PG_KF_HD uint32_t pg_kf_code_of_byte(uint32_t byte) {
    if (byte >= 'a' && byte <= 'z') byte -= 32;
    if (byte == '=') return 0;
    for (uint32_t c = 1; c < 15; c++)
        if (pg_kf_letter(c) == byte) return c;
    return 15;
}
