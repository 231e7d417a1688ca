"""Cases of the F1-score metric shared by the host suite (tests/test_f1_host.py: the restatement against them) and the device suite
(tests/test_gpu_f1_edges.py: the kernels and the CLI against them).

QUIRKS: (id, ss1, si1, ss2, si2, options of f1_ref.pair_counts, [TP, FP, TN, FN]). Every expected row is derived by hand from the
reference's f1score.py; the derivation stands beside the row. A point with refs (r1, r2) counts TN / FP / FN on the value -1 and then
ALSO TP when |r1 - r2| <= threshold, else FP."""
import itertools

QUIRKS = [
    # both sides unmapped: TN, and |-1 - -1| = 0 <= 0: TP
    ("both_unmapped", b"3I", "0,3,10,20", b"3I", "0,3,50,60", {}, [3, 0, 3, 0]),
    # r1 unmapped against mapped: FP, then FP again for |-1 - 10| > 0
    ("r1_unmapped", b"2I", "0,2,10,0", b"2,", "0,2,10,0", {}, [0, 4, 0, 0]),
    # r2 unmapped: FN, then FP
    ("r2_unmapped", b"2,", "0,2,10,0", b"2I", "0,2,10,0", {}, [0, 2, 0, 2]),
    # side 1 from ref -2: one point at -2 (FN, FP), one at -1 by arithmetic (TN and TP against side 2's I)
    ("arithmetic_minus_one", b"1,1,", "0,2,-2,0", b"2I", "0,2,7,0", {}, [1, 1, 1, 1]),
    # RNA steps down from si[2]; side 2 (102 - 2): 100, 100, 99, 99 on both sides
    ("rna_base_shift", b"2,2,", "0,4,100,98", b"2,2,", "0,4,102,100", dict(rna=True, base_shift=-2), [4, 0, 0, 0]),
    ("rna_no_shift", b"2,2,", "0,4,100,98", b"2,2,", "0,4,102,100", dict(rna=True), [0, 4, 0, 0]),
    ("rna_threshold_2", b"2,2,", "0,4,100,98", b"2,2,", "0,4,102,100", dict(rna=True, threshold=2), [4, 0, 0, 0]),
    # "1," at 5, "1D" moves the ref 6 -> 7, "1," at 7: against 5, 5
    ("dna_deletion", b"1,1D1,", "0,2,5,0", b"3,", "0,3,5,0", {}, [1, 1, 0, 0]),
    ("negative_threshold", b"4,", "0,4,1,0", b"4,", "0,4,1,0", dict(threshold=-1), [0, 4, 0, 0]),
    # "0," steps the ref without a point: 2 points at 11
    ("zero_match_steps", b"0,2,", "0,2,10,0", b"2,", "0,2,11,0", {}, [2, 0, 0, 0]),
    # "5X" eats its digits, "M" has none: 2 points at 10
    ("unknown_letters", b"5XM2,", "0,2,10,0", b"2,", "0,2,10,0", {}, [2, 0, 0, 0]),
    ("disjoint", b"3,", "0,3,1,0", b"3,", "3,6,1,0", {}, [0, 0, 0, 0]),
    ("one_common_point", b"3,", "0,3,1,0", b"3,", "2,5,1,0", {}, [1, 0, 0, 0]),
    # signals 1, 2: refs 2, 3 against 2, 2
    ("partial_window", b"1,1,1,", "0,3,1,0", b"2,", "1,3,2,0", {}, [1, 1, 0, 0]),
    # refs 9, 10, 11: only r1 + 1 == 11 is kept, 10 against 0
    ("region_r1_plus_one", b"1,1,1,", "0,3,9,0", b"3,", "0,3,0,0", dict(region=(11, 11)), [0, 1, 0, 0]),
    # int() takes blanks, a sign and single underscores
    ("si_python_int", b"1,", " +0 , 1_0 ,1,1", b"1,", "0,1,1,1", {}, [1, 0, 0, 0]),
    # ---- a zero-point op as the last op of a side: nothing follows it, 3 points at 5 on both sides
    ("trailing_D", b"3,2D", "0,3,5,0", b"3,", "0,3,5,0", {}, [3, 0, 0, 0]),
    ("trailing_zero_match", b"3,0,", "0,3,5,0", b"3,", "0,3,5,0", {}, [3, 0, 0, 0]),
    ("trailing_X", b"3,5X", "0,3,5,0", b"3,", "0,3,5,0", {}, [3, 0, 0, 0]),
    ("trailing_X_side_2", b"3,", "0,3,5,0", b"3,5X", "0,3,5,0", {}, [3, 0, 0, 0]),
    ("trailing_D_side_2", b"3,", "0,3,5,0", b"2,1,4D", "0,3,5,0", {}, [2, 1, 0, 0]),  # 5, 5, 5 against 5, 5, 6
    # ---- as the first op: "0I" does nothing; "2D" moves the ref 5 -> 7 before the first point
    ("leading_zero_I", b"0I2,", "0,2,5,0", b"2,", "0,2,5,0", {}, [2, 0, 0, 0]),
    ("leading_D", b"2D2,", "0,2,5,0", b"2,", "0,2,7,0", {}, [2, 0, 0, 0]),
    ("leading_D_side_2", b"2,", "0,2,5,0", b"2D2,", "0,2,5,0", {}, [0, 2, 0, 0]),
    # ---- adjacent zero-point ops: point at 5, ref 6 -> 7 -> 8 -> 9, point at 9; side 2: 5, then 6 + 3 = 9
    ("adjacent_zero_ops", b"1,0,0,0,1,", "0,2,5,0", b"1,3D1,", "0,2,5,0", {}, [2, 0, 0, 0]),
    ("adjacent_zero_ops_miss", b"1,0,0,0,1,", "0,2,5,0", b"1,1,", "0,2,5,0", {}, [1, 1, 0, 0]),  # 5, 9 against 5, 6
    # ---- letters without digits do nothing: 5, 5, -1 against 5, 5, 5; the last point is FP (r1 unmapped) and FP (|-1 - 5| > 0)
    ("bare_letters", b",I2,D,1I", "0,3,5,0", b"X3,", "0,3,5,0", {}, [2, 2, 0, 0]),
    # ---- I against I under a region: the filter sees r1 + 1 = 0. (0, 0) keeps both points (TN and TP each); (1, 5) drops them
    ("ins_ins_region_0_0", b"2I", "0,2,5,0", b"2I", "0,2,5,0", dict(region=(0, 0)), [2, 0, 2, 0]),
    ("ins_ins_region_1_5", b"2I", "0,2,5,0", b"2I", "0,2,5,0", dict(region=(1, 5)), [0, 0, 0, 0]),
    # ---- window edges
    ("window_of_one_point", b"3,", "0,3,5,0", b"1,", "1,2,5,0", {}, [1, 0, 0, 0]),
    # side 1: signals 0, 1, 2 at refs 5, 6, 7; side 2 starts at signal 2 with ref 7 ...
    ("side_2_at_last_point", b"1,1,1,", "0,3,5,0", b"2,", "2,4,7,0", {}, [1, 0, 0, 0]),
    # ... and one past it
    ("side_2_one_past", b"1,1,1,", "0,3,5,0", b"2,", "3,5,7,0", {}, [0, 0, 0, 0]),
    ("side_1_one_past", b"2,", "3,5,7,0", b"1,1,1,", "0,3,5,0", {}, [0, 0, 0, 0]),
    # ---- a difference of exactly 1 (5 against 6)
    ("diff_1_threshold_minus_1", b"2,", "0,2,5,0", b"2,", "0,2,6,0", dict(threshold=-1), [0, 2, 0, 0]),
    ("diff_1_threshold_0", b"2,", "0,2,5,0", b"2,", "0,2,6,0", dict(threshold=0), [0, 2, 0, 0]),
    ("diff_1_threshold_1", b"2,", "0,2,5,0", b"2,", "0,2,6,0", dict(threshold=1), [2, 0, 0, 0]),
    # ---- RNA refs that descend through -1: 0, -1, -2 on both sides; the middle point is TN too
    ("rna_through_minus_one", b"1,1,1,", "0,3,0,0", b"1,1,1,", "0,3,0,0", dict(rna=True), [3, 0, 1, 0]),
    # against 3I: 0 / -1: FN, FP; -1 / -1: TN, TP; -2 / -1: FN, FP
    ("rna_through_minus_one_vs_I", b"1,1,1,", "0,3,0,0", b"3I", "0,3,0,0", dict(rna=True), [1, 2, 1, 2]),
]


def small_strings(counts=(0, 1, 3), kinds=b",IDX", max_tokens=2):
    """every ss string of 1 to max_tokens tokens <count><kind>, in a fixed order"""
    tokens = [str(c).encode() + bytes([k]) for c in counts for k in kinds]
    out = []
    for n in range(1, max_tokens + 1):
        out += [b"".join(t) for t in itertools.product(tokens, repeat=n)]
    return out


def maps_a_point(ss: bytes) -> bool:
    """a token "<n>," or "<n>I" with n > 0 (for strings made of whole tokens)"""
    num = b""
    for c in ss:
        if 48 <= c < 58:
            num += bytes([c])
            continue
        if num and int(num) > 0 and c in b",I":
            return True
        num = b""
    return False


M = (1 << 62) - 1
D = b"4294967295D"
# values near 2^62, whose sums and differences leave int64: (pair, rna, threshold, region) with pair = (ss1, sig1, ref1, ss2, sig2, ref2);
# the expectations come from f1_ref.pair_counts_py (Python ints)
LARGE = [
    ((b"2," + D + b"1," + D + b"3,", 0, M, b"2," + D + b"2," + D + b"2,", 0, M), False, 0, None),
    ((b"2," + D + b"1," + D + b"3,", 0, -M, b"2," + D + b"2," + D + b"2,", 0, -M), False, 0, None),
    ((b"2," + D + b"1," + D + b"3,", 0, M, b"2," + D + b"2," + D + b"2,", 0, M), True, 0, None),
    ((b"2," + D + b"1," + D + b"3,", 0, -M, b"2," + D + b"2," + D + b"2,", 0, -M + 1), True, 1, None),
    # the two refs 2^63 and more apart: the difference does not fit int64, and it is larger than any threshold
    ((b"1," + D * 3 + b"1,", 0, M, b"2,", 0, -M), False, (1 << 63) - 1, None),
    ((b"1," + D * 3 + b"1,", 0, -M, b"2,", 0, M), True, (1 << 63) - 1, None),
    ((b"1," + D * 3 + b"1,", 0, M, b"2,", 0, -M), False, 1 << 62, None),
    # signal starts near +-2^62 with a small overlap, and with none
    ((b"20,", M - 10, 5, b"10,10I", M - 5, 5), False, 0, None),
    ((b"20,", -M, 5, b"10,10I", -M + 17, 5), False, 0, None),
    ((b"20,", -M, 5, b"20,", M, 5), False, 0, None),
    ((b"20,", M, 5, b"20,", -M, 5), False, 0, None),
    # a threshold the difference just meets (M - 0) and just misses (M + 1 - 0), and a region that keeps r1 + 1 = 2^62 only
    ((b"1,1,", 0, M, b"2,", 0, 0), False, M, None),
    ((b"1,1,1,", 0, M - 1, b"3,", 0, M), False, 0, (M + 1, M + 1)),
    ((b"1,1,1,", 0, -M + 1, b"3,", 0, -M), True, 0, (-M - 1, -M)),
]
