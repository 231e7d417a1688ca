"""Hand-written dump files for `poregen model` (tests/test_dump_model_host.py, tests/test_gpu_dump_model.py): what gmove writes without -d
(the strict grammar the device parses) and everything else the pipeline's text tools may meet."""
import os
import shutil

# (name, content, inside the strict grammar  (-?D+.DDDDDDDD[,;])*  with |value| < 4e7 and every event closed by ';')
ODD_FILES = [
    ("AAAAA", "1.00000000,2.00000000;:3.00000000,4.50000000;:", False),           # -d output: datamash stops at ":3.00000000"
    ("AAAAC", ":1.00000000,2.00000000;3.00000000;", False),                        # a leading ':' goes with the value tail drops
    ("AAAAG", "1.00000000,2.00000000,4.00000000;\n", False),                       # a trailing newline
    ("AAAAT", "1.00000000,1e2,3.00000000;", False),
    ("AAACA", "1.00000000,+1.5,3.00000000;", False),
    ("AAACC", "1.00000000, 2.5,3.00000000;", False),
    ("AAACG", "1.00000000,2.5000000,3.00000000;", False),                          # 7 decimals
    ("AAACT", "1.00000000,2.500000001,3.00000000;", False),                        # 9 decimals
    ("AAAGA", "5.00000000,-0.00000000,2.00000000;3.25000000;", True),              # a negative zero that is not the median
    ("AAAGC", "7.25000000,8.50000000;", True),                                     # a single value behind tail: sstdev nan
    ("AAAGG", "", True),                                                           # an empty file
    ("AAAGT", "1.00000000,2.00000000,3.00000000", False),                          # a single event without the final ';'
    ("AAATA", "1.00000000,40000000.00000000,3.00000000;", False),                  # 4e7: outside the fixed-point view
    ("AAATC", "1.00000000,inf,3.00000000;", False),
    ("AAATG", "1.00000000,2.00000000;3.00000000,4.00000000,5.50000000;-6.25000000;", True),
    ("AAATT", "0.12345678;", True),                                                # one value: nothing is left behind tail
    ("AACAA", "-12.50000000,250.75000000;100.12500000,-3.00000000;", True),
]


def write_odd_dir(path):
    """the files above plus a dot file and a subdirectory, which the tool skips; returns (n_strict, n_outside)"""
    os.makedirs(path)
    for name, content, _ in ODD_FILES:
        with open(os.path.join(path, name), "w") as f:
            f.write(content)
    with open(os.path.join(path, ".hidden"), "w") as f:
        f.write("1.00000000,2.00000000;")
    os.makedirs(os.path.join(path, "sub"))
    with open(os.path.join(path, "sub", "CCCCC"), "w") as f:
        f.write("1.00000000,2.00000000;")
    n_strict = sum(1 for f in ODD_FILES if f[2])
    return n_strict, len(ODD_FILES) - n_strict


def regular_files_only(src, dst):
    """what the shell glob src/* yields that is a file, copied to dst: the directory the oracle (which opens whatever it lists) is run on"""
    os.makedirs(dst)
    for name in os.listdir(src):
        p = os.path.join(src, name)
        if not name.startswith(".") and os.path.isfile(p):
            shutil.copyfile(p, os.path.join(dst, name))
    return dst


def concatenated(dirs, dst):
    """`cat a/K b/K ...` for every name K of the union, written by the test itself"""
    os.makedirs(dst)
    names = sorted({n for d in dirs for n in os.listdir(d) if not n.startswith(".") and os.path.isfile(os.path.join(d, n))})
    for n in names:
        with open(os.path.join(dst, n), "wb") as out:
            for d in dirs:
                p = os.path.join(d, n)
                if os.path.isfile(p):
                    with open(p, "rb") as f:
                        out.write(f.read())
    return dst
