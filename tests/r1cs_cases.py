"""The matrices of the t cases, shared by tests/test_gpu_r1cs.py (the kernels against the model) and tests/test_r1cs_model.py (the table builder of
csrc/marlin_host.hpp under sanitizers, through tests/t_tables_host_check.cpp).  Every count is derived from T_SEG and T_HEAVY_SEGMENTS as csrc/gpu.hpp states them, so a
re-tuned constant moves the cases with it -- and a case that can no longer be built raises instead of passing on something else.

A case places entry counts on POSITIONS of H and maps them back to variables (the inverse of reindex_by_subdomain), because "heavy", "empty" and "next to" are properties
of the bucketed columns.  A column's entries are (matrix, row) pairs taken in the order A's rows, B's rows, C's rows: a column of 2 rows entries is dense in A and B only."""
import os
import random
import re
import struct

import numpy as np

import r1cs_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aes_zero_knowledge_proof_circuit_amd", "csrc")


def gpu_hpp_constant(name):
    text = open(os.path.join(CSRC, "gpu.hpp")).read()
    m = re.search(r"\b%s = (\d+)\b" % name, text)
    assert m, "constant %s not found in gpu.hpp" % name
    return int(m.group(1))


T_SEG, T_HEAVY_SEGMENTS = gpu_hpp_constant("T_SEG"), gpu_hpp_constant("T_HEAVY_SEGMENTS")
THRESHOLD = T_SEG * T_HEAVY_SEGMENTS                    # the most entries of a column that is NOT heavy
COEFFS = [1, -1, 2, -128, 1 << 40, -(1 << 40)]          # +-1 take their own branches of k_t_partials; GCM reaches -128; +-2^40 is beyond anything a circuit holds
T_N = 4096
T_SHAPES = [(T_N, m, rows) for m in (1, 64) for rows in (T_N, T_N - 5)]


def variable_at(n, m, h):
    """the variable whose bucketed column is position h of H"""
    kind, i = rm.h_map(n, m, h)
    return i if kind == "x" else m + i


def triple_from_columns(n, m, rows, counts, seed):
    """counts: {position on H: entries} -> ((A, B, C) as CSR triples of numpy arrays, {position: entries}); coefficients cycle through COEFFS from a seeded start"""
    per = [[[] for _ in range(rows)] for _ in range(3)]              # per[matrix][row] = [(variable, coefficient)]
    rng = random.Random(seed)
    for h, count in sorted(counts.items()):
        if count > 3 * rows:
            raise AssertionError("a column of %d entries does not fit 3 x %d rows: T_SEG x T_HEAVY_SEGMENTS outgrew the case" % (count, rows))
        var, at = variable_at(n, m, h), rng.randrange(len(COEFFS))
        for e in range(count):
            per[e // rows][e % rows].append((var, COEFFS[(at + e) % len(COEFFS)]))
    mats = []
    for q in range(3):
        rowptr, col, coeff = [0], [], []
        for row in per[q]:
            for var, c in row:
                col.append(var); coeff.append(c)
            rowptr.append(len(col))
        mats.append((np.array(rowptr, dtype=np.uint32), np.array(col, dtype=np.uint32), np.array(coeff, dtype=np.int64)))
    return mats, dict(counts)


def segments(count):
    return -(-count // T_SEG)


def expected_stats(counts):
    segs = [segments(c) for c in counts.values()]
    return {"nseg": sum(segs), "n_heavy": sum(1 for s in segs if s > T_HEAVY_SEGMENTS), "max_segments": max(segs, default=0)}


def t_case(name, n, m, rows):
    """(A, B, C), {position: entries}) of the named case"""
    seed = sum(map(ord, name)) * 131 + m * 7 + rows
    if name == "boundary":        # exactly the threshold (not heavy) | one entry more (heavy, its last segment holds one entry) | dense in A, B and C
        counts = {5: THRESHOLD, 6: THRESHOLD + 1, 7: 3 * rows}
        assert segments(THRESHOLD) == T_HEAVY_SEGMENTS and segments(THRESHOLD + 1) == T_HEAVY_SEGMENTS + 1 and (THRESHOLD + 1) % T_SEG == 1
        assert 3 * rows > THRESHOLD + 1, "3 x rows entries no longer reach past the threshold"
    elif name == "segments":      # one segment -1 / exactly / +1; a heavy column between two empty ones; heavy columns at both ends of H's interior; the last column
        counts = {10: T_SEG - 1, 11: T_SEG, 12: T_SEG + 1, 100: THRESHOLD + T_SEG + 1, 1: 3, n - 2: THRESHOLD + 1, n - 1: 2}
        assert 99 not in counts and 101 not in counts and n - 3 not in counts
    elif name == "light":         # no heavy column at all
        counts = {0: 1, 3: T_SEG + 5, 64: 2 * T_SEG, 65: 1, n - 1: T_SEG - 1, n // 2: THRESHOLD}
    elif name == "empty":         # an entirely empty matrix triple: no segment, every output zero
        counts = {}
    else:
        raise ValueError(name)
    return triple_from_columns(n, m, rows, counts, seed)


T_CASE_NAMES = ["boundary", "segments", "light", "empty"]


def random_triple(n, m, rows, per_row, seed):
    """a random sparse triple: about per_row entries per row and matrix, distinct columns within a row"""
    rng = random.Random(seed)
    mats = []
    for _ in range(3):
        rowptr, col, coeff = [0], [], []
        for _row in range(rows):
            cols = sorted(rng.sample(range(n), rng.randrange(0, 2 * per_row + 1)))
            col += cols
            coeff += [rng.choice(COEFFS + [3, -7]) for _ in cols]
            rowptr.append(len(col))
        mats.append((np.array(rowptr, dtype=np.uint32), np.array(col, dtype=np.uint32), np.array(coeff, dtype=np.int64)))
    return mats


def write_cases(path, cases):
    """cases: [(n, m, rows, (A, B, C))] -> the little-endian file tests/t_tables_host_check.cpp reads: u64 count, then per case u64 n, m, rows, T_SEG,
    T_HEAVY_SEGMENTS and per matrix u64 nnz, u32 rowptr[rows + 1], u32 col[nnz], i64 coeff[nnz]"""
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(cases)))
        for n, m, rows, mats in cases:
            f.write(struct.pack("<5Q", n, m, rows, T_SEG, T_HEAVY_SEGMENTS))
            for rowptr, col, coeff in mats:
                f.write(struct.pack("<Q", len(col)))
                f.write(np.ascontiguousarray(rowptr, dtype="<u4").tobytes() + np.ascontiguousarray(col, dtype="<u4").tobytes() + np.ascontiguousarray(coeff, dtype="<i8").tobytes())
