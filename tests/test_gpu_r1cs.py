"""GPU parity tests of the layer between the AES trace and the prover's polynomials -- the sparse products, the index maps, round 2's t, the Lagrange-basis scalars,
round 3's f and the ChaCha field stream (csrc/kernels_witness.hip, csrc/kernels_poly.hip) -- each through its kernel-level C entry point against the big-integer model
of tests/r1cs_model.py (validated on the CPU by tests/test_r1cs_model.py).

The arithmetic is exact, so every comparison is BYTE EQUALITY of packed Montgomery limbs or of int8 / uint8 arrays: no tolerance anywhere.  The entry points fill every
output and scratch buffer with 0xAB bytes before the call, so a slot a kernel does not write is a mismatch.  T_SEG, T_HEAVY_SEGMENTS and VQ_STEP are READ from the
source, so that a re-tuned constant moves its cases with it; the t cases assert through the statistics of the tables built that they hit what they meant to hit."""
import ctypes as C
import random

import numpy as np
import pytest

import r1cs_cases as rc
import r1cs_model as rm
from test_gpu_poly import BOUND_KINDS, POINTWISE_N, R, RR, VQ_STEP, _scalars, assert_canonical, pattern, rep

pytestmark = pytest.mark.gpu

POISON = b"\xab" * 32
KEY = [0x03020100 + 0x04040404 * i for i in range(8)]           # the bytes 0, 1, .., 31 as eight little-endian words


def bits(n, seed):
    return np.random.RandomState(seed).randint(0, 2, size=max(n, 1), dtype=np.uint8)[:n]


def test_the_constants_the_cases_are_derived_from(zko):
    assert R == zko.R377 == rm.R377
    assert rc.T_SEG >= 2 and rc.T_HEAVY_SEGMENTS >= 128 and 2 <= VQ_STEP <= 11        # (k_t_heavy sums with 256 lanes: a heavy column has a partial for every lane of its tree's upper half)


# ---- z_A = A z, z_B = B z and their clamped int8 classes ------------------------------------------------------------------------------------------------------------------
def random_csr(rows, ncols, seed):
    rng = random.Random(seed)
    rowptr, col, coeff = [0], [], []
    for _ in range(rows):
        for _ in range(rng.choice([0, 1, 2, 3, 3, 7])):
            col.append(rng.randrange(ncols)); coeff.append(rng.choice([1, -1, 2, -2, 1, -1, 100, -100, 63]))
        rowptr.append(len(col))
    return rowptr, col, coeff


def check_spmv(zko, api, rowptr, col, coeff, rows, rows_out, z, what):
    want_field, want_small = rm.spmv(rowptr, col, coeff, rows, rows_out, z)
    field, small = api.spmv_bits(rowptr, col, coeff, rows, rows_out, z)
    assert field == zko.fr_pack(want_field), what
    assert small.dtype == np.int8 and small.tolist() == want_small, what
    assert field[32 * rows:] == bytes(32 * (rows_out - rows)) and not small[rows:].any(), what + ": padding rows"
    field_only, none = api.spmv_bits(rowptr, col, coeff, rows, rows_out, z, want_small=False)           # small_out null
    assert none is None and field_only == field, what
    return want_small


@pytest.mark.parametrize("rows_out", [1, 255, 256, 257, 1024])
def test_spmv_bits_shapes(zko, api, rows_out):
    """one 256-lane workgroup +- 1 and four of them; rows = rows_out, three padding rows, and no row at all (every output is padding).
    Sums beyond +-2^62 and INT64_MIN are outside the contract of from_i64 and are not tested."""
    ncols = 97
    z = bits(ncols, rows_out)
    for rows in sorted({rows_out, max(rows_out - 3, 0), 0}):
        rowptr, col, coeff = random_csr(rows, ncols, 10 * rows_out + rows)
        check_spmv(zko, api, rowptr, col, coeff, rows, rows_out, z, "rows %d of %d" % (rows, rows_out))


def test_spmv_bits_at_the_clamp_and_beyond(zko, api):
    """a hand-built matrix: a row for every sum around the +-127 clamp of the int8 classes, sums that cancel, an empty row, +-2^40 and a row of 300 entries.
    z holds only 0 and 1 (column 0 is a zero bit, column 1 a one).  INT64_MIN and sums beyond +-2^62 are outside the contract of from_i64 and are not tested."""
    ncols = 40
    z = np.array([0, 1] + [1] * 19 + [0] * 19, dtype=np.uint8)          # columns 1..20 are set
    rows_spec = [[(1, 5), (2, -5)], [], [(1, 9), (0, 77)], [(0, 3)]]     # 0 by cancellation | 0 from an empty row | an entry under a zero bit adds nothing | only zero bits
    for v in (1, 2, 126, 127, 128, 129):
        rows_spec += [[(3, v)], [(4, -v)], [(5, v - 1), (0, 1000), (6, 1)], [(7, -v + 1), (8, -1)]]
    rows_spec += [[(9, 1 << 40)], [(10, -(1 << 40))], [(11, 1 << 40), (12, -(1 << 40)), (13, -128)]]
    rng = random.Random(300)
    long_row = [(rng.randrange(ncols), rng.choice([1, -1, 2, 3])) for _ in range(300)]
    rows_spec.append(long_row)
    rows_spec.append([(1 + i % 20, 1) for i in range(127)]); rows_spec.append([(1 + i % 20, 1) for i in range(128)]); rows_spec.append([(1 + i % 20, -1) for i in range(128)])
    rowptr, col, coeff = [0], [], []
    for spec in rows_spec:
        for c, v in spec:
            col.append(c); coeff.append(v)
        rowptr.append(len(col))
    rows = len(rows_spec)
    acc = rm.spmv_acc(rowptr, col, coeff, rows, rows, z.tolist())
    for v in (0, 1, -1, 2, -2, 126, -126, 127, -127, 128, -128, 129, -129, 1 << 40, -(1 << 40)):
        assert v in acc, "the matrix lost its row of sum %d" % v
    small = check_spmv(zko, api, rowptr, col, coeff, rows, rows + 5, z.tolist(), "hand-built")
    assert {127, -127, 126, -126} <= set(small) and max(small) == 127 and min(small) == -127


# ---- position on H -> instance / witness variable, in its three inline copies ---------------------------------------------------------------------------------------------
INDEX_SHAPES = [(2, 1), (4, 1), (4, 2), (8, 2), (64, 16), (512, 1), (1024, 512), (1024, 4)]


@pytest.mark.parametrize("n,m", INDEX_SHAPES)
def test_index_maps(zko, api, n, m):
    """k_w_classes, k_w_evals, k_z_evals_h and k_bits_to_field against the model's h_map -- and z_evals_h against reindex, the host helper that buckets the t tables"""
    one, zero = rep(RR), bytes(32)
    for nw in sorted({0, 1, n - m - 1, n - m}):
        if nw < 0:
            continue
        z = bits(m + nw, 1000 * n + 10 * m + nw)
        zl = z.tolist()
        for kind in BOUND_KINDS:
            x_raw = pattern(kind, n, n + nw)
            classes, w, zh, xf = api.w_maps(z, n, m, nw, x_raw)
            what = "n %d, m %d, %d witness variables, x_evals %s" % (n, m, nw, kind)
            assert classes.tolist() == rm.w_classes(zl, n, m, nw), what
            # (1 - x) R = R - x R: the model on raw representatives, the witness bit raised to the representative of one
            want_w = rm.w_evals([b * RR for b in zl], rm.raw_unpack(x_raw), n, m, nw)
            assert w == rm.raw_pack(want_w), what
            want_zh = rm.z_on_h(zl, n, m, nw)
            assert zh == b"".join(one if b else zero for b in want_zh), what
            assert xf == b"".join(one if b else zero for b in zl[:m]), what
            for i, b in enumerate(zl):                                   # the kernels' inline map is the inverse of reindex_by_subdomain
                h = rm.reindex(n, m, i)
                assert zh[32 * h:32 * h + 32] == (one if b else zero), (what, i)
            assert_canonical(w)


# ---- round 2's t -----------------------------------------------------------------------------------------------------------------------------------------------------------
def check_t(zko, api, n, m, rows, mats, kinds, what):
    stats = None
    lists = [(rp.tolist(), cl.tolist(), co.tolist()) for rp, cl, co in mats]
    for ra_kind, eta_kind in kinds:
        ra_raw = pattern(ra_kind, n, n + rows)
        etas = _scalars(eta_kind, 3, m + rows)
        got, stats = api.t_evals(n, m, rows, mats, ra_raw, *[zko.fr_pack([e]) for e in etas])
        want = rm.t_model(n, m, rows, lists, rm.raw_unpack(ra_raw), etas)      # (linear in r_alpha: raw representatives in, raw representatives out)
        bad = [h for h in range(n) if got[32 * h:32 * h + 32] != want[h].to_bytes(32, "little")]
        assert not bad, "%s, r_alpha %s, etas %s: %d positions differ, first %d (unwritten: %s)" % (what, ra_kind, eta_kind, len(bad), bad[0], got[32 * bad[0]:32 * bad[0] + 32] == POISON)
    return stats


ALL_KINDS = [(a, b) for a in BOUND_KINDS for b in BOUND_KINDS]


@pytest.mark.parametrize("n,m,rows", rc.T_SHAPES)
@pytest.mark.parametrize("name", rc.T_CASE_NAMES)
def test_t_evals_at_the_segment_and_heavy_boundaries(zko, api, name, n, m, rows):
    """k_t_partials, k_t_columns, k_t_heavy over the tables of the prover's own builder.  boundary: a column of exactly T_SEG x T_HEAVY_SEGMENTS entries (summed by its
    lane) beside one of one more (summed by a workgroup, last segment of one entry) and one dense in A, B and C; segments: T_SEG - 1, T_SEG, T_SEG + 1 entries, a heavy
    column between empty ones, the last column; light: no heavy column; empty: no entry at all, every output zero.  Coefficients from {1, -1, 2, -128, 2^40, -2^40}."""
    mats, counts = rc.t_case(name, n, m, rows)
    kinds = ALL_KINDS if name == "boundary" and rows == n else [("random", "random"), ("max_rep", "minus_one"), ("minus_one", "max_rep")]
    stats = check_t(zko, api, n, m, rows, mats, kinds, name)
    assert stats == rc.expected_stats(counts), "the tables are not the case that was meant"
    if name == "boundary":
        assert stats["n_heavy"] == 2 and stats["max_segments"] == rc.segments(3 * rows) > rc.T_HEAVY_SEGMENTS + 1
        assert sorted(rc.segments(c) for c in counts.values())[:2] == [rc.T_HEAVY_SEGMENTS, rc.T_HEAVY_SEGMENTS + 1]
    if name == "segments":
        assert stats["n_heavy"] == 2
    if name == "light":
        assert stats["n_heavy"] == 0 and stats["max_segments"] == rc.T_HEAVY_SEGMENTS
    if name == "empty":
        assert stats == {"nseg": 0, "n_heavy": 0, "max_segments": 0}
        assert api.t_evals(n, m, rows, mats, pattern("random", n, 1), rep(RR), rep(RR), rep(RR))[0] == bytes(32 * n)


@pytest.mark.parametrize("m,rows", [(1, 256), (16, 251), (128, 256)])
def test_t_evals_of_a_random_sparse_triple(zko, api, m, rows):
    n = 256
    mats = rc.random_triple(n, m, rows, 2, 7 * m + rows)                # about 4 entries per row over A, B, C... per matrix 0..4
    stats = check_t(zko, api, n, m, rows, mats, [("random", "random"), ("zero", "random"), ("random", "zero")], "random triple")
    assert stats["n_heavy"] == 0 and stats["nseg"] > 0


# ---- the Lagrange-basis scalars ---------------------------------------------------------------------------------------------------------------------------------------------
LAGRANGE_SHAPES = sorted({(lg_n, lg_m) for lg_n in (1, 3, VQ_STEP - 1, VQ_STEP, VQ_STEP + 1, 12) for lg_m in (0, 1, lg_n - 1) if 0 <= lg_m < lg_n})


@pytest.mark.parametrize("lg_n,lg_m", LAGRANGE_SHAPES)
def test_lagrange_scalars(zko, api, lg_n, lg_m):
    """the product tree of one launch, at the switch to two and beyond it, then k_lagrange_finish.  beta = r - 1 lies IN H (it is g^(n/2)): L_k(beta) is then the
    indicator of k = n / 2, which the product tree delivers without a division; lag_w divides by beta^m - 1, which is zero there for every m >= 2 -- the inverse of zero
    is outside the contract, so at beta = r - 1 lag_w is compared for m = 1 only."""
    for beta in (random.Random(100 * lg_n + lg_m).randrange(2, R), R - 1):
        lag, lag_w = api.lagrange_scalars(lg_n, lg_m, zko.fr_pack([beta]))
        want, want_w = rm.lagrange(lg_n, lg_m, beta)
        assert lag == zko.fr_pack(want), "lag, beta %x" % beta
        assert sum(want) % R == 1
        assert (want_w is None) == (beta == R - 1 and lg_m >= 1)
        if want_w is not None:
            assert lag_w == zko.fr_pack(want_w), "lag_w, beta %x" % beta
        ratio = 1 << (lg_n - lg_m)
        assert all(lag_w[32 * k:32 * k + 32] == bytes(32) for k in range(0, 1 << lg_n, ratio))


# ---- round 3's f on K -------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", POINTWISE_N)
@pytest.mark.parametrize("data", BOUND_KINDS)
@pytest.mark.parametrize("consts", BOUND_KINDS)
def test_f_evals_from_tables(zko, api, k, data, consts):
    """k_f_from_tables: the three-term dot product in the lazy form, the short cut of a zero numerator (all-zero values; all-zero scalars), two gathers"""
    n = 64
    va, vb, vc = [pattern(data, k, k + 11 * j) for j in range(3)]
    ra, rb = pattern(data if data != "zero" else "random", n, k + 50), pattern("random", n, k + 51)
    es = _scalars(consts, 3, k)
    rng = random.Random(k)
    for ri, ci in (([rng.randrange(n) for _ in range(k)], [rng.randrange(n) for _ in range(k)]), ([n - 1] * k, [n - 1] * k)):
        got = api.f_evals_from_tables(va, vb, vc, *[zko.fr_pack([e]) for e in es], ra, rb, ri, ci)
        want = rm.f_model(*[zko.fr_unpack(a) for a in (va, vb, vc)], *es, zko.fr_unpack(ra), zko.fr_unpack(rb), ri, ci)
        assert got == zko.fr_pack(want)
        assert_canonical(got)


# ---- prover randomness ------------------------------------------------------------------------------------------------------------------------------------------------------
WORD_POSITIONS = [0, 1, 7, 15, 16, 17, 16 * (2 ** 32 - 2) + 5]            # (the last: the block counter crosses into its high word inside the batch)


@pytest.mark.parametrize("rounds", [12, 20])
@pytest.mark.parametrize("word_pos", WORD_POSITIONS)
def test_chacha_field_stream(api, rounds, word_pos):
    """k_chacha_blocks, k_rand_flags, the scan, k_rand_compact from positions inside a candidate, at a block's last word, at and past a block boundary"""
    for count in (1, 7, 1000):
        got, nxt = api.chacha_field_stream(KEY, rounds, word_pos, count)
        want, want_next = rm.field_stream(KEY, rounds, word_pos, count)
        assert got == rm.raw_pack(want), (count, word_pos)
        assert nxt == want_next and (nxt - word_pos) % 8 == 0
        assert_canonical(got)
    if word_pos > 2 ** 32:
        assert rm.chacha_block(KEY, 2 ** 32, rounds) != rm.chacha_block(KEY, 0, rounds) and nxt // 16 > 2 ** 32      # blocks on both sides of the carry were used


@pytest.mark.parametrize("rounds", [12, 20])
def test_chacha_field_stream_equals_the_oracle_from_the_start(zko, api, rounds):
    seed, n = bytes(range(32)), 1000
    out = C.create_string_buffer(32 * n)
    zko.lib().zko_api_fr_rand_stream(377, seed, rounds, C.c_size_t(n), out)
    assert api.chacha_field_stream(KEY, rounds, 0, n)[0] == out.raw


@pytest.mark.parametrize("count,max_cand", [(300, 1), (300, 64), (300, 97), (64, 64)])
def test_chacha_field_stream_refill_batches_are_invisible(api, count, max_cand):
    """the second and later batches of chacha_field_stream -- their own position bookkeeping, which an uncapped call never reaches: the elements and the final position are
    those of the uncapped call and of the model, from an aligned and from an odd start"""
    for word_pos in (0, 21):
        want, want_next = rm.field_stream(KEY, 12, word_pos, count)
        capped = api.chacha_field_stream(KEY, 12, word_pos, count, max_cand=max_cand)
        assert capped == (rm.raw_pack(want), want_next), (count, max_cand, word_pos)
        assert capped == api.chacha_field_stream(KEY, 12, word_pos, count)


def test_chacha_field_stream_chains_and_draws_nothing_for_no_element(api):
    for a, b, cap in ((100, 37, 0), (5, 300, 0), (100, 37, 16)):
        first, mid = api.chacha_field_stream(KEY, 12, 3, a, max_cand=cap)
        second, end = api.chacha_field_stream(KEY, 12, mid, b, max_cand=cap)
        assert (first + second, end) == api.chacha_field_stream(KEY, 12, 3, a + b)
    for pos in (0, 5, 2 ** 40 + 3):
        assert api.chacha_field_stream(KEY, 20, pos, 0) == (b"", pos)
        assert api.chacha_field_stream(KEY, 20, pos, 0, max_cand=1) == (b"", pos)


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("data", BOUND_KINDS)
def test_mask_fixup(api, n, data):
    p = pattern(data, 3 * n, 40 + n)
    got = api.mask_fixup(p, n)
    vals = rm.raw_unpack(got)
    assert (vals[0] + vals[n] + vals[2 * n]) % R == 0                       # (linear: true on the raw representatives as on the values)
    assert got == rm.raw_pack(rm.mask_fixup(rm.raw_unpack(p), n))
    assert got[32:] == p[32:]
    assert_canonical(got)


# ---- refusals: an error, no launch, nothing held --------------------------------------------------------------------------------------------------------------------------
def refused(api, match, call):
    with pytest.raises(api.ZkAesError, match=match):
        call()


def nothing_leaks(api, warm, calls):
    warm()                                                                  # the runtime's own pools, before the first reading
    free0, _ = api.mem_info()
    for _ in range(3):
        for match, call in calls:
            refused(api, match, call)
    free1, _ = api.mem_info()
    assert free0 - free1 < 16 << 20, "device memory leaked on the error path: %d bytes" % (free0 - free1)
    warm()                                                                  # the good path works afterwards


def test_spmv_bits_refusals(api):
    z = [1, 0, 1]
    good = lambda: api.spmv_bits([0, 1, 2], [0, 2], [1, 1], 2, 4, z)
    nothing_leaks(api, good, [
        ("rows must not exceed rows_out", lambda: api.spmv_bits([0, 1, 2], [0, 2], [1, 1], 2, 1, z)),
        ("rowptr must not decrease", lambda: api.spmv_bits([0, 2, 1], [0, 2], [1, 1], 2, 4, z)),
        ("column index out of range", lambda: api.spmv_bits([0, 1, 2], [0, 3], [1, 1], 2, 4, z)),
        ("rows_out out of range", lambda: api.spmv_bits([0], [], [], 0, 0, z)),
    ])


def test_w_maps_refusals(api):
    x = bytes(32 * 8)
    nothing_leaks(api, lambda: api.w_maps([1, 0, 1], 8, 2, 1, x), [
        ("powers of two", lambda: api.w_maps([1] * 6, 6, 2, 1, x)),
        ("powers of two", lambda: api.w_maps([1] * 6, 8, 3, 1, x)),
        ("m must be below n", lambda: api.w_maps([1] * 8, 8, 8, 0, x)),
        ("m must be below n", lambda: api.w_maps([1] * 16, 8, 16, 0, x)),
        ("num_witness must not exceed", lambda: api.w_maps([1] * 9, 8, 2, 7, x)),
    ])


def test_t_evals_refusals(api):
    n, one = 8, rep(RR)
    empty = ([0] * 5, [], [])
    a = ([0, 1, 1, 2, 2], [3, 7], [1, -1])
    ra = bytes(32 * n)
    nothing_leaks(api, lambda: api.t_evals(n, 2, 4, [a, empty, a], ra, one, one, one), [
        ("powers of two", lambda: api.t_evals(12, 2, 4, [a, empty, a], bytes(32 * 12), one, one, one)),
        ("m must be below n", lambda: api.t_evals(n, 8, 4, [a, empty, a], ra, one, one, one)),
        ("rows must not exceed n", lambda: api.t_evals(4, 2, 5, [([0] * 6, [], [])] * 3, ra, one, one, one)),
        ("column index out of range", lambda: api.t_evals(n, 2, 4, [a, empty, ([0, 1, 1, 1, 1], [8], [1])], ra, one, one, one)),
        ("rowptr must not decrease", lambda: api.t_evals(n, 2, 4, [a, ([0, 2, 1, 2, 2], [1, 2], [1, 1]), a], ra, one, one, one)),
    ])


def test_lagrange_scalars_refusals(api):
    beta = rep(5)
    nothing_leaks(api, lambda: api.lagrange_scalars(4, 2, beta), [
        ("lg_m must be in", lambda: api.lagrange_scalars(4, 4, beta)),
        ("lg_m must be in", lambda: api.lagrange_scalars(4, 7, beta)),
        ("lg_m must be in", lambda: api.lagrange_scalars(4, -1, beta)),
        ("2-adicity", lambda: api.lagrange_scalars(48, 2, beta)),
        ("must not exceed 24", lambda: api.lagrange_scalars(25, 2, beta)),
    ])


def test_f_evals_from_tables_refusals(api):
    v, t, e = bytes(32 * 3), bytes(32 * 4), rep(RR)
    nothing_leaks(api, lambda: api.f_evals_from_tables(v, v, v, e, e, e, t, t, [0, 3, 1], [3, 3, 3]), [
        ("index out of range", lambda: api.f_evals_from_tables(v, v, v, e, e, e, t, t, [0, 4, 1], [3, 3, 3])),
        ("index out of range", lambda: api.f_evals_from_tables(v, v, v, e, e, e, t, t, [0, 3, 1], [3, 3, 2 ** 32 - 1])),
        ("out of range", lambda: api.f_evals_from_tables(b"", b"", b"", e, e, e, t, t, [], [])),
    ])


def test_chacha_field_stream_refusals(api):
    nothing_leaks(api, lambda: api.chacha_field_stream(KEY, 12, 0, 10), [
        ("rounds must be", lambda: api.chacha_field_stream(KEY, 13, 0, 10)),
        ("rounds must be", lambda: api.chacha_field_stream(KEY, 0, 0, 10)),
        ("count out of range", lambda: api.chacha_field_stream(KEY, 12, 0, (1 << 24) + 1)),
        ("word_pos too close", lambda: api.chacha_field_stream(KEY, 12, 2 ** 64 - 1, 1)),
    ])
    out, nxt = C.create_string_buffer(32), C.c_uint64()
    assert api.lib().zkaes_chacha_field_stream(None, 12, C.c_uint64(0), C.c_size_t(1), C.c_uint32(0), out, C.byref(nxt)) != 0 and b"null" in api.lib().zkaes_last_error()


def test_mask_fixup_refusals(api):
    nothing_leaks(api, lambda: api.mask_fixup(bytes(96), 1), [
        ("n out of range", lambda: api.mask_fixup(bytes(96), 0)),
        ("n out of range", lambda: api.mask_fixup(bytes(96), (1 << 24) + 1)),
    ])
    assert api.lib().zkaes_mask_fixup(None, C.c_size_t(1)) != 0 and b"null" in api.lib().zkaes_last_error()
