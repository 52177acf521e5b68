"""The model of tests/r1cs_model.py against things it shares no code with -- closed forms, dense products, the CPU oracle -- and the prover's table builder
(csrc/marlin_host.hpp build_t_tables) on the host under sanitizers.  No GPU."""
import ctypes as C
import os
import random
import subprocess
import tempfile

import pytest

import r1cs_cases as rc
import r1cs_model as rm
from test_cbc_host import CLANG, CSRC, ROOT

R = rm.R377
INDEX_SHAPES = [(2, 1), (4, 1), (4, 2), (8, 2), (64, 16), (512, 1), (1024, 512), (1024, 4)]          # the (n, m) of tests/test_gpu_r1cs.py's index-map cases
T_SHAPES = sorted({(n, m) for n, m, _ in rc.T_SHAPES} | {(256, 16)})
SEED = bytes(range(1, 33))


def key_words(seed):
    return [int.from_bytes(seed[4 * i:4 * i + 4], "little") for i in range(8)]


def test_the_modulus_and_the_domain_generator(zko):
    assert R == zko.R377 and R.bit_length() == rm.FR_BITS and (R - 1) % (1 << rm.TWO_ADICITY) == 0 and (R - 1) % (1 << (rm.TWO_ADICITY + 1)) != 0
    for lg in (1, 3, 12):
        g = rm.domain_gen(lg)
        assert pow(g, 1 << lg, R) == 1 and pow(g, 1 << (lg - 1), R) == R - 1
    # the oracle's transform uses the same generator: the transform of X is (g^i)
    n = 8
    buf = C.create_string_buffer(zko.fr_pack([0, 1] + [0] * (n - 2)), 32 * n)
    assert zko.lib().zko_api_ntt(377, buf, C.c_size_t(n), 0) == 0
    assert zko.fr_unpack(buf.raw) == [pow(rm.domain_gen(3), i, R) for i in range(n)]


@pytest.mark.parametrize("n,m", sorted(set(INDEX_SHAPES + T_SHAPES)))
def test_reindex_is_a_bijection_and_h_map_inverts_it(n, m):
    seen = [rm.reindex(n, m, i) for i in range(n)]
    assert sorted(seen) == list(range(n))
    for i, h in enumerate(seen):
        assert rm.h_map(n, m, h) == (("x", i) if i < m else ("w", i - m))
        assert rc.variable_at(n, m, h) == i
    assert [rm.reindex(n, m, i) for i in range(m)] == [i * (n // m) for i in range(m)]               # the instance sits on the subdomain X of H


def test_the_maps_place_every_variable():
    n, m, nw = 8, 2, 5
    z = [1, 0] + [1, 1, 0, 1, 1]
    zh = rm.z_on_h(z, n, m, nw)
    assert [zh[rm.reindex(n, m, i)] for i in range(m + nw)] == z and zh[rm.reindex(n, m, m + nw)] == 0
    assert rm.w_classes(z, n, m, nw) == [0 if k % 4 == 0 else zh[k] for k in range(n)]
    x = [5] * n
    assert rm.w_evals(z, x, n, m, nw) == [0 if k % 4 == 0 else (zh[k] - 5) % R for k in range(n)]


@pytest.mark.parametrize("lg_n,lg_m", [(1, 0), (3, 1), (5, 4)])
def test_the_lagrange_scalars_sum_to_one_and_vanish_on_x(lg_n, lg_m):
    beta = random.Random(lg_n).randrange(2, R)
    lag, lag_w = rm.lagrange(lg_n, lg_m, beta)
    assert sum(lag) % R == 1
    vx = (pow(beta, 1 << lg_m, R) - 1) % R
    ratio = 1 << (lg_n - lg_m)
    assert all((w == 0) if k % ratio == 0 else (w * vx % R == lag[k]) for k, w in enumerate(lag_w))
    # beta inside H: L_k is the indicator of beta; where beta^m = 1 there is no lag_w
    g = rm.domain_gen(lg_n)
    for k in range(1 << lg_n):
        lag, lag_w = rm.lagrange(lg_n, lg_m, pow(g, k, R))
        assert lag == [int(j == k) for j in range(1 << lg_n)] and (lag_w is None) == (k % ratio == 0)


def test_the_lagrange_scalars_are_the_oracles_interpolants_at_beta(zko):
    """L_k = the inverse transform of the k-th unit vector, evaluated at beta by Horner"""
    lg_n, n = 3, 8
    beta = random.Random(8).randrange(2, R)
    lag, _ = rm.lagrange(lg_n, 0, beta)
    for k in range(n):
        buf = C.create_string_buffer(zko.fr_pack([int(j == k) for j in range(n)]), 32 * n)
        assert zko.lib().zko_api_ntt(377, buf, C.c_size_t(n), 1) == 0
        acc = 0
        for c in reversed(zko.fr_unpack(buf.raw)):
            acc = (acc * beta + c) % R
        assert acc == lag[k], k


@pytest.mark.parametrize("rounds", [12, 20])
def test_the_chacha_words_are_the_oracles(zko, rounds):
    n = 16 * 9 + 3                                           # past two of the oracle's four-block refills
    w = (C.c_uint32 * n)()
    zko.lib().zko_api_chacha_words(SEED, rounds, C.c_size_t(n), w)
    assert rm.chacha_words(key_words(SEED), rounds, 0, n) == [int(x) for x in w]
    assert rm.chacha_words(key_words(SEED), rounds, 37, 20) == [int(x) for x in w[37:57]]
    assert rm.chacha_block(key_words(SEED), 1 << 32, rounds) != rm.chacha_block(key_words(SEED), 0, rounds)      # the counter's high word is part of the state


def test_chacha20_known_answer():
    ks = b"".join(x.to_bytes(4, "little") for x in rm.chacha_block([0] * 8, 0, 20))
    assert ks.hex().startswith("76b8e0ada0f13d90405d6ae55386bd28bdd219b8a08ded1aa836efcc8b770dc7")


@pytest.mark.parametrize("rounds", [12, 20])
def test_the_field_stream_is_the_oracles(zko, rounds):
    n = 200
    out = C.create_string_buffer(32 * n)
    zko.lib().zko_api_fr_rand_stream(377, SEED, rounds, C.c_size_t(n), out)
    got, pos = rm.field_stream(key_words(SEED), rounds, 0, n)
    assert rm.raw_pack(got) == out.raw
    assert pos % 8 == 0 and pos // 8 > n                     # some candidate was rejected (acceptance is about 0.58)
    # a stream resumed at next_word_pos continues the same sequence, also from a position that is no multiple of 8 or 16
    head, mid = rm.field_stream(key_words(SEED), rounds, 0, 77)
    tail, end = rm.field_stream(key_words(SEED), rounds, mid, n - 77)
    assert head + tail == got and end == pos
    assert rm.field_stream(key_words(SEED), rounds, 5, 3)[0] != got[:3] and rm.field_stream(key_words(SEED), rounds, 5, 0) == ([], 5)


def test_spmv_and_t_against_dense_products():
    """a 16 x 16 case: z_M = M z and t = sum_M eta_M M^T r_alpha with the columns carried to their positions on H, through dense matrices"""
    n, m, rows = 16, 4, 13
    rng = random.Random(16)
    mats = rc.random_triple(n, m, rows, 2, 160)
    z = [rng.randrange(2) for _ in range(n)]
    r_alpha, etas = [rng.randrange(R) for _ in range(n)], [rng.randrange(R) for _ in range(3)]
    dense = []
    for rowptr, col, coeff in mats:
        d = [[0] * n for _ in range(n)]
        for row in range(rows):
            for i in range(rowptr[row], rowptr[row + 1]):
                d[row][col[i]] += int(coeff[i])
        dense.append(d)
    for (rowptr, col, coeff), d in zip(mats, dense):
        want = [sum(d[row][c] * z[c] for c in range(n)) for row in range(n)]
        field, small = rm.spmv(rowptr, col, coeff, rows, n, z)
        assert field == [w % R for w in want] and small == [max(-127, min(127, w)) for w in want]
    want_t = [0] * n
    for c in range(n):
        want_t[rm.reindex(n, m, c)] = sum(etas[q] * dense[q][row][c] * r_alpha[row] for q in range(3) for row in range(n)) % R
    assert rm.t_model(n, m, rows, mats, r_alpha, etas) == want_t
    assert any(want_t) and rm.mask_fixup([3, 4, 5], 1) == [(R - 9) % R, 4, 5]


def test_the_t_cases_are_what_they_claim():
    """the case lists of tests/r1cs_cases.py at the constants as they stand: the boundary case holds a column of exactly T_HEAVY_SEGMENTS segments beside one of one more"""
    for n, m, rows in rc.T_SHAPES:
        _, counts = rc.t_case("boundary", n, m, rows)
        segs = sorted(rc.segments(c) for c in counts.values())
        assert segs[0] == rc.T_HEAVY_SEGMENTS and segs[1] == rc.T_HEAVY_SEGMENTS + 1 and rc.expected_stats(counts)["n_heavy"] == 2
        assert rc.expected_stats(rc.t_case("light", n, m, rows)[1])["n_heavy"] == 0
        assert rc.expected_stats(rc.t_case("light", n, m, rows)[1])["max_segments"] == rc.T_HEAVY_SEGMENTS
        assert rc.expected_stats(rc.t_case("empty", n, m, rows)[1]) == {"nseg": 0, "n_heavy": 0, "max_segments": 0}


def test_the_table_builder_under_asan_ubsan():
    """tests/t_tables_host_check.cpp over the matrices of every t case of tests/test_gpu_r1cs.py: every entry exactly once, segments non-empty and at most T_SEG long,
    col_seg_ptr monotone, the heavy list exactly the columns above the threshold -- and the statistics the GPU test will assert.  A stand-alone program: nothing is
    loaded into python."""
    cases, want = [], []
    for n, m, rows in rc.T_SHAPES:
        for name in rc.T_CASE_NAMES:
            mats, counts = rc.t_case(name, n, m, rows)
            cases.append((n, m, rows, mats)); want.append(rc.expected_stats(counts))
    cases.append((256, 16, 251, rc.random_triple(256, 16, 251, 2, 7))); want.append(None)
    cxx = CLANG if os.path.exists(CLANG) else "g++"
    flags = ["-x", "c++", "-O1", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC]
    if cxx == CLANG:
        flags += ["-mllvm", "-asan-globals=0"]        # (as tests/test_keytag_host.py)
    with tempfile.TemporaryDirectory() as d:
        exe, data = os.path.join(d, "t_tables_host_check"), os.path.join(d, "cases.bin")
        rc.write_cases(data, cases)
        subprocess.check_call([cxx] + flags + [os.path.join(ROOT, "tests", "t_tables_host_check.cpp"), "-o", exe])
        env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
        out = subprocess.run([exe, data], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    lines = out.stdout.split("\n")
    assert lines[len(cases)] == "t_tables_host_check ok"
    for i, w in enumerate(want):
        if w is not None:
            assert lines[i] == "case %d %d %d %d" % (i, w["nseg"], w["n_heavy"], w["max_segments"])
