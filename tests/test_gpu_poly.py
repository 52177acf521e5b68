"""GPU parity tests of the prover's polynomial layer (csrc/kernels_poly.hip) and of the transform entry points the prover uses but zkaes_ntt does not reach, each through its
kernel-level C entry point against the big-integer model of tests/poly_model.py (validated on the CPU by tests/test_poly_model.py).

The arithmetic is exact and a canonical representative < r is part of the contract, so every comparison is BYTE EQUALITY of packed Montgomery limbs: no tolerance anywhere.
The shapes are the boundaries of the code as it stands -- block, chunk, level and dispatch constants, READ from the source below, so that a re-tuned constant moves its
cases with it -- and the inputs include the structured ones (all r - 1, all zero, one non-zero coefficient) that reach the value bounds of the lazy arithmetic, which
pseudo-random field elements never approach."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import poly_model as pm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 0x12ab655e9a2ca55660b44d1e5c37b00159aa76fed00000010a11800000000001          # BLS12-377 Fr (asserted against the oracle's below)
RR = pm.R_MONT % R                                                             # Montgomery R mod r: the raw representative of 1
MINUS_ONE = (R - 1) * RR % R                                                   # the raw representative of the VALUE r - 1


def _constant(name):
    text = open(os.path.join(ROOT, "aes_zero_knowledge_proof_circuit_amd", "csrc", "kernels_poly.hip")).read()
    m = re.search(r"\b%s = (\d+)\b" % name, text)
    assert m, "constant %s not found in kernels_poly.hip" % name
    return int(m.group(1))


DL_B = _constant("DL_B")                                # coefficients per lane of the blocked synthetic division
DL_TOP = _constant("DL_TOP_THREADS") * DL_B             # longest sequence the single-workgroup top kernel divides alone
EV_CHUNK, EV_COMBINE_MAX = _constant("EV_CHUNK"), _constant("EV_COMBINE_MAX")
BI_BLOCK = _constant("BI_BLOCK")                        # lanes per workgroup of k_batch_inverse<4> / <16>
VQ_STEP = _constant("VQ_STEP")                          # tree levels per launch of the vanishing-quotient product tree
DIVVAN_C, DIVVAN_MIN_CHAIN = 16, 64                     # divide_by_vanishing: steps per segment / shortest chain that takes the segmented kernels


def test_the_constants_the_shapes_below_are_derived_from(zko):
    assert R == zko.R377
    text = open(os.path.join(ROOT, "aes_zero_knowledge_proof_circuit_amd", "csrc", "kernels_poly.hip")).read()
    assert "const size_t C = %d," % DIVVAN_C in text and "chain >= %d && scratch" % DIVVAN_MIN_CHAIN in text
    assert DL_B >= 2 and DL_TOP > 2 * DL_B + 1 and EV_CHUNK >= 2 and EV_COMBINE_MAX > 256 and BI_BLOCK >= 64 and 1 <= VQ_STEP <= 11       # (what the case lists assume)


# ---- inputs: raw Montgomery representatives (any value < r is one)
def rand_raw_bytes(n, seed):
    """n pseudo-random 32-byte values below 2^252 < r, without a Python loop"""
    a = np.random.RandomState(seed).randint(0, 256, size=(max(n, 1), 32), dtype=np.uint8)
    a[:, 31] &= 0x0f
    return a.tobytes()[:32 * n]


def rep(v, n=1):
    return v.to_bytes(32, "little") * n


def pattern(kind, n, seed):
    """the coefficient patterns of the issue: pseudo-random; every LIMB pattern r - 1 (the largest representative); every VALUE r - 1; all zero; only the top / only the
    constant coefficient non-zero"""
    if kind == "random":
        return rand_raw_bytes(n, seed)
    if kind == "max_rep":
        return rep(R - 1, n)
    if kind == "minus_one":
        return rep(MINUS_ONE, n)
    if kind == "zero":
        return bytes(32 * n)
    if kind == "top_only":
        return bytes(32 * (n - 1)) + rep(R - 1 - seed % 7)
    if kind == "p0_only":
        return rep(R - 1 - seed % 7) + bytes(32 * (n - 1))
    raise ValueError(kind)


PATTERNS = ["random", "max_rep", "minus_one", "zero", "top_only", "p0_only"]
R_LIMBS = [(R >> (64 * k)) & (2 ** 64 - 1) for k in range(4)]


def assert_canonical(buf):
    """every 32-byte word of buf is < r"""
    a = np.frombuffer(buf, dtype="<u8").reshape(-1, 4)
    lt, eq = np.zeros(len(a), dtype=bool), np.ones(len(a), dtype=bool)
    for k in (3, 2, 1, 0):
        lt |= eq & (a[:, k] < np.uint64(R_LIMBS[k]))
        eq &= a[:, k] == np.uint64(R_LIMBS[k])
    assert lt.all(), "non-canonical element at index %d" % int(np.argmin(lt))


def special_points(zko, seed):
    """(name, true value) of the evaluation / division points: random, 0, 1, r - 1"""
    return [("random", random.Random(seed).randrange(2, R - 1)), ("zero", 0), ("one", 1), ("minus_one", R - 1)]


# ---- p / (X - z)
DIVLIN_LENGTHS = ([1, 2, DL_B - 1, DL_B, DL_B + 1, 2 * DL_B - 1, 2 * DL_B, 2 * DL_B + 1]       # one block of k_divlin_top's lanes +- 1, two blocks +- 1
                  + [DL_TOP - 1, DL_TOP, DL_TOP + 1]                                            # k_divlin_top alone | one k_divlin_local / k_divlin_apply level over it
                  + [DL_B * DL_TOP - 1, DL_B * DL_TOP, DL_B * DL_TOP + 1]                       # ... | the first length with TWO local levels
                  + [(1 << 20) - 3])                                                            # an odd length near |H| of a 6-block proof


@pytest.mark.parametrize("n", DIVLIN_LENGTHS)
def test_divide_by_linear(zko, api, n):
    """k_divlin_local / k_divlin_top / k_divlin_apply against q_i = p_(i+1) + z q_(i+1).  The remainder is dropped by the kernel, so the quotient at these lengths is all
    that pins the top block, the carries between blocks and the power table of every level."""
    points = special_points(zko, n)
    cases = [(z, k) for z in points for k in PATTERNS] if n <= DL_B * DL_TOP + 1 else [(points[0], "random")]      # (2^20 coefficients: one model run)
    for (zname, z), kind in cases:
        p = pattern(kind, n, n)
        got = api.poly_divide_by_linear(p, zko.fr_pack([z]))
        want, _ = pm.divide_by_linear(pm.raw_unpack(p), z, R)
        assert len(got) == 32 * (n - 1)
        assert got == pm.raw_pack(want), "len %d, z %s, coefficients %s" % (n, zname, kind)
        assert_canonical(got)


# ---- p / (X^m - 1)
def _divvan_cases():
    cases = []
    for m in (1, 5, 64, 100):                                                   # (m = 1; a power of two; two that are not)
        cases += [(m + 1, m), (2 * m, m), (2 * m + 1, m)]
    for m in (3, 64):
        for steps in (DIVVAN_MIN_CHAIN - 1, DIVVAN_MIN_CHAIN, DIVVAN_MIN_CHAIN + 1):      # the longest chain has exactly `steps` steps: the switch between the two kernels
            cases += [(m * steps + 1, m), (m * steps + m, m)]                  # (one class with `steps`, the others one fewer | every class `steps`)
    cases += [(80, 64), (9, 7)]                                                 # len - m < m: residue classes with no quotient coefficient
    cases += [(2, 1), (17, 1), (1000, 1), (5001, 1)]                            # m = 1: ONE chain; 5000 steps = 313 segments summed per lane
    cases += [((1 << 17) + 1, 64)]                                              # round 1's shape: |H| + 1 coefficients by v_X, 2048-step chains
    cases += [(100 * 70 + 37, 100), (3 * DIVVAN_C * 5 + 2, 3)]                  # m not a power of two with a ragged top segment
    return sorted(set(cases))


@pytest.mark.parametrize("n,m", _divvan_cases())
def test_divide_by_vanishing(zko, api, n, m):
    """k_div_vanishing (one lane per residue class) and the segmented k_divvan_sums / k_divvan_apply, each with and without scratch and with and without the remainder"""
    for kind in ("random", "max_rep", "p0_only", "top_only"):
        p = pattern(kind, n, 31 * n + m)
        q_want, rem_want = pm.divide_by_vanishing(pm.raw_unpack(p), m, R)
        for with_scratch in (False, True):
            for want_rem in (True, False):
                q, rem = api.poly_divide_by_vanishing(p, m, with_scratch=with_scratch, want_rem=want_rem)
                what = "len %d, m %d, %s, scratch %s, remainder %s" % (n, m, kind, with_scratch, want_rem)
                assert q == pm.raw_pack(q_want), what
                assert (rem == pm.raw_pack(rem_want)) if want_rem else rem is None, what
                assert_canonical(q)


def test_divide_by_vanishing_refuses_a_dividend_no_longer_than_the_divisor(api):
    for n, m in ((4, 4), (3, 4), (1, 1), (5, 0)):
        for with_scratch in (False, True):
            with pytest.raises(api.ZkAesError, match="divide_by_vanishing: dividend shorter than divisor"):
                api.poly_divide_by_vanishing(bytes(32 * n), m, with_scratch=with_scratch)


# ---- evaluation
ONE_LEVEL = EV_CHUNK * EV_COMBINE_MAX            # longest polynomial with one level of k_eval_chunks under k_eval_combine


@pytest.mark.parametrize("lens", [
    [0, 1, EV_CHUNK - 1, EV_CHUNK, EV_CHUNK + 1, ONE_LEVEL - 1, ONE_LEVEL, ONE_LEVEL + 1],      # one chunk +- 1; one chunk level against two; mixed in ONE 8-polynomial call
    [EV_CHUNK * ONE_LEVEL + 1, EV_CHUNK * ONE_LEVEL, 0, 255 * EV_CHUNK + 1],                     # three levels | two, full; 256 partials + 1 for the combine's stride
    [ONE_LEVEL + 1],
    [0],
])
def test_poly_eval_multi(zko, api, lens):
    """k_eval_chunks level by level + k_eval_combine against Horner"""
    polys = [pattern("random", n, 17 * n + i) for i, n in enumerate(lens)]
    raws = [pm.raw_unpack(p) for p in polys]
    points = special_points(zko, sum(lens))
    rng = random.Random(sum(lens))
    runs = [[rng.randrange(R) for _ in lens], [points[i % 4][1] for i in range(len(lens))]] + [[z] * len(lens) for _, z in points[1:]]
    for xs in runs:
        got = api.poly_eval_multi(polys, [zko.fr_pack([x]) for x in xs])
        want = [rep(pm.horner(p, x, R)) for p, x in zip(raws, xs)]
        assert got == want, "lens %s, points %s" % (lens, xs)
        assert_canonical(b"".join(got))


@pytest.mark.parametrize("n", [EV_CHUNK + 1, ONE_LEVEL + 1])
def test_poly_eval_of_structured_coefficients(zko, api, n):
    for kind in ("max_rep", "minus_one", "zero", "top_only", "p0_only"):
        p = pattern(kind, n, n)
        for name, x in special_points(zko, n):
            assert api.poly_eval_multi([p], [zko.fr_pack([x])]) == [rep(pm.horner(pm.raw_unpack(p), x, R))], (kind, name)


def test_poly_eval_multi_refuses_more_than_eight(api):
    with pytest.raises(api.ZkAesError, match="1..8"):
        api.poly_eval_multi([bytes(32)] * 9, [bytes(32)] * 9)


# ---- batch inversion
def _check_inverses(zko, api, v, post, throughput):
    postb = None if post is None else zko.fr_pack([post])
    got = api.batch_inverse(v, post=postb, throughput_variant=throughput)
    assert len(got) == len(v)
    assert_canonical(got)
    xs, ys = pm.raw_unpack(v), pm.raw_unpack(got)
    bad = pm.inverse_mismatch(xs, ys, R, post=1 if post is None else post, unit=RR * RR % R)
    assert bad is None, "element %d of %d: %x -> %x (post %s, throughput variant %s)" % (bad, len(xs), xs[bad], ys[bad], post, throughput)
    for i in (0, len(xs) // 2, len(xs) - 1):                                    # and a few against the inverse computed outright
        x = zko.fr_unpack(v[32 * i:32 * i + 32])[0]
        assert zko.fr_unpack(got[32 * i:32 * i + 32])[0] == (pow(x, -1, R) * (1 if post is None else post) % R if x else 0)


@pytest.mark.parametrize("throughput", [False, True], ids=["chunk4_euclid", "chunk16_fermat"])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 4 * BI_BLOCK - 1, 4 * BI_BLOCK, 4 * BI_BLOCK + 1, 16 * BI_BLOCK - 1, 16 * BI_BLOCK, 16 * BI_BLOCK + 1, 3 * 16 * BI_BLOCK + 77])
def test_batch_inverse(zko, api, n, throughput):
    """both template variants of k_batch_inverse (picked by the library's own rule: a ThroughputWaits scope is held for <16>): one workgroup of each +- 1, several workgroups
    with a ragged tail, zeros wherever a prefix product could swallow them, with and without the post factor"""
    post = random.Random(n).randrange(2, R)
    base = bytearray(rand_raw_bytes(n, 5 * n + 1))
    _check_inverses(zko, api, bytes(base), None, throughput)
    _check_inverses(zko, api, bytes(base), post, throughput)
    v = bytearray(base)                                                         # zeros at position 0 and at the end, the values 1 and r - 1, the largest representative
    v[0:32] = bytes(32)
    v[32 * (n - 1):32 * n] = bytes(32)
    if n >= 5:
        v[32:64], v[64:96], v[96:128] = rep(RR), rep(MINUS_ONE), rep(R - 1)
    _check_inverses(zko, api, bytes(v), post, throughput)
    if n > 64:                                                                  # a whole lane's chunk of zeros (16 aligned elements cover a lane of either variant), a zero next to it
        v = bytearray(base)
        v[32 * 32:32 * 48] = bytes(32 * 16)
        v[32 * 49:32 * 50] = bytes(32)
        _check_inverses(zko, api, bytes(v), None, throughput)
    if n > 16 * BI_BLOCK:                                                       # a whole workgroup of zeros (the first 16 x 512 elements: four workgroups of <4>, one of <16>)
        v = bytearray(base)
        v[0:32 * 16 * BI_BLOCK] = bytes(32 * 16 * BI_BLOCK)
        _check_inverses(zko, api, bytes(v), post, throughput)
    assert api.batch_inverse(bytes(32 * n), post=zko.fr_pack([post]), throughput_variant=throughput) == bytes(32 * n)      # all zeros stay zero
    assert api.batch_inverse(rep(RR, n), throughput_variant=throughput) == rep(RR, n)                                      # 1 / 1
    assert api.batch_inverse(rep(MINUS_ONE, n), throughput_variant=throughput) == rep(MINUS_ONE, n)                        # 1 / -1


def test_batch_inverse_above_two_to_the_21_takes_the_throughput_kernel_in_a_lone_call(zko, api):
    n = (1 << 21) + 3
    v = bytearray(rand_raw_bytes(n, 21))
    v[0:32] = bytes(32)
    v[32 * (n - 1):] = bytes(32)
    _check_inverses(zko, api, bytes(v), random.Random(21).randrange(2, R), False)


def test_batch_inverse_of_nothing(api):
    assert api.batch_inverse(b"") == b""


# ---- vanishing quotients
def _domain_gen(zko, cid, n):
    g = C.create_string_buffer(32)
    zko.lib().zko_api_domain_gen(cid, C.c_size_t(n), g)
    return zko.fr_unpack(g.raw, cid)[0]


@pytest.mark.parametrize("lg_n", list(range(0, 23)))
def test_vanishing_quotient_evals(zko, api, lg_n):
    """k_vq_top alone up to lg n = VQ_STEP; one k_vq_expand with a first step of every length 1..VQ_STEP for the next VQ_STEP sizes; two expands above (21, 22: the
    prover's |H|).  out (a - y) == a^n - y^n at y = g h_i, with y^n = g^n on the whole coset, and n a^(n-1) where a IS the coset point; a few indices also through
    pm.vq_holds, which takes y^n by exponentiation.  Whole tables up to 2^16, index 0, n - 1, the special point and 3,000 sampled indices per coset above."""
    n, rng = 1 << lg_n, random.Random(lg_n)
    w = _domain_gen(zko, 377, n)
    ncosets = 3 if lg_n >= 20 else 1 + lg_n % 3
    gs = [1 if (c + lg_n) % 2 == 0 else rng.randrange(2, R) for c in range(ncosets)]      # g = 1 (no product in vq_factor) mixed with g != 1 in one call
    if ncosets == 3:
        gs[2] = rng.randrange(2, R)
    i_special = n // 3
    a_on_coset = gs[-1] * pow(w, i_special, R) % R
    if lg_n <= 16:
        idx = None
        indices = range(n)
    else:
        indices = sorted(set([0, n - 1, i_special] + [rng.randrange(n) for _ in range(3000)]))
        idx = indices
    for a in (rng.randrange(2, R), a_on_coset):
        tables = api.vanishing_quotient_evals(lg_n, [zko.fr_pack([g]) for g in gs], zko.fr_pack([a]), indices=idx)
        an = pow(a, n, R)
        for c, g in enumerate(gs):
            assert_canonical(tables[c])
            out = pm.raw_unpack(tables[c])
            assert len(out) == len(indices)
            rhs = (an - pow(g, n, R)) * RR % R
            at_a = n * pow(a, n - 1, R) * RR % R
            h, prev = 1, 0
            for o, i in zip(out, indices):
                h = h * w % R if i == prev + 1 else pow(w, i, R)
                prev = i
                y = g * h % R
                ok = o == at_a if y == a else o * (a - y) % R == rhs
                assert ok, "lg_n %d, coset %d (g %s 1), index %d, a %s" % (lg_n, c, "==" if g == 1 else "!=", i, "on the coset" if a == a_on_coset else "random")
            for k in (0, len(out) // 2, len(out) - 1):
                assert pm.vq_holds(out[k], a, g * pow(w, indices[k], R) % R, n, R, unit=RR)
            if a == a_on_coset and c == ncosets - 1 and n > 1:                  # a^n == y^n on this coset: every value but the one at a itself is zero
                k = list(indices).index(i_special)
                assert out[k] == at_a and all(o == 0 for j, o in enumerate(out) if j != k)


def test_vanishing_quotient_evals_refuses_bad_arguments(api):
    one = rep(RR)
    for lg_n, ncosets in ((25, 1), (-1, 1), (4, 0), (4, 4)):
        with pytest.raises(api.ZkAesError, match="lg_n|cosets"):
            api.vanishing_quotient_evals(lg_n, [one] * ncosets, one, indices=[0])
    with pytest.raises(api.ZkAesError, match="index out of range"):
        api.vanishing_quotient_evals(4, [one], one, indices=[16])


# ---- pointwise kernels and the linear combination at their value bounds
def _operands(kind, count, n, seed):
    """`count` arrays of n elements: every LIMB pattern r - 1, every VALUE r - 1, all zero, or pseudo-random"""
    return [pattern(kind, n, seed + 101 * j) for j in range(count)]


def _scalars(kind, count, seed):
    if kind == "random":
        rng = random.Random(seed)
        return [rng.randrange(R) for _ in range(count)]
    return [{"max_rep": (R - 1) * pow(RR, -1, R) % R, "minus_one": R - 1, "zero": 0}[kind]] * count      # (max_rep: the VALUE whose representative is r - 1)


POINTWISE_N = [1, 255, 256, 257]                        # one 256-lane workgroup +- 1
BOUND_KINDS = ["max_rep", "minus_one", "zero", "random"]


@pytest.mark.parametrize("n", POINTWISE_N)
@pytest.mark.parametrize("data", BOUND_KINDS)
@pytest.mark.parametrize("consts", BOUND_KINDS)
def test_q1_coset_pointwise(zko, api, n, data, consts):
    """k_q1_coset: sums of two canonical values (< 2 p), shl5 of them, a three-term and a two-term dot product, 2 p - z: the stated bounds are reached by r - 1 everywhere"""
    arrs = _operands(data, 5, n, n)
    cs = _scalars(consts, 6, n)
    got = api.q1_coset_pointwise(*arrs, *[zko.fr_pack([c]) for c in cs])
    want = pm.q1_coset_pointwise(*[zko.fr_unpack(a) for a in arrs], *cs, R)
    assert got == zko.fr_pack(want)
    assert_canonical(got)


@pytest.mark.parametrize("n", POINTWISE_N)
@pytest.mark.parametrize("data", BOUND_KINDS)
@pytest.mark.parametrize("consts", BOUND_KINDS)
def test_h2_coset(zko, api, n, data, consts):
    """k_h2_coset: alpha beta + row_col - (alpha row + beta col) + 2 p (< 4 p) through shl5 (needs < 2^256) into a product"""
    arrs = _operands(data, 7, n, 3 * n)
    cs = _scalars(consts, 7, 3 * n)
    got = api.h2_coset(*arrs, *[zko.fr_pack([c]) for c in cs])
    want = pm.h2_coset(*[zko.fr_unpack(a) for a in arrs], *cs, R)
    assert got == zko.fr_pack(want)
    assert_canonical(got)


@pytest.mark.parametrize("n", POINTWISE_N)
@pytest.mark.parametrize("data", BOUND_KINDS)
def test_q1_combine_coset_scale_and_z_poly(zko, api, n, data):
    q0, q1, q3 = _operands(data, 3, n, 7 * n)
    mask = pattern(data, 3 * n, 7 * n + 5)
    rng = random.Random(n)
    zeta = rng.randrange(2, R)
    inv2, inv2zeta = pow(2, -1, R), pow(2 * zeta, -1, R)
    h1, g1 = api.q1_combine(q0, q1, q3, mask, zko.fr_pack([inv2]), zko.fr_pack([inv2zeta]))
    h1_want, g1_want = pm.q1_combine(*[zko.fr_unpack(a) for a in (q0, q1, q3, mask)], inv2, inv2zeta, R)
    assert h1 == zko.fr_pack(h1_want) and g1 == zko.fr_pack(g1_want)
    assert_canonical(h1)
    # coset_scale: 16 coefficients per lane, one power per lane; the input shorter than the output
    for g in (rng.randrange(2, R), 0, 1, R - 1):
        for in_len in sorted({0, 1, n // 2, max(n - 1, 0), n}):
            src = pattern(data, in_len, n + in_len)
            for out_n in sorted({n, n + 15, n + 16, n + 17}):
                got = api.coset_scale(src, zko.fr_pack([g]), out_n)
                assert got == pm.raw_pack(pm.coset_scale(pm.raw_unpack(src), g, out_n, R)), (g, in_len, out_n)
    # z_poly_from_w: w (X^m - 1) + x, n + 1 coefficients, w shorter than, equal to and longer than n + 1 - m
    for m in sorted({1, 2, max(n // 4, 1)}):
        for wlen in sorted({0, 1, max(n - m, 0), max(n + 1 - m, 0), n + 1}):
            wv, xv = pattern(data, wlen, n + wlen), pattern(data, m, n + m + 1)
            got = api.z_poly_from_w(wv, xv, n)
            want = pm.z_poly_from_w(pm.raw_unpack(wv), pm.raw_unpack(xv), n, R)       # (index by index: a w longer than n + 1 - m is cut at n + 1 coefficients)
            assert got == pm.raw_pack(want), (m, wlen)
            assert_canonical(got)


@pytest.mark.parametrize("n", POINTWISE_N)
@pytest.mark.parametrize("count", [1, 4, 5, 8])
@pytest.mark.parametrize("data", BOUND_KINDS)
def test_poly_lincomb(zko, api, n, count, data):
    """k_lincomb_n: one four-term dot product, or two added (count > 4), terms shorter than the result contributing below their own length only"""
    rng = random.Random(100 * n + count)
    lens = [n if (j == 0 or n == 1) else rng.randrange(1, n) for j in range(count)]       # 0 < len_j < n (and one full-length term)
    if count > 1 and n > 1:
        lens[-1] = n - 1
    polys = [pattern(data, lens[j], n + 31 * j) for j in range(count)]
    for sc_kind in BOUND_KINDS:
        sc = _scalars(sc_kind, count, n + count)
        got = api.poly_lincomb(polys, [zko.fr_pack([s]) for s in sc], n)
        want = pm.lincomb([pm.raw_unpack(p) for p in polys], sc, n, R)
        assert got == pm.raw_pack(want), (lens, sc_kind)
        assert_canonical(got)


def test_poly_lincomb_refuses_bad_arguments(api):
    with pytest.raises(api.ZkAesError, match="1..8 terms"):
        api.poly_lincomb([bytes(32)] * 9, [bytes(32)] * 9, 1)
    with pytest.raises(api.ZkAesError, match="longer than the result"):
        api.poly_lincomb([bytes(64)], [bytes(32)], 1)


# ---- transforms of short inputs (the gather pads with zeros) and on a coset of a generator that is no root of unity
FR_ALL = {377: R, 381: 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001}


def _oracle_ntt(zko, cid, data, n, inverse=False):
    buf = C.create_string_buffer(data, 32 * n)
    assert zko.lib().zko_api_ntt(cid, buf, C.c_size_t(n), 1 if inverse else 0) == 0
    return buf.raw


def _in_lens(n):
    return sorted({0, 1, n // 4, n // 2 + 1, n - 1, n})


@pytest.mark.parametrize("cid", [377, 381])
@pytest.mark.parametrize("lg", [3, 10, 11, 14, 18])
def test_ntt_of_a_short_input_equals_the_oracle_transform_of_the_padded_vector(zko, api, cid, lg):
    """in_len < n (kernels_ntt.hip: `if (sidx < in_len) v = src[sidx]; else v = Fr::zero()`), one- and two-pass plans, plain and on the odd cosets of the 4x domain, where the
    coefficient's power of g rides on the same gather"""
    n, r = 1 << lg, FR_ALL[cid]
    assert r == zko.FR[cid]
    data = rand_raw_bytes(n, 900 + lg + cid)
    raw = pm.raw_unpack(data)
    for coset_c in (0, 1, 3):
        if coset_c:
            g = pow(_domain_gen(zko, cid, 4 * n), coset_c, r)
            scaled = pm.raw_pack(pm.coset_scale(raw, g, n, r))
        for in_len in _in_lens(n):
            src = (scaled if coset_c else data)[:32 * in_len] + bytes(32 * (n - in_len))
            want = _oracle_ntt(zko, cid, src, n)
            got = api.ntt_padded(cid, data[:32 * in_len], n, coset_c=coset_c, lg_big=lg + 2)
            assert got == want, "field %d, lg %d, coset %d, in_len %d" % (cid, lg, coset_c, in_len)


def sampled_outputs_match(got, raw_in, point_of, indices, r):
    """got[i] == sum_j raw_in[j] point_of(i)^j for the sampled i: Horner over the raw representatives"""
    for i in indices:
        want = pm.horner(raw_in, point_of(i), r)
        if got[32 * i:32 * i + 32] != want.to_bytes(32, "little"):
            return i
    return None


@pytest.mark.parametrize("cid", [377, 381])
def test_three_pass_ntt_of_a_short_input_at_sampled_outputs(zko, api, cid):
    lg = 19
    n, r = 1 << lg, FR_ALL[cid]
    data = rand_raw_bytes(n, 1900 + cid)
    raw = pm.raw_unpack(data)
    w, rng = _domain_gen(zko, cid, n), random.Random(cid)
    for coset_c in (0, 3):
        g = pow(_domain_gen(zko, cid, 4 * n), coset_c, r)
        for in_len in _in_lens(n):
            got = api.ntt_padded(cid, data[:32 * in_len], n, coset_c=coset_c, lg_big=lg + 2)
            if in_len == 0:
                assert got == bytes(32 * n)
                continue
            samples = [rng.randrange(n) | 1, rng.randrange(n)]
            bad = sampled_outputs_match(got, raw[:in_len], lambda i: g * pow(w, i, r) % r, samples, r)
            assert bad is None, "field %d, coset %d, in_len %d, output %d" % (cid, coset_c, in_len, bad)


@pytest.mark.parametrize("lg", [1, 3, 10, 11, 14, 18])
def test_ntt_scaled_equals_the_oracle_transform_of_scaled_coefficients(zko, api, lg):
    """coset_power_table + ntt_scaled with g the field's multiplicative generator (round 3's coset of K) and a pseudo-random g: scale by g^k in Python, then the oracle's
    plain transform; the inverse (table of g^-k at the last store) undoes it, also for a short input"""
    n = 1 << lg
    data = rand_raw_bytes(n, 2200 + lg)
    raw = pm.raw_unpack(data)
    for g in (22, random.Random(lg).randrange(2, R)):
        scaled = pm.raw_pack(pm.coset_scale(raw, g, n, R))
        for in_len in _in_lens(n):
            want = _oracle_ntt(zko, 377, scaled[:32 * in_len] + bytes(32 * (n - in_len)), n)
            got = api.ntt_scaled(zko.fr_pack([g]), data[:32 * in_len], n)
            assert got == want, "lg %d, g %d, in_len %d" % (lg, g, in_len)
            assert api.ntt_scaled(zko.fr_pack([g]), got, n, inverse=True) == data[:32 * in_len] + bytes(32 * (n - in_len))
        # the inverse on its own: values -> coefficients, against the oracle's inverse followed by the scaling by g^-k
        plain = pm.raw_unpack(_oracle_ntt(zko, 377, data, n, inverse=True))
        assert api.ntt_scaled(zko.fr_pack([g]), data, n, inverse=True) == pm.raw_pack(pm.coset_scale(plain, pow(g, -1, R), n, R))


def test_ntt_padded_and_scaled_refuse_bad_arguments(api):
    with pytest.raises(api.ZkAesError, match="in_len"):
        api.ntt_padded(377, bytes(32 * 5), 4)
    with pytest.raises(api.ZkAesError, match="power of two"):
        api.ntt_padded(377, bytes(32), 6)
    with pytest.raises(api.ZkAesError, match="field_id"):
        api.ntt_padded(1, bytes(32), 4)
    with pytest.raises(api.ZkAesError, match="must not be zero"):
        api.ntt_scaled(bytes(32), bytes(64), 4)
    with pytest.raises(api.ZkAesError, match="in_len"):
        api.ntt_scaled(rep(RR), bytes(32 * 5), 4)
