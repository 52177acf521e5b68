"""CPU checks of tests/poly_model.py -- the big-integer reference tests/test_gpu_poly.py compares the HIP kernels with -- against itself (every division multiplied back,
schoolbook) and against the CPU oracle where the oracle has the operation.  This is what makes the model a reference and not a second guess."""
import ctypes as C
import random

import pytest

import poly_model as pm


def rand_poly(rng, n, r):
    return [rng.randrange(r) for _ in range(n)]


def add_poly(a, b, r):
    n = max(len(a), len(b))
    return [((a[i] if i < len(a) else 0) + (b[i] if i < len(b) else 0)) % r for i in range(n)]


@pytest.mark.parametrize("n", [1, 2, 3, 16, 17, 100])
def test_division_by_a_linear_factor_multiplies_back(zko, n):
    r, rng = zko.R377, random.Random(n)
    for z in (rng.randrange(r), 0, 1, r - 1):
        p = rand_poly(rng, n, r)
        q, rem = pm.divide_by_linear(p, z, r)
        assert len(q) == n - 1 and rem == pm.horner(p, z, r)
        back = add_poly(pm.poly_mul(q, [(-z) % r, 1], r), [rem], r)
        assert back == p


@pytest.mark.parametrize("n,m", [(2, 1), (5, 4), (8, 4), (9, 4), (10, 3), (40, 7), (130, 64)])
def test_division_by_a_vanishing_polynomial_multiplies_back(zko, n, m):
    r, rng = zko.R377, random.Random(100 * n + m)
    p = rand_poly(rng, n, r)
    q, rem = pm.divide_by_vanishing(p, m, r)
    assert len(q) == n - m and len(rem) == m
    assert add_poly(pm.poly_mul(q, [r - 1] + [0] * (m - 1) + [1], r), rem, r) == p


def test_linear_operations_commute_with_the_montgomery_factor(zko):
    """the raw representatives x R of the data go through the linear operations unchanged in form: the model of R p is R times the model of p"""
    r, rng = zko.R377, random.Random(5)
    p = rand_poly(rng, 37, r)
    z = rng.randrange(r)
    raw = pm.raw_unpack(zko.fr_pack(p))
    assert raw == [v * pm.R_MONT % r for v in p] and pm.raw_pack(raw) == zko.fr_pack(p)
    assert zko.fr_unpack(pm.raw_pack(pm.divide_by_linear(raw, z, r)[0])) == pm.divide_by_linear(p, z, r)[0]
    assert zko.fr_unpack(pm.raw_pack(pm.divide_by_vanishing(raw, 5, r)[0])) == pm.divide_by_vanishing(p, 5, r)[0]
    assert zko.fr_unpack(pm.raw_pack([pm.horner(raw, z, r)])) == [pm.horner(p, z, r)]
    assert zko.fr_unpack(pm.raw_pack(pm.coset_scale(raw, z, 40, r))) == pm.coset_scale(p, z, 40, r)


@pytest.mark.parametrize("cid", [377, 381])
@pytest.mark.parametrize("lg", [0, 1, 3, 6])
def test_transform_by_definition_equals_the_oracle(zko, cid, lg):
    n, r, rng = 1 << lg, zko.FR[cid], random.Random(lg + cid)
    a = rand_poly(rng, n, r)
    g = C.create_string_buffer(32)
    zko.lib().zko_api_domain_gen(cid, C.c_size_t(n), g)
    w = zko.fr_unpack(g.raw, cid)[0]
    assert pow(w, n, r) == 1 and (n == 1 or pow(w, n // 2, r) == r - 1)
    buf = C.create_string_buffer(zko.fr_pack(a, cid), 32 * n)
    assert zko.lib().zko_api_ntt(cid, buf, C.c_size_t(n), 0) == 0
    want = pm.ntt_by_definition(a, w, r)
    assert zko.fr_unpack(buf.raw, cid) == want
    assert zko.lib().zko_api_ntt(cid, buf, C.c_size_t(n), 1) == 0          # and the oracle's inverse undoes it
    assert zko.fr_unpack(buf.raw, cid) == a
    ninv = pow(n, -1, r)
    assert [v * ninv % r for v in pm.ntt_by_definition(want, pow(w, -1, r), r)] == a


def test_inverses_are_checked_by_multiplying_back(zko):
    r, rng = zko.R377, random.Random(9)
    xs = [rng.randrange(1, r) for _ in range(50)] + [0, 1, r - 1]
    ys = [pow(x, -1, r) if x else 0 for x in xs]
    assert pm.inverse_mismatch(xs, ys, r) is None
    post = rng.randrange(r)
    assert pm.inverse_mismatch(xs, [y * post % r for y in ys], r, post=post) is None
    raw = lambda v: [x * pm.R_MONT % r for x in v]
    assert pm.inverse_mismatch(raw(xs), raw([y * post % r for y in ys]), r, post=post, unit=pm.R_MONT * pm.R_MONT % r) is None
    bad = list(ys)
    bad[7] = (bad[7] + 1) % r
    assert pm.inverse_mismatch(xs, bad, r) == 7
    bad = list(ys)
    bad[50] = 1                                                             # a zero must stay zero
    assert pm.inverse_mismatch(xs, bad, r) == 50
    a, b = C.create_string_buffer(zko.fr_pack([xs[3]])), C.create_string_buffer(32)
    zko.lib().zko_api_fr_inv(377, a, b)
    assert zko.fr_unpack(b.raw) == [ys[3]]


@pytest.mark.parametrize("lg_n", [0, 1, 2, 5, 8])
def test_vanishing_quotient_table_against_the_product_formula(zko, lg_n):
    """(a^n - y^n) / (a - y) on a coset g H: the division-free check the GPU test uses accepts exactly the product formula's values, including the point a == y"""
    n, r, rng = 1 << lg_n, zko.R377, random.Random(lg_n)
    gb = C.create_string_buffer(32)
    zko.lib().zko_api_domain_gen(377, C.c_size_t(n), gb)
    w = zko.fr_unpack(gb.raw)[0]
    for g in (1, rng.randrange(2, r)):
        for a in (rng.randrange(r), g * pow(w, n // 3, r) % r, 0):
            for i in range(n):
                y = g * pow(w, i, r) % r
                v = pm.vq_product(a, y, lg_n, r)
                assert pm.vq_holds(v, a, y, n, r)
                assert pm.vq_holds(v * pm.R_MONT % r, a, y, n, r, unit=pm.R_MONT % r)
                assert not pm.vq_holds((v + 1) % r, a, y, n, r)
                if y != a:
                    assert v == (pow(a, n, r) - pow(y, n, r)) * pow(a - y, -1, r) % r


def test_pointwise_formulas_agree_with_their_derivations(zko):
    r, rng = zko.R377, random.Random(11)
    n = 6
    # q1_combine recovers h_1 and g_1 from the three interpolants of a polynomial given in thirds
    lo, mid, hi, mask = rand_poly(rng, n, r), rand_poly(rng, n, r), rand_poly(rng, n, r), rand_poly(rng, 3 * n, r)
    zeta = rng.randrange(1, r)
    q0 = [(lo[i] + mid[i] + hi[i]) % r for i in range(n)]
    q1 = [(lo[i] + zeta * mid[i] - hi[i]) % r for i in range(n)]
    q3 = [(lo[i] - zeta * mid[i] - hi[i]) % r for i in range(n)]
    h1, g1 = pm.q1_combine(q0, q1, q3, mask, pow(2, -1, r), pow(2 * zeta, -1, r), r)
    total = add_poly(lo + mid + hi, mask, r)
    q, rem = pm.divide_by_vanishing(total, n, r)
    assert h1 == q and g1 == rem[1:]
    # z_poly_from_w is w (X^m - 1) + x
    w, x = rand_poly(rng, 9, r), rand_poly(rng, 4, r)
    want = add_poly(pm.poly_mul(w, [r - 1, 0, 0, 0, 1], r), x, r)
    assert pm.z_poly_from_w(w, x, 12, r) == want and pm.z_poly_from_w(w, x, 15, r) == want + [0, 0, 0]
    assert pm.z_poly_from_w(w[:5], x, 12, r) == add_poly(pm.poly_mul(w[:5], [r - 1, 0, 0, 0, 1], r), x, r) + [0] * 4
    # coset_scale gives the coefficients of p(g X); lincomb is linear
    p, g, pt = rand_poly(rng, 10, r), rng.randrange(r), rng.randrange(r)
    assert pm.horner(pm.coset_scale(p, g, 13, r), pt, r) == pm.horner(p, g * pt % r, r)
    polys, sc = [rand_poly(rng, k, r) for k in (10, 3, 7)], rand_poly(rng, 3, r)
    assert pm.horner(pm.lincomb(polys, sc, 10, r), pt, r) == sum(s * pm.horner(q, pt, r) for q, s in zip(polys, sc)) % r
    # the two round kernels' formulas at one point, spelled out with the oracle's field arithmetic
    L = zko.lib()

    def f_mul(a, b):
        out = C.create_string_buffer(32)
        L.zko_api_fr_mul(377, zko.fr_pack([a]), zko.fr_pack([b]), out)
        return zko.fr_unpack(out.raw)[0]

    v = rand_poly(rng, 11, r)
    A, B, Z = (v[1] + v[5]) % r, (v[2] + v[6]) % r, (v[4] + v[7]) % r
    want = (f_mul(v[0], (f_mul(v[8], A) + f_mul(v[9], B) + f_mul(v[10], f_mul(A, B))) % r) - f_mul(v[3], Z)) % r
    assert pm.q1_coset_pointwise([v[0]], [v[1]], [v[2]], [v[3]], [v[4]], *v[5:11], r) == [want]
    v = rand_poly(rng, 14, r)
    a = (f_mul(v[10], v[2]) + f_mul(v[11], v[3]) + f_mul(v[12], v[4])) % r
    b = (v[9] - f_mul(v[7], v[0]) - f_mul(v[8], v[1]) + v[5]) % r
    assert pm.h2_coset(*[[x] for x in v[:7]], *v[7:14], r) == [f_mul((a - f_mul(b, v[6])) % r, v[13])]
