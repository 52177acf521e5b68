"""The model of tests/keysynth_model.py against things it shares no code with: the CPU oracle's scalar multiplication and fixed-base batch, the oracle's indexer on the xor
and add circuits, and the Niels encoding of tests/arith_model.py.  No GPU.  The oracle helpers at the top are also what tests/test_gpu_keysynth.py takes its references from."""
import ctypes as C
import random

import pytest

import arith_model as am
import keysynth_model as km

CURVES = [377, 381]
SMALL_SRS = (200, 200, 600)


# ---- the oracle as a reference for points: 96-byte affine in and out, infinity as 96 zero bytes
def oracle_generator(zko, cid):
    out = C.create_string_buffer(96)
    zko.lib().zko_api_g1_generator(cid, out)
    return out.raw


def oracle_mul(zko, cid, xy, k):
    """k * P by the oracle (k any integer, reduced modulo r); P must not be infinity: the oracle's loader does not read 96 zero bytes as such"""
    assert xy != bytes(96)
    out = C.create_string_buffer(96)
    inf = zko.lib().zko_api_g1_mul(cid, bytes(xy), zko.fr_pack([k % zko.FR[cid]], cid), out)
    return bytes(96) if inf else out.raw


def oracle_muls(zko, cid, xy, scalars):
    return b"".join(oracle_mul(zko, cid, xy, k) for k in scalars)


def oracle_points(zko, cid, scalars):
    """[k * G] by the oracle's fixed-base batch; zero scalars are answered here (infinity), never passed on"""
    r = zko.FR[cid]
    nz = [k % r for k in scalars if k % r]
    out = C.create_string_buffer(96 * max(len(nz), 1))
    zko.lib().zko_api_fixed_base(cid, zko.fr_pack(nz, cid), C.c_size_t(len(nz)), out)
    it = iter(out.raw[96 * i:96 * i + 96] for i in range(len(nz)))
    return [next(it) if k % r else bytes(96) for k in scalars]


# ---- points
@pytest.mark.parametrize("cid", CURVES)
def test_the_generator_and_the_byte_form(zko, cid):
    assert km.pt_bytes(km.GEN[cid], cid) == oracle_generator(zko, cid)
    assert km.pt_from_bytes(oracle_generator(zko, cid), cid) == km.GEN[cid]
    assert km.pt_bytes(None, cid) == bytes(96) and km.pt_from_bytes(bytes(96), cid) is None


@pytest.mark.parametrize("cid", CURVES)
def test_scalar_multiples_equal_the_oracles(zko, cid):
    r, rnd = km.FR[cid], random.Random(cid)
    scalars = [0, 1, 2, r - 1, r, 1 << 64, 255 << 248 if cid == 381 else 255 << 240] + [rnd.randrange(r) for _ in range(4)]
    g = oracle_generator(zko, cid)
    got = km.scalar_multiples(km.GEN[cid], scalars, cid)
    assert km.pts_bytes(got, cid) == oracle_muls(zko, cid, g, scalars)
    assert got[0] is None and got[4] is None and got[1] == km.GEN[cid]
    assert [km.pt_bytes(p, cid) for p in got] == oracle_points(zko, cid, scalars)
    other = km.mul(0xC0FFEE, km.GEN[cid], cid)                               # a base that is not the generator
    assert km.pts_bytes(km.scalar_multiples(other, scalars[:6], cid), cid) == oracle_muls(zko, cid, km.pt_bytes(other, cid), scalars[:6])


@pytest.mark.parametrize("cid", CURVES)
def test_powers_equal_the_oracles_multiples_by_the_powers(zko, cid):
    r, g = km.FR[cid], oracle_generator(zko, cid)
    for beta, start in ((0, 0), (0, 1), (1, 5), (r - 1, (1 << 32) - 1), (2, (1 << 40) + 5), (random.Random(7).randrange(r), (1 << 32) - 2)):
        want = oracle_muls(zko, cid, g, [pow(beta, start + i, r) for i in range(4)])
        assert km.pts_bytes(km.powers(km.GEN[cid], beta, start, 4, cid), cid) == want
    assert km.powers(km.GEN[cid], 0, 0, 3, cid) == [km.GEN[cid], None, None]             # 0^0 = 1
    assert km.power_scalars(r - 1, (1 << 32) - 1, 3, cid) == [r - 1, 1, r - 1]


# ---- window tables
@pytest.mark.parametrize("cid", CURVES)
@pytest.mark.parametrize("c", [13, 20])
def test_table_copies_equal_the_oracles_multiples_by_two_to_the_offset(zko, cid, c):
    nwin, c_hi, n_hi = km.table_layout(c, cid)
    bits = km.FR[cid].bit_length() + 1
    assert nwin == -(-bits // c) and n_hi * c_hi + (nwin - n_hi) * (c_hi - 1) == bits and 1 <= n_hi <= nwin
    assert [km.table_offset(c, j, cid) for j in range(nwin)] == [sum(km.table_width(c, i, cid) for i in range(j)) for j in range(nwin)]
    pt = km.mul(0xBEEF, km.GEN[cid], cid)
    xy = km.pt_bytes(pt, cid)
    for j in sorted({0, 1, n_hi - 1, n_hi, min(n_hi + 1, nwin - 1), nwin - 1}):
        assert km.pt_bytes(km.table_copy(pt, c, j, cid), cid) == oracle_mul(zko, cid, xy, 1 << km.table_offset(c, j, cid)), (c, j)
    assert km.table_copy(None, c, 3, cid) is None


def test_the_table_layouts_the_gpu_tests_rely_on():
    """c = 13: twenty windows, the first fourteen 13 bits wide, the rest 12; c = 20: thirteen windows, seven of 20 bits and six of 19 (BLS12-377).  The boundary n_hi lies
    strictly inside both, so copies on either side of it exist."""
    assert km.table_layout(13, 377) == (20, 13, 14) and km.table_layout(20, 377) == (13, 20, 7)
    assert km.table_layout(13, 381) == (20, 13, 16) and km.table_layout(20, 381) == (13, 20, 9)


def test_the_order_two_point_doubles_to_infinity():
    x, y = km.ORDER2_377
    assert (y * y - x * x * x - 1) % km.cm.Q377 == 0
    assert km.table_copy(km.ORDER2_377, 13, 1) is None and km.table_copy(km.ORDER2_377, 13, 0) == km.ORDER2_377
    q381 = km.cm.Q381
    assert q381 % 3 == 1 and pow(-4 % q381, (q381 - 1) // 3, q381) != 1, "y^2 = x^3 + 4 over BLS12-381's base field has no point with y = 0: -4 is not a cube there"


# ---- the Edwards form
def test_the_niels_triple_is_the_encoded_edwards_point():
    for k in am.SCALARS + [-3, -0x1234]:
        want = am.niels_enc(am.te_affine(k))
        got = km.niels_triple(am.wpoint(377, k))
        assert [am.G377.unmont(want[14 * i:14 * i + 14]) for i in range(3)] == list(got), k
        assert sum((am.G377.limbs(c * am.G377.r % am.Q) for c in got), []) == want
    assert km.niels_triple(None) == (1, 1, 0)
    assert [am.G377.unmont(am.NIELS_IDENTITY[14 * i:14 * i + 14]) for i in range(3)] == [1, 1, 0]


# ---- the index polynomials
@pytest.mark.parametrize("circuit", ["xor", "add"])
def test_index_values_equal_the_oracles_indexer(zko, circuit):
    cs, _ = zko.synth_ops(circuit, 0, 0, field=377)
    cs.pad_for_marlin()
    mats = [cs.matrix(q) for q in range(3)]
    ix = zko.Index(cs, srs=SMALL_SRS)
    info = ix.info()
    n, k, m = info["h"], info["k"], info["num_instance"]
    assert m & (m - 1) == 0, "the padded instance fills its domain X"
    ci, ri, ca, cb, cc = km.index_inputs(mats, n, m)
    assert len(ci) == info["num_non_zero"] and n >= info["num_constraints"] and k >= len(ci)
    got = km.index_values(ci, ri, ca, cb, cc, k.bit_length() - 1, n.bit_length() - 1)
    for which, name in enumerate(("row", "col", "val_a", "val_b", "val_c", "row_col")):
        assert zko.fr_pack(got[name]) == ix.poly(which, 0), name
    if circuit == "add":
        assert max(abs(v) for v in ca + cb + cc) >= 1 << 31, "the add circuit is here for its wide coefficients"
    assert any(v < 0 for v in ca + cb + cc) and len(ci) < k


def test_index_values_of_a_hand_made_matrix():
    """one entry at row 1, column position 3 of the domain of size 4 with coefficients (5, 0, -1): row = g^3, col = g, u_H(x, x) = 4 x^3"""
    r, g = km.cm.R377, km.r1cs_model.domain_gen(2)
    v = km.index_values([3], [1], [5], [0], [-1], 1, 2)
    u = 4 * pow(g, 9, r) % r
    assert v["row"] == [pow(g, 3, r), 1] and v["col"] == [g, 1] and v["row_col"] == [1, 1]                        # g^4 = 1
    assert v["val_a"] == [5 * pow(u, -1, r) % r, 0] and v["val_b"] == [0, 0] and v["val_c"] == [(r - 1) * pow(u, -1, r) % r, 0]
    assert v["u_inv"] == [pow(u, -1, r), 0]
    # u_H(x, x) = |H| x^(|H| - 1) = |H| / x on H: the kernel's elems[(n - c) mod n] |H|
    assert u == 4 * pow(g, (4 - 3) % 4, r) % r
