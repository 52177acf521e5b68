"""The batch verifier on the GPU: its three kernels against big-integer models, verify_batch(device=True) against the host back end and the per-proof
verifier over valid, damaged and hostile batches, the chunked form, and the variable-base MSM on the base patterns an attacker can choose.

Keys are the smallest the GPU suites use: 16-byte ECB and 16-byte CTR (one tag block), each over an SRS sized from its own circuit, without window tables, made once
per module with their proofs."""
import ctypes as C
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import curve_math as cm  # noqa: E402

pytestmark = pytest.mark.gpu

Q, R = cm.Q377, cm.R377
G = cm.G1_377
OK, INF, OFF_CURVE, OFF_SUBGROUP, MALFORMED = 0, 1, 2, 3, 4
OFF_W_BETA = 131                     # bytes from the end of a serialized proof to its first opening proof


def compress(P, flip=False):
    x, y = P
    gt = (y > Q - y) != flip
    return (x | ((1 << 383) if gt else 0)).to_bytes(48, "little")


def neg(P):
    return (P[0], (Q - P[1]) % Q)


def on_curve_from_x(x):
    y = cm.fp_sqrt((x * x * x + 1) % Q, Q)
    return None if y is None else (x, y)


def bits_of(data):
    return bytes((b >> k) & 1 for b in data for k in range(8))


# ---- kernels ---------------------------------------------------------------------------------------------------------------------------------------------------------
def test_g1_decompress_batch_against_the_integer_model(api, zko):
    rnd = random.Random(0x61DE)
    cases = []                       # (48 bytes, expected status, expected point or None)
    P = None
    for k in range(32):              # 64 subgroup points: multiples of the generator under both sign flags (the flag picks y or -y; both lie in the subgroup)
        P = cm.ec_add(P, cm.ec_mul(rnd.randrange(1, 1 << 64), G, Q), Q)
        big = P if P[1] > Q - P[1] else neg(P)
        cases.append((compress(big), OK, big))
        cases.append((compress(big, flip=True), OK, neg(big)))
    cases.append(((1 << 382).to_bytes(48, "little"), INF, None))
    found = 0
    x = rnd.randrange(Q)
    while found < 16:                # x^3 + 1 a non-residue
        x += 1
        if on_curve_from_x(x) is None:
            cases.append((x.to_bytes(48, "little"), OFF_CURVE, None))
            found += 1
    outside = [(0, 1)]               # order 3
    assert cm.ec_mul(3, (0, 1), Q) is None and cm.ec_mul(R, (0, 1), Q) is not None
    x = rnd.randrange(Q)
    while len(outside) < 16:         # on the curve, outside the prime-order subgroup
        x += 1
        pt = on_curve_from_x(x)
        if pt is not None and cm.ec_mul(R, pt, Q) is not None:
            outside.append(pt)
    for pt in outside:
        cases.append((compress(pt), OFF_SUBGROUP, None))
    for _ in range(8):               # random points of the curve: whatever the model says
        pt = None
        while pt is None:
            pt = on_curve_from_x(rnd.randrange(Q))
        cases.append((compress(pt), OK if cm.ec_mul(R, pt, Q) is None else OFF_SUBGROUP, pt))
    cases.append(((Q + 5).to_bytes(48, "little"), MALFORMED, None))                               # x >= q
    cases.append((((1 << 383) | (1 << 382)).to_bytes(48, "little"), MALFORMED, None))             # both flags
    cases.append((((1 << 382) | 7).to_bytes(48, "little"), MALFORMED, None))                      # infinity over a non-zero x
    rnd.shuffle(cases)               # lanes of one wave meet every kind
    xy, status = api.g1_decompress_batch(b"".join(c[0] for c in cases))
    assert status == [c[1] for c in cases]
    got = zko.pt_unpack(xy)
    for i, (_, st, pt) in enumerate(cases):
        assert got[i] == (pt if st == OK else (0, 0)), "point %d" % i


def test_fq_sqrt_batch_every_loop_count(api, zko):
    rnd = random.Random(0x5A27)
    s, t = 46, (Q - 1) >> 46
    assert t & 1 and (Q - 1) == t << s
    z = 2
    while pow(z, (Q - 1) // 2, Q) != Q - 1:
        z += 1
    zeta = pow(z, t, Q)              # a generator of the 2^46-th roots of unity
    vals, want = [0, 1], [1, 1]
    for k in range(46):              # a square whose 2-power component has order 2^k: that many rounds of the Tonelli-Shanks loop pattern
        a = pow(zeta, 1 << (s - k), Q) * pow(rnd.randrange(2, Q), 1 << s, Q) % Q
        e, o = pow(a, t, Q), 0
        while e != 1:
            e, o = e * e % Q, o + 1
        assert o == k
        vals.append(a)
        want.append(1)
    while len(vals) < 48 + 32:       # 32 non-residues
        a = rnd.randrange(2, Q)
        if pow(a, (Q - 1) // 2, Q) == Q - 1:
            vals.append(a)
            want.append(0)
    order = list(range(len(vals)))
    rnd.shuffle(order)
    packed = b"".join(zko.fq_to_mont(vals[i]).to_bytes(48, "little") for i in order)
    out, sq = api.fq_sqrt_batch(packed)
    assert sq == [want[i] for i in order]
    for j, i in enumerate(order):
        root = zko.fq_from_mont(int.from_bytes(out[48 * j:48 * j + 48], "little"))
        assert (root * root % Q == vals[i]) if want[i] else root == 0


def model_xhat(m, g, beta, row):
    xs = [1] + list(row) + [0] * (m - 1 - len(row))
    e = 1
    for j in range(m):
        if e == beta:
            return xs[j]
        e = e * g % R
    vx, acc, e = (pow(beta, m, R) - 1) % R, 0, 1
    for j in range(m):
        if xs[j]:
            acc = (acc + e * pow(beta - e, -1, R)) % R
        e = e * g % R
    return acc * vx % R * pow(m, -1, R) % R


@pytest.mark.parametrize("lg_m,n_bits", [(0, 0), (1, 1), (8, 255), (10, 1000), (10, 1023)])
def test_public_input_eval_against_the_integer_model(api, zko, lg_m, n_bits):
    rnd = random.Random(0xE7A1 + lg_m)
    m = 1 << lg_m
    gb = C.create_string_buffer(32)
    zko.lib().zko_api_domain_gen(377, C.c_size_t(m), gb)
    g = zko.fr_unpack(gb.raw)[0] if m > 1 else 1
    assert pow(g, m, R) == 1 and (m == 1 or pow(g, m // 2, R) != 1)
    rows = [bytes(n_bits), bytes([1] * n_bits), bytes(rnd.randrange(2) for _ in range(n_bits))]
    in_x = pow(g, 3, R)              # beta in X: the indicator branch
    for rot in range(3):             # every kind of row meets the indicator once
        betas = [rnd.randrange(R), rnd.randrange(R), rnd.randrange(R)]
        betas[rot] = in_x
        got = zko.fr_unpack(api.public_input_eval(lg_m, zko.fr_pack(betas), rows))
        assert got == [model_xhat(m, g, betas[i], rows[i]) for i in range(3)]


# ---- proofs ----------------------------------------------------------------------------------------------------------------------------------------------------------
N = 33


def _small_key(api, circuit, key_tag_blocks=0):
    ci = api.circuit_info(circuit, 16, key_tag_blocks=key_tag_blocks)
    srs = (int(ci["constraints"]), int(ci["instance"]), int(ci["nnz_a"] + ci["nnz_b"] + ci["nnz_c"]))
    return api.synthesize_keys(16, circuit=circuit, srs=srs, flags=api.KEY_NO_TABLES, key_tag_blocks=key_tag_blocks)


@pytest.fixture(scope="module")
def ecb(api):
    """33 valid 16-byte ECB proofs under one key with their public-input rows and the per-proof verifier's answers; made once, never modified"""
    from conftest import mt_bytes
    pk, vk = _small_key(api, api.CIRCUIT_AES)
    try:
        msgs = [mt_bytes(16, 100 + i) for i in range(N)]
        keys = [mt_bytes(16, 200 + i) for i in range(N)]
        proofs = pk.encrypt_batch(msgs, keys, zk_seed=bytes(range(32)))
        rows = [bits_of(api.ecb_ciphertext(m, k)) for m, k in zip(msgs, keys)]
    finally:
        pk.free()
    assert [vk.verify(p, r) for p, r in zip(proofs, rows)] == [True] * N
    return vk, proofs, rows


@pytest.fixture(scope="module")
def ctr(api):
    """a 5-chunk CTR job of 16-byte chunks under a key with one tag block"""
    from conftest import mt_bytes
    pk, vk = _small_key(api, api.CIRCUIT_AES_CTR, key_tag_blocks=1)
    try:
        msg, key, icb = mt_bytes(80, 300), mt_bytes(16, 301), mt_bytes(16, 302)
        ct, proofs = pk.encrypt_ctr_chunked(msg, key, icb, zk_seed=bytes(range(1, 33)))
    finally:
        pk.free()
    return vk, proofs, ct, icb, api.key_tag(key, 1)


def per_proof(api, vk, proof, row):
    try:
        return vk.verify(proof, row)
    except api.ZkAesError:
        return False


def agree(api, vk, proofs, rows, want):
    """device == host back end == the per-proof verifier == want"""
    assert [per_proof(api, vk, p, r) for p, r in zip(proofs, rows)] == want
    assert api.verify_batch(vk, proofs, rows, device=False) == want
    assert api.verify_batch(vk, proofs, rows, device=True) == want


@pytest.mark.parametrize("n", [1, 2, 5, 33])
def test_valid_batches(api, ecb, n):
    vk, proofs, rows = ecb
    agree(api, vk, proofs[:n], rows[:n], [True] * n)
    if n == 33:
        assert api.verify_batch_timings()["sub_batches"] == 1


def flipped(row, bit=5):
    return row[:bit] + bytes([row[bit] ^ 1]) + row[bit + 1:]


@pytest.mark.parametrize("pos", [0, 16, 32])
def test_one_wrong_ciphertext_of_33(api, ecb, pos):
    vk, proofs, rows = ecb
    bad = list(rows)
    bad[pos] = flipped(rows[pos])
    agree(api, vk, proofs, bad, [i != pos for i in range(N)])
    assert api.verify_batch_timings()["sub_batches"] <= 1 + 2 * 6      # the bisection bound: 2 ceil(log2 33) further sub-batches


def test_swapped_repeated_and_all_bad(api, ecb):
    vk, proofs, rows = ecb
    agree(api, vk, proofs[:5], [rows[1], rows[0]] + rows[2:5], [False, False, True, True, True])       # two proofs with their public inputs swapped
    agree(api, vk, [proofs[3]] * 4, [rows[3]] * 4, [True] * 4)                                          # the same proof four times: every base four times
    agree(api, vk, proofs[:5], [flipped(r, 100) for r in rows[:5]], [False] * 5)


def with_first_point(proof, b48):
    return proof[:16] + b48 + proof[64:]        # u64 rounds, u64 round length, then the first commitment


def test_points_off_the_curve_and_outside_the_subgroup(api, ecb):
    vk, proofs, rows = ecb
    x = int.from_bytes(proofs[2][16:64], "little") & ((1 << 382) - 1)
    while on_curve_from_x(x) is not None:
        x += 1
    off_curve = with_first_point(proofs[2], x.to_bytes(48, "little"))
    agree(api, vk, proofs[:2] + [off_curve] + proofs[3:5], rows[:5], [True, True, False, True, True])
    x = 2
    while True:
        pt = on_curve_from_x(x)
        if pt is not None and cm.ec_mul(R, pt, Q) is not None:
            break
        x += 1
    outside = with_first_point(proofs[4], compress(pt))
    agree(api, vk, proofs[:4] + [outside], rows[:5], [True, True, True, True, False])
    order3 = proofs[0][:len(proofs[0]) - OFF_W_BETA] + compress((0, 1)) + proofs[0][len(proofs[0]) - OFF_W_BETA + 48:]      # an opening proof of order 3
    agree(api, vk, [order3] + proofs[1:5], rows[:5], [False, True, True, True, True])


def test_truncated_proof_is_a_rejection(api, ecb):
    vk, proofs, rows = ecb
    agree(api, vk, [proofs[0], proofs[1][:-1], proofs[2]], rows[:3], [True, False, True])
    agree(api, vk, [b""], rows[:1], [False])


def test_ctr_proofs_under_the_ecb_key(api, ecb, ctr):
    vk, _, rows = ecb
    _, ctr_proofs, _, _, _ = ctr
    agree(api, vk, ctr_proofs[:3], rows[:3], [False] * 3)


def test_verify_chunked_batch(api, ctr):
    vk, proofs, ct, icb, tag = ctr
    serial = api.verify_chunked_tagged(vk, api.CIRCUIT_AES_CTR, proofs, ct, tag, iv=icb)
    assert serial == [True] * 5
    for device in (False, True):
        assert api.verify_chunked_batch(vk, api.CIRCUIT_AES_CTR, proofs, ct, header=icb, key_tag=tag, device=device) == serial
    bad = bytearray(ct)
    bad[3 * 16 + 7] ^= 0x10
    bad = bytes(bad)
    want = [True, True, True, False, True]
    assert api.verify_chunked_tagged(vk, api.CIRCUIT_AES_CTR, proofs, bad, tag, iv=icb) == want
    for device in (False, True):
        assert api.verify_chunked_batch(vk, api.CIRCUIT_AES_CTR, proofs, bad, header=icb, key_tag=tag, device=device) == want


# ---- the MSM under bases an attacker chooses ---------------------------------------------------------------------------------------------------------------------------
def test_msm_repeated_negated_and_infinity_bases(api, zko):
    """zkaes_msm -- the Weierstrass accumulation the batch path runs on -- over 40 bases holding one point eight times, a point and its negation under equal scalars,
    and two infinity bases, against the oracle's sum of the collapsed coefficients"""
    rnd = random.Random(0x3D5E)
    pts = [cm.ec_mul(rnd.randrange(1, R), G, Q) for _ in range(12)]
    ids = list(range(12)) * 3 + [0, 0, 0, 0]              # 40 bases
    for at in (3, 9, 17, 21, 30, 33, 38, 39):
        ids[at] = 5                                       # point 5 eight times (with its three regular slots: more)
    bases = [pts[i] for i in ids]
    sign = [1] * 40
    scalars = [rnd.randrange(R) for _ in range(40)]
    same = scalars[3]
    for at in (3, 9, 17, 21):
        scalars[at] = same                                # ... four of them under the SAME scalar: every window adds P to a bucket that holds P
    bases[10], sign[10] = neg(pts[7]), -1                 # P and -P under equal scalars: every window meets P + (-P) in one bucket
    ids[10] = 7
    scalars[10] = scalars[7] if ids[7] == 7 else scalars[10]
    assert ids[7] == 7 and scalars[10] == scalars[7]
    inf_at = (0, 25)
    packed = bytearray(zko.pt_pack(bases))
    for at in inf_at:
        packed[96 * at:96 * at + 96] = bytes(96)          # (0, 0): the library's affine infinity
    coeff = {}
    for i in range(40):
        if i not in inf_at:
            coeff[ids[i]] = (coeff.get(ids[i], 0) + sign[i] * scalars[i]) % R
    items = sorted((p, c) for p, c in coeff.items() if c)
    want = C.create_string_buffer(96)
    want_inf = zko.lib().zko_api_msm(377, zko.pt_pack([pts[p] for p, _ in items]), zko.fr_pack([c for _, c in items]), C.c_size_t(len(items)), want)
    xy, inf = api.msm(377, bytes(packed), zko.fr_pack(scalars))
    assert bool(inf) == bool(want_inf) and (inf or xy == want.raw)
    # everything cancels: the sum is the point at infinity
    xy, inf = api.msm(377, zko.pt_pack([pts[1], neg(pts[1]), pts[2], neg(pts[2])]), zko.fr_pack([same, same, 77, 77]))
    assert inf
