"""GPU tests of the Fp28 product's carry-seeded upper columns (csrc/ff28.cuh: pinned multiply-add chains on the device; te28.cuh te_madd_hot: the chains of three and of
four products zipped) through the existing probes of csrc/arith_probe.cuh, one operation per launch, LIMB FOR LIMB against big-integer arithmetic: a Montgomery product of
integers is one determined integer, (T + m p) / R' with m = -T p^-1 mod R', also for lazy operands.

Operands: 0, 1, p - 1, p, 2 p re-limbed and all limbs 2^28 - 1, every pair of them; the lazy extremes of te_madd_hot with EVERY limb at its bound (in units of 2^28:
E < 3, H < 2, U < 4, V < 3 -- the six products the addition takes, E U and U V the widest), the bound in one limb position at a time; the same for fma2 and sqr
(normalized limbs, all ones); seeded pseudo-random pairs that fill the launch up to whole waves and one case more (two waves and a partly idle third).
te_madd_hot runs in chains of seven on 64 lanes: both signs of the current and of the next digit, the identity record (1, 1, 0) among the records, a lane that adds a
point to itself, accumulators that start at the identity."""
import random

import pytest

import arith_model as am

pytestmark = pytest.mark.gpu
N = 14
U28 = 1 << 28
MASK = U28 - 1


def run(api, name, ins):
    return am.unpack(api.arith_probe(name, am.pack(ins)), am.ARITH_OPS[name][2])


def fill(ins, make, waves=2):
    """pad the case list with make() up to `waves` whole waves of 64 lanes and one case more"""
    want = max(waves, -(-len(ins) // 64)) * 64 + 1
    return ins + [make() for _ in range(want - len(ins))]


def flat(limb, top=None):
    return [limb] * (N - 1) + [limb if top is None else top]


def operands(f):
    R = am.X28[f]
    p, L = R.p, R.limbs
    sp = [L(0), L(1), L(p - 1), L(p), L(2 * p), flat(MASK)]
    E, H, U, V = flat(3 * U28 - 1), flat(2 * U28 - 1), flat(4 * U28 - 1), flat(3 * U28 - 1)
    hot = [(E, U), (U, V), (E, V), (V, H), (U, H), (E, H)]
    hot += [(b, a) for a, b in hot]
    for i in range(N):                                          # the bound in one limb position of each operand
        e, u = flat(MASK, 0), flat(MASK, 0)
        e[i], u[N - 1 - i] = 3 * U28 - 1, 4 * U28 - 1
        hot += [(e, u), (u, e)]
    return R, sp, hot


def rand_norm(R, rnd, kp):
    return R.limbs(rnd.randrange(kp * R.p))


def product(R, t):
    return R.limbs(R.mont(t))


@pytest.mark.parametrize("f", ["fq377x28", "fq381x28"])
def test_products_equal_the_integer_model(api, f):
    R, sp, hot = operands(f)
    rnd = random.Random("columns" + f)
    kp = 64 if f == "fq377x28" else 22                          # the product's contract (ff28.cuh): below 64 p; a b < 500 p^2
    pairs = [(a, b) for a in sp for b in sp] + hot
    pairs = fill(pairs, lambda: (rand_norm(R, rnd, kp), rand_norm(R, rnd, kp)))
    ins = [a + b for a, b in pairs]
    want = [product(R, R.val(a) * R.val(b)) for a, b in pairs]
    names = ["mul"] + (["mul_biased"] if f == "fq377x28" else [])          # mul_biased: the opaque SGPR bias of the hot loop
    for op in names:
        got = run(api, "%s.%s" % (f, op), ins)
        bad = [i for i in range(len(ins)) if got[i] != want[i]]
        assert not bad, "%s.%s: %d of %d cases differ; first: a = %s, b = %s, got %s, want %s" % (
            f, op, len(bad), len(ins), *([hex(x) for x in v] for v in (pairs[bad[0]][0], pairs[bad[0]][1], got[bad[0]], want[bad[0]])))
    # sqr: normalized limbs, all ones; a top limb with excess; the specials; random values
    sq = sp + [flat(MASK, (1 << 24) - 1)]
    sq = fill(sq, lambda: rand_norm(R, rnd, kp))
    assert run(api, f + ".sqr", sq) == [product(R, R.val(a) ** 2) for a in sq]
    # fma2: a b + c d in one reduction; every operand all ones; the specials against all ones; random values below 5 p (a b + c d < 64 p^2)
    ones = flat(MASK)
    quads = [(ones, ones, ones, ones)] + [(a, b, b, a) for a in sp for b in sp] + [(ones, a, a, ones) for a in sp] + [(a, ones, ones, ones) for a in sp]
    quads = fill(quads, lambda: tuple(rand_norm(R, rnd, 5) for _ in range(4)))
    assert run(api, f + ".fma2", [a + b + c + d for a, b, c, d in quads]) == [product(R, R.val(a) * R.val(b) + R.val(c) * R.val(d)) for a, b, c, d in quads]


# ---- te_madd_hot, modelled on integers: every lazy limb operation keeps the VALUE it documents (sub_lazy<K>: a - b + K p, add_lazy: a + b, dbl_lazy: 2 a) and every
# product is the determined integer above, so the four output coordinates are determined limb for limb
def hot_model(acc, rec, neg):
    R = am.G377
    p = R.p
    M = lambda t: R.mont(t)
    X, Y, Z, T = (R.val(acc[N * i:N * i + N]) for i in range(4))
    ymx, ypx, td = (R.val(rec[N * i:N * i + N]) for i in range(3))
    A, B, C = M((Y - X + 3 * p) * ymx), M((Y + X) * ypx), M(T * td)
    E, H, D = B + 2 * p - A, B + A, 2 * Z
    U, V = D + 2 * p - C, D + C
    F, G = (V, U) if neg else (U, V)
    return sum((R.limbs(M(t)) for t in (E * F, G * H, F * G, E * H)), [])          # x, y, z, t: the order of AccTE


def signed(rec, neg):
    return rec[N:2 * N] + rec[:N] + rec[2 * N:] if neg else rec                     # as niels_load_signed leaves it


def hot_chains():
    """64 lanes: (start, eight records as multiples of G -- 0 is the identity record (1, 1, 0) --, eight signs)"""
    rnd = random.Random("hotcolumns")
    ks = am.SCALARS
    chains = []
    for c in range(64):
        recs = [rnd.choice(ks + [0]) for _ in range(8)]
        negs = [rnd.random() < 0.5 for _ in range(8)]
        start = rnd.choice(ks) if c % 3 else 0
        if c < 4:
            negs[0], negs[1] = bool(c & 1), bool(c & 2)          # both signs of the current digit x both signs of the next one at step 0
        if c == 4:
            start, recs, negs = ks[2], [ks[2]] * 8, [False] * 8   # a point added to itself: P + P, then 3 P, 4 P, ...
        if c == 5:
            start, recs, negs = 0, [0] * 8, [False, True] * 4     # the identity plus the identity record, both signs
        if c == 6:
            recs[0], recs[3], negs[3] = 0, 0, True                # the identity record first and in mid-chain
        if c == 7:
            start, recs, negs = ks[4], [ks[4]] * 8, [True, False] * 4     # P - P = the identity, then P again
        chains.append((start, recs, negs))
    return chains


def test_hot_addition_chains_limb_for_limb(api):
    chains = hot_chains()
    assert any(0 in r for _, r, _ in chains) and {(n[0], n[1]) for _, _, n in chains} == {(a, b) for a in (False, True) for b in (False, True)}
    rnd = random.Random("hotcolumns-z")
    acc = [am.te_enc(am.te_affine(s), rnd, 1 if s == 0 else None) for s, _, _ in chains]
    total = [s for s, _, _ in chains]
    for step in range(7):
        ins, want = [], []
        for c, (_, recs, negs) in enumerate(chains):
            cur = signed(am.niels_enc(am.te_affine(recs[step])), negs[step])
            nxt = am.niels_enc(am.te_affine(recs[step + 1]))
            ins.append(acc[c] + cur + nxt + [int(negs[step]), int(negs[step + 1])])
            want.append(hot_model(acc[c], cur, negs[step]) + signed(nxt, negs[step + 1]))
            total[c] += -recs[step] if negs[step] else recs[step]
        got = run(api, am.HOT, ins)
        bad = [c for c in range(64) if got[c] != want[c]]
        assert not bad, "te_madd_hot step %d: lanes %s differ from the integer model; lane %d got %s, want %s" % (
            step, bad, bad[0], [hex(x) for x in got[bad[0]][:56]], [hex(x) for x in want[bad[0]][:56]])
        for c in range(64):                                       # ... and the model's integers are the right POINT (tools/curve_math.py)
            pt, t_ok = am.te_dec(got[c])
            assert pt == am.te_affine(total[c]) and t_ok, ("te_madd_hot", step, chains[c])
        acc = [g[:56] for g in got]
