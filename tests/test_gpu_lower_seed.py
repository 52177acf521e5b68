"""GPU tests of the Fq377 product's lower half carry-seeded on a bias of -1 (csrc/ff28.cuh mul_low_zip: pinned, zipped multiply-add chains, an arithmetic shift per
column, the unsigned fallback columns of the two wide products) through the zip probes of csrc/arith_probe.cuh and the te_madd_hot probe, one operation per launch, LIMB
FOR LIMB against the big-integer model of tests/arith_model.py: (T + m p) / R' with m = -T p^-1 mod R' is one determined integer, also for lazy operands.

Operands, per pair of limb bounds (in units of 2^28) that te_madd_hot multiplies -- (5, 1), (2, 1), (1, 1) on the first level; E < 3, H < 2, U < 4, V < 3 on the second:
an all-zero operand on either side (every column t = 0: the seed stays -1), the low limb zero, EVERY limb at its bound (the wide products leave the signed range above
column 8 there: the fallback columns run), limbs from {0, 1, bound - 1}, seeded pseudo-random limbs up to two whole waves and one case more.
te_madd_hot runs in chains of seven on 64 lanes from the identity accumulator (all-zero x and t) and from generic ones, both signs of the current and the next digit."""
import random

import pytest

import arith_model as am
from test_gpu_product_columns import hot_model, signed

pytestmark = pytest.mark.gpu
N = 14
U28 = 1 << 28
R = am.G377


def run(api, name, ins):
    return am.unpack(api.arith_probe(name, am.pack(ins)), api.ARITH_ZIP_OPS[name][2])


def operand_pairs(xa, xb, rnd, n_random):
    za, ba, bb = [0] * N, [xa * U28 - 1] * N, [xb * U28 - 1] * N
    lazy = lambda x: [rnd.randrange(x * U28) for _ in range(N)]
    edge = lambda x: [rnd.choice((0, 1, x * U28 - 1)) for _ in range(N)]
    pairs = [(ba, bb), (za, bb), (ba, za), (za, za), (za, lazy(xb)), (lazy(xa), za)]
    pairs += [([0] + lazy(xa)[1:], lazy(xb)), (lazy(xa), [0] + lazy(xb)[1:]), ([0] + lazy(xa)[1:], [0] + lazy(xb)[1:])]
    pairs += [(edge(xa), edge(xb)) for _ in range(24)]
    return pairs + [(lazy(xa), lazy(xb)) for _ in range(n_random)]


def product(a, b):
    return R.limbs(R.mont(R.val(a) * R.val(b)))


# probe -> per product slot, the operand-bound pairs te_madd_hot puts there (F, G = U, V or V, U by the digit's sign)
ZIPS = {
    "fq377x28.mul_zip_12": [[(3, 4), (3, 3), (4, 3)]],
    "fq377x28.mul_zip_8": [[(4, 2), (3, 2)]],
    "fq377x28.mul_zip_5_2_1": [[(5, 1)], [(2, 1)], [(1, 1)]],
    "fq377x28.mul_zip_12_8_6_12": [[(3, 4), (3, 3)], [(4, 2), (3, 2)], [(3, 2)], [(4, 3), (3, 4)]],
}


@pytest.mark.parametrize("name", sorted(ZIPS))
def test_zipped_products_equal_the_integer_model(api, name):
    rnd = random.Random("lower-seed" + name)
    slots = []
    for bounds in ZIPS[name]:
        col = sum((operand_pairs(xa, xb, rnd, 4) for xa, xb in bounds), [])
        slots.append(col)
    lanes = 2 * 64 + 1                                          # two whole waves and a partly idle third
    for bounds, col in zip(ZIPS[name], slots):
        assert len(col) < lanes
        while len(col) < lanes - 1:
            xa, xb = rnd.choice(bounds)
            col.append(([rnd.randrange(xa * U28) for _ in range(N)], [rnd.randrange(xb * U28) for _ in range(N)]))
        rnd.shuffle(col)                                        # the specials of one slot meet ordinary operands in the others
        xa, xb = bounds[0]
        col.append(([xa * U28 - 1] * N, [xb * U28 - 1] * N))     # ... and the last lane holds every slot's first pair at its bound
    ins = [sum((slots[s][c][0] + slots[s][c][1] for s in range(len(slots))), []) for c in range(lanes)]
    want = [sum((product(*slots[s][c]) for s in range(len(slots))), []) for c in range(lanes)]
    got = run(api, name, ins)
    bad = [c for c in range(lanes) if got[c] != want[c]]
    assert not bad, "%s: %d of %d cases differ; first: lane %d, in %s, got %s, want %s" % (
        name, len(bad), lanes, bad[0], [hex(x) for x in ins[bad[0]]], [hex(x) for x in got[bad[0]]], [hex(x) for x in want[bad[0]]])


def test_zip_probes_reject_nothing_the_table_lists(api):
    assert set(api.ARITH_ZIP_OPS) == set(ZIPS) and not set(api.ARITH_ZIP_OPS) & set(api.ARITH_OPS)
    assert all(nin == 2 * N * len(ZIPS[k]) and nout == N * len(ZIPS[k]) for k, (_, nin, nout) in api.ARITH_ZIP_OPS.items())


def test_hot_addition_chains_from_the_identity_and_from_generic_points(api):
    rnd = random.Random("lower-seed-chains")
    ks = am.SCALARS
    chains = []
    for c in range(64):
        start = 0 if c % 2 == 0 else rnd.choice(ks)             # even lanes start at the identity accumulator: x = t = 0, the t = 0 columns
        recs = [rnd.choice(ks + [0]) for _ in range(8)]
        negs = [rnd.random() < 0.5 for _ in range(8)]
        if c < 8:
            negs[0], negs[1] = bool(c & 2), bool(c & 4)         # both starts x both signs of the current digit x both signs of the next one at step 0
        chains.append((start, recs, negs))
    acc = [am.te_enc(am.te_affine(s), rnd, 1 if s == 0 else None) for s, _, _ in chains]
    acc = [[0] * N + a[N:3 * N] + [0] * N if s == 0 else a for a, (s, _, _) in zip(acc, chains)]      # as te_identity holds it: all-zero limbs, not the representative p
    total = [s for s, _, _ in chains]
    for step in range(7):
        ins, want = [], []
        for c, (_, recs, negs) in enumerate(chains):
            cur = signed(am.niels_enc(am.te_affine(recs[step])), negs[step])
            nxt = am.niels_enc(am.te_affine(recs[step + 1]))
            ins.append(acc[c] + cur + nxt + [int(negs[step]), int(negs[step + 1])])
            want.append(hot_model(acc[c], cur, negs[step]) + signed(nxt, negs[step + 1]))
            total[c] += -recs[step] if negs[step] else recs[step]
        got = am.unpack(api.arith_probe(am.HOT, am.pack(ins)), am.ARITH_OPS[am.HOT][2])
        bad = [c for c in range(64) if got[c] != want[c]]
        assert not bad, "te_madd_hot step %d: lanes %s differ from the integer model; lane %d got %s, want %s" % (
            step, bad, bad[0], [hex(x) for x in got[bad[0]][:56]], [hex(x) for x in want[bad[0]][:56]])
        for c in range(64):
            pt, t_ok = am.te_dec(got[c])
            assert pt == am.te_affine(total[c]) and t_ok, ("te_madd_hot", step, chains[c])
        acc = [g[:56] for g in got]
