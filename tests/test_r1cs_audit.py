"""The constraint systems themselves ("constraint systems"): is every circuit this library compiles DETERMINED by its statement?

The other suites pin that an honest witness satisfies every row and that a flipped instance bit breaks one.  Neither sees an under-constrained circuit -- a carry
without its booleanity row, a q bit no row ties to its column sum, an output a row forgot to bind -- where every honest proof still verifies and a cheating prover
proves a false ciphertext, tag or digest.  tests/r1cs_audit.py decides it structurally from the matrices alone (two rules, argued in its docstring); here it is shown
to refuse each unsound neighbour of its rules on toy systems, to name the affected variables when one row is deleted from a real circuit, and then run over every
circuit family at its smallest shapes:
  (a) with One and the raw instance known, the variables that have to be declared free are exactly the statement's hidden inputs -- message bits, key bits and, for a
      segment, Y_in and the salts -- stated here from the statement's definition (`Shape.witness_fields`), and every one has its booleanity row;
  (b) with One, those hidden inputs and the public INPUTS known (iv / icb, aad, H_in, ctr0, length block), every public OUTPUT (ciphertext, GCM tag, key tag, H_out,
      commitments) and every witness variable is determined: no second instance, not merely no second witness;
  (c) no variable of the raw instance or raw witness is absent from every row, and no padding variable is in one.
The solver mode is pinned against the oracle's whole ECB witness and, for the modes without an oracle, its public outputs against the byte-level models: a witness
reference that shares neither trace_layout.h nor the descriptors with the kernels (tests/test_gpu_witness_replay.py compares the device's z with it).
"""
import time

import numpy as np
import pytest

import gcm_segment_model as seg_model
import r1cs_audit as ra
import sha256_model
from test_gcm_host import model_gcm
from test_keysize_host import ks_cbc, ks_ctr, ks_ecb, ks_gcm

SEGMENT_ROLES = ("head", "mid", "tail")


def bits(data):
    """8 LSB-first bits per byte: the public-input encoding"""
    return [(b >> i) & 1 for b in data for i in range(8)]


def unbits(values):
    return bytes(sum(int(values[8 * i + k]) << k for k in range(8)) for i in range(len(values) // 8))


class Shape:
    """one circuit: mode "ecb" | "cbc" | "ctr" | "gcm" (length = message bytes) or a segment role "head" | "mid" (length = c, the data blocks) | "tail" (length = the
    bytes of the record's last segment); aad bytes, key-tag blocks, digest kind and prefix as the synthesis calls take them"""

    def __init__(self, mode, key_bits=128, length=16, aad=0, tag_blocks=0, digest=None, prefix=0):
        self.mode, self.key_bits, self.length, self.aad, self.tag_blocks, self.digest, self.prefix = mode, key_bits, length, aad, tag_blocks, digest, prefix
        self.segment = mode in SEGMENT_ROLES
        self.message_bytes = 16 * length if mode in ("head", "mid") else length
        self.key_bytes = key_bits // 8

    def __repr__(self):
        return "%s%d-L%d-A%d-T%d-%s-P%d" % (self.mode, self.key_bits, self.length, self.aad, self.tag_blocks, self.digest, self.prefix)

    def kind(self, api):
        return {"ecb": api.CIRCUIT_AES, "cbc": api.CIRCUIT_AES_CBC, "ctr": api.CIRCUIT_AES_CTR, "gcm": api.CIRCUIT_AES_GCM}[self.mode]

    def info(self, api):
        if self.segment:
            return api.circuit_info_gcm_segment(self.mode, self.length, self.aad, self.key_bits)
        return api.circuit_info(self.kind(api), self.length, self.aad, self.key_bits, self.tag_blocks, self.digest, self.prefix)

    def matrices(self, api):
        if self.segment:
            return [api.circuit_matrix_gcm_segment(self.mode, self.length, which, self.aad, self.key_bits) for which in range(3)]
        return [api.circuit_matrix(self.kind(api), self.length, which, self.aad, self.key_bits, self.tag_blocks, self.digest, self.prefix) for which in range(3)]

    # ---- the statement, from its definition (include/zkaes.h): (field, bits, is a public input) in instance order behind One, and the hidden
    # inputs in witness order from witness 0
    def instance_fields(self):
        m = 8 * self.message_bytes
        if self.segment:
            head = [("iv", 96, True), ("ctr0", 32, True)]
            return head + {"head": [("aad", 8 * self.aad, True), ("ct", m, False), ("com_out", 256, False)],
                           "mid": [("ct", m, False), ("com_in", 256, False), ("com_out", 256, False)],
                           "tail": [("ct", m, False), ("len", 128, True), ("tag", 128, False), ("com_in", 256, False)]}[self.mode]
        f = {"ecb": [], "cbc": [("iv", 128, True)], "ctr": [("iv", 128, True)], "gcm": [("iv", 96, True), ("aad", 8 * self.aad, True)]}[self.mode]
        f = f + [("ct", m, False)] + ([("tag", 128, False)] if self.mode == "gcm" else [])
        if self.tag_blocks:
            f.append(("key_tag", 128 * self.tag_blocks, False))
        if self.digest:
            f += [("h_in", 256, True), ("h_out", 256, False)]
        return f

    def witness_fields(self):
        f = [("msg", 8 * self.message_bytes), ("key", 8 * self.key_bytes)]
        if self.segment and self.mode != "head":
            f += [("y_in", 128), ("salt_in", 128)]
        if self.segment and self.mode != "tail":
            f.append(("salt_out", 128))
        return f

    def columns(self, info):
        """{field: the columns of its bits}, "inputs", "outputs" and "hidden" (lists of columns), from the statement and the padded instance size alone"""
        cols, at = {}, 1
        inputs, outputs = [], []
        for name, n, is_input in self.instance_fields():
            cols[name] = list(range(at, at + n))
            (inputs if is_input else outputs).extend(cols[name])
            at += n
        assert at == info["raw_instance"], (at, info["raw_instance"])
        at, hidden = int(info["instance"]), []
        for name, n in self.witness_fields():
            cols[name] = list(range(at, at + n))
            hidden.extend(cols[name])
            at += n
        cols["inputs"], cols["outputs"], cols["hidden"] = inputs, outputs, hidden
        return cols


_last = {}


def system_of(api, shape):
    """(System, info, columns) of a shape; the last one built is kept (a System of a million rows is a few hundred MB with its occurrence lists)"""
    if _last.get("at") != repr(shape):
        _last.clear()
        info = shape.info(api)
        _last.update(at=repr(shape), value=(ra.System(shape.matrices(api), int(info["instance"] + info["witness"])), info, shape.columns(info)))
    return _last["value"]


# ---- the auditor must be able to fail: toy systems.  Variable 0 is One; booleanity(u) = (1 - u) u = 0
def toy(rows, n_vars):
    return ra.System([ra.csr([r[s] for r in rows]) for s in range(3)], n_vars)


def booleanity(u):
    return ({0: 1, u: -1}, {u: 1}, {})


def linear(terms):
    """(terms) * One = 0, the difference in A as enforce_equal and the parity rows have it"""
    return (terms, {0: 1}, {})


def audit(system, known):
    return ra.propagate(system, known).undetermined.tolist()


def test_decomposition_rule_and_its_unsound_neighbours():
    # k = x1 + 2 x2 + 4 x3 with k (variable 1) known: determined.  Variables 2, 3, 4
    good = toy([booleanity(2), booleanity(3), booleanity(4), linear({1: 1, 2: -1, 3: -2, 4: -4})], 5)
    assert good.boolean.tolist() == [False, False, True, True, True] and audit(good, [0, 1]) == []
    # a repeated weight: x1 + x2 = 1 has two solutions
    assert audit(toy([booleanity(2), booleanity(3), booleanity(4), linear({1: 1, 2: -1, 3: -1, 4: -4})], 5), [0, 1]) == [2, 3, 4]
    # one member without a booleanity row: x1 + 2 x2 = 2 has (0, 1) and (2, 0)
    assert audit(toy([booleanity(2), booleanity(4), linear({1: 1, 2: -1, 3: -2, 4: -4})], 5), [0, 1]) == [2, 3, 4]
    # mixed signs: x1 - 2 x2 + 4 x3
    assert audit(toy([booleanity(2), booleanity(3), booleanity(4), linear({1: 1, 2: -1, 3: 2, 4: -4})], 5), [0, 1]) == [2, 3, 4]
    # a weight that is no power of two: 3 x2
    assert audit(toy([booleanity(2), booleanity(3), booleanity(4), linear({1: 1, 2: -1, 3: -3, 4: -4})], 5), [0, 1]) == [2, 3, 4]
    # the members become known one by one: with x3 known the rest is a sound decomposition again, with two known it is R1
    assert audit(toy([booleanity(2), booleanity(4), linear({1: 1, 2: -1, 3: -2, 4: -4})], 5), [0, 1, 3]) == []
    # the same sum on the C side of a product of known factors, and on the B side against a constant A
    assert audit(toy([booleanity(3), booleanity(4), ({1: 1}, {2: 1}, {3: 1, 4: 2})], 5), [0, 1, 2]) == []
    assert audit(toy([booleanity(3), booleanity(4), ({0: 5}, {3: 1, 4: 2}, {1: 1})], 5), [0, 1]) == []


def test_single_unknown_rule_and_its_unsound_neighbours():
    # x (variable 3) times a constant: determined; times a known but non-constant factor: not (b = 0 leaves x free)
    assert audit(toy([({3: 1}, {0: 3}, {2: 1})], 4), [0, 1, 2]) == []
    assert audit(toy([({3: 1}, {1: 1}, {2: 1})], 4), [0, 1, 2]) == [3]
    assert audit(toy([({3: 1}, {0: 1, 1: 1}, {2: 1})], 4), [0, 1, 2]) == [3]        # 1 + b is no constant either
    # on the C side it takes every variable of A and B known
    assert audit(toy([({1: 1}, {2: 1}, {3: 7})], 4), [0, 1, 2]) == []
    assert audit(toy([({1: 1}, {2: 1}, {3: 7})], 4), [0, 1]) == [2, 3]
    # an unknown on the C side AND in a factor (the xor gate read backwards: 2 a b = a + b - r with r and b known) is value dependent
    xor = ({1: 2}, {2: 1}, {1: 1, 2: 1, 3: -1})
    assert audit(toy([xor], 4), [0, 1, 2]) == [] and audit(toy([xor], 4), [0, 2, 3]) == [1]
    # one extra unknown in a row of R1's shape and it determines nothing
    assert audit(toy([({1: 1}, {2: 1}, {3: 7, 4: 1})], 5), [0, 1, 2]) == [3, 4]
    # the linear side must be the only place an unknown sits: C unknown blocks the A side
    assert audit(toy([({3: 1}, {0: 3}, {2: 1})], 4), [0, 1]) == [2, 3]
    # an empty factor is no non-zero constant
    assert audit(toy([({3: 1}, {}, {})], 4), [0]) == [3]


def test_booleanity_detection():
    u = 1
    marks = lambda row: toy([row], 3).boolean[u]
    assert marks(booleanity(u)) and marks(({u: 1}, {0: 1, u: -1}, {})) and marks(({0: -3, u: 3}, {u: 5}, {}))
    assert not marks(({0: 2, u: -1}, {u: 1}, {}))                                 # roots {0, 2}
    assert not marks(({0: 1, u: -1}, {0: 1, u: -1}, {}))                           # a double root at 1
    assert not marks(({u: 1}, {u: 1}, {}))                                         # a double root at 0
    assert not marks(({0: 1, u: -1}, {u: 1}, {2: 1}))                              # C is not empty
    assert not marks(({0: 1, u: -1}, {2: 1}, {}))                                  # another variable's factor
    assert not marks(({0: 1, u: -1, 2: 1}, {u: 1}, {}))                            # not affine in u and One alone
    assert not marks(({0: 1}, {u: 1}, {}))                                         # A does not hold u


def test_a_variable_in_no_row_is_reported():
    s = toy([booleanity(1)], 4)
    real = [True, True, True, False]
    missing, stray = ra.dangling(s, real)
    assert missing.tolist() == [2] and stray.tolist() == []
    missing, stray = ra.dangling(s, [True, False, False, False])
    assert missing.tolist() == [] and stray.tolist() == [1]


def test_canonical_rows_merge_duplicates():
    # x + x - 2 x = 0 x is no occurrence; 1 x + 1 x is 2 x
    mats = [(np.array([0, 3]), np.array([2, 2, 2]), np.array([1, 1, -2])), (np.array([0, 1]), np.array([0]), np.array([1])), (np.array([0, 2]), np.array([1, 1]), np.array([1, 1]))]
    s = ra.System(mats, 3)
    assert s.count[0].tolist() == [0] and s.coeff[2].tolist() == [2] and not s.occurs[2]


def test_solver_on_toy_systems():
    rows = [booleanity(2), booleanity(3), booleanity(4), linear({1: 1, 2: -1, 3: -2, 4: -4}), ({2: 1}, {4: 1}, {5: 3})]
    s = toy(rows, 6)
    z, res = ra.solve(s, {0: 1, 1: 5})
    assert z == [1, 5, 1, 0, 1, pow(3, -1, ra.R)] and sorted(res.used_rows) == [3, 4]
    with pytest.raises(ra.Unsolvable) as e:                                      # 9 is no sum of 1, 2, 4
        ra.solve(s, {0: 1, 1: 9})
    assert e.value.row == 3
    # a row that solves nothing is a check: x2 + x3 = 1 fails for k = 3 and holds for k = 2
    checked = toy(rows + [linear({2: 1, 3: 1, 0: -1})], 6)
    with pytest.raises(ra.Unsolvable) as e:
        ra.solve(checked, {0: 1, 1: 3})
    assert e.value.row == 5
    assert ra.solve(checked, {0: 1, 1: 6})[0][:5] == [1, 6, 0, 1, 1]
    with pytest.raises(ra.Unsolvable) as e:                                      # an undetermined variable is no solution
        ra.solve(s, {0: 1})
    assert e.value.row == -1
    # a negative residue and a division: -x = 1 - 3  ->  x = 2;  (2 x) (4 One) = c
    assert ra.solve(toy([linear({0: -2, 1: 1})], 2), {0: 1})[0] == [1, 2]
    assert ra.solve(toy([({1: 2}, {0: 4}, {2: 1})], 3), {0: 1, 2: 24})[0] == [1, 3, 24]


def test_perturbation_takes_both_arithmetic_paths():
    big = 1 << 60
    rows = [booleanity(1), booleanity(2), ({1: big}, {2: 4}, {3: 4 * big}), ({1: 1}, {2: 1}, {4: 1}), ({5: 1}, {0: -1, 1: 1}, {})]
    s = toy(rows, 6)
    z = [1, 1, 1, 1, 1, 1]
    assert s.unsatisfied(z) == ([], 4, 1)
    assert s.unsatisfied([1, 1, 0, 1, 1, 1]) == ([2, 3], 4, 1)                      # row 2 through Python integers: 0 != 2^62
    reps = {"flip": lambda v: 1 - v, "two": lambda v: np.full_like(v, 2), "minus": lambda v: np.full_like(v, -1)}
    left, paths = ra.unperturbable(s, z, reps)
    assert paths == {"pairs": 13, "int64": 10, "python": 3}                        # the three variables of the big row
    # variable 5 sits only under the factor x1 - 1 = 0: no value of it breaks a row, and the sweep says so; variable 3, in the big row only, is caught through
    # Python integers
    assert {k: v.tolist() for k, v in left.items()} == {"flip": [5], "two": [5], "minus": [5]}


# ---- a real circuit with one row deleted
GCM_17_5 = Shape("gcm", 128, 17, 5)
CTR_17_T1_FINAL = Shape("ctr", 128, 17, 0, 1, "final")


def seeds_b(cols):
    return [0] + cols["inputs"] + cols["hidden"]


def gate_behind(s, public_bit):
    """the witness variable an output bit is set equal to: its equality row is (w - bit) * One = 0, the only row with the bit in A and a constant B"""
    (row,) = [r for r in s.defining_rows(public_bit, side=0) if s.constant[1][r]]
    lo = s.rowptr[0][row]
    assert s.count[0][row] == 2 and s.count[2][row] == 0 and s.col[0][lo] == public_bit
    return int(s.col[0][lo + 1])


def test_gcm_with_one_row_deleted(api):
    s, info, cols = system_of(api, GCM_17_5)
    ni, real_witness = int(info["instance"]), range(int(info["instance"]), int(info["instance"] + info["raw_witness"]))
    # a key bit's booleanity row: the audit of (a) still finds the bit free, and no longer boolean
    key_bit = cols["key"][77]
    cut = s.without_rows([int(s.boolean_row[key_bit])])
    assert s.boolean[key_bit] and not cut.boolean[key_bit] and cut.boolean.sum() == s.boolean.sum() - 1
    free = ra.propagate(cut, range(int(info["raw_instance"])), greedy=real_witness).free
    assert free == cols["hidden"] and [v for v in free if not cut.boolean[v]] == [key_bit]
    # the booleanity row of one GHASH q bit: its parity row (y_k + 2 sum 2^j q_kj = the column sum) no longer decomposes -- y_k, the seven q of that
    # output bit and everything behind them (the later multiplications, the tag) are undetermined; the ciphertext is not touched
    parity = np.unique(s.row[0][s.coeff[0] == -128])
    assert len(parity) == 128 * 4                                                 # one aad block, two data blocks, the length block: four multiplications
    row = int(parity[5])
    lo, hi = s.rowptr[0][row], s.rowptr[0][row + 1]
    members = {int(k): int(v) for v, k in zip(s.col[0][lo:hi], s.coeff[0][lo:hi]) if k < 0}
    assert sorted(members) == [-128, -64, -32, -16, -8, -4, -2, -1]
    cut = s.without_rows([int(s.boolean_row[members[-8]])])
    left = set(ra.propagate(cut, seeds_b(cols)).undetermined.tolist())
    assert set(members.values()) <= left and set(cols["tag"]) <= left and not left & set(cols["ct"]) and not left & set(range(ni, members[-1]))
    # a row of R1's shape with one more unknown: the xor gate behind the first ciphertext bit, with a padding witness added to its C side
    gate_out = gate_behind(s, cols["ct"][0])
    assert gate_out >= ni
    xor_row = s.defining_rows(gate_out, side=2)[0]                                # a + b - out: its own gate is the first row that holds it
    assert s.count[2][xor_row] == 3 and s.coeff[2][s.rowptr[2][xor_row] + 2] == -1 and s.col[2][s.rowptr[2][xor_row] + 2] == gate_out
    spare = ni + int(info["raw_witness"])
    assert spare < s.n_vars and not s.occurs[spare]
    left = ra.propagate(s.with_entry(2, xor_row, spare, 1), seeds_b(cols)).undetermined.tolist()
    assert set(left) >= {cols["ct"][0], gate_out, spare} and not set(left) & set(cols["ct"][8:])


def test_ctr_digest_with_one_row_deleted(api):
    """the lone GCM circuit has constant counters and no SHA-256; the carries are cut out of CTR-128 17 B with a key tag and a final digest"""
    s, info, cols = system_of(api, CTR_17_T1_FINAL)
    ni = int(info["instance"])
    # the incrementer: counter bit i is bit i % 8 of byte 15 - i / 8; c_1 = x_0 folds away and c_2 = x_1 & x_0 is the first and gate
    x0, x1 = cols["iv"][8 * 15], cols["iv"][8 * 15 + 1]
    gate = [r for r in s.defining_rows(x1, side=0) if s.count[0][r] == 1 and s.count[1][r] == 1 and s.col[1][s.rowptr[1][r]] == x0 and s.count[2][r] == 1]
    assert len(gate) == 1
    carry = int(s.col[2][s.rowptr[2][gate[0]]])
    left = set(ra.propagate(s.without_rows(gate), seeds_b(cols)).undetermined.tolist())
    assert carry in left and set(cols["ct"][128:]) <= left and not left & set(cols["ct"][:128]) and min(left - set(cols["outputs"])) == carry
    # a SHA-256 carry (one row per addition, the carries at 2^32 and up): without the booleanity row of one carry bit the addition's 32 result bits and
    # its carries stay open, and H_out behind them
    adds = np.unique(s.row[0][s.coeff[0] == -(1 << 32)])
    assert len(adds) > 64
    row = int(adds[3])
    lo, hi = s.rowptr[0][row], s.rowptr[0][row + 1]
    carry0 = int(s.col[0][lo:hi][s.coeff[0][lo:hi] == -(1 << 32)][0])
    members = list(range(carry0 - 32, carry0 + 1))                                # the 32 result bits are allocated right ahead of the carries
    in_row = {int(v): int(k) for v, k in zip(s.col[0][lo:hi], s.coeff[0][lo:hi])}
    assert [in_row[v] for v in members] == [-(1 << i) for i in range(33)]
    left = set(ra.propagate(s.without_rows([int(s.boolean_row[carry0])]), seeds_b(cols)).undetermined.tolist())
    assert set(members) <= left and min(left - set(cols["outputs"])) == members[0]
    assert set(cols["h_out"]) <= left and not left & set(cols["ct"]) and not left & set(cols["key_tag"])


# ---- every family at its smallest shapes (the shapes of the GPU suites)
SHAPES = [Shape("ecb", 128, 16), Shape("ecb", 192, 16), Shape("ecb", 256, 16), Shape("ecb", 256, 32),
          Shape("cbc", 128, 32), Shape("cbc", 256, 32),
          Shape("ctr", 128, 1), Shape("ctr", 128, 17), Shape("ctr", 128, 48),
          Shape("gcm", 128, 1, 0), GCM_17_5, Shape("gcm", 128, 16, 20), Shape("gcm", 256, 17, 5),
          Shape("ecb", 128, 16, 0, 1), Shape("ecb", 128, 16, 0, 2), Shape("ecb", 256, 16, 0, 1), Shape("ecb", 256, 16, 0, 2), Shape("gcm", 128, 17, 5, 1), Shape("gcm", 128, 17, 5, 2),
          Shape("ecb", 128, 64, 0, 0, "chain"), Shape("cbc", 192, 64, 0, 1, "chain"), CTR_17_T1_FINAL, Shape("ctr", 128, 56, 0, 0, "final"), Shape("gcm", 256, 17, 5, 1, "final", 64),
          Shape("head", 128, 1, 5), Shape("mid", 128, 1), Shape("tail", 128, 5), Shape("tail", 128, 16), Shape("head", 256, 1, 5), Shape("tail", 256, 5)]
# what the statement hides, counted from its definition: 8 (L + key bytes) for the plain modes; a segment adds Y_in and salt_in (mid, tail) and salt_out (head, mid)
FREE_INPUTS = {"ecb128-L16": 256, "gcm128-L17-A5": 264, "ctr128-L17-T1-final": 264, "cbc192-L64-T1-chain": 704, "head128-c1": 384, "mid128-c1": 640, "tail128-L5": 424}


def test_the_free_input_counts_of_the_design():
    count = lambda sh: sum(n for _, n in sh.witness_fields())
    got = {"ecb128-L16": count(SHAPES[0]), "gcm128-L17-A5": count(GCM_17_5), "ctr128-L17-T1-final": count(CTR_17_T1_FINAL), "cbc192-L64-T1-chain": count(SHAPES[20]),
           "head128-c1": count(SHAPES[24]), "mid128-c1": count(SHAPES[25]), "tail128-L5": count(SHAPES[26])}
    assert got == FREE_INPUTS
    for sh in SHAPES:
        if not sh.segment:
            assert count(sh) == 8 * (sh.length + sh.key_bits // 8)


@pytest.mark.parametrize("shape", SHAPES, ids=repr)
def test_circuit_is_determined_by_its_statement(api, shape):
    t0 = time.time()
    s, info, cols = system_of(api, shape)
    ri, ni, rw = int(info["raw_instance"]), int(info["instance"]), int(info["raw_witness"])
    # (c) no dangling variable, no padding variable in a row
    real = np.zeros(s.n_vars, dtype=bool)
    real[:ri] = True
    real[ni:ni + rw] = True
    missing, stray = ra.dangling(s, real)
    assert len(missing) == 0 and len(stray) == 0, (missing[:8], stray[:8])
    # (a) exactly the hidden inputs are free, and each is boolean
    res = ra.propagate(s, range(ri), greedy=range(ni, ni + rw))
    assert len(res.undetermined) == 0
    assert res.free == cols["hidden"], (len(res.free), len(cols["hidden"]), sorted(set(res.free) ^ set(cols["hidden"]))[:8])
    assert s.boolean[cols["hidden"]].all()
    # (b) outputs and witness are determined by the inputs, public and hidden
    seeds = seeds_b(cols)
    assert len(seeds) + len(cols["outputs"]) == ri + len(cols["hidden"])
    res = ra.propagate(s, seeds)
    assert len(res.undetermined) == 0, (len(res.undetermined), res.undetermined[:8])
    assert res.known[cols["outputs"]].all() and res.known[ni:ni + rw].all()
    print("%r: %d rows, %d witness variables, %d free inputs, %.1f s" % (shape, s.n_rows, rw, len(cols["hidden"]), time.time() - t0))


# ---- the solver against the oracle and the byte-level models
def statement(api, shape, seed, zero=False):
    """{field: bytes} of one statement of this shape -- the public inputs and the hidden inputs drawn from `seed` (zero: an all-zero message and key), the public
    outputs from the byte-level models"""
    rs = np.random.RandomState(seed)
    v = {"msg": bytes(shape.message_bytes) if zero else rs.bytes(shape.message_bytes), "key": bytes(shape.key_bytes) if zero else rs.bytes(shape.key_bytes)}
    msg, key = v["msg"], v["key"]
    if shape.segment:
        role = shape.mode
        v["iv"], ctr0 = rs.bytes(12), int(rs.randint(2, 1 << 31))
        v["ctr0"] = ctr0.to_bytes(4, "big")
        v["aad"] = rs.bytes(shape.aad)
        v["y_in"], v["salt_in"], v["salt_out"], v["len"] = rs.bytes(16), rs.bytes(16), rs.bytes(16), seg_model.length_block(5, 16 * (ctr0 - 2) + len(msg))
        tr = seg_model.segment_trace(role, msg, key, v["iv"], ctr0, v["y_in"], v["aad"], v["len"])
        v["ct"] = tr["ct"]
        if role == "tail":
            v["tag"] = tr["tag"]
        else:
            v["com_out"] = seg_model.commitment(key, tr["ys"][-1].to_bytes(16, "big"), v["salt_out"])
        if role != "head":
            v["com_in"] = seg_model.commitment(key, v["y_in"], v["salt_in"])
        return v
    if shape.mode == "ecb":
        v["ct"] = ks_ecb(msg, key)
    elif shape.mode == "cbc":
        v["iv"] = rs.bytes(16)
        v["ct"] = ks_cbc(msg, key, v["iv"])
    elif shape.mode == "ctr":
        v["iv"] = b"\xff" * 15 + b"\xfe" if seed % 2 else rs.bytes(16)            # every other statement wraps the counter at its second increment
        v["ct"] = ks_ctr(msg, key, v["iv"])
    else:
        v["iv"], v["aad"] = rs.bytes(12), rs.bytes(shape.aad)
        v["ct"], v["tag"] = ks_gcm(msg, key, v["iv"], v["aad"])
        if shape.key_bits == 128:
            assert (v["ct"], v["tag"]) == model_gcm(msg, key, v["iv"], v["aad"])
    if shape.tag_blocks:
        v["key_tag"] = api.key_tag(key, shape.tag_blocks)
    if shape.digest:
        h_in = None if zero else rs.bytes(32)
        v["h_in"] = sha256_model.IV if h_in is None else h_in
        v["h_out"] = sha256_model.h_out(shape.digest, msg, h_in, shape.prefix)
    return v


def replay(api, shape, values):
    """z from the matrices, One, the public inputs and the hidden inputs alone; then its public outputs against the models.  Returns (z, System, info, columns)"""
    s, info, cols = system_of(api, shape)
    seeded = {0: 1}
    fields = [f for f, _, is_input in shape.instance_fields() if is_input] + [f for f, _ in shape.witness_fields()]
    for f in fields:
        seeded.update(zip(cols[f], bits(values[f])))
    assert sorted(seeded) == sorted(seeds_b(cols))
    z, _ = ra.solve(s, seeded)
    for f, _, is_input in shape.instance_fields():
        if not is_input:
            assert unbits([z[c] for c in cols[f]]) == values[f], f
    assert set(z) <= {0, 1}
    return z, s, info, cols


def test_solver_reproduces_the_oracles_ecb_witness(api, zko, vectors):
    key, pt = bytes(vectors["key"]), bytes(vectors["plaintext"])
    cs, ct = zko.synth_aes(pt, key)
    cs.pad_for_marlin()
    ins, wit = cs.assignment()
    shape = Shape("ecb", 128, 16)
    z, s, info, cols = replay(api, shape, {"msg": pt, "key": key, "ct": bytes(ct)})
    rw = int(info["instance"] + info["raw_witness"])
    assert z[:rw] == list(ins + wit)[:rw]


@pytest.mark.parametrize("shape", [Shape("gcm", 128, 1, 0), CTR_17_T1_FINAL, Shape("mid", 128, 1), Shape("tail", 128, 5)], ids=repr)
def test_solver_outputs_equal_the_models(api, shape):
    for seed, zero in ((0xA0D1, False), (0xA0D2, True)):
        replay(api, shape, statement(api, shape, seed, zero))
    # and the solver can fail: with the whole instance seeded and one ciphertext bit of it flipped, the bit's equality row hands the wrong value to the gate output
    # behind it, and the gate's own row, which then solves nothing, is violated
    s, info, cols = system_of(api, shape)
    values = statement(api, shape, 0xA0D1)
    seeded = {0: 1}
    for f in [f for f, _, _ in shape.instance_fields()] + [f for f, _ in shape.witness_fields()]:
        seeded.update(zip(cols[f], bits(values[f])))
    seeded[cols["ct"][3]] ^= 1
    with pytest.raises(ra.Unsolvable) as e:
        ra.solve(s, seeded)
    assert e.value.row in s.defining_rows(gate_behind(s, cols["ct"][3]))
