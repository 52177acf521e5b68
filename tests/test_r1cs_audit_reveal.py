"""The reveal circuits through the structural audit of tests/r1cs_audit.py, over the shapes of tests/reveal_trace_emu.cpp, smallest first:
  (a) with One and the raw instance known -- the mask and the revealed bytes among it -- the variables that have to be declared free are exactly the family's hidden
      inputs, message bits and key bits, as many as DESIGN.md 2b counts for the key without reveal.  A revealed bit sits on the C side of mask_i * m_ij = r_ij with the
      message bit in a factor next to a known but NON-CONSTANT mask bit: the auditor's single-unknown rule does not run that product backwards (mask_i = 0 leaves m_ij
      free), so revealing adds no way to determine a message bit structurally;
  (b) with One, the hidden inputs and the public INPUTS known -- the mask is one -- every revealed bit and every other public output is determined;
  (c) every raw variable is in a row and no padding variable is.
One-row deletions that must be caught: without the product row of one revealed bit, that bit comes back undetermined; without the zero pin of one mask padding bit, that
bit is in no row but the booleanity row Builder::alloc gave it -- the issue's "in no row" holds up to that row, which every allocated bit has -- so the check here is
"every raw instance variable is in a row that is not its own booleanity row", and it names the bit.
"""
import time

import numpy as np
import pytest

import r1cs_audit as ra
from test_r1cs_audit import Shape, seeds_b


class RevealShape(Shape):
    """a Shape whose key was synthesized with reveal = True: the instance ends in the mask (an input) and the revealed bytes (an output)"""

    def __repr__(self):
        return Shape.__repr__(self) + "-R1"

    def info(self, api):
        return api.circuit_info(self.kind(api), self.length, self.aad, self.key_bits, self.tag_blocks, self.digest, self.prefix, reveal=True)

    def matrices(self, api):
        return [api.circuit_matrix(self.kind(api), self.length, which, self.aad, self.key_bits, self.tag_blocks, self.digest, self.prefix, reveal=True) for which in range(3)]

    def instance_fields(self):
        return Shape.instance_fields(self) + [("mask", 8 * ((self.length + 7) // 8), True), ("revealed", 8 * self.length, False)]


CTR_17 = RevealShape("ctr", 128, 17, 0, 1, "final")
SHAPES = [RevealShape("ctr", 128, 1, 0, 1, "final"), RevealShape("ecb", 128, 16), CTR_17, RevealShape("cbc", 192, 32), RevealShape("gcm", 256, 17, 5), RevealShape("ecb", 256, 64, 0, 2, "chain")]
# the hidden inputs of DESIGN.md 2b's table, unchanged by reveal: 8 (L + key bytes)
FREE_INPUTS = {"ctr128-L1-A0-T1-final-P0-R1": 136, "ecb128-L16-A0-T0-None-P0-R1": 256, "ctr128-L17-A0-T1-final-P0-R1": 264, "cbc192-L32-A0-T0-None-P0-R1": 448, "gcm256-L17-A5-T0-None-P0-R1": 392,
               "ecb256-L64-A0-T2-chain-P0-R1": 768}

_last = {}


def system_of(api, shape):
    if _last.get("at") != repr(shape):
        _last.clear()
        info = shape.info(api)
        _last.update(at=repr(shape), value=(ra.System(shape.matrices(api), int(info["instance"] + info["witness"])), info, shape.columns(info)))
    return _last["value"]


def beyond_booleanity(s, variables):
    """the variables among these that no row holds but their own booleanity row"""
    out = []
    for v in variables:
        rows = set(s.defining_rows(v))
        if s.boolean[v]:
            rows.discard(int(s.boolean_row[v]))
        if not rows:
            out.append(v)
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=repr)
def test_reveal_circuit_is_determined_by_its_statement(api, shape):
    t0 = time.time()
    s, info, cols = system_of(api, shape)
    ri, ni, rw = int(info["raw_instance"]), int(info["instance"]), int(info["raw_witness"])
    # (c) no dangling variable, no padding variable in a row; and no instance variable that only its booleanity row holds
    real = np.zeros(s.n_vars, dtype=bool)
    real[:ri] = True
    real[ni:ni + rw] = True
    missing, stray = ra.dangling(s, real)
    assert len(missing) == 0 and len(stray) == 0, (missing[:8], stray[:8])
    assert beyond_booleanity(s, cols["mask"] + cols["revealed"]) == []
    # (a) exactly the hidden inputs are free, as many as without reveal, and each is boolean
    res = ra.propagate(s, range(ri), greedy=range(ni, ni + rw))
    assert len(res.undetermined) == 0
    assert res.free == cols["hidden"], (len(res.free), len(cols["hidden"]), sorted(set(res.free) ^ set(cols["hidden"]))[:8])
    assert len(cols["hidden"]) == FREE_INPUTS[repr(shape)] == 8 * (shape.length + shape.key_bits // 8)
    assert s.boolean[cols["hidden"]].all() and s.boolean[cols["mask"]].all() and s.boolean[cols["revealed"]].all()
    # (b) outputs -- the revealed bits among them -- and witness are determined by the inputs, public and hidden
    seeds = seeds_b(cols)
    assert set(cols["mask"]) <= set(seeds) and not set(cols["revealed"]) & set(seeds)
    assert len(seeds) + len(cols["outputs"]) == ri + len(cols["hidden"])
    res = ra.propagate(s, seeds)
    assert len(res.undetermined) == 0, (len(res.undetermined), res.undetermined[:8])
    assert res.known[cols["outputs"]].all() and res.known[cols["revealed"]].all() and res.known[ni:ni + rw].all()
    print("%r: %d rows, %d witness variables, %d free inputs, %.1f s" % (shape, s.n_rows, rw, len(cols["hidden"]), time.time() - t0))


def test_reveal_with_one_row_deleted(api):
    s, info, cols = system_of(api, CTR_17)
    # the product row of revealed bit 3 of byte 5: the only row with that bit on its C side
    bit = cols["revealed"][8 * 5 + 3]
    (row,) = s.defining_rows(bit, side=2)
    assert s.count[0][row] == s.count[1][row] == s.count[2][row] == 1
    assert int(s.col[0][s.rowptr[0][row]]) == cols["mask"][5] and int(s.col[1][s.rowptr[1][row]]) == cols["msg"][8 * 5 + 3]
    left = ra.propagate(s.without_rows([row]), seeds_b(cols)).undetermined.tolist()
    assert left == [bit]
    # the zero pin of mask bit 20 (17 bytes: bits 17 .. 23 are padding): its only row beside booleanity
    pad = cols["mask"][20]
    pins = [r for r in s.defining_rows(pad, side=0) if r != int(s.boolean_row[pad])]
    assert len(pins) == 1 and s.constant[1][pins[0]] and s.count[2][pins[0]] == 0 and s.count[0][pins[0]] == 1
    assert beyond_booleanity(s, cols["mask"]) == []
    assert beyond_booleanity(s.without_rows(pins), cols["mask"]) == [pad]
    # a mask bit below the length has its eight product rows and no pin
    live = cols["mask"][16]
    assert len([r for r in s.defining_rows(live, side=0) if r != int(s.boolean_row[live])]) == 8
