"""The GCM segment circuits with reveal = 1 through the structural audit of tests/r1cs_audit.py: head, mid and tail at c = 1 (the tail at Lt = 7, so that
its mask has a padding bit).
  (a) with One and the raw instance known -- the mask slice and the revealed slice among it -- the variables that have to be declared free are exactly the segment's
      hidden inputs: key, message, Y_in and salt_in (mid, tail), salt_out (head, mid), as many as DESIGN.md 9g counts for the key without reveal.  Revealing adds no way to
      determine a message bit structurally (tests/test_r1cs_audit_reveal.py says why);
  (b) with One, the hidden inputs and the public INPUTS known -- the mask is one -- every revealed bit and every other public output is determined;
  (c) every raw variable is in a row, no padding variable is, and no mask or revealed bit is held by its booleanity row alone.
Deleting the product row of one revealed bit leaves exactly that bit undetermined.
"""
import time

import numpy as np
import pytest

import r1cs_audit as ra
from test_r1cs_audit import Shape, seeds_b
from test_r1cs_audit_reveal import beyond_booleanity


class SegmentRevealShape(Shape):
    """a segment Shape whose key was synthesized with reveal = True: the instance ends in the segment's mask slice (an input) and its revealed slice (an output)"""

    def __repr__(self):
        return Shape.__repr__(self) + "-R1"

    def info(self, api):
        return api.circuit_info_gcm_segment(self.mode, self.length, self.aad, self.key_bits, reveal=True)

    def matrices(self, api):
        return [api.circuit_matrix_gcm_segment(self.mode, self.length, which, self.aad, self.key_bits, reveal=True) for which in range(3)]

    def instance_fields(self):
        return Shape.instance_fields(self) + [("mask", 8 * ((self.message_bytes + 7) // 8), True), ("revealed", 8 * self.message_bytes, False)]


HEAD, MID, TAIL = SegmentRevealShape("head", 128, 1, 13), SegmentRevealShape("mid", 128, 1), SegmentRevealShape("tail", 128, 7)
# key, message, then Y_in and salt_in (mid, tail), salt_out (head, mid): the hidden inputs of DESIGN.md 9g, unchanged by reveal
FREE_INPUTS = {repr(HEAD): 128 + 128 + 128, repr(MID): 128 + 128 + 256 + 128, repr(TAIL): 128 + 56 + 256}

_last = {}


def system_of(api, shape):
    if _last.get("at") != repr(shape):
        _last.clear()
        info = shape.info(api)
        _last.update(at=repr(shape), value=(ra.System(shape.matrices(api), int(info["instance"] + info["witness"])), info, shape.columns(info)))
    return _last["value"]


@pytest.mark.parametrize("shape", [HEAD, MID, TAIL], ids=repr)
def test_reveal_segment_is_determined_by_its_statement(api, shape):
    t0 = time.time()
    s, info, cols = system_of(api, shape)
    ri, ni, rw = int(info["raw_instance"]), int(info["instance"]), int(info["raw_witness"])
    # (c)
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
    hidden_names = ["msg", "key"] + (["y_in", "salt_in"] if shape.mode != "head" else []) + (["salt_out"] if shape.mode != "tail" else [])
    assert cols["hidden"] == [v for name in hidden_names for v in cols[name]]
    assert len(cols["hidden"]) == FREE_INPUTS[repr(shape)]
    assert s.boolean[cols["hidden"]].all() and s.boolean[cols["mask"]].all() and s.boolean[cols["revealed"]].all()
    # (b) outputs -- the revealed bits among them -- and witness are determined by the inputs, public and hidden
    seeds = seeds_b(cols)
    assert set(cols["mask"]) <= set(seeds) and not set(cols["revealed"]) & set(seeds)
    assert len(seeds) + len(cols["outputs"]) == ri + len(cols["hidden"])
    res = ra.propagate(s, seeds)
    assert len(res.undetermined) == 0, (len(res.undetermined), res.undetermined[:8])
    assert res.known[cols["outputs"]].all() and res.known[cols["revealed"]].all() and res.known[ni:ni + rw].all()
    # one product row deleted: exactly that revealed bit comes back undetermined
    byte, k = shape.message_bytes - 2, 3
    bit = cols["revealed"][8 * byte + k]
    (row,) = s.defining_rows(bit, side=2)
    assert s.count[0][row] == s.count[1][row] == s.count[2][row] == 1
    assert int(s.col[0][s.rowptr[0][row]]) == cols["mask"][byte] and int(s.col[1][s.rowptr[1][row]]) == cols["msg"][8 * byte + k]
    assert ra.propagate(s.without_rows([row]), seeds).undetermined.tolist() == [bit]
    print("%r: %d rows, %d witness variables, %d free inputs, %.1f s" % (shape, s.n_rows, rw, len(cols["hidden"]), time.time() - t0))


def test_tail_mask_padding_bit_is_pinned(api):
    """Lt = 7: mask bit 7 is at the length; its one row beside booleanity is the zero pin, and without it nothing but booleanity holds the bit"""
    s, info, cols = system_of(api, TAIL)
    pad = cols["mask"][7]
    pins = [r for r in s.defining_rows(pad, side=0) if r != int(s.boolean_row[pad])]
    assert len(pins) == 1 and s.constant[1][pins[0]] and s.count[2][pins[0]] == 0 and s.count[0][pins[0]] == 1
    assert beyond_booleanity(s.without_rows(pins), cols["mask"]) == [pad]
    live = cols["mask"][6]
    assert len([r for r in s.defining_rows(live, side=0) if r != int(s.boolean_row[live])]) == 8
