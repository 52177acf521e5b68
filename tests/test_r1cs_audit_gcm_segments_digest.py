"""The segment circuits of a DIGEST record through the structural audit of tests/r1cs_audit.py: head (c = 4, A = 13), mid (c = 4), last (Lr = 17: one
compression, a ragged final block; Lr = 56: two compressions) and the closing tail.
  (a) with One and the raw instance known -- the states, commitments and the tag among it -- the variables that have to be declared free are exactly the hidden inputs:
      message, key, Y_in and the salts.  The digest adds no free variable: its inputs are the message witnesses the cipher already has;
  (b) with One, the hidden inputs and the public INPUTS known -- iv, ctr0, aad, the length block, H_in, total_bits -- every public output is determined: the ciphertext,
      every commitment, the tag and H_out, and so is every witness;
  (c) every raw variable is in a row and no padding variable is.
H_in and H_out sit behind the role's inputs of 9g and a last's total_bits behind them, where DESIGN.md 9m puts them.
"""
import time

import numpy as np
import pytest

import r1cs_audit as ra
from test_r1cs_audit import Shape, seeds_b


class DigestSegmentShape(Shape):
    """a segment Shape whose key was synthesized with digest=True: role "head" | "mid" (length = c) | "last" (length = Lr bytes) | "tail" (length = 0)"""

    def __init__(self, role, length, aad=0, key_bits=128):
        Shape.__init__(self, role, key_bits, length, aad)
        self.segment = True
        self.message_bytes = 16 * length if role in ("head", "mid") else length

    def __repr__(self):
        return "dg-" + Shape.__repr__(self)

    def info(self, api):
        return api.circuit_info_gcm_segment(self.mode, self.length, self.aad, self.key_bits, digest=True)

    def matrices(self, api):
        return [api.circuit_matrix_gcm_segment(self.mode, self.length, which, self.aad, self.key_bits, digest=True) for which in range(3)]

    def instance_fields(self):
        m, head = 8 * self.message_bytes, [("iv", 96, True), ("ctr0", 32, True)]
        states = [("h_in", 256, True), ("h_out", 256, False)]
        return head + {"head": [("aad", 8 * self.aad, True), ("ct", m, False), ("com_out", 256, False)] + states,
                       "mid": [("ct", m, False), ("com_in", 256, False), ("com_out", 256, False)] + states,
                       "last": [("ct", m, False), ("com_in", 256, False), ("com_out", 256, False)] + states + [("total_bits", 64, True)],
                       "tail": [("len", 128, True), ("tag", 128, False), ("com_in", 256, False)]}[self.mode]


SHAPES = [DigestSegmentShape("head", 4, 13), DigestSegmentShape("mid", 4), DigestSegmentShape("last", 17), DigestSegmentShape("last", 56), DigestSegmentShape("tail", 0)]
_last = {}


def system_of(api, shape):
    if _last.get("at") != repr(shape):
        _last.clear()
        info = shape.info(api)
        _last.update(at=repr(shape), value=(ra.System(shape.matrices(api), int(info["instance"] + info["witness"])), info, shape.columns(info)))
    return _last["value"]


@pytest.mark.parametrize("shape", SHAPES, ids=repr)
def test_digest_segment_is_determined_by_its_statement(api, shape):
    t0 = time.time()
    s, info, cols = system_of(api, shape)
    ri, ni, rw = int(info["raw_instance"]), int(info["instance"]), int(info["raw_witness"])
    role = shape.mode
    # the documented positions: the states last, total_bits behind them; the closing tail has neither
    if role == "tail":
        assert "h_in" not in cols and cols["com_in"][-1] == ri - 1 and shape.message_bytes == 0 and len(cols["msg"]) == 0
    else:
        assert cols["h_in"][0] == cols["com_out"][-1] + 1 and cols["h_out"][0] == cols["h_in"][-1] + 1
        assert (cols["total_bits"][0] == cols["h_out"][-1] + 1 and cols["total_bits"][-1] == ri - 1) if role == "last" else cols["h_out"][-1] == ri - 1
    # (c)
    real = np.zeros(s.n_vars, dtype=bool)
    real[:ri] = True
    real[ni:ni + rw] = True
    missing, stray = ra.dangling(s, real)
    assert len(missing) == 0 and len(stray) == 0, (missing[:8], stray[:8])
    # (a) exactly message, key, Y_in and the salts are free
    res = ra.propagate(s, range(ri), greedy=range(ni, ni + rw))
    assert len(res.undetermined) == 0
    assert res.free == cols["hidden"], (len(res.free), len(cols["hidden"]), sorted(set(res.free) ^ set(cols["hidden"]))[:8])
    want = cols["msg"] + cols["key"] + ([] if role == "head" else cols["y_in"] + cols["salt_in"]) + ([] if role == "tail" else cols["salt_out"])
    assert cols["hidden"] == want and len(want) == 8 * shape.message_bytes + 128 + (0 if role == "head" else 256) + (0 if role == "tail" else 128)
    assert s.boolean[cols["hidden"]].all() and s.boolean[cols["outputs"]].all() and s.boolean[cols["inputs"]].all()
    # (b) every state, commitment and tag follows from the inputs, public and hidden
    seeds = seeds_b(cols)
    assert not set(cols["outputs"]) & set(seeds)
    assert len(seeds) + len(cols["outputs"]) == ri + len(cols["hidden"])
    res = ra.propagate(s, seeds)
    assert len(res.undetermined) == 0, (len(res.undetermined), res.undetermined[:8])
    assert res.known[cols["outputs"]].all() and res.known[ni:ni + rw].all()
    for name in ("h_out", "com_in", "com_out", "tag", "ct"):
        if name in cols:
            assert res.known[cols[name]].all()
    # one equality row of H_out deleted: exactly that bit comes back undetermined
    if role != "tail":
        bit = cols["h_out"][77]
        rows = [r for r in s.defining_rows(bit, side=0) if r != int(s.boolean_row[bit])]
        assert len(rows) == 1 and s.constant[1][rows[0]] and s.count[2][rows[0]] == 0 and s.count[0][rows[0]] == 2
        assert ra.propagate(s.without_rows(rows), seeds).undetermined.tolist() == [bit]
    print("%r: %d rows, %d witness variables, %d free inputs, %.1f s" % (shape, s.n_rows, rw, len(cols["hidden"]), time.time() - t0))
