"""The GCM segment HEAD circuit with key-tag blocks through the structural audit of tests/r1cs_audit.py: a head at c = 1, A = 13, T = 1, without and
with reveal.
  (a) with One and the raw instance known -- the tag bits among it -- the variables that have to be declared free are exactly the hidden inputs of the untagged head:
      key, message and salt_out.  The tag adds no free variable, and knowing it does not determine a key bit structurally (AES is not inverted by propagation);
  (b) with One, the hidden inputs and the public INPUTS known, every tag bit and every other public output is determined, and so is every witness of the tag blocks;
  (c) every raw variable is in a row and no padding variable is.
The tag bits sit behind com_out and ahead of the mask, where DESIGN.md 9l puts them.  Deleting the equality row of one tag bit leaves exactly that bit undetermined.
"""
import time

import numpy as np
import pytest

import r1cs_audit as ra
from test_r1cs_audit import Shape, seeds_b


class TaggedHeadShape(Shape):
    """a head Shape whose key was synthesized with key_tag_blocks = T (and reveal = R): the instance gains the key tag (an output) behind com_out, then the mask slice
    (an input) and the revealed slice (an output)"""

    def __init__(self, key_bits, c, aad, tag_blocks, reveal):
        Shape.__init__(self, "head", key_bits, c, aad, tag_blocks)
        self.reveal = reveal

    def __repr__(self):
        return Shape.__repr__(self) + "-R%d" % self.reveal

    def info(self, api):
        return api.circuit_info_gcm_segment(self.mode, self.length, self.aad, self.key_bits, reveal=bool(self.reveal), key_tag_blocks=self.tag_blocks)

    def matrices(self, api):
        return [api.circuit_matrix_gcm_segment(self.mode, self.length, which, self.aad, self.key_bits, reveal=bool(self.reveal), key_tag_blocks=self.tag_blocks) for which in range(3)]

    def instance_fields(self):
        f = Shape.instance_fields(self) + [("key_tag", 128 * self.tag_blocks, False)]
        if self.reveal:
            f += [("mask", 8 * ((self.message_bytes + 7) // 8), True), ("revealed", 8 * self.message_bytes, False)]
        return f


PLAIN, REVEAL = TaggedHeadShape(128, 1, 13, 1, 0), TaggedHeadShape(128, 1, 13, 1, 1)
FREE_INPUTS = 128 + 128 + 128                                                  # message, key, salt_out: the hidden inputs of the untagged head (tests/test_r1cs_audit_gcm_segments_reveal.py)

_last = {}


def system_of(api, shape):
    if _last.get("at") != repr(shape):
        _last.clear()
        info = shape.info(api)
        _last.update(at=repr(shape), value=(ra.System(shape.matrices(api), int(info["instance"] + info["witness"])), info, shape.columns(info)))
    return _last["value"]


@pytest.mark.parametrize("shape", [PLAIN, REVEAL], ids=repr)
def test_tagged_head_is_determined_by_its_statement(api, shape):
    t0 = time.time()
    s, info, cols = system_of(api, shape)
    ri, ni, rw = int(info["raw_instance"]), int(info["instance"]), int(info["raw_witness"])
    untagged = api.circuit_info_gcm_segment("head", shape.length, shape.aad, shape.key_bits, reveal=bool(shape.reveal))
    assert ri == untagged["raw_instance"] + 128 and rw == untagged["raw_witness"] + 147_760
    # the documented position: behind com_out, ahead of the mask
    assert cols["key_tag"][0] == cols["com_out"][-1] + 1 and len(cols["key_tag"]) == 128
    if shape.reveal:
        assert cols["mask"][0] == cols["key_tag"][-1] + 1
    else:
        assert cols["key_tag"][-1] == ri - 1
    # (c)
    real = np.zeros(s.n_vars, dtype=bool)
    real[:ri] = True
    real[ni:ni + rw] = True
    missing, stray = ra.dangling(s, real)
    assert len(missing) == 0 and len(stray) == 0, (missing[:8], stray[:8])
    # (a) exactly the hidden inputs of the untagged head are free
    res = ra.propagate(s, range(ri), greedy=range(ni, ni + rw))
    assert len(res.undetermined) == 0
    assert res.free == cols["hidden"], (len(res.free), len(cols["hidden"]), sorted(set(res.free) ^ set(cols["hidden"]))[:8])
    assert cols["hidden"] == cols["msg"] + cols["key"] + cols["salt_out"] and len(cols["hidden"]) == FREE_INPUTS
    assert s.boolean[cols["hidden"]].all() and s.boolean[cols["key_tag"]].all()
    # (b) every tag variable follows from the inputs, public and hidden
    seeds = seeds_b(cols)
    assert not set(cols["key_tag"]) & set(seeds)
    assert len(seeds) + len(cols["outputs"]) == ri + len(cols["hidden"])
    res = ra.propagate(s, seeds)
    assert len(res.undetermined) == 0, (len(res.undetermined), res.undetermined[:8])
    assert res.known[cols["outputs"]].all() and res.known[cols["key_tag"]].all() and res.known[ni:ni + rw].all()
    # the tag blocks' witnesses are the last ones allocated (reveal allocates none): all of them follow
    assert res.known[ni + rw - 147_760:ni + rw].all()
    # one equality row deleted: exactly that tag bit comes back undetermined
    bit = cols["key_tag"][77]
    rows = [r for r in s.defining_rows(bit, side=0) if r != int(s.boolean_row[bit])]
    assert len(rows) == 1 and s.constant[1][rows[0]] and s.count[2][rows[0]] == 0 and s.count[0][rows[0]] == 2
    assert ra.propagate(s.without_rows(rows), seeds).undetermined.tolist() == [bit]
    print("%r: %d rows, %d witness variables, %d free inputs, %.1f s" % (shape, s.n_rows, rw, len(cols["hidden"]), time.time() - t0))
