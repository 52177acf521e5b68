"""The device's witness of a reveal segment key against a second witness generator, in the way of tests/test_gpu_witness_replay.py: one tail (Lt = 7) with
reveal = 1.  z is computed a second time by tests/r1cs_audit.py's solver from the matrices, One, the public inputs -- the mask slice among them -- and the hidden inputs'
bits alone: no trace, no descriptor, no layout.  It must equal the device's z at every variable, and its public outputs -- the revealed bytes among them -- must equal the
byte-level models.  Then every variable that occurs in a row is replaced, one at a time, by 1 - z, 2 and -1, and each replacement must leave at least one row unsatisfied.
"""
import numpy as np
import pytest

import gcm_segment_reveal_model as model
import r1cs_audit as ra
from test_gpu_witness_replay import REPLACEMENTS
from test_r1cs_audit import replay, statement
from test_r1cs_audit_gcm_segments_reveal import TAIL

pytestmark = pytest.mark.gpu


def test_replayed_reveal_tail_witness_and_every_perturbation(api):
    shape = TAIL
    ci = shape.info(api)
    srs = (int(ci["constraints"]), int(ci["instance"]), int(ci["nnz_a"] + ci["nnz_b"] + ci["nnz_c"]))
    pk, _ = api.synthesize_keys_gcm_segment("tail", shape.length, 0, srs=srs, flags=api.KEY_NO_TABLES, reveal=True)
    try:
        cases = []
        for opened in ([0, 3, 6], []):                                           # three bytes open; nothing open
            v = statement(api, shape, 0x2E91B)
            v["mask"] = api.reveal_mask(opened, shape.message_bytes)
            v["revealed"] = model.revealed_of(v["msg"], v["mask"])
            header = api.gcm_segment_header(v["iv"], int.from_bytes(v["ctr0"], "big"), v["y_in"], v["salt_in"], None, v["len"])
            cases.append((v, pk.witness_gcm_segment(v["msg"], v["key"], header, mask=v["mask"])))
    finally:
        pk.free()
    for v, dev in cases:
        z, s, info, cols = replay(api, shape, v)                                 # the solver's z, its public outputs checked against the models
        ri, ni, rw = int(info["raw_instance"]), int(info["instance"]), int(info["raw_witness"])
        assert len(dev) == s.n_vars == int(info["instance"] + info["witness"]) and set(dev) <= {0, 1}
        real = np.zeros(s.n_vars, dtype=bool)
        real[:ri] = True
        real[ni:ni + rw] = True
        assert np.array_equal(real, s.occurs)
        dz = np.frombuffer(dev, dtype=np.uint8).astype(np.int64)
        differ = np.nonzero((dz != np.array(z, dtype=np.int64)) & real)[0]
        assert len(differ) == 0, "device z differs from the replayed z at %d variables, the first %s" % (len(differ), differ[:8].tolist())
        assert not dz[ri:ni].any()
        assert bytes(dz[cols["revealed"]].astype(np.uint8).tolist()) == model.bits(v["revealed"]) and bytes(dz[cols["mask"]].astype(np.uint8).tolist()) == model.bits(v["mask"])
    # every single-variable replacement of the last witness (nothing open: every product row has a zero factor) is rejected; the cap on skipped variables is zero
    left, paths = ra.unperturbable(s, dz, REPLACEMENTS)
    assert paths["int64"] + paths["python"] == paths["pairs"] and paths["pairs"] >= int(s.occurs.sum())
    for name in REPLACEMENTS:
        assert len(left[name]) == 0, "replacing z by %s goes unnoticed at %d variables, the first %s" % (name, len(left[name]), left[name][:8].tolist())
