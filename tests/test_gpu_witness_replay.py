"""The device's witness against a second witness generator, and every single-variable change of it against the rows ("constraint systems").

For CBC, CTR, GCM, key tags, digests and segments there is no oracle: the mode suites check the GPU-made z against the matrices it was built for, and
k_witness_expand's descriptors and trace_layout.h come from the compiler that made those matrices.  Here z is computed a second time by tests/r1cs_audit.py's solver
from the matrices, One, the public inputs and the hidden inputs' bits alone -- no trace, no descriptor, no layout -- and must equal the device's z at every variable;
its public outputs must equal the byte-level models (test_r1cs_audit.replay).  Then every variable that occurs in a row is replaced, one at a time, by 1 - z, 2 and
-1, and each replacement must leave at least one row unsatisfied: no variable is skipped.

One shape per family, one key per shape for the module, over an SRS sized from the circuit's own counts and without window tables, as the mode suites synthesize
theirs; two inputs per shape, one random and one with an all-zero message and key.
"""
import time

import numpy as np
import pytest

import r1cs_audit as ra
from test_r1cs_audit import Shape, replay, statement

pytestmark = pytest.mark.gpu

SHAPES = [Shape("ecb", 128, 16), Shape("cbc", 192, 32), Shape("ctr", 128, 17, 0, 1, "final"), Shape("gcm", 128, 1, 0), Shape("gcm", 256, 17, 5), Shape("mid", 128, 1),
          Shape("tail", 128, 5)]
REPLACEMENTS = {"1 - z": lambda v: 1 - v, "2": lambda v: np.full_like(v, 2), "-1": lambda v: np.full_like(v, -1)}
_keys = {}


@pytest.fixture(scope="module")
def replay_key(api):
    def get(shape):
        if repr(shape) not in _keys:
            ci = shape.info(api)
            srs = (int(ci["constraints"]), int(ci["instance"]), int(ci["nnz_a"] + ci["nnz_b"] + ci["nnz_c"]))
            if shape.segment:
                pk, _ = api.synthesize_keys_gcm_segment(shape.mode, shape.length, shape.aad, srs=srs, flags=api.KEY_NO_TABLES, key_bits=shape.key_bits)
            elif shape.mode == "gcm":
                pk, _ = api.synthesize_keys_gcm(shape.length, shape.aad, srs=srs, flags=api.KEY_NO_TABLES, key_bits=shape.key_bits)
            else:
                pk, _ = api.synthesize_keys(shape.length, circuit=shape.kind(api), srs=srs, flags=api.KEY_NO_TABLES, key_bits=shape.key_bits, key_tag_blocks=shape.tag_blocks,
                                            digest=shape.digest, digest_prefix=shape.prefix)
            _keys[repr(shape)] = pk
        return _keys[repr(shape)]
    yield get
    for pk in _keys.values():
        pk.free()
    _keys.clear()


def device_witness(api, pk, shape, v):
    """z as the device makes it, through the witness entry of the shape's mode"""
    msg, key = v["msg"], v["key"]
    if shape.segment:
        tail = shape.mode == "tail"
        header = api.gcm_segment_header(v["iv"], int.from_bytes(v["ctr0"], "big"), v["y_in"], v["salt_in"], None if tail else v["salt_out"], v["len"] if tail else None)
        return pk.witness_gcm_segment(msg, key, header)
    if shape.digest:
        header = None if shape.mode == "ecb" else v["iv"] + v["aad"] if shape.mode == "gcm" else v["iv"]
        return pk.witness_digest(msg, key, header, v["h_in"])
    if shape.mode == "ecb":
        return pk.witness(msg, key)
    if shape.mode == "cbc":
        return pk.witness_cbc(msg, key, v["iv"])
    if shape.mode == "ctr":
        return pk.witness_ctr(msg, key, v["iv"])
    return pk.witness_gcm(msg, key, v["iv"], v["aad"])


@pytest.mark.parametrize("zero", [False, True], ids=["random", "zero-message-and-key"])
@pytest.mark.parametrize("shape", SHAPES, ids=repr)
def test_replayed_witness_and_every_perturbation(api, replay_key, shape, zero):
    t0 = time.time()
    pk = replay_key(shape)
    v = statement(api, shape, 0x2E91A + 2 * SHAPES.index(shape) + 1, zero)       # an odd seed: the CTR counter wraps at its second increment
    dev = device_witness(api, pk, shape, v)
    t1 = time.time()
    z, s, info, cols = replay(api, shape, v)                                     # the solver's z, its public outputs checked against the models
    t2 = time.time()
    ri, ni, rw = int(info["raw_instance"]), int(info["instance"]), int(info["raw_witness"])
    assert len(dev) == s.n_vars == int(info["instance"] + info["witness"]) and set(dev) <= {0, 1}
    real = np.zeros(s.n_vars, dtype=bool)
    real[:ri] = True
    real[ni:ni + rw] = True
    assert np.array_equal(real, s.occurs)                                        # the solver is silent about a variable no row holds: there is none among the real ones
    dz = np.frombuffer(dev, dtype=np.uint8).astype(np.int64)
    differ = np.nonzero((dz != np.array(z, dtype=np.int64)) & real)[0]
    assert len(differ) == 0, "device z differs from the replayed z at %d variables, the first %s" % (len(differ), differ[:8].tolist())
    assert not dz[ri:ni].any()                                                   # the padded instance is zero
    # every single-variable replacement is rejected; the cap on skipped variables is zero
    left, paths = ra.unperturbable(s, dz, REPLACEMENTS)
    assert paths["int64"] + paths["python"] == paths["pairs"] and paths["pairs"] >= int(s.occurs.sum())
    for name in REPLACEMENTS:
        assert len(left[name]) == 0, "replacing z by %s goes unnoticed at %d variables, the first %s" % (name, len(left[name]), left[name][:8].tolist())
    print("%r %s: %d variables, (variable, row) pairs %s, device %.2f s, replay %.1f s, perturbation %.1f s" % (shape, "zero" if zero else "random", int(s.occurs.sum()), paths, t1 - t0,
                                                                                                                 t2 - t1, time.time() - t2))
