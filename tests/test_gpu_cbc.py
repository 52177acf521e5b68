"""AES-128-CBC proving on the GPU: the trace kernel's CBC instantiation, the witness against the circuit's own matrices, lone and chunked proofs.

There is no upstream CBC circuit and no oracle for it, so nothing here is byte parity.  Correctness rests on the pure-Python AES-CBC model of test_cbc_host.py, the NIST vector
(SP 800-38A F.2.1) and a row-by-row check of (A z) o (B z) = C z in int64 numpy over the matrices zkaes_circuit_matrix returns.  The shapes are the smallest where the
feature can go wrong: nb = 1 (the IV only), nb = 2 (one chained block), nb = 3 (a lane that walks two predecessors); every key is synthesized over an SRS sized for its own
circuit, without window tables, so each test takes seconds.
"""
import numpy as np
import pytest

from test_cbc_host import NIST_CT, NIST_IV, NIST_KEY, NIST_PT, model_cbc, model_ecb

pytestmark = pytest.mark.gpu

TR_BLOCK0, TR_BLOCK_STRIDE, TR_BL_MSG, TR_BL_S = 272, 1072, 0, 16          # csrc/trace_layout.h


def bits(data):
    """8 LSB-first bits per byte, one byte (0/1) each: the public-input encoding"""
    return bytes((b >> i) & 1 for b in data for i in range(8))


_keys = {}


@pytest.fixture(scope="module")
def cbc_key(api):
    """(pk, vk) for an nb-block CBC chunk over an SRS sized from the circuit's own counts, no window tables; one per nb for the module"""
    def get(nb):
        if nb not in _keys:
            ci = api.circuit_info(api.CIRCUIT_AES_CBC, 16 * nb)
            srs = (int(ci["constraints"]), int(ci["instance"]), int(ci["nnz_a"] + ci["nnz_b"] + ci["nnz_c"]))
            _keys[nb] = api.synthesize_keys(16 * nb, circuit=api.CIRCUIT_AES_CBC, srs=srs, flags=api.KEY_NO_TABLES)
        return _keys[nb]
    yield get
    for pk, _ in _keys.values():
        pk.free()
    _keys.clear()


_mats = {}


def unsatisfied_rows(api, nb, z):
    """indices of the rows where (A z) * (B z) != C z, in int64 (coefficients are small integers, z is 0/1)"""
    if nb not in _mats:
        _mats[nb] = [api.circuit_matrix(api.CIRCUIT_AES_CBC, 16 * nb, which) for which in range(3)]
    zz = np.frombuffer(z, dtype=np.uint8).astype(np.int64)
    prods = []
    for rowptr, col, coeff in _mats[nb]:
        assert len(zz) == len(rowptr) - 1                                    # square after padding
        cs = np.concatenate([[0], np.cumsum(coeff * zz[col])])
        prods.append(cs[rowptr[1:].astype(np.int64)] - cs[rowptr[:-1].astype(np.int64)])
    return np.nonzero(prods[0] * prods[1] != prods[2])[0]


@pytest.mark.parametrize("nb", [1, 2, 3])
def test_witness_satisfies_every_constraint(api, cbc_key, nb):
    pk, _ = cbc_key(nb)
    info = pk.info()
    assert (info["raw_instance"], info["instance"]) == (129 + 128 * nb, 512 if nb < 3 else 1024)
    rs = np.random.RandomState(0xC0 + nb)
    cases = [(NIST_PT[:16 * nb], NIST_KEY, NIST_IV), (rs.bytes(16 * nb), rs.bytes(16), rs.bytes(16)), (bytes(16 * nb), bytes(16), b"\xff" * 16)]
    for msg, key, iv in cases:
        z = pk.witness_cbc(msg, key, iv)
        assert len(z) == info["instance"] + info["witness"] and set(z) <= {0, 1}
        ct = model_cbc(msg, key, iv)
        assert z[0] == 1
        assert z[1:129] == bits(iv)
        assert z[129:129 + 128 * nb] == bits(ct)
        assert not any(z[129 + 128 * nb:info["instance"]])                   # the instance padding
        bad = unsatisfied_rows(api, nb, z)
        assert len(bad) == 0, bad[:10]
        # the checker itself can fail: one ciphertext bit, then one IV bit, of the instance flipped
        for at in (129 + 128 * nb - 3, 5):
            zf = bytearray(z)
            zf[at] ^= 1
            assert len(unsatisfied_rows(api, nb, bytes(zf))) >= 1
    assert NIST_CT[:16 * nb] == model_cbc(*cases[0])


def test_trace_tail_and_chained_blocks(api, cbc_key):
    """after one proof: the tail behind the blocks is IV || X_0 || X_1 || X_2 of the model, every block keeps its plaintext and its S_10 is its ciphertext block"""
    nb = 3
    pk, vk = cbc_key(nb)
    rs = np.random.RandomState(0x7ACE)
    msg, key, iv = rs.bytes(16 * nb), rs.bytes(16), rs.bytes(16)
    ct, proof = api.encrypt_cbc(msg, key, iv, pk)
    want = model_cbc(msg, key, iv)
    assert ct == want and api.verify_encryption_cbc(vk, proof, iv, ct)
    tr = pk.debug_fetch("trace")
    cbc = TR_BLOCK0 + nb * TR_BLOCK_STRIDE
    assert len(tr) == cbc + 16 + 16 * nb
    assert tr[:16] == key
    assert tr[cbc:cbc + 16] == iv
    prev = iv
    for b in range(nb):
        base = TR_BLOCK0 + b * TR_BLOCK_STRIDE
        x = bytes(m ^ p for m, p in zip(msg[16 * b:16 * b + 16], prev))
        assert tr[cbc + 16 + 16 * b:cbc + 32 + 16 * b] == x, b
        assert tr[base + TR_BL_MSG:base + TR_BL_MSG + 16] == msg[16 * b:16 * b + 16], b
        assert tr[base + TR_BL_S:base + TR_BL_S + 16] == bytes(a ^ k for a, k in zip(x, key)), b      # S_0 = X_b ^ key
        assert tr[base + TR_BL_S + 160:base + TR_BL_S + 176] == want[16 * b:16 * b + 16], b           # S_10
        prev = want[16 * b:16 * b + 16]


@pytest.mark.parametrize("nb", [1, 2])
def test_lone_proof_nist_prefix(api, cbc_key, nb):
    pk, vk = cbc_key(nb)
    msg, want = NIST_PT[:16 * nb], NIST_CT[:16 * nb]
    ct, proof = api.encrypt_cbc(msg, NIST_KEY, NIST_IV, pk)
    assert ct == want
    assert api.verify_encryption_cbc(vk, proof, NIST_IV, ct) is True
    assert vk.verify(proof, bits(NIST_IV) + bits(ct)) is True               # the layout, independently of the new verifier: IV bits, then ciphertext bits
    assert api.proof_roundtrip(proof) == proof
    flipped_ct = bytearray(ct); flipped_ct[-1] ^= 0x10
    flipped_iv = bytearray(NIST_IV); flipped_iv[3] ^= 0x01
    assert api.verify_encryption_cbc(vk, proof, NIST_IV, bytes(flipped_ct)) is False
    assert api.verify_encryption_cbc(vk, proof, bytes(flipped_iv), ct) is False
    assert api.verify_encryption_cbc(vk, proof, NIST_IV, model_ecb(msg, NIST_KEY)) is False
    assert vk.verify(proof, bits(ct) + bits(NIST_IV)) is False              # the two halves swapped
    other_iv = bytes(range(16, 32))
    ct2, proof2 = api.encrypt_cbc(msg, NIST_KEY, other_iv, pk)
    assert ct2 == model_cbc(msg, NIST_KEY, other_iv) and ct2 != ct
    assert api.verify_encryption_cbc(vk, proof2, other_iv, ct2) is True
    assert api.verify_encryption_cbc(vk, proof2, NIST_IV, ct) is False       # a proof made under another IV
    assert api.verify_encryption_cbc(vk, proof2, NIST_IV, ct2) is False
    # a caller's seed gives a different, still valid proof of the same statement
    ct3, proof3 = api.encrypt_cbc(msg, NIST_KEY, NIST_IV, pk, zk_seed=bytes(range(32)))
    assert ct3 == ct and proof3 != proof and api.verify_encryption_cbc(vk, proof3, NIST_IV, ct)


def test_chunked_three_chunks_two_contexts(api, cbc_key):
    nb, n_chunks = 2, 3
    chunk = 16 * nb
    pk, vk = cbc_key(nb)
    rs = np.random.RandomState(0xC4A1)
    msg, key, iv = NIST_PT + rs.bytes(32), NIST_KEY, NIST_IV
    want = model_cbc(msg, key, iv)
    assert want[:64] == NIST_CT
    pk.set_contexts(2)
    try:
        ct, proofs = pk.encrypt_cbc_chunked(msg, key, iv, zk_seed=api.PARITY)
        assert ct == want and len(proofs) == n_chunks
        assert api.verify_cbc_chunked(vk, proofs, iv, ct) == [True, True, True]
        for j in range(n_chunks):                                             # each chunk is a lone statement under the chaining value entering it
            iv_j = iv if j == 0 else ct[chunk * j - 16:chunk * j]
            assert api.verify_encryption_cbc(vk, proofs[j], iv_j, ct[chunk * j:chunk * (j + 1)]) is True
        assert api.verify_cbc_chunked(vk, [proofs[1], proofs[0], proofs[2]], iv, ct) == [False, False, True]
        assert api.verify_encryption_cbc(vk, proofs[1], iv, ct[chunk:2 * chunk]) is False            # chunk 1 under the message IV instead of its chained IV
        bad = bytearray(ct); bad[chunk - 1] ^= 1                              # the last byte of chunk 0 is also chunk 1's IV
        assert api.verify_cbc_chunked(vk, proofs, iv, bytes(bad)) == [False, False, True]
        # byte-identical under the fixed prover stream, whichever context proved which chunk
        ct_b, proofs_b = pk.encrypt_cbc_chunked(msg, key, iv, zk_seed=api.PARITY)
        assert ct_b == ct and proofs_b == proofs
        # chunks 1-2 by a separate call: its iv is the ciphertext block ahead of them, its first proof has the job-global index 1
        seed = bytes(range(100, 132))
        ct_all, proofs_all = pk.encrypt_cbc_chunked(msg, key, iv, zk_seed=seed)
        ct_tail, proofs_tail = pk.encrypt_cbc_chunked(msg[chunk:], key, api.cbc_ciphertext(msg, key, iv)[chunk - 16:chunk], zk_seed=seed, first_proof_index=1)
        assert ct_tail == want[chunk:] and proofs_tail == proofs_all[1:]
        assert api.verify_cbc_chunked(vk, [proofs_all[0]] + proofs_tail, iv, want) == [True, True, True]
        assert len({bytes(p) for p in proofs_all}) == 3 and proofs_all[0] != proofs[0]
        # a fresh OS seed per call: valid, and not the fixed stream
        ct_f, proofs_f = pk.encrypt_cbc_chunked(msg, key, iv)
        assert ct_f == want and api.verify_cbc_chunked(vk, proofs_f, iv, ct_f) == [True] * 3 and proofs_f[0] != proofs[0]
        with pytest.raises(api.ZkAesError):
            pk.encrypt_cbc_chunked(msg[:-16], key, iv)
    finally:
        pk.set_contexts(0)


def test_bench_shape_six_block_chunks_over_the_default_srs(api):
    """the reference's SRS literal (the default of synthesize_keys) holds a 6-block CBC chunk: |H|, |K|, |X| as the 6-block ECB chunk the benchmark proves"""
    free_b, _ = api.mem_info()
    if free_b < (24 << 30):
        pytest.skip("needs ~24 GB of free device memory (the universal SRS without tables + two 6-block prover contexts)")
    pk, vk = api.synthesize_keys(96, circuit=api.CIRCUIT_AES_CBC, flags=api.KEY_NO_TABLES)
    try:
        info = pk.info()
        e = api.circuit_info(api.CIRCUIT_AES, 96)
        assert (info["raw_constraints"], info["raw_instance"]) == (927_296, 897)
        assert (info["h"], info["instance"]) == (1 << 20, 1024) and info["instance"] == e["instance"]
        print("6-block CBC chunk: joint nnz %d, |K| = %d" % (info["joint_nnz"], info["k"]))
        pk.set_contexts(2)
        rs = np.random.RandomState(0x6B10)
        msg, key, iv = rs.bytes(192), rs.bytes(16), rs.bytes(16)
        ct, proofs = pk.encrypt_cbc_chunked(msg, key, iv, zk_seed=bytes(32))
        assert ct == model_cbc(msg, key, iv)
        assert api.verify_cbc_chunked(vk, proofs, iv, ct) == [True, True]
        assert api.verify_cbc_chunked(vk, proofs[::-1], iv, ct) == [False, False]
    finally:
        pk.free()


def test_entry_points_refuse_the_other_mode(api, cbc_key):
    pk_cbc, vk_cbc = cbc_key(1)
    msg, key, iv = NIST_PT[:16], NIST_KEY, NIST_IV
    for call in (lambda: api.encrypt(msg, key, pk_cbc), lambda: pk_cbc.encrypt_chunked(msg, key, zk_seed=api.PARITY), lambda: pk_cbc.encrypt_batch([msg], [key], zk_seed=api.PARITY),
                 lambda: pk_cbc.witness(msg, key), lambda: pk_cbc.prove_ops(1, 2), lambda: pk_cbc.op_lists(msg, key)):
        with pytest.raises(api.ZkAesError):
            call()
    ci = api.circuit_info(api.CIRCUIT_AES, 16)
    pk_ecb, vk_ecb = api.synthesize_keys(16, srs=(int(ci["constraints"]), int(ci["instance"]), int(ci["nnz_a"] + ci["nnz_b"] + ci["nnz_c"])), flags=api.KEY_NO_TABLES)
    try:
        for call in (lambda: api.encrypt_cbc(msg, key, iv, pk_ecb), lambda: pk_ecb.encrypt_cbc_chunked(msg, key, iv, zk_seed=api.PARITY), lambda: pk_ecb.encrypt_cbc_chunked(msg, key, iv),
                     lambda: pk_ecb.witness_cbc(msg, key, iv)):
            with pytest.raises(api.ZkAesError):
                call()
        pk_ops, _ = api.synthesize_keys(0, circuit=api.CIRCUIT_OPS_XOR, srs=(200, 200, 600))
        with pytest.raises(api.ZkAesError):
            api.encrypt_cbc(msg, key, iv, pk_ops)
        with pytest.raises(api.ZkAesError):
            pk_ops.witness_cbc(msg, key, iv)
        pk_ops.free()
        # the ECB key still proves ECB, and neither verifier takes the other mode's proof
        proof = api.encrypt(msg, key, pk_ecb)
        assert api.verify_encryption(vk_ecb, proof, model_ecb(msg, key)) is True
        assert api.verify_encryption_cbc(vk_ecb, proof, iv, model_ecb(msg, key)) is False
        ct, proof_cbc = api.encrypt_cbc(msg, key, iv, pk_cbc)
        assert api.verify_encryption(vk_cbc, proof_cbc, ct) is False
    finally:
        pk_ecb.free()
    # wrong lengths on a CBC key
    for n in (0, 15, 32):
        with pytest.raises(api.ZkAesError):
            api.encrypt_cbc(bytes(n), key, iv, pk_cbc)
