"""AES-128-CTR proving on the GPU: the CTR trace kernel, the witness against the circuit's own matrices, lone proofs of byte-granular lengths, seekable chunk-proofs.

There is no upstream CTR circuit and no oracle for it, so nothing here is byte parity.  Correctness rests on the pure-Python CTR model of test_ctr_host.py (counters as
Python integers), the NIST vector (SP 800-38A F.5.1) and a row-by-row check of (A z) o (B z) = C z in int64 numpy over the matrices zkaes_circuit_matrix returns.  The
shapes are the smallest where the kernel can go wrong: L = 1 (one partial block), L = 17 (a whole block + 1 byte, one increment), L = 48 (three whole blocks, two
increments); every key is synthesized over an SRS sized for its own circuit, without window tables, so each test takes seconds.
"""
import numpy as np
import pytest

from test_cbc_host import model_cbc, model_ecb
from test_ctr_host import NIST_CTR_CT, NIST_ICB, NIST_KEY, NIST_PT, model_counter, model_ctr

pytestmark = pytest.mark.gpu

TR_BLOCK0, TR_BLOCK_STRIDE, TR_BL_MSG, TR_BL_S = 272, 1072, 0, 16          # csrc/trace_layout.h
TR_CTR_BLOCK0, TR_CTR_BLOCK_STRIDE = 16, 48                                 # behind the icb: per block CTR_b, K_b, C_b

ICB_ONES = b"\xff" * 16                                                     # wraps to zero at the first increment
ICB_7F = bytes(11) + b"\x7f" + b"\xff" * 4                                  # ..7f ffffffff: the carry runs through 39 bits and stops inside byte 11
ICB_FE = b"\xff" * 15 + b"\xfe"                                             # wraps at the second increment


def bits(data):
    """8 LSB-first bits per byte, one byte (0/1) each: the public-input encoding"""
    return bytes((b >> i) & 1 for b in data for i in range(8))


def small_srs(api, kind, length):
    ci = api.circuit_info(kind, length)
    return (int(ci["constraints"]), int(ci["instance"]), int(ci["nnz_a"] + ci["nnz_b"] + ci["nnz_c"]))


_keys = {}


@pytest.fixture(scope="module")
def ctr_key(api):
    """(pk, vk) for an L-byte CTR statement over an SRS sized from the circuit's own counts, no window tables; one per L for the module"""
    def get(length):
        if length not in _keys:
            _keys[length] = api.synthesize_keys(length, circuit=api.CIRCUIT_AES_CTR, srs=small_srs(api, api.CIRCUIT_AES_CTR, length), flags=api.KEY_NO_TABLES)
        return _keys[length]
    yield get
    for pk, _ in _keys.values():
        pk.free()
    _keys.clear()


_mats = {}


def unsatisfied_rows(api, length, z):
    """indices of the rows where (A z) * (B z) != C z, in int64 (coefficients are small integers, z is 0/1)"""
    if length not in _mats:
        _mats[length] = [api.circuit_matrix(api.CIRCUIT_AES_CTR, length, which) for which in range(3)]
    zz = np.frombuffer(z, dtype=np.uint8).astype(np.int64)
    prods = []
    for rowptr, col, coeff in _mats[length]:
        assert len(zz) == len(rowptr) - 1                                    # square after padding
        cs = np.concatenate([[0], np.cumsum(coeff * zz[col])])
        prods.append(cs[rowptr[1:].astype(np.int64)] - cs[rowptr[:-1].astype(np.int64)])
    return np.nonzero(prods[0] * prods[1] != prods[2])[0]


def carries(prev):
    """K_b of trace_layout.h from CTR_{b-1}: bit i (weight 2^i, bit i % 8 of byte 15 - i / 8) is set iff bits 0..i of prev are all one"""
    x, out = int.from_bytes(prev, "big"), 0
    for i in range(128):
        if not (x >> i) & 1:
            break
        out |= 1 << i
    return out.to_bytes(16, "big")


@pytest.mark.parametrize("length", [1, 17, 48])
def test_witness_satisfies_every_constraint(api, ctr_key, length):
    pk, _ = ctr_key(length)
    info = pk.info()
    assert info["raw_instance"] == 129 + 8 * length and info["instance"] == {1: 256, 17: 512, 48: 1024}[length]
    rs = np.random.RandomState(0xC7 + length)
    cases = [(NIST_PT[:length], NIST_KEY, NIST_ICB), (rs.bytes(length), rs.bytes(16), rs.bytes(16)), (rs.bytes(length), rs.bytes(16), ICB_ONES), (bytes(length), bytes(16), ICB_7F)]
    for msg, key, icb in cases:
        z = pk.witness_ctr(msg, key, icb)
        assert len(z) == info["instance"] + info["witness"] and set(z) <= {0, 1}
        ct = model_ctr(msg, key, icb)
        assert z[0] == 1
        assert z[1:129] == bits(icb)
        assert z[129:129 + 8 * length] == bits(ct)
        assert not any(z[129 + 8 * length:info["instance"]])                  # the instance padding
        bad = unsatisfied_rows(api, length, z)
        assert len(bad) == 0, bad[:10]
        # the checker itself can fail: one ciphertext bit (in the last, partial byte), then counter bit 0, of the instance flipped
        for at in (129 + 8 * length - 3, 1 + 8 * 15):
            zf = bytearray(z)
            zf[at] ^= 1
            assert len(unsatisfied_rows(api, length, bytes(zf))) >= 1
    assert NIST_CTR_CT[:length] == model_ctr(*cases[0])


def test_trace_tail_counters_carries_and_partial_block(api, ctr_key):
    """after one proof at L = 33 under ff..fe (block 1 is ff..ff, block 2 wraps to zero): the tail behind the blocks is icb, then per block CTR_b, K_b, C_b; message
    slots hold M_b with zeros beyond L; S_0 = CTR_b ^ key; S_10 ^ M_b = C_b on the bytes that exist"""
    length, nb = 33, 3
    pk, vk = ctr_key(length)
    rs = np.random.RandomState(0x7ACE)
    msg, key, icb = rs.bytes(length), rs.bytes(16), ICB_FE
    ct, proof = api.encrypt_ctr(msg, key, icb, pk)
    want = model_ctr(msg, key, icb)
    assert ct == want and api.verify_encryption_ctr(vk, proof, icb, ct)
    tr = pk.debug_fetch("trace")
    tail = TR_BLOCK0 + nb * TR_BLOCK_STRIDE
    assert len(tr) == tail + 16 + 48 * nb
    assert tr[:16] == key
    assert tr[tail:tail + 16] == icb
    padded, padded_ct = msg + bytes(16 * nb - length), want + bytes(16 * nb - length)
    for b in range(nb):
        base, slot = TR_BLOCK0 + b * TR_BLOCK_STRIDE, tail + TR_CTR_BLOCK0 + b * TR_CTR_BLOCK_STRIDE
        counter = model_counter(icb, b)
        assert tr[slot:slot + 16] == counter, b
        assert tr[slot + 16:slot + 32] == (carries(model_counter(icb, b - 1)) if b else bytes(16)), b
        assert tr[slot + 32:slot + 48] == padded_ct[16 * b:16 * b + 16], b
        assert tr[base + TR_BL_MSG:base + TR_BL_MSG + 16] == padded[16 * b:16 * b + 16], b
        assert tr[base + TR_BL_S:base + TR_BL_S + 16] == bytes(a ^ k for a, k in zip(counter, key)), b        # S_0 = CTR_b ^ key
        have = min(16, length - 16 * b)
        s10 = tr[base + TR_BL_S + 160:base + TR_BL_S + 176]
        assert bytes(s ^ m for s, m in zip(s10[:have], msg[16 * b:])) == want[16 * b:16 * b + have], b
    assert model_counter(icb, 1) == ICB_ONES and model_counter(icb, 2) == bytes(16)
    assert carries(ICB_ONES) == ICB_ONES and carries(ICB_FE) == bytes(16)


@pytest.mark.parametrize("length", [17, 1])
def test_lone_proof_nist_prefix(api, ctr_key, length):
    pk, vk = ctr_key(length)
    msg, want = NIST_PT[:length], NIST_CTR_CT[:length]
    ct, proof = api.encrypt_ctr(msg, NIST_KEY, NIST_ICB, pk)
    assert ct == want
    assert api.verify_encryption_ctr(vk, proof, NIST_ICB, ct) is True
    assert vk.verify(proof, bits(NIST_ICB) + bits(ct)) is True               # the layout, independently of the new verifier: icb bits, then ciphertext bits
    assert api.proof_roundtrip(proof) == proof
    flipped_ct = bytearray(ct); flipped_ct[-1] ^= 0x10                        # in the partial block's only byte
    flipped_icb = bytearray(NIST_ICB); flipped_icb[3] ^= 0x01
    assert api.verify_encryption_ctr(vk, proof, NIST_ICB, bytes(flipped_ct)) is False
    assert api.verify_encryption_ctr(vk, proof, bytes(flipped_icb), ct) is False
    assert api.verify_encryption_ctr(vk, proof, NIST_ICB, model_ecb(msg + bytes(32 - length), NIST_KEY)[:length]) is False
    assert vk.verify(proof, bits(ct) + bits(NIST_ICB)) is False              # the two halves swapped
    with pytest.raises(api.ZkAesError):                                      # the length is part of the statement
        api.verify_encryption_ctr(vk, proof, NIST_ICB, ct + b"\0")
    next_icb = api.ctr_counter_add(NIST_ICB, 1)
    ct2, proof2 = api.encrypt_ctr(msg, NIST_KEY, next_icb, pk)
    assert ct2 == model_ctr(msg, NIST_KEY, next_icb) and ct2 != ct
    assert api.verify_encryption_ctr(vk, proof2, next_icb, ct2) is True
    assert api.verify_encryption_ctr(vk, proof2, NIST_ICB, ct2) is False      # a proof made under icb + 1, checked under icb
    assert api.verify_encryption_ctr(vk, proof2, NIST_ICB, ct) is False
    # a caller's seed gives a different, still valid proof of the same statement
    ct3, proof3 = api.encrypt_ctr(msg, NIST_KEY, NIST_ICB, pk, zk_seed=bytes(range(32)))
    assert ct3 == ct and proof3 != proof and api.verify_encryption_ctr(vk, proof3, NIST_ICB, ct)


def test_chunked_three_chunks_two_contexts(api, ctr_key):
    chunk, n_chunks, nb = 32, 3, 2
    pk, vk = ctr_key(chunk)
    rs = np.random.RandomState(0xC4A1)
    msg, key, icb = NIST_PT + rs.bytes(32), NIST_KEY, NIST_ICB
    want = model_ctr(msg, key, icb)
    assert want[:64] == NIST_CTR_CT
    pk.set_contexts(2)
    try:
        ct, proofs = pk.encrypt_ctr_chunked(msg, key, icb, zk_seed=api.PARITY)
        assert ct == want and len(proofs) == n_chunks
        assert api.verify_ctr_chunked(vk, proofs, icb, ct) == [True, True, True]
        for j in range(n_chunks):                                             # each chunk is a lone statement under icb + j nb: seekable
            icb_j = api.ctr_counter_add(icb, nb * j)
            assert icb_j == model_counter(icb, nb * j)
            assert api.verify_encryption_ctr(vk, proofs[j], icb_j, ct[chunk * j:chunk * (j + 1)]) is True
        assert api.verify_ctr_chunked(vk, [proofs[1], proofs[0], proofs[2]], icb, ct) == [False, False, True]
        assert api.verify_encryption_ctr(vk, proofs[1], icb, ct[chunk:2 * chunk]) is False            # chunk 1 under the job's icb instead of icb + 2
        # byte-identical under the fixed prover stream, whichever context proved which chunk
        ct_b, proofs_b = pk.encrypt_ctr_chunked(msg, key, icb, zk_seed=api.PARITY)
        assert ct_b == ct and proofs_b == proofs
        # chunks 1-2 by a separate call: its icb is the advanced counter, its first proof has the job-global index 1
        seed = bytes(range(100, 132))
        ct_all, proofs_all = pk.encrypt_ctr_chunked(msg, key, icb, zk_seed=seed)
        ct_tail, proofs_tail = pk.encrypt_ctr_chunked(msg[chunk:], key, api.ctr_counter_add(icb, nb), zk_seed=seed, first_proof_index=1)
        assert ct_all == want and ct_tail == want[chunk:] and proofs_tail == proofs_all[1:]
        assert api.verify_ctr_chunked(vk, [proofs_all[0]] + proofs_tail, icb, want) == [True, True, True]
        assert len({bytes(p) for p in proofs_all}) == 3 and proofs_all[0] != proofs[0]
        # a counter that wraps inside the job: chunk 0 is ff..fe, ff..ff, chunk 1 starts at zero
        want_w = model_ctr(msg, key, ICB_FE)
        ct_w, proofs_w = pk.encrypt_ctr_chunked(msg, key, ICB_FE, zk_seed=seed)
        assert ct_w == want_w and api.verify_ctr_chunked(vk, proofs_w, ICB_FE, ct_w) == [True, True, True]
        assert api.verify_encryption_ctr(vk, proofs_w[1], bytes(16), ct_w[chunk:2 * chunk]) is True
        for bad_len in (len(msg) - 16, len(msg) - 1, 0):
            with pytest.raises(api.ZkAesError):
                pk.encrypt_ctr_chunked(msg[:bad_len], key, icb)
    finally:
        pk.set_contexts(0)


def test_ragged_job_of_69_bytes(api, ctr_key):
    """two chunks of the 32-byte key plus a lone proof under a 5-byte key and the counter advanced by 4 blocks: ECB's remainder-key arrangement, with a byte-granular tail"""
    pk, vk = ctr_key(32)
    pk_tail, vk_tail = ctr_key(5)
    rs = np.random.RandomState(0x69)
    msg, key, icb = rs.bytes(69), rs.bytes(16), ICB_7F
    ct_head, proofs = pk.encrypt_ctr_chunked(msg[:64], key, icb, zk_seed=bytes(32))
    icb_tail = api.ctr_counter_add(icb, 4)
    ct_tail, proof_tail = api.encrypt_ctr(msg[64:], key, icb_tail, pk_tail, zk_seed=bytes(32))
    assert ct_head + ct_tail == model_ctr(msg, key, icb)
    assert api.verify_ctr_chunked(vk, proofs, icb, ct_head) == [True, True]
    assert api.verify_encryption_ctr(vk_tail, proof_tail, icb_tail, ct_tail) is True
    assert api.verify_encryption_ctr(vk_tail, proof_tail, icb, ct_tail) is False
    with pytest.raises(api.ZkAesError):                                      # a chunked call takes a key for whole blocks
        pk_tail.encrypt_ctr_chunked(msg[:10], key, icb)


def test_bench_shape_six_block_chunks_over_the_default_srs(api):
    """the reference's SRS literal (the default of synthesize_keys) holds a 6-block CTR chunk: |H|, |X| as the 6-block ECB chunk the benchmark proves"""
    free_b, _ = api.mem_info()
    if free_b < (24 << 30):
        pytest.skip("needs ~24 GB of free device memory (the universal SRS without tables + two 6-block prover contexts)")
    pk, vk = api.synthesize_keys(96, circuit=api.CIRCUIT_AES_CTR, flags=api.KEY_NO_TABLES)
    try:
        info = pk.info()
        assert (info["raw_constraints"], info["raw_instance"], info["h"], info["instance"]) == (928_561, 897, 1 << 20, 1024)
        print("6-block CTR chunk: joint nnz %d, |K| = %d" % (info["joint_nnz"], info["k"]))
        pk.set_contexts(2)
        rs = np.random.RandomState(0x6B10)
        msg, key, icb = rs.bytes(192), rs.bytes(16), rs.bytes(16)
        ct, proofs = pk.encrypt_ctr_chunked(msg, key, icb, zk_seed=bytes(32))
        assert ct == model_ctr(msg, key, icb)
        assert api.verify_ctr_chunked(vk, proofs, icb, ct) == [True, True]
        assert api.verify_ctr_chunked(vk, proofs[::-1], icb, ct) == [False, False]
    finally:
        pk.free()


def test_entry_points_refuse_the_other_modes(api, ctr_key):
    pk_ctr, vk_ctr = ctr_key(16)
    msg, key, iv = NIST_PT[:16], NIST_KEY, NIST_ICB
    for call in (lambda: api.encrypt(msg, key, pk_ctr), lambda: pk_ctr.encrypt_chunked(msg, key, zk_seed=api.PARITY), lambda: pk_ctr.encrypt_batch([msg], [key], zk_seed=api.PARITY),
                 lambda: pk_ctr.witness(msg, key), lambda: pk_ctr.prove_ops(1, 2), lambda: pk_ctr.op_lists(msg, key),
                 lambda: api.encrypt_cbc(msg, key, iv, pk_ctr), lambda: pk_ctr.encrypt_cbc_chunked(msg, key, iv, zk_seed=api.PARITY), lambda: pk_ctr.witness_cbc(msg, key, iv)):
        with pytest.raises(api.ZkAesError):
            call()
    others = {"ecb": api.synthesize_keys(16, srs=small_srs(api, api.CIRCUIT_AES, 16), flags=api.KEY_NO_TABLES),
              "cbc": api.synthesize_keys(16, circuit=api.CIRCUIT_AES_CBC, srs=small_srs(api, api.CIRCUIT_AES_CBC, 16), flags=api.KEY_NO_TABLES),
              "ops": api.synthesize_keys(0, circuit=api.CIRCUIT_OPS_XOR, srs=(200, 200, 600))}
    try:
        for name, (pk, _) in others.items():
            for call in (lambda: api.encrypt_ctr(msg, key, iv, pk), lambda: pk.encrypt_ctr_chunked(msg, key, iv, zk_seed=api.PARITY), lambda: pk.encrypt_ctr_chunked(msg, key, iv),
                         lambda: pk.witness_ctr(msg, key, iv)):
                with pytest.raises(api.ZkAesError):
                    call()
        # every key still proves its own mode, and no verifier takes another mode's proof
        pk_ecb, vk_ecb = others["ecb"]
        pk_cbc, vk_cbc = others["cbc"]
        proof_ecb = api.encrypt(msg, key, pk_ecb)
        ct_cbc, proof_cbc = api.encrypt_cbc(msg, key, iv, pk_cbc)
        ct_ctr, proof_ctr = api.encrypt_ctr(msg, key, iv, pk_ctr)
        assert api.verify_encryption(vk_ecb, proof_ecb, model_ecb(msg, key)) is True
        assert ct_cbc == model_cbc(msg, key, iv) and api.verify_encryption_cbc(vk_cbc, proof_cbc, iv, ct_cbc) is True
        assert ct_ctr == model_ctr(msg, key, iv) and api.verify_encryption_ctr(vk_ctr, proof_ctr, iv, ct_ctr) is True
        with pytest.raises(api.ZkAesError):                                  # an ECB key's statement has 128 public bits, which no CTR length has
            api.verify_encryption_ctr(vk_ecb, proof_ecb, iv, model_ecb(msg, key))
        # (a 16-byte CBC key and a 16-byte CTR key take the same input shape, 16 bytes then the ciphertext, so verify_encryption_cbc and verify_encryption_ctr build the
        # same vector: it is the verifying key that names the relation.  The cross checks therefore pair each mode's key, through its own verifier, with the other
        # modes' proofs)
        assert api.verify_encryption_ctr(vk_ctr, proof_cbc, iv, ct_cbc) is False
        assert api.verify_encryption_ctr(vk_ctr, proof_ecb, iv, model_ecb(msg, key)) is False
        assert api.verify_encryption_cbc(vk_cbc, proof_ctr, iv, ct_ctr) is False
        assert api.verify_encryption(vk_ctr, proof_ctr, ct_ctr) is False
        assert api.verify_encryption(vk_ecb, proof_ctr, ct_ctr) is False
    finally:
        for pk, _ in others.values():
            pk.free()
    # wrong lengths on a CTR key
    for n in (0, 15, 17, 32):
        with pytest.raises(api.ZkAesError):
            api.encrypt_ctr(bytes(n), key, iv, pk_ctr)
        with pytest.raises(api.ZkAesError):
            pk_ctr.witness_ctr(bytes(n), key, iv)
