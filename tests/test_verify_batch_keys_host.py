"""The multi-key batch verifier's host back end (zkaes_verify_batch_keys) against the per-proof verifier: proofs of three keys of one setup in one batch,
damage and mislabelling, K = 1 against verify_batch, the errors of the call, a cross-key forgery that only the randomizers catch, a Python restatement of the segment
rows of a GCM record, and a sanitizer build fed with mutated multi-key batches.  No GPU."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CSRC = os.path.join(ROOT, "aes_zero_knowledge_proof_circuit_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import curve_math as cm  # noqa: E402

from test_verify_batch_host import OFF_W_BETA, SMALL_SRS, _bits, _compress, _damage, _decompress, per_proof  # noqa: E402

Q, R = cm.Q377, cm.R377
XOR, ADD, AES = 0, 1, 2                      # the key indices of the mixed batch
# the ark-serialize image of a verifying key (marlin_codec.cpp serialize_vk_ark): 4 x u64, u64 6, 6 x (48 + tag), g 48, gamma_g 48, then h and beta_h, 96 bytes each
ARK_H = 32 + 8 + 6 * 49 + 48 + 48


def make_mixed(zko, api, vectors):
    """(keys, items, handles): the xor, add and golden AES keys -- |X| = 1, 1 and 256, one setup -- and nine (key index, proof, row) in the order 4 xor, 3 add, the golden
    proof against the right and against a wrong ciphertext; handles: the oracle's proof objects of the seven ops proofs, and the two oracle indices"""
    from test_marlin_cpu import vk_for
    keys, items, handles, indices = [], [], [], []
    for which, count in (("xor", 4), ("add", 3)):
        cs, _ = zko.synth_ops(which, 0, 0, field=377)
        ix = zko.Index(cs, srs=SMALL_SRS)
        keys.append(vk_for(api, zko, ix, 0))
        indices.append(ix)
        for i in range(count):
            cs, _ = zko.synth_ops(which, 0x2000 + 911 * i, 0xC0DE ^ (37 * i), field=377)
            p = ix.prove(cs, bytes([16 * len(keys) + i + 1] * 32))
            handles.append(p)
            items.append((len(keys) - 1, p.to_bytes(), b""))
    keys.append(api.VerifyingKey.from_bytes(open(os.path.join(GOLD, "gpu_aes16_vk.bin"), "rb").read()))
    proof = open(os.path.join(GOLD, "gpu_aes16_proof.bin"), "rb").read()
    items.append((AES, proof, _bits(bytes(vectors["ciphertext"]))))
    items.append((AES, proof, _bits(bytes(vectors["wrong_ciphertext_16"]))))
    assert len({it[1] for it in items}) == 8
    return keys, items, handles, indices


INTERLEAVED = [0, 4, 7, 1, 5, 2, 8, 6, 3]     # xor add aes xor add xor aes(wrong) add xor
WANT = [True] * 8 + [False]


@pytest.fixture(scope="module")
def mixed(zko, api, vectors):
    return make_mixed(zko, api, vectors)


def serial(api, keys, items):
    return [per_proof(api, keys[k], p, r) for k, p, r in items]


def batch(api, keys, items, device=False):
    return api.verify_batch_keys(keys, [k for k, _, _ in items], [p for _, p, _ in items], [r for _, _, r in items], device=device)


def test_the_three_keys_share_one_setup(mixed):
    keys = mixed[0]
    arks = [k.to_ark_bytes() for k in keys]
    assert len({a[ARK_H - 96:ARK_H + 192] for a in arks}) == 1          # g, gamma_g, h, beta_h
    assert [int.from_bytes(a[24:32], "little") for a in arks] == [1, 1, 256]      # |X|
    assert len({a[40:88] for a in arks}) == 3                             # three index commitments: three keys


def test_mixed_batch_agrees_with_the_per_proof_verifier(api, mixed):
    keys, items, _, _ = mixed
    assert serial(api, keys, items) == WANT
    assert batch(api, keys, items) == WANT
    order = [items[i] for i in INTERLEAVED]
    want = [WANT[i] for i in INTERLEAVED]
    assert serial(api, keys, order) == want
    assert batch(api, keys, order) == want


@pytest.mark.parametrize("n", [1, 2, 5])
def test_prefixes_of_the_interleaved_order(api, mixed, n):
    keys, items, _, _ = mixed
    order = [items[i] for i in INTERLEAVED][:n]
    want = [WANT[i] for i in INTERLEAVED][:n]
    assert serial(api, keys, order) == want
    assert batch(api, keys, order) == want


@pytest.mark.parametrize("kind", ["eval", "random_v", "truncated"])
@pytest.mark.parametrize("pos", [0, 4, 8])
def test_damaged_mixed_batches(api, mixed, kind, pos):
    keys, items, _, _ = mixed
    order = [items[i] for i in INTERLEAVED]
    k, p, r = order[pos]
    order[pos] = (k, _damage(p, kind), r)
    want = [WANT[i] and j != pos for j, i in enumerate(INTERLEAVED)]
    assert serial(api, keys, order) == want
    assert batch(api, keys, order) == want


def test_a_proof_under_another_key_is_rejected_alone(api, mixed):
    keys, items, _, _ = mixed
    order = [items[i] for i in INTERLEAVED]
    assert order[0][0] == XOR
    order[0] = (ADD, order[0][1], order[0][2])                            # an xor proof labelled with the add key: same |X|, other index commitments
    want = serial(api, keys, order)
    assert want == [False] + [WANT[i] for i in INTERLEAVED][1:]
    assert batch(api, keys, order) == want


def test_one_key_agrees_with_verify_batch(api, mixed):
    keys, items, _, _ = mixed
    proofs = [p for k, p, _ in items if k == XOR] + [p for k, p, _ in items if k == ADD]      # seven proofs, one key: the add proofs are rejected under it
    want = [True] * 4 + [False] * 3
    assert api.verify_batch(keys[XOR], proofs, [b""] * 7, device=False) == want
    assert api.verify_batch_keys([keys[XOR]], [0] * 7, proofs, [b""] * 7, device=False) == want
    proofs[2] = _damage(proofs[2], "eval")
    want[2] = False
    assert api.verify_batch(keys[XOR], proofs, [b""] * 7, device=False) == want
    assert api.verify_batch_keys([keys[XOR]], [0] * 7, proofs, [b""] * 7, device=False) == want


def test_seven_xor_proofs_under_one_key_agree_with_verify_batch(api, zko):
    """the seven XOR proofs of test_verify_batch_host.py's fixture, valid and with one damaged, through both entries"""
    from test_marlin_cpu import vk_for
    cs, _ = zko.synth_ops("xor", 0, 0, field=377)
    ix = zko.Index(cs, srs=SMALL_SRS)
    vk = vk_for(api, zko, ix, 0)
    proofs = []
    for i in range(7):
        cs, _ = zko.synth_ops("xor", 0x1000 + 977 * i, 0xBEEF ^ (31 * i), field=377)
        proofs.append(ix.prove(cs, bytes([i + 1] * 32)).to_bytes())
    for bad in (None, 3):
        batch_ = list(proofs)
        if bad is not None:
            batch_[bad] = _damage(proofs[bad], "random_v")
        want = [i != bad for i in range(7)]
        assert api.verify_batch(vk, batch_, [b""] * 7, device=False) == want
        assert api.verify_batch_keys([vk], [0] * 7, batch_, [b""] * 7, device=False) == want


def test_errors_of_the_call(api, mixed):
    keys, items, _, _ = mixed
    k, p, r = items[0]
    with pytest.raises(api.ZkAesError, match="names key 3 of 3"):
        api.verify_batch_keys(keys, [0, 3], [p, p], [r, r], device=False)
    with pytest.raises(api.ZkAesError, match="at least one verifying key"):
        api.verify_batch_keys([], [0], [p], [r], device=False)
    # a key of another setup: the golden key's image with h and beta_h exchanged -- both are valid G2 points, so the deserializer takes it
    ark = keys[AES].to_ark_bytes()
    swapped = api.VerifyingKey.from_ark_bytes(ark[:ARK_H] + ark[ARK_H + 96:ARK_H + 192] + ark[ARK_H:ARK_H + 96] + ark[ARK_H + 192:])
    assert swapped.to_ark_bytes() != ark
    with pytest.raises(api.ZkAesError, match="do not share one setup"):
        api.verify_batch_keys([keys[XOR], swapped], [0], [p], [r], device=False)
    with pytest.raises(api.ZkAesError, match="do not share one setup"):
        api.verify_batch_keys([swapped, keys[XOR]], [1], [p], [r], device=False)
    assert api.verify_batch_keys([swapped], [0], [p], [r], device=False) == [False]      # alone it is one setup: the proof is checked under it, and fails


def test_a_row_that_does_not_fit_its_key_rejects_that_proof_only(api, mixed):
    keys, items, _, _ = mixed
    order = [items[i] for i in INTERLEAVED]
    want = [WANT[i] for i in INTERLEAVED]
    assert order[2][0] == AES and want[2]
    order[2] = (AES, order[2][1], order[2][2][:-1])                       # 127 bits pad to |X| = 128, not the key's 256
    order[3] = (XOR, order[3][1], b"\x00")                                # one bit pads to |X| = 2, not 1
    want[2] = want[3] = False
    assert serial(api, keys, order) == want
    assert batch(api, keys, order) == want
    order[2] = (AES, order[2][1], order[2][2] + bytes(74))                # 201 bits, zeros appended: pads to 256, the same statement
    want[2] = True
    assert serial(api, keys, order) == want
    assert batch(api, keys, order) == want


def test_randomizers_matter_across_keys(api, mixed):
    """test_verify_batch_host.py's test_randomizers_matter across two keys: an xor and an add proof whose beta-openings are shifted against each other so that the
    UNWEIGHTED sum of their two checks balances.  Both keys open under the same beta h, so the residuals cancel across keys as they do under one"""
    keys, items, handles, indices = mixed
    beta, _, _ = indices[0].srs_trapdoor()
    assert indices[1].srs_trapdoor()[0] == beta
    A, B = items[0][1], items[4][1]
    assert items[0][0] == XOR and items[4][0] == ADD
    zA, zB = handles[0].scalars()["beta"], handles[4].scalars()["beta"]

    def w_beta(p):
        return _decompress(p[len(p) - OFF_W_BETA:len(p) - OFF_W_BETA + 48])

    def with_w_beta(p, W):
        return p[:len(p) - OFF_W_BETA] + _compress(W) + p[len(p) - OFF_W_BETA + 48:]
    D = cm.ec_mul(5, cm.G1_377, Q)
    k = (zA - beta) * pow(zB - beta, -1, R) % R
    kD = cm.ec_mul(k, D, Q)
    WA, WB = w_beta(A), w_beta(B)
    WA2, WB2 = cm.ec_add(WA, D, Q), cm.ec_add(WB, (kD[0], Q - kD[1]), Q)
    A2, B2 = with_w_beta(A, WA2), with_w_beta(B, WB2)
    neg = lambda P: (P[0], Q - P[1])      # noqa: E731
    resA = cm.ec_mul((beta - zA) % R, cm.ec_add(WA2, neg(WA), Q), Q)
    resB = cm.ec_mul((beta - zB) % R, cm.ec_add(WB2, neg(WB), Q), Q)
    assert resA is not None and resB is not None and cm.ec_add(resA, resB, Q) is None
    assert keys[XOR].verify(A, b"") and keys[ADD].verify(B, b"")
    assert keys[XOR].verify(A2, b"") is False and keys[ADD].verify(B2, b"") is False
    assert api.verify_batch_keys(keys, [XOR, ADD], [A2, B2], [b"", b""], device=False) == [False, False]
    assert api.verify_batch_keys(keys, [XOR, ADD, XOR], [A2, B2, items[1][1]], [b""] * 3, device=False) == [False, False, True]


# ---- segment rows ------------------------------------------------------------------------------------------------------------------------------------------------------
def segment_row(s, n, c, iv, aad, ct, tag, coms, mask, revealed):
    """the layout of capi_host.cpp gcm_segment_public_input, every byte LSB first: iv and ctr0 = 2 + s c (big endian); the aad (head); the segment's ciphertext; the
    length block and the tag (tail); commitments[s - 1] (not the head) and commitments[s] (not the tail); with a mask the segment's slice of it and of the revealed bytes"""
    lo = 16 * c * s
    seg = ct[lo:] if s == n - 1 else ct[lo:lo + 16 * c]
    parts = [iv + (2 + s * c).to_bytes(4, "big")]
    if s == 0:
        parts.append(aad)
    parts.append(seg)
    if s == n - 1:
        parts += [(8 * len(aad)).to_bytes(8, "big") + (8 * len(ct)).to_bytes(8, "big"), tag]
    if s > 0:
        parts.append(coms[s - 1])
    if s < n - 1:
        parts.append(coms[s])
    if mask is not None:
        parts += [mask[lo // 8:lo // 8 + (len(seg) + 7) // 8], revealed[lo:lo + len(seg)]]
    return _bits(b"".join(parts))


@pytest.mark.parametrize("c", [1, 2])
@pytest.mark.parametrize("length", [39, 65])
@pytest.mark.parametrize("aad_len", [0, 13])
@pytest.mark.parametrize("with_mask", [False, True])
def test_gcm_segment_rows(api, c, length, aad_len, with_mask):
    from conftest import mt_bytes
    iv, aad, ct, tag = mt_bytes(12, 41), mt_bytes(aad_len, 42), mt_bytes(length, 43), mt_bytes(16, 44)
    n = ((length + 15) // 16 + c - 1) // c
    coms = [mt_bytes(32, 50 + s) for s in range(n - 1)]
    mask = revealed = None
    if with_mask:                                         # bytes on both sides of every segment boundary, and the record's last byte
        opened = sorted({i for b in range(16 * c, length, 16 * c) for i in (b - 1, b, b + 1) if i < length} | {length - 1})
        mask = api.reveal_mask(opened, length)
        revealed = api.reveal_bytes(mt_bytes(length, 45), mask)
    rows, roles = api.gcm_segment_public_inputs(n, iv, aad, ct, tag, coms, c, mask=mask, revealed=revealed)
    assert roles == ["head"] + ["mid"] * (n - 2) + ["tail"]
    want = [segment_row(s, n, c, iv, aad, ct, tag, coms, mask, revealed) for s in range(n)]
    assert [len(r) for r in rows] == [len(w) for w in want]
    assert rows == want
    lt = length - 16 * c * (n - 1)
    rv = lambda nbytes: 8 * ((nbytes + 7) // 8) + 8 * nbytes if with_mask else 0      # noqa: E731
    assert len(rows[0]) == 128 + 8 * aad_len + 128 * c + 256 + rv(16 * c)              # the counts verify_gcm_segments pins the keys to
    assert len(rows[-1]) == 128 + 8 * lt + 128 + 128 + 256 + rv(lt)
    assert all(len(r) == 128 + 128 * c + 512 + rv(16 * c) for r in rows[1:-1])


def test_gcm_segment_rows_refuse_what_verify_gcm_segments_refuses(api):
    from conftest import mt_bytes
    vk = api.VerifyingKey.from_bytes(open(os.path.join(GOLD, "gpu_aes16_vk.bin"), "rb").read())      # any key: the lengths and counts are checked before the keys
    iv, aad, ct, tag = mt_bytes(12, 41), mt_bytes(13, 42), mt_bytes(39, 43), mt_bytes(16, 44)
    coms = [mt_bytes(32, 50 + s) for s in range(4)]

    def both(n, ct_, coms_, c, mask=None, revealed=None):
        msgs = []
        for call in (lambda: api.gcm_segment_public_inputs(n, iv, aad, ct_, tag, coms_, c, mask=mask, revealed=revealed),
                     lambda: api.verify_gcm_segments((vk, vk, vk), [b""] * n, iv, aad, ct_, tag, coms_, c, mask=mask, revealed=revealed)):
            with pytest.raises(api.ZkAesError) as e:
                call()
            msgs.append(str(e.value))
        assert msgs[0] == msgs[1].replace("verify_gcm_segments_reveal", "gcm_segment_public_inputs")
        return msgs[0]
    assert "has 3 segments of 1 blocks" in both(2, ct, coms[:1], 1)
    assert "96 bytes for this record" not in both(3, ct, coms[:1], 1) and "64 bytes for this record" in both(3, ct, coms[:1], 1)
    assert "fits one segment" in both(1, ct[:16], [], 1)
    assert "fits one segment" in both(1, ct, [], 3)
    assert "at least one block" in both(3, ct, coms[:2], 0)
    assert "at least one block" in both(3, b"", coms[:2], 1)
    assert "a mask over 39 bytes has 5 bytes" in both(3, ct, coms[:2], 1, mask=bytes(4), revealed=bytes(39))
    assert "mask bit is 0" in both(3, ct, coms[:2], 1, mask=bytes(5), revealed=bytes(38) + b"\x01")


# ---- sanitizer build ---------------------------------------------------------------------------------------------------------------------------------------------------
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
BATCHES = 10_000


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang")
def test_mutated_multi_key_batches_under_asan_ubsan():
    """A stand-alone program over the host-only sources, built with -fsanitize=address,undefined exactly as test_verify_batch_host.py builds its own, feeds 10^4 mutated
    batches of the golden proof x 3 under two handles of the golden key through zkaes_verify_batch_keys in exactly sized heap buffers.  Any sanitizer report, any accepted
    row that is not the golden statement, any rejected golden row and any key index out of range that is not refused fails it."""
    from aes_zero_knowledge_proof_circuit_amd.build import HOST_ONLY_SOURCES
    out = os.path.join(CSRC, "build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "verify_batch_keys_host_check")
    sources = [os.path.join(ROOT, "tests", "verify_batch_keys_host_check.cpp")] + [os.path.join(CSRC, f) for f in HOST_ONLY_SOURCES]
    deps = sources + [os.path.join(CSRC, h) for h in ("marlin.hpp", "marlin_host.hpp", "capi_common.hpp", "pairing.hpp", "transcript.hpp", "ff.cuh", "ec.cuh", "circuit.hpp", "fq_sqrt.cuh", "verify_batch.hpp",
                                                      "statement.hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call([CLANG, "-x", "c++", "-O2", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined", "-mllvm", "-asan-globals=0", "-I", CSRC,
                               "-fsanitize=address,undefined"] + sources + ["-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    procs = max(1, min(8, os.cpu_count() or 1))
    per = -(-BATCHES // procs)
    ps = [subprocess.Popen([exe, GOLD, str(per), str(seed)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for seed in range(1, procs + 1)]
    total = 0
    for p in ps:
        out_, err = p.communicate(timeout=1500)
        assert p.returncode == 0, "sanitizer report or finding:\n" + (err or out_)[-4000:]
        line = [ln for ln in out_.splitlines() if ln.startswith("verify_batch_keys_host_check:")][-1]
        total += int(line.split(" batches ok")[0].split()[-1])
    assert total >= BATCHES
