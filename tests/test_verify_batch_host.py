"""The batch verifier's host back end (zkaes_verify_batch) against the per-proof verifier, the committed GPU-made fixture, a forgery that only the
randomizers catch, a Python restatement of the chunked public-input layout, and a sanitizer build fed with mutated batches.  No GPU."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CSRC = os.path.join(ROOT, "aes_zero_knowledge_proof_circuit_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import curve_math as cm  # noqa: E402

SMALL_SRS = (200, 200, 600)
Q, R = cm.Q377, cm.R377
# byte offsets from the END of a serialized proof (marlin_codec.cpp serialize_proof): ... evals | u64 3, 3 x None | u64 2 | W_beta 48, tag, random_v 32 | W_gamma 48, tag | tag
OFF_W_BETA, OFF_RANDOM_V, OFF_W_GAMMA = 131, 82, 50
OFF_EVALS = 131 + 8 + 3 + 8 + 4 * 32


def per_proof(api, vk, proof, bits):
    """the per-proof verifier's answer; bytes it refuses to parse are a rejection"""
    try:
        return vk.verify(proof, bits)
    except api.ZkAesError:
        return False


@pytest.fixture(scope="module")
def xor_batch(zko, api):
    """seven valid oracle proofs of the XOR circuit, distinct inputs and seeds, under one key; made once and never modified"""
    from test_marlin_cpu import vk_for
    cs, _ = zko.synth_ops("xor", 0, 0, field=377)
    ix = zko.Index(cs, srs=SMALL_SRS)
    vk = vk_for(api, zko, ix, 0)
    proofs, handles = [], []
    for i in range(7):
        cs, _ = zko.synth_ops("xor", 0x1000 + 977 * i, 0xBEEF ^ (31 * i), field=377)
        p = ix.prove(cs, bytes([i + 1] * 32))
        handles.append(p)
        proofs.append(p.to_bytes())
    assert len(set(proofs)) == 7
    return ix, vk, proofs, handles


@pytest.mark.parametrize("n", [1, 2, 7])
def test_valid_batches_agree_with_the_per_proof_verifier(api, xor_batch, n):
    _, vk, proofs, _ = xor_batch
    want = [per_proof(api, vk, p, b"") for p in proofs[:n]]
    assert want == [True] * n
    assert api.verify_batch(vk, proofs[:n], [b""] * n, device=False) == want
    assert vk.verify_batch(proofs[:n], [b""] * n, device=False) == want


def _damage(proof, kind):
    bad = bytearray(proof)
    if kind == "eval":
        bad[len(proof) - OFF_EVALS + 32] ^= 1
    elif kind == "random_v":
        bad[len(proof) - OFF_RANDOM_V] ^= 1
    else:
        return bytes(proof[:-7])
    return bytes(bad)


@pytest.mark.parametrize("kind", ["eval", "random_v", "truncated"])
@pytest.mark.parametrize("pos", [0, 3, 6])
def test_damaged_batches_agree_with_the_per_proof_verifier(api, xor_batch, kind, pos):
    _, vk, proofs, _ = xor_batch
    batch = list(proofs)
    batch[pos] = _damage(proofs[pos], kind)
    want = [i != pos for i in range(7)]
    assert [per_proof(api, vk, p, b"") for p in batch] == want
    assert api.verify_batch(vk, batch, [b""] * 7, device=False) == want      # a truncated proof is a rejection, not an exception


def _bits(data):
    return bytes((b >> k) & 1 for b in data for k in range(8))


def test_golden_fixture_rows(api, vectors):
    vk = api.VerifyingKey.from_bytes(open(os.path.join(GOLD, "gpu_aes16_vk.bin"), "rb").read())
    proof = open(os.path.join(GOLD, "gpu_aes16_proof.bin"), "rb").read()
    good, wrong = _bits(bytes(vectors["ciphertext"])), _bits(bytes(vectors["wrong_ciphertext_16"]))
    assert api.verify_batch(vk, [proof] * 3, [good, good, wrong], device=False) == [True, True, False]      # a 128-bit public input; the same proof twice
    assert api.verify_batch(vk, [proof], [good[:-1]], device=False) == [False]                              # 127 bits pad to |X| = 128, not the key's 256


def _decompress(b48):
    x = int.from_bytes(b48, "little")
    gt = bool(x >> 383)
    x &= (1 << 382) - 1
    y = cm.fp_sqrt((x * x * x + 1) % Q, Q)
    assert y is not None
    if (y > Q - y) != gt:
        y = Q - y
    return (x, y)


def _compress(P):
    x, y = P
    return (x | ((1 << 383) if y > Q - y else 0)).to_bytes(48, "little")


def test_randomizers_matter(api, xor_batch):
    """Two proofs whose beta-openings are shifted against each other so that the UNWEIGHTED sum of their two checks still balances: the opening proofs are not absorbed
    by the transcript, so nothing else about the proofs changes.  Only weights the forger could not predict separate them."""
    ix, vk, proofs, handles = xor_batch
    beta, _, _ = ix.srs_trapdoor()
    A, B = proofs[0], proofs[1]
    zA, zB = handles[0].scalars()["beta"], handles[1].scalars()["beta"]

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
    # the model: a valid proof satisfies (beta - z) W = E for its own E; the forged pair's residuals (beta - z)(W' - W) are non-zero each and cancel in the equal-weights sum
    neg = lambda P: (P[0], Q - P[1])      # noqa: E731
    resA = cm.ec_mul((beta - zA) % R, cm.ec_add(WA2, neg(WA), Q), Q)
    resB = cm.ec_mul((beta - zB) % R, cm.ec_add(WB2, neg(WB), Q), Q)
    assert resA is not None and resB is not None and cm.ec_add(resA, resB, Q) is None
    assert vk.verify(A, b"") and vk.verify(B, b"")
    assert vk.verify(A2, b"") is False and vk.verify(B2, b"") is False
    assert api.verify_batch(vk, [A2, B2], [b"", b""], device=False) == [False, False]
    assert api.verify_batch(vk, [A2, B2, proofs[2]], [b""] * 3, device=False) == [False, False, True]


def _counter_add(icb, n):
    return ((int.from_bytes(icb, "big") + n) % (1 << 128)).to_bytes(16, "big")


def _row(circuit, api, j, chunk, ct, header, key_tag, states):
    """the documented layout: every byte LSB first; the mode header, the chunk's ciphertext, the tag, (H_in, H_out)"""
    parts = []
    if circuit == api.CIRCUIT_AES_CBC:
        parts.append(header if j == 0 else ct[chunk * j - 16:chunk * j])
    if circuit == api.CIRCUIT_AES_CTR:
        parts.append(_counter_add(header, j * (chunk // 16)))
    parts.append(ct[chunk * j:chunk * (j + 1)])
    if key_tag is not None:
        parts.append(key_tag)
    if states is not None:
        parts += [states[j], states[j + 1]]
    return _bits(b"".join(parts))


@pytest.mark.parametrize("mode", ["ecb", "cbc", "ctr"])
@pytest.mark.parametrize("extras", ["plain", "tag", "tag+states", "states"])
def test_chunk_public_input_rows(api, mode, extras):
    from conftest import mt_bytes
    circuit = {"ecb": api.CIRCUIT_AES, "cbc": api.CIRCUIT_AES_CBC, "ctr": api.CIRCUIT_AES_CTR}[mode]
    n, chunk = 3, 32
    ct = mt_bytes(n * chunk, 11)
    header = None if mode == "ecb" else bytes([0xff] * 15 + [0xfe])           # (a counter whose low byte carries at j = 1)
    tag = mt_bytes(32, 12) if "tag" in extras else None
    states = [mt_bytes(32, 20 + i) for i in range(n + 1)] if "states" in extras else None
    rows = api.chunk_public_inputs(circuit, ct, header=header, key_tag=tag, states=states, n_chunks=n)
    assert rows == [_row(circuit, api, j, chunk, ct, header, tag, states) for j in range(n)]


def test_chunk_rows_feed_the_same_statement_as_the_chunked_verifier(api, vectors):
    vk = api.VerifyingKey.from_bytes(open(os.path.join(GOLD, "gpu_aes16_vk.bin"), "rb").read())
    proof = open(os.path.join(GOLD, "gpu_aes16_proof.bin"), "rb").read()
    for ct in (bytes(vectors["ciphertext"]), bytes(vectors["wrong_ciphertext_16"])):
        (row,) = api.chunk_public_inputs(api.CIRCUIT_AES, ct)
        assert row == _bits(ct)
        assert vk.verify(proof, row) == api.verify_encryption(vk, proof, ct)
        assert api.verify_chunked_batch(vk, api.CIRCUIT_AES, [proof], ct, device=False) == [api.verify_encryption(vk, proof, ct)]


CLANG = "/opt/rocm/lib/llvm/bin/clang++"
BATCHES = 10_000


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang")
def test_mutated_batches_under_asan_ubsan():
    """A stand-alone program over the host-only sources, built with -fsanitize=address,undefined (flags of test_fuzz_host.py; -asan-globals=0: this toolchain's ASan
    trips over its own registration of merged string literals before main() runs), feeds 10^4 mutated batches of the golden proof x 3 through zkaes_verify_batch in
    exactly sized heap buffers.  Any sanitizer report, any accepted row that is not the golden statement and any rejected golden row fails it."""
    from aes_zero_knowledge_proof_circuit_amd.build import HOST_ONLY_SOURCES
    out = os.path.join(CSRC, "build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "verify_batch_host_check")
    sources = [os.path.join(ROOT, "tests", "verify_batch_host_check.cpp")] + [os.path.join(CSRC, f) for f in HOST_ONLY_SOURCES]
    deps = sources + [os.path.join(CSRC, h) for h in ("marlin.hpp", "marlin_host.hpp", "capi_common.hpp", "pairing.hpp", "transcript.hpp", "ff.cuh", "ec.cuh", "circuit.hpp", "fq_sqrt.cuh", "verify_batch.hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call([CLANG, "-x", "c++", "-O2", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined", "-mllvm", "-asan-globals=0", "-I", CSRC,
                               "-fsanitize=address,undefined"] + sources + ["-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    procs = max(1, min(8, os.cpu_count() or 1))                  # one program, the batches split over seeds as test_fuzz_host.py splits its cases
    per = -(-BATCHES // procs)
    ps = [subprocess.Popen([exe, GOLD, str(per), str(seed)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for seed in range(1, procs + 1)]
    total = 0
    for p in ps:
        out_, err = p.communicate(timeout=1500)
        assert p.returncode == 0, "sanitizer report or finding:\n" + (err or out_)[-4000:]
        line = [ln for ln in out_.splitlines() if ln.startswith("verify_batch_host_check:")][-1]
        total += int(line.split(" batches ok")[0].split()[-1])
    assert total >= BATCHES
