"""GCM segments on the host: the model's cut GHASH chain against the lone GCM model and the published vectors, the commitment against the host's
SHA-256, the segment circuits' counts against closed forms and an independent count of the commitment's compression, the capacity table over the default SRS, the lone
GCM circuit unchanged, the three new kernels' source run lane by lane under sanitizers, and the host-only entries under sanitizers (no GPU, no oracle).

A GCM record that does not fit one proof is proven as n >= 2 segment-proofs (head, mid ..., tail), chained by salted commitments to (key, Y) that are public input on
both sides of every boundary; the conjunction of the n proofs is the lone GCM statement for the whole record.
"""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import gcm_segment_model as model
import sha256_model
from test_cbc_host import CLANG, CSRC, GOLD, ROOT
from test_gcm_host import COUNTS, TC3_CT, TC3_IV, TC3_KEY, TC3_PT, TC4_AAD, VECTORS, model_gcm

# the largest c per role whose |H| and |K| stay inside the default SRS literal (866_944, 513, 4_062_064: |H| <= 2^22, |K| <= 2^22), measured through circuit_info and
# the joint matrix; (joint non-zeros at that c, at c + 1).  DESIGN.md 9g has the table
CAPACITY = {
    128: {("head", 0): (5, 4_127_750, 4_785_515), ("head", 13): (5, 4_186_778, 4_844_543), ("mid", 0): (4, 3_581_221, 4_238_966), ("tail", 0): (4, 4_126_607, 4_784_352)},
    192: {("head", 0): (4, 4_031_146, 4_806_677), ("head", 13): (4, 4_090_652, 4_866_183), ("mid", 0): (4, 4_142_984, 4_918_515), ("tail", 0): (3, 4_029_579, 4_805_158)},
    256: {("head", 0): (3, 3_792_165, 4_683_919), ("head", 13): (3, 3_851_579, 4_743_333), ("mid", 0): (3, 3_904_625, 4_796_379), ("tail", 0): (2, 3_790_719, 4_682_445)},
}


@pytest.mark.parametrize("tc", [2, 3])
@pytest.mark.parametrize("c", [1, 2, 3])
def test_cut_chain_gives_the_published_tag(tc, c):
    """McGrew-Viega test cases 3 and 4 as segments of c blocks: ciphertext and tag are the published ones, for every cut that leaves at least two segments"""
    key, iv, pt, aad, ct, tag = VECTORS[tc]
    got_ct, got_tag, ys = model.segmented_gcm(pt, key, iv, aad, c)
    assert (got_ct, got_tag) == (ct, tag) and len(ys) == model.plan(len(pt), c)[0] - 1 >= 1


@pytest.mark.parametrize("alen", [0, 5, 20])
@pytest.mark.parametrize("length", [17, 32, 39, 64, 65])
def test_cut_chain_at_every_block_boundary(api, length, alen):
    """the GHASH chain cut at every block boundary (c = 1), and at c = 2 and 3, with the public length block last, equals model_gcm's tag; the host's boundaries are the
    model's"""
    rs = np.random.RandomState(0x5E6 + 64 * length + alen)
    msg, key, iv, aad = rs.bytes(length), rs.bytes(16), rs.bytes(12), rs.bytes(alen)
    want = model_gcm(msg, key, iv, aad)
    for c in (1, 2, 3):
        if model.plan(length, c)[0] < 2:
            continue
        ct, tag, ys = model.segmented_gcm(msg, key, iv, aad, c)
        assert (ct, tag) == want
        assert api.gcm_boundaries(msg, key, iv, aad, c) == ys
    assert api.gcm_encrypt(msg, key, iv, aad) == want


@pytest.mark.parametrize("key_bytes", [16, 24, 32])
def test_commitment_is_one_compression(api, key_bytes):
    rs = np.random.RandomState(0xC0 + key_bytes)
    key, y, salt = rs.bytes(key_bytes), rs.bytes(16), rs.bytes(16)
    block = key + bytes(32 - key_bytes) + y + salt
    want = sha256_model.compress(sha256_model.IV, block)
    assert model.commitment(key, y, salt) == want == api.sha256_chain(block) == api.gcm_commit(key, y, salt)
    assert api.gcm_commit(key, y, bytes(16)) != want and api.gcm_commit(key, bytes(16), salt) != want
    for bad in ((key[:15], y, salt), (key, y[:15], salt), (key, y, salt + b"\0")):
        with pytest.raises(api.ZkAesError):
            api.gcm_commit(*bad)


def test_plan(api):
    p = api.gcm_segment_plan(39, 5, 1)
    assert p["n"] == 3 and p["tail_bytes"] == 7 and [s["role"] for s in p["segments"]] == ["head", "mid", "tail"] and [s["ctr0"] for s in p["segments"]] == [2, 3, 4]
    p = api.gcm_segment_plan(60, 20, 2)
    assert p["n"] == 2 and p["tail_bytes"] == 28 and [s["offset"] for s in p["segments"]] == [0, 32]
    p = api.gcm_segment_plan(16384, 13)                                                            # a full TLS record at the default c = 4: 256 segments
    assert p["c"] == 4 == api.GCM_SEGMENT_DEFAULT_C[128] and p["n"] == 256 and p["tail_bytes"] == 64
    assert api.gcm_segment_plan(65, 0)["n"] == 2 and api.gcm_segment_plan(65, 0)["tail_bytes"] == 1
    for bad in ((64, 0, 4), (16, 0, 1), (0, 0, 1), ((1 << 20) + 1, 0, 4), (100, 1 << 17, 4), (100, 0, 0)):
        with pytest.raises(api.ZkAesError):
            api.gcm_segment_plan(*bad)


def _ecb(api, bits):
    cache = {}

    def info(blocks):
        if blocks not in cache:
            i = api.circuit_info(api.CIRCUIT_AES, 16 * blocks, 0, bits)
            cache[blocks] = (int(i["raw_constraints"]), int(i["raw_witness"]))
        return cache[blocks]
    return info


@pytest.mark.parametrize("bits", [128, 256])
def test_closed_form_counts(api, bits):
    """rows, instance and witnesses per role at c = 1, 2 and the default c (a tail at 16 c bytes, and ragged), against gcm_segment_model.segment_size"""
    dc = api.GCM_SEGMENT_DEFAULT_C[bits]
    ecb = _ecb(api, bits)
    shapes = [(role, c, a) for c in sorted({1, 2, dc}) for role, a in (("head", 0), ("head", 13), ("mid", 0))]
    shapes += [("tail", units, 0) for units in sorted({7, 16, 32, 16 * dc, 16 * dc - 9})]
    for role, units, a in shapes:
        got = api.circuit_info_gcm_segment(role, units, a, bits)
        want = model.segment_size(role, units, a, bits, ecb)
        print(bits, role, units, a, "->", int(got["raw_constraints"]), int(got["raw_instance"]), int(got["raw_witness"]))
        assert (got["raw_constraints"], got["raw_instance"], got["raw_witness"]) == want
        assert got["constraints"] == got["instance"] + got["witness"]                              # square after padding
    # the commitment: a compression from the constant initial value costs less than one over a block of variables from a variable state, and a short key's zero words
    # fold more of the schedule away
    sizes = [model.commitment_size(b) for b in (128, 192, 256)]
    assert sizes == [(26396, 25700), (26518, 25822), (26640, 25944)]
    assert all(rows - 512 < sha256_model.COMPRESSION_ROWS for rows, _ in sizes)


def _joint(api, role, units, a, bits):
    seen = []
    for which in range(3):
        rowptr, col, _ = api.circuit_matrix_gcm_segment(role, units, which, a, bits)
        rows = np.repeat(np.arange(len(rowptr) - 1, dtype=np.uint64), np.diff(rowptr).astype(np.int64))
        seen.append((rows << np.uint64(32)) | col.astype(np.uint64))
    return len(np.unique(np.concatenate(seen)))


@pytest.mark.parametrize("bits", [128, 192, 256])
def test_capacity_over_the_default_srs(api, bits):
    """per role the largest c inside the default SRS literal (|K| = 2^22 is what binds; |H| stays at 2^20 or 2^21), one more block is over, and the job helper's default
    c is the minimum over the three roles.  The joint matrix is measured at the bound and one past it"""
    cap = CAPACITY[bits]
    for (role, a), (c, joint_at, joint_over) in cap.items():
        for cc, want in ((c, joint_at), (c + 1, joint_over)):
            info = api.circuit_info_gcm_segment(role, 16 * cc if role == "tail" else cc, a, bits)
            print(bits, role, a, cc, "padded rows", int(info["constraints"]), "joint non-zeros", int(info["joint_nnz"]), "|H|", int(info["h"]), "|K|", int(info["k"]))
            assert info["joint_nnz"] == want and info["h"] <= 1 << 21 and info["k"] == (1 << 22 if cc == c else 1 << 23)
        assert joint_at <= 1 << 22 < joint_over
    assert api.GCM_SEGMENT_DEFAULT_C[bits] == min(c for c, _, _ in cap.values())
    if bits == 128:                                                                                 # the query's joint count is the matrices' own
        assert _joint(api, "mid", 1, 0, 128) == api.circuit_info_gcm_segment("mid", 1)["joint_nnz"] == 1_607_898


def test_lone_gcm_circuit_is_unchanged(api):
    """compile_aes_gcm_circuit shares the V table and the multiplication rows with the segment compiler: its figures of DESIGN.md 9c stay what they were"""
    for shape in ((17, 5), (64, 0)):
        c = api.circuit_info(api.CIRCUIT_AES_GCM, *shape)
        want = COUNTS[shape]
        assert (c["raw_constraints"], c["raw_instance"], c["raw_witness"]) == want[:3] and (c["nnz_a"], c["nnz_b"], c["nnz_c"]) == want[3]


def test_refusals(api):
    with pytest.raises(api.ZkAesError):
        api.circuit_info_gcm_segment("body", 1)
    for role, units, a in (("head", 0, 0), ("tail", 0, 0), ("mid", 1, 5), ("tail", 7, 5), ("head", 1, (1 << 16) + 1)):
        with pytest.raises(api.ZkAesError):
            api.circuit_info_gcm_segment(role, units, a)
    with pytest.raises(api.ZkAesError):
        api.circuit_info_gcm_segment("mid", 1, 0, 100)
    with pytest.raises(api.ZkAesError, match="_gcm_seg"):                                          # the generic queries have no role to give
        api.circuit_info(api.CIRCUIT_AES_GCM_SEG, 16)
    with pytest.raises(api.ZkAesError, match="no HIP device|role"):
        api.synthesize_keys(16, circuit=api.CIRCUIT_AES_GCM_SEG)


def test_segment_kernels_on_host_under_sanitizers():
    """k_aes_trace_gcm_seg and k_ghash_trace_seg (csrc/kernels_witness.cuh), k_commit_trace (csrc/kernels_digest.cuh) and k_witness_expand -- the very headers the library
    compiles for the device -- compiled for the host and run lane by lane under ASan + UBSan (tests/gcm_segment_trace_emu.cpp, a stand-alone program: nothing is loaded
    into python), over the shapes listed there, two proofs per launch"""
    wit = open(os.path.join(CSRC, "kernels_witness.cuh")).read()
    dig = open(os.path.join(CSRC, "kernels_digest.cuh")).read()
    assert "k_aes_trace_gcm_seg" in wit and "k_ghash_trace_seg" in wit and "k_witness_expand" in wit and "k_commit_trace" in dig
    for word in ("atomic", "__shared__", "__syncthreads", "__shfl", "hipLaunch"):                   # one writer per byte needs no atomics; no LDS, barrier or cross-lane operation
        assert word not in wit and word not in dig
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "gcm_segment_trace_emu")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wno-unknown-pragmas", "-I", CSRC, "-I", os.path.join(ROOT, "tests"),
                               os.path.join(ROOT, "tests", "gcm_segment_trace_emu.cpp")] + [os.path.join(CSRC, f) for f in ("circuit.cpp", "marlin_codec.cpp", "capi_host.cpp")] + ["-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=1800)
        assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
        print(out.stdout)
        assert out.stdout.splitlines()[-1] == "total bad 0"
        assert out.stdout.count("unsatisfied 0, instance mismatches 0,") == 14 and "wrap: unsatisfied 0, mismatches 0" in out.stdout


def test_host_entry_points_under_sanitizers():
    """tests/gcm_segment_host_check.cpp with the three host-only sources under -fsanitize=address,undefined: boundaries and commitments into exactly sized buffers, the
    circuit queries, and the committed ECB fixture proof -- whole, truncated at every length, garbage -- through zkaes_verify_gcm_segments with a short commitments array:
    never accepted.  A stand-alone program: nothing is loaded into python."""
    cxx = CLANG if os.path.exists(CLANG) else "g++"
    srcs = [os.path.join(ROOT, "tests", "gcm_segment_host_check.cpp")] + [os.path.join(CSRC, f) for f in ("circuit.cpp", "marlin_codec.cpp", "capi_host.cpp")]
    flags = ["-x", "c++", "-O1", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC]
    if cxx == CLANG:
        flags += ["-mllvm", "-asan-globals=0"]        # (as tests/test_fuzz_host.py: this toolchain's ASan trips over its own registration of merged string literals)
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "gcm_segment_host_check")
        subprocess.check_call([cxx] + flags + srcs + ["-o", exe])
        env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
        out = subprocess.run([exe, GOLD], capture_output=True, text=True, env=env, timeout=900)
        assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
        assert out.stdout.split() == ["gcm_segment_host_check", "ok"]
