"""Selective disclosure on segmented GCM records, on the host: reveal = 0 unchanged through the new queries, the closed forms of a reveal segment circuit
against the builder's counts, the capacity table over the default SRS, the reveal rows of a tail read back entry by entry, the public-input layout against a Python
restatement, the refusals and the verifier's two invalid-argument cases that need no device, and two stand-alone programs under sanitizers -- the segment kernels and
k_reveal_trace run lane by lane, and the host-only verifier (no GPU, no oracle).

A segment key synthesized with reveal = True proves, beside its role's statement of DESIGN.md 9g, revealed[i] = mask_i ? M[i] : 0 over the segment's own len bytes (16 c
for a head or mid, Lt for a tail) and exposes its slice of the record's ONE mask (ceil(len / 8) bytes), then its slice of the record's ONE revealed array (len bytes), as
the LAST public inputs: head, mid and tail together are the lone reveal statement of DESIGN.md 9i for (iv, aad, ciphertext, tag).
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import gcm_segment_reveal_model as model
from test_cbc_host import CLANG, CSRC, GOLD, ROOT

HOST_SOURCES = [os.path.join(CSRC, f) for f in ("circuit.cpp", "marlin_codec.cpp", "capi_host.cpp")]
ROLE_ID = {"head": 0, "mid": 1, "tail": 2}

# per role the largest c whose |K| stays inside the default SRS literal (866_944, 513, 4_062_064: |K| <= 2^22) WITH reveal, measured through circuit_info_gcm_segment(...,
# reveal=True); (joint non-zeros at that c, at c + 1).  The bounds are those of the plain table (tests/test_gcm_segments_host.py CAPACITY): reveal adds 42 joint
# non-zeros per message byte, 672 c.  DESIGN.md 9j has the table
CAPACITY_REVEAL = {
    128: {("head", 0): (5, 4_131_110, 4_789_547), ("head", 13): (5, 4_190_138, 4_848_575), ("mid", 0): (4, 3_583_909, 4_242_326), ("tail", 0): (4, 4_129_295, 4_787_712)},
    192: {("head", 0): (4, 4_033_834, 4_810_037), ("head", 13): (4, 4_093_340, 4_869_543), ("mid", 0): (4, 4_145_672, 4_921_875), ("tail", 0): (3, 4_031_595, 4_807_846)},
    256: {("head", 0): (3, 3_794_181, 4_686_607), ("head", 13): (3, 3_853_595, 4_746_021), ("mid", 0): (3, 3_906_641, 4_799_067), ("tail", 0): (2, 3_792_063, 4_684_461)},
}
ROLE_SHAPES = [("head", 1, 13), ("mid", 1, 0), ("tail", 7, 0)]


def test_reveal_zero_is_the_plain_query(api):
    """the _rv queries at reveal = 0 answer element for element what zkaes_circuit_info_gcm_seg and zkaes_circuit_matrix_gcm_seg answer, for the three roles"""
    L = api.lib()
    for role, units, a in ROLE_SHAPES + [("head", 2, 0), ("tail", 17, 0)]:
        plain, rv = (C.c_uint64 * 12)(), (C.c_uint64 * 12)()
        assert L.zkaes_circuit_info_gcm_seg(ROLE_ID[role], C.c_uint(128), C.c_size_t(units), C.c_size_t(a), plain) == 0
        assert L.zkaes_circuit_info_gcm_seg_rv(ROLE_ID[role], C.c_uint(128), C.c_uint(0), C.c_size_t(units), C.c_size_t(a), rv) == 0
        assert list(plain) == list(rv)
        assert api.circuit_info_gcm_segment(role, units, a, reveal=False) == api.circuit_info_gcm_segment(role, units, a) == dict(zip(api.circuit_info_gcm_segment(role, units, a), plain))
    for role, units, a in ROLE_SHAPES:
        for which in range(3):
            rows, nnz = C.c_uint64(), C.c_uint64()
            head = (ROLE_ID[role], C.c_uint(128), C.c_size_t(units), C.c_size_t(a), which)
            assert L.zkaes_circuit_matrix_gcm_seg(*head, C.byref(rows), C.byref(nnz), None, None, None) == 0
            rowptr, col, coeff = np.zeros(rows.value + 1, np.uint32), np.zeros(nnz.value, np.uint32), np.zeros(nnz.value, np.int64)
            assert L.zkaes_circuit_matrix_gcm_seg(*head, None, None, rowptr.ctypes.data_as(C.c_void_p), col.ctypes.data_as(C.c_void_p), coeff.ctypes.data_as(C.c_void_p)) == 0
            got = api.circuit_matrix_gcm_segment(role, units, which, a, reveal=False)
            assert (got[0] == rowptr).all() and (got[1] == col).all() and (got[2] == coeff).all()
    assert api.gcm_segment_plan(16384, 13) == api.gcm_segment_plan(16384, 13, reveal=False)          # the R = 0 plan is what it was


def _ecb(api, bits):
    cache = {}

    def info(blocks):
        if blocks not in cache:
            i = api.circuit_info(api.CIRCUIT_AES, 16 * blocks, 0, bits)
            cache[blocks] = (int(i["raw_constraints"]), int(i["raw_witness"]))
        return cache[blocks]
    return info


@pytest.mark.parametrize("bits", [128, 192, 256])
def test_closed_form_counts(api, bits):
    """rows = the 9g rows + 16 ceil(len / 8) + 15 len, instance = the 9g instance + 8 ceil(len / 8) + 8 len, no witness: head, mid and tail at c = 1, 2 and the default c;
    tails at Lt = 1, 7, 16, 17 and 16 c.  Against gcm_segment_reveal_model.segment_size (the closed form) and against the builder's own R = 0 counts"""
    assert model.reveal_size(16) == (272, 144, 0) and model.reveal_size(64) == (1088, 576, 0) and model.reveal_size(1) == (31, 16, 0)
    assert model.reveal_size(7) == (121, 64, 0) and model.reveal_size(17) == (303, 160, 0)
    dc = api.GCM_SEGMENT_DEFAULT_C[bits]
    ecb = _ecb(api, bits)
    shapes = [(role, c, a) for c in sorted({1, 2, dc}) for role, a in (("head", 0), ("head", 13), ("mid", 0))]
    shapes += [("tail", units, 0) for units in sorted({1, 7, 16, 17, 32, 16 * dc})]
    for role, units, a in shapes:
        plain = api.circuit_info_gcm_segment(role, units, a, bits)
        got = api.circuit_info_gcm_segment(role, units, a, bits, reveal=True)
        want = model.segment_size(role, units, a, bits, ecb)
        length = model.segment_bytes(role, units)
        rows, inst, wits = model.reveal_size(length)
        print(bits, role, units, a, "reveal rows", rows, "instance", inst, "->", int(got["raw_constraints"]), int(got["raw_instance"]), int(got["raw_witness"]))
        assert (got["raw_constraints"], got["raw_instance"], got["raw_witness"]) == want
        assert (got["raw_constraints"], got["raw_instance"], got["raw_witness"]) == (plain["raw_constraints"] + rows, plain["raw_instance"] + inst, plain["raw_witness"] + wits)
        assert got["constraints"] == got["instance"] + got["witness"]                              # square after padding
        assert got["joint_nnz"] >= plain["joint_nnz"] + 8 * length


@pytest.mark.parametrize("bits", [128, 192, 256])
def test_capacity_over_the_default_srs_with_reveal(api, bits):
    """|K| <= 2^22 binds the segment shapes.  With reveal every entry of DESIGN.md 9g's capacity table stays inside the bound and one more block is over, for the three key
    sizes; reveal costs 42 joint non-zeros per message byte; the default c stays 4 / 3 / 2 and gcm_segment_plan(..., reveal=True) returns it"""
    import test_gcm_segments_host as plain_table
    cap = CAPACITY_REVEAL[bits]
    for (role, a), (c, joint_at, joint_over) in cap.items():
        c_plain, plain_at, plain_over = plain_table.CAPACITY[bits][(role, a)]
        assert c == c_plain and joint_at == plain_at + 42 * 16 * c and joint_over == plain_over + 42 * 16 * (c + 1)
        for cc, want in ((c, joint_at), (c + 1, joint_over)):
            info = api.circuit_info_gcm_segment(role, 16 * cc if role == "tail" else cc, a, bits, reveal=True)
            print(bits, role, a, cc, "padded rows", int(info["constraints"]), "joint non-zeros", int(info["joint_nnz"]), "|H|", int(info["h"]), "|K|", int(info["k"]))
            assert info["joint_nnz"] == want and info["h"] <= 1 << 21 and info["k"] == (1 << 22 if cc == c else 1 << 23)
        assert joint_at <= 1 << 22 < joint_over
    assert api.GCM_SEGMENT_REVEAL_DEFAULT_C[bits] == min(c for c, _, _ in cap.values()) == api.GCM_SEGMENT_DEFAULT_C[bits]
    p = api.gcm_segment_plan(16384, 13, key_bits=bits, reveal=True)
    assert p["c"] == api.GCM_SEGMENT_REVEAL_DEFAULT_C[bits] and p["n"] == api.gcm_segment_plan(16384, 13, key_bits=bits)["n"]
    assert all(s["mask_offset"] == s["offset"] // 8 and s["mask_bytes"] == (s["bytes"] + 7) // 8 for s in p["segments"])


def test_reveal_rows_of_a_tail_are_what_the_design_says(api):
    """a tail with Lt = 17: behind the R = 0 circuit's rows come 24 booleanity rows of the mask, 7 pins (mask bits 17 .. 23: A = the bit, B = One, C empty), then per
    message byte 8 booleanity rows of its revealed bits and 8 product rows with ONE entry a side: the byte's mask input in A, the message witness (witness 8 i + k: the
    message is allocated first) in B, the revealed input in C.  The R = 0 rows ahead are the plain circuit's, entry for entry"""
    n, mb = 17, 3
    plain = api.circuit_info_gcm_segment("tail", n)
    info = api.circuit_info_gcm_segment("tail", n, reveal=True)
    A, B, Cm = [api.circuit_matrix_gcm_segment("tail", n, which, reveal=True) for which in range(3)]
    r0, ri0, ni = int(plain["raw_constraints"]), int(plain["raw_instance"]), int(info["instance"])
    assert ri0 == 1 + 128 + 8 * n + 128 + 128 + 256 and info["raw_instance"] == ri0 + 8 * mb + 8 * n
    row = lambda m, r: list(zip(m[1][m[0][r]:m[0][r + 1]].tolist(), m[2][m[0][r]:m[0][r + 1]].tolist()))
    for i in range(8 * mb):                                                                          # booleanity of mask bit i: (One - b) * b = 0
        assert sorted(row(A, r0 + i) + row(B, r0 + i)) == sorted([(0, 1), (ri0 + i, -1), (ri0 + i, 1)]) and row(Cm, r0 + i) == []
    for i in range(n, 8 * mb):
        r = r0 + 8 * mb + (i - n)
        assert row(A, r) == [(ri0 + i, 1)] and row(B, r) == [(0, 1)] and row(Cm, r) == []
    at = r0 + 8 * mb + (8 * mb - n)
    for i in range(n):
        for k in range(8):
            r = at + 16 * i + 8 + k
            assert row(A, r) == [(ri0 + i, 1)] and row(B, r) == [(ni + 8 * i + k, 1)] and row(Cm, r) == [(ri0 + 8 * mb + 8 * i + k, 1)]
    assert at + 16 * n == info["raw_constraints"]
    # same instance padding (1024), so the witness columns do not move and the R = 0 rows are the plain circuit's own
    assert info["instance"] == plain["instance"]
    for which, m in enumerate((A, B, Cm)):
        p = api.circuit_matrix_gcm_segment("tail", n, which)
        end = int(p[0][r0])
        assert (m[0][:r0 + 1] == p[0][:r0 + 1]).all() and (m[1][:end] == p[1][:end]).all() and (m[2][:end] == p[2][:end]).all()


def test_public_input_layout(api):
    """the Python restatement of a segment's public input (gcm_segment_reveal_model.public_input) has the builder's instance count for every role, its R = 0 part is the
    plain restatement, and its last 8 ceil(len / 8) + 8 len bits are the statement layer's slices of ONE mask and ONE revealed array: a 39-byte record at c = 1 under a
    mask that opens bytes 14 .. 18, across the head / mid boundary, and byte 38"""
    rs = np.random.RandomState(0x9A)
    msg, iv, aad, tag = rs.bytes(39), rs.bytes(12), rs.bytes(13), rs.bytes(16)
    ct, coms = rs.bytes(39), [rs.bytes(32), rs.bytes(32)]
    mask = api.reveal_mask([range(14, 19), 38], 39)
    assert mask == model.mask_of(list(range(14, 19)) + [38], 39) == bytes([0, 0xc0, 0x07, 0, 0x40])
    revealed = api.reveal_bytes(msg, mask)
    assert revealed == model.revealed_of(msg, mask)
    cuts = model.slices(mask, revealed, 39, 1)
    assert cuts == [(mask[0:2], revealed[0:16]), (mask[2:4], revealed[16:32]), (mask[4:5], revealed[32:39])]
    assert b"".join(r for _, r in cuts) == revealed and b"".join(m for m, _ in cuts) == mask          # the slices tile the record: one statement
    for s, (role, units, a) in enumerate(ROLE_SHAPES):
        plain = model.public_input(s, 3, 1, iv, aad, ct, tag, coms)
        full = model.public_input(s, 3, 1, iv, aad, ct, tag, coms, mask, revealed)
        assert len(plain) + 1 == api.circuit_info_gcm_segment(role, units, a)["raw_instance"]
        assert len(full) + 1 == api.circuit_info_gcm_segment(role, units, a, reveal=True)["raw_instance"]
        assert full[:len(plain)] == plain and full[len(plain):] == model.bits(cuts[s][0]) + model.bits(cuts[s][1])
    plan = api.gcm_segment_plan(39, 13, 1, reveal=True)
    assert [(s["mask_offset"], s["mask_bytes"]) for s in plan["segments"]] == [(0, 2), (2, 2), (4, 1)]
    assert len(api.gcm_segment_header(iv, 3, mask=cuts[1][0])) == 80 + 2 and api.gcm_segment_header(iv, 3, mask=cuts[1][0])[80:] == mask[2:4]
    assert api.gcm_segment_header(iv, 2, aad=aad, mask=cuts[0][0]) == api.gcm_segment_header(iv, 2, aad=aad) + mask[0:2]


def test_refusals(api):
    L = api.lib()
    out = (C.c_uint64 * 12)()
    assert L.zkaes_circuit_info_gcm_seg_rv(1, C.c_uint(128), C.c_uint(2), C.c_size_t(1), C.c_size_t(0), out) != 0
    assert b"reveal must be 0 or 1" in L.zkaes_last_error()
    rows, nnz = C.c_uint64(), C.c_uint64()
    assert L.zkaes_circuit_matrix_gcm_seg_rv(1, C.c_uint(128), C.c_uint(2), C.c_size_t(1), C.c_size_t(0), 0, C.byref(rows), C.byref(nnz), None, None, None) != 0
    for role, units, a in (("head", 0, 0), ("tail", 0, 0), ("mid", 1, 5), ("tail", 7, 5)):           # the segment compiler's own refusals stand
        with pytest.raises(api.ZkAesError):
            api.circuit_info_gcm_segment(role, units, a, reveal=True)
    with pytest.raises(api.ZkAesError, match="no HIP device|role"):
        api.synthesize_keys_gcm_segment("body", 1, reveal=True)
    with pytest.raises(api.ZkAesError, match="_gcm_seg"):                                          # the generic query still has no role to give
        api.circuit_info(6, 16, reveal=True)


def test_verifier_refuses_the_two_invalid_arguments_and_the_other_kind(api):
    """a mask bit at or beyond L and a non-zero revealed byte under a zero mask bit RAISE in verify_gcm_segments(..., mask=, revealed=) whatever the keys; a mask or a
    revealed array of the wrong length raises; and the committed ECB proof, a proof of a key without reveal, is never accepted: the stored key knows its public-input
    count and raises, the transported key (|X| alone) rejects"""
    vk = api.VerifyingKey.from_bytes(open(os.path.join(GOLD, "gpu_aes16_vk.bin"), "rb").read())
    ark = api.VerifyingKey.from_ark_bytes(vk.to_ark_bytes())
    proof = open(os.path.join(GOLD, "gpu_aes16_proof.bin"), "rb").read()
    iv, tag, coms, ct = bytes(range(12)), bytes(16), [bytes(32)], bytes(range(1, 18))
    for keys in ((vk, None, vk), (ark, None, ark)):
        call = lambda mask, revealed: api.verify_gcm_segments(keys, [proof, proof], iv, b"", ct, tag, coms, 1, mask=mask, revealed=revealed)
        with pytest.raises(api.ZkAesError, match="at or beyond"):
            call(bytes([0, 0, 0x02]), bytes(17))                                                   # bit 17 of a 17-byte record
        with pytest.raises(api.ZkAesError, match="mask bit is 0"):
            call(bytes([0xfe, 0xff, 0x01]), bytes([1]) + bytes(16))
        with pytest.raises(api.ZkAesError, match="mask bit is 0"):
            call(bytes(3), bytes(16) + b"\x01")                                                    # in the tail's slice
        with pytest.raises(api.ZkAesError):
            call(bytes(2), bytes(17))                                                              # a mask one byte short
        with pytest.raises(api.ZkAesError):
            call(bytes(3), bytes(16))                                                              # a revealed array one byte short
        with pytest.raises(api.ZkAesError, match="go together"):
            call(bytes(3), None)
    with pytest.raises(api.ZkAesError, match="not synthesized for this segment's lengths"):
        api.verify_gcm_segments((vk, None, vk), [proof, proof], iv, b"", ct, tag, coms, 1, mask=bytes(3), revealed=bytes(17))
    assert api.verify_gcm_segments((ark, None, ark), [proof, proof], iv, b"", ct, tag, coms, 1, mask=bytes(3), revealed=bytes(17)) == [False, False]
    assert api.verify_gcm_segments((ark, None, ark), [proof, proof], iv, b"", ct, tag, coms, 1) == [False, False]


def _signature(text, kernel):
    a = text.index("__global__ void %s(" % kernel)
    return text[a:text.index(") {", a)]


def test_segment_reveal_kernels_on_host_under_sanitizers():
    """k_aes_trace_gcm_seg and k_ghash_trace_seg (csrc/kernels_witness.cuh), k_commit_trace (csrc/kernels_digest.cuh), k_reveal_trace (csrc/kernels_reveal.cuh) and
    k_witness_expand -- the very headers the library compiles for the device -- compiled for the host and run lane by lane under ASan + UBSan
    (tests/gcm_segment_reveal_trace_emu.cpp, a stand-alone program: nothing is loaded into python), over the shapes listed there, two proofs per launch"""
    wit, dig, rev = (open(os.path.join(CSRC, "kernels_%s.cuh" % name)).read() for name in ("witness", "digest", "reveal"))
    assert "k_aes_trace_gcm_seg" in wit and "k_ghash_trace_seg" in wit and "k_witness_expand" in wit and "k_commit_trace" in dig and "k_reveal_trace" in rev
    for word in ("atomic", "__shared__", "__syncthreads", "__shfl", "hipLaunch"):                   # one writer per byte needs no atomics; no LDS, barrier or cross-lane operation
        assert word not in wit and word not in dig and word not in rev
    assert "revealed" not in _signature(rev, "k_reveal_trace")                                     # the kernel is never handed `revealed`
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "gcm_segment_reveal_trace_emu")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wno-unknown-pragmas", "-I", CSRC, "-I", os.path.join(ROOT, "tests"),
                               os.path.join(ROOT, "tests", "gcm_segment_reveal_trace_emu.cpp")] + HOST_SOURCES + ["-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=1800)
        assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
        print(out.stdout)
        assert out.stdout.splitlines()[-1] == "total bad 0"
        assert out.stdout.count("unsatisfied 0, instance and region mismatches 0,") == 12
        assert out.stdout.count("bytes with two writers 0, guard bytes written 0, alignment bytes written 0, reveal region bytes without their one writer 0, lane faults 0") == 6


def test_host_entry_points_under_sanitizers():
    """tests/gcm_segment_reveal_host_check.cpp with the three host-only sources under -fsanitize=address,undefined: the _rv circuit queries, and the committed ECB fixture
    proof -- whole, truncated at every length, garbage -- and a mask and a revealed array one byte short through zkaes_verify_gcm_segments_reveal: never accepted.  A
    stand-alone program: nothing is loaded into python"""
    cxx = CLANG if os.path.exists(CLANG) else "g++"
    flags = ["-x", "c++", "-O1", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC]
    if cxx == CLANG:
        flags += ["-mllvm", "-asan-globals=0"]        # (as tests/test_fuzz_host.py: this toolchain's ASan trips over its own registration of merged string literals)
    name = "gcm_segment_reveal_host_check"
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, name)
        subprocess.check_call([cxx] + flags + [os.path.join(ROOT, "tests", name + ".cpp")] + HOST_SOURCES + ["-o", exe])
        env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
        out = subprocess.run([exe, GOLD], capture_output=True, text=True, env=env, timeout=900)
        assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
        assert out.stdout.split() == [name, "ok"]
