"""Key tags on segmented GCM records, on the host: T = 0 unchanged through the new queries, what a tag block adds to a head against DESIGN.md 9e's
table, the capacity table over the default SRS, the public-input layout against a Python restatement, the refusals, and two stand-alone programs under sanitizers --
the segment kernels, k_key_tag_trace and k_reveal_trace run lane by lane, and the host-only verifiers (no GPU, no oracle).

A HEAD segment key synthesized with key_tag_blocks = T proves, beside the head's statement of DESIGN.md 9g, tag_t = AES_K(D_t), t < T, and exposes the 128 T tag bits
behind com_out and ahead of a reveal key's mask and revealed bits.  The boundary commitments carry the head's key to every later segment, so one tag covers the record
and a mid or tail takes T = 0 only.
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import gcm_segment_keytag_model as model
import gcm_segment_reveal_model as rv_model
from test_cbc_host import CLANG, CSRC, GOLD, ROOT

HOST_SOURCES = [os.path.join(CSRC, f) for f in ("circuit.cpp", "marlin_codec.cpp", "capi_host.cpp")]
ROLE_ID = {"head": 0, "mid": 1, "tail": 2}

# DESIGN.md 9l's capacity table: per key size, T, reveal and A the largest c whose head stays inside the default SRS literal (866_944, 513, 4_062_064: |K| <= 2^22),
# measured through circuit_info_gcm_segment(..., key_tag_blocks=T); (c, joint non-zeros at that c, at c + 1).  {bits: {(T, reveal, A): ...}}
CAPACITY_KEYTAG = {
    128: {(1, False, 0): (4, 4_053_539, 4_711_284), (1, False, 13): (4, 4_112_567, 4_770_312), (1, True, 0): (4, 4_056_227, 4_714_644), (1, True, 13): (4, 4_115_255, 4_773_672),
          (2, False, 0): (3, 3_979_301, 4_637_094), (2, False, 13): (3, 4_038_329, 4_696_122), (2, True, 0): (3, 3_981_317, 4_639_782), (2, True, 13): (3, 4_040_345, 4_698_810)},
    192: {(1, False, 0): (3, 3_955_937, 4_731_516), (1, False, 13): (3, 4_015_443, 4_791_022), (1, True, 0): (3, 3_957_953, 4_734_204), (1, True, 13): (3, 4_017_459, 4_793_710),
          (2, False, 0): (2, 3_880_777, 4_656_328), (2, False, 13): (2, 3_940_283, 4_715_834), (2, True, 0): (2, 3_882_121, 4_658_344), (2, True, 13): (2, 3_941_627, 4_717_850)},
    256: {(1, False, 0): (2, 3_717_193, 4_608_919), (1, False, 13): (2, 3_776_607, 4_668_333), (1, True, 0): (2, 3_718_537, 4_610_935), (1, True, 13): (2, 3_777_951, 4_670_349),
          (2, False, 0): (1, 3_642_242, 4_533_968), (2, False, 13): (1, 3_701_656, 4_593_382), (2, True, 0): (1, 3_642_914, 4_535_312), (2, True, 13): (1, 3_702_328, 4_594_726)},
}
# what ONE tag block adds to the joint matrix of a head, whatever c, A and reveal: below the A + B + C sum 706,382 / 847,809 / 988,482 of a lone GCM key's tag block
JOINT_PER_BLOCK = {128: 583_534, 192: 700_370, 256: 816_754}
# the largest A at which a T = 1 head still fits at the default c (with and without reveal): (A, joint non-zeros there without reveal, at A + 1)
LARGEST_AAD = {128: (16, 4_125_553, 4_196_967), 192: (48, 4_173_701, 4_245_689), 256: (96, 4_152_025, 4_223_897)}


def _matrix_raw(fn, head):
    rows, nnz = C.c_uint64(), C.c_uint64()
    assert fn(*head, C.byref(rows), C.byref(nnz), None, None, None) == 0
    rowptr, col, coeff = np.zeros(rows.value + 1, np.uint32), np.zeros(max(nnz.value, 1), np.uint32), np.zeros(max(nnz.value, 1), np.int64)
    assert fn(*head, None, None, rowptr.ctypes.data_as(C.c_void_p), col.ctypes.data_as(C.c_void_p), coeff.ctypes.data_as(C.c_void_p)) == 0
    return rowptr, col[:nnz.value], coeff[:nnz.value]


@pytest.mark.parametrize("bits", [128, 256])
def test_no_tag_blocks_is_todays_circuit(api, bits):
    """the _kt queries at T = 0 answer element for element what the _rv queries answer: the 12 info words and all three matrices, for head, mid and tail, at c = 1 and
    the default c, with reveal off and on; and the Python forms at key_tag_blocks = 0 are the calls they were"""
    L = api.lib()
    dc = api.GCM_SEGMENT_DEFAULT_C[bits]
    for c in (1, dc):
        for role, units, a in (("head", c, 13), ("mid", c, 0), ("tail", 16 * c - 9, 0)):
            for rv in (0, 1):
                old, new = (C.c_uint64 * 12)(), (C.c_uint64 * 12)()
                assert L.zkaes_circuit_info_gcm_seg_rv(ROLE_ID[role], C.c_uint(bits), C.c_uint(rv), C.c_size_t(units), C.c_size_t(a), old) == 0
                assert L.zkaes_circuit_info_gcm_seg_kt(ROLE_ID[role], C.c_uint(bits), C.c_uint(rv), C.c_uint(0), C.c_size_t(units), C.c_size_t(a), new) == 0
                assert list(old) == list(new)
                assert api.circuit_info_gcm_segment(role, units, a, bits, reveal=bool(rv), key_tag_blocks=0) == api.circuit_info_gcm_segment(role, units, a, bits, reveal=bool(rv))
                if rv and c != 1:
                    continue                                                                       # (the matrices of the largest shapes once)
                for which in range(3):
                    want = _matrix_raw(L.zkaes_circuit_matrix_gcm_seg_rv, (ROLE_ID[role], C.c_uint(bits), C.c_uint(rv), C.c_size_t(units), C.c_size_t(a), which))
                    got = _matrix_raw(L.zkaes_circuit_matrix_gcm_seg_kt, (ROLE_ID[role], C.c_uint(bits), C.c_uint(rv), C.c_uint(0), C.c_size_t(units), C.c_size_t(a), which))
                    assert all(len(g) == len(w) and (g == w).all() for g, w in zip(got, want))
                    py = api.circuit_matrix_gcm_segment(role, units, which, a, bits, reveal=bool(rv), key_tag_blocks=0)
                    assert all(len(g) == len(w) and (g == w).all() for g, w in zip(py, want))
    assert api.gcm_segment_plan(16384, 13, key_bits=bits) == api.gcm_segment_plan(16384, 13, key_bits=bits, key_tag_blocks=0)
    assert api.GCM_SEGMENT_KEYTAG_DEFAULT_C[0] == api.GCM_SEGMENT_DEFAULT_C


@pytest.mark.parametrize("bits", [128, 192, 256])
def test_a_tag_block_adds_exactly_the_table_of_9e(api, bits):
    """per tag block a head gains 148,016 / 177,680 / 207,344 raw constraints, 147,760 / 177,424 / 207,088 witnesses and 128 instance entries: T = 1 and 2, reveal on
    and off, c = 1 and 2; the same block costs a lone GCM key the same (circuit_info(..., key_tag_blocks=))"""
    rows, inst, wits = model.PER_BLOCK[bits]
    lone = [api.circuit_info(api.CIRCUIT_AES_GCM, 17, 5, bits, t) for t in (0, 1)]
    assert (lone[1]["raw_constraints"] - lone[0]["raw_constraints"], lone[1]["raw_instance"] - lone[0]["raw_instance"], lone[1]["raw_witness"] - lone[0]["raw_witness"]) == (rows, inst, wits)
    for c in (1, 2):
        for rv in (False, True):
            plain = api.circuit_info_gcm_segment("head", c, 5, bits, reveal=rv)
            for blocks in (1, 2):
                got = api.circuit_info_gcm_segment("head", c, 5, bits, reveal=rv, key_tag_blocks=blocks)
                print(bits, c, rv, blocks, int(got["raw_constraints"]), int(got["raw_instance"]), int(got["raw_witness"]), int(got["joint_nnz"]))
                assert model.key_tag_size(bits, blocks) == (blocks * rows, blocks * inst, blocks * wits)
                assert got["raw_constraints"] == plain["raw_constraints"] + blocks * rows
                assert got["raw_instance"] == plain["raw_instance"] + blocks * inst
                assert got["raw_witness"] == plain["raw_witness"] + blocks * wits
                assert got["constraints"] == got["instance"] + got["witness"]                      # square after padding
                # block 0 adds the same joint non-zeros whatever c, A and reveal; block 1 a few more (D_1 has one more set bit than D_0: a key bit enters negated, and the
                # rows that use it gain an entry in the One column); both stay below the A + B + C sum of a lone key's tag block
                first = JOINT_PER_BLOCK[bits]
                if blocks == 1:
                    assert got["joint_nnz"] == plain["joint_nnz"] + first
                else:
                    assert first <= got["joint_nnz"] - plain["joint_nnz"] - first < {128: 706_382, 192: 847_809, 256: 988_482}[bits]


@pytest.mark.parametrize("bits", [128, 192, 256])
def test_capacity_over_the_default_srs_with_key_tags(api, bits):
    """|K| <= 2^22 binds.  DESIGN.md 9l's table: one tag block keeps the default c 4 / 3 / 2 of every key size, two need 3 / 2 / 1 -- with and without reveal, at A = 0
    and 13 -- the bound and one past it; GCM_SEGMENT_DEFAULT_C is untouched; the largest aad of a T = 1 head at the default c"""
    for (blocks, rv, a), (c, joint_at, joint_over) in CAPACITY_KEYTAG[bits].items():
        for cc, want in ((c, joint_at), (c + 1, joint_over)):
            info = api.circuit_info_gcm_segment("head", cc, a, bits, reveal=rv, key_tag_blocks=blocks)
            print(bits, "T", blocks, "R", int(rv), "A", a, "c", cc, "joint non-zeros", int(info["joint_nnz"]), "|H|", int(info["h"]), "|K|", int(info["k"]))
            assert info["joint_nnz"] == want and info["h"] <= 1 << 21 and info["k"] == (1 << 22 if cc == c else 1 << 23)
        assert joint_at <= 1 << 22 < joint_over
        assert api.GCM_SEGMENT_KEYTAG_DEFAULT_C[blocks][bits] == c
    assert api.GCM_SEGMENT_DEFAULT_C == {128: 4, 192: 3, 256: 2} == api.GCM_SEGMENT_KEYTAG_DEFAULT_C[1]
    assert api.GCM_SEGMENT_KEYTAG_DEFAULT_C[2] == {128: 3, 192: 2, 256: 1}
    a, at, over = LARGEST_AAD[bits]
    dc = api.GCM_SEGMENT_KEYTAG_DEFAULT_C[1][bits]
    for aa, want in ((a, at), (a + 1, over)):
        info = api.circuit_info_gcm_segment("head", dc, aa, bits, key_tag_blocks=1)
        assert info["joint_nnz"] == want and info["k"] == (1 << 22 if aa == a else 1 << 23)
        assert api.circuit_info_gcm_segment("head", dc, aa, bits, reveal=True, key_tag_blocks=1)["k"] == info["k"]
    assert a >= 13 and at <= 1 << 22 < over


def test_plan_defaults(api):
    for bits in (128, 192, 256):
        for rv in (False, True):
            p0, p1, p2 = (api.gcm_segment_plan(16384, 13, key_bits=bits, reveal=rv, key_tag_blocks=t) for t in (0, 1, 2))
            assert p0["c"] == api.GCM_SEGMENT_DEFAULT_C[bits] == p1["c"] and p1 == p0
            assert p2["c"] == api.GCM_SEGMENT_KEYTAG_DEFAULT_C[2][bits] == p0["c"] - 1 and p2["n"] > p0["n"]
            assert api.gcm_segment_plan(16384, 13, 2, key_bits=bits, reveal=rv, key_tag_blocks=2)["c"] == 2      # a c that is given is taken
    with pytest.raises(api.ZkAesError, match="0, 1 or 2"):
        api.gcm_segment_plan(16384, 13, key_tag_blocks=3)


def test_public_input_layout(api):
    """the tag bits sit behind com_out and ahead of the mask in gcm_segment_public_inputs' head row, LSB first per byte, and equal key_tag(key, T); the mid and tail
    rows are unchanged; every row has the builder's instance count.  A 39-byte record at c = 1 (head, mid, tail), plain and under a mask"""
    rs = np.random.RandomState(0x91)
    msg, key, iv, aad, tag = rs.bytes(39), rs.bytes(16), rs.bytes(12), rs.bytes(13), rs.bytes(16)
    ct, coms = rs.bytes(39), [rs.bytes(32), rs.bytes(32)]
    mask = api.reveal_mask([range(14, 19), 38], 39)
    revealed = api.reveal_bytes(msg, mask)
    for blocks in (1, 2):
        kt = api.key_tag(key, blocks)
        assert kt == model.key_tag(key, blocks) and len(kt) == 16 * blocks
        for m, r in ((None, None), (mask, revealed)):
            plain_rows, roles = api.gcm_segment_public_inputs(3, iv, aad, ct, tag, coms, 1, mask=m, revealed=r)
            rows, roles_kt = api.gcm_segment_public_inputs(3, iv, aad, ct, tag, coms, 1, mask=m, revealed=r, key_tag=kt)
            assert roles == roles_kt == ["head", "mid", "tail"]
            assert rows[1] == plain_rows[1] and rows[2] == plain_rows[2]                           # mid and tail: unchanged
            com_end = 128 + 8 * 13 + 128 + 256                                                     # iv, ctr0, aad, ct, com_out
            assert rows[0][:com_end] == plain_rows[0][:com_end] and rows[0][com_end:com_end + 128 * blocks] == rv_model.bits(kt)
            assert rows[0][com_end + 128 * blocks:] == plain_rows[0][com_end:]                     # the mask and revealed slices (or nothing) stay last
            assert rows[0][com_end - 256:com_end] == rv_model.bits(coms[0])
            for s, (role, units, a) in enumerate((("head", 1, 13), ("mid", 1, 0), ("tail", 7, 0))):
                assert rows[s] == model.public_input(s, 3, 1, iv, aad, ct, tag, coms, kt, m, r)
                info = api.circuit_info_gcm_segment(role, units, a, reveal=m is not None, key_tag_blocks=blocks if s == 0 else 0)
                assert len(rows[s]) + 1 == info["raw_instance"]


def test_refusals(api):
    L = api.lib()
    out = (C.c_uint64 * 12)()
    for role, units in (("mid", 1), ("tail", 7)):
        for blocks in (1, 2):
            with pytest.raises(api.ZkAesError, match="head carries the record's key tag.*commitments carry the key"):
                api.circuit_info_gcm_segment(role, units, key_tag_blocks=blocks)
            with pytest.raises(api.ZkAesError, match="head carries the record's key tag.*commitments carry the key"):
                api.circuit_matrix_gcm_segment(role, units, 0, key_tag_blocks=blocks)
            assert L.zkaes_circuit_info_gcm_seg_kt(ROLE_ID[role], C.c_uint(128), C.c_uint(0), C.c_uint(blocks), C.c_size_t(units), C.c_size_t(0), out) != 0
    assert L.zkaes_circuit_info_gcm_seg_kt(0, C.c_uint(128), C.c_uint(0), C.c_uint(3), C.c_size_t(1), C.c_size_t(0), out) != 0      # T = 3
    assert b"key_tag_blocks must be 0, 1 or 2" in L.zkaes_last_error()
    for call in (lambda: api.circuit_info_gcm_segment("head", 1, key_tag_blocks=3), lambda: api.circuit_matrix_gcm_segment("head", 1, 0, key_tag_blocks=3),
                 lambda: api.synthesize_keys_gcm_segment("head", 1, key_tag_blocks=3)):
        with pytest.raises(api.ZkAesError, match="0, 1 or 2"):
            call()
    with pytest.raises(api.ZkAesError, match="no HIP device|head carries"):
        api.synthesize_keys_gcm_segment("tail", 7, key_tag_blocks=1)
    iv, tag, coms, ct = bytes(range(12)), bytes(16), [bytes(32)], bytes(range(1, 18))
    for bad in (bytes(15), bytes(17), bytes(0), bytes(33)):                                        # a tag of 15 bytes
        with pytest.raises(api.ZkAesError, match="16 or 32"):
            api.gcm_segment_public_inputs(2, iv, b"", ct, tag, coms, 1, key_tag=bad)
    nbits, roles = (C.c_size_t * 2)(), (C.c_int * 2)()
    assert L.zkaes_gcm_segment_public_inputs_kt(C.c_size_t(2), C.c_size_t(1), iv, None, C.c_size_t(0), ct, C.c_size_t(17), tag, coms[0], C.c_size_t(32), bytes(15), C.c_size_t(15), None, C.c_size_t(0),
                                                None, None, nbits, roles) != 0
    assert b"key_tag_len must be 16 or 32" in L.zkaes_last_error()


def test_verifiers_refuse_a_tag_that_does_not_fit_the_head(api):
    """the committed ECB key and proof as head and tail of a 17-byte record: with a key tag of 16 or 32 bytes (the fixture key is no tagged head: the case of "a tag of
    32 bytes for a T = 1 key", a count that is not the key's) the stored key, which knows its public-input count, RAISES; the transported key (|X| alone) REJECTS the
    head; a tag of 15 bytes raises under either.  Through verify_gcm_segments, verify_gcm_segments_batch(device=False) and verify_gcm_records_batch(device=False)"""
    vk = api.VerifyingKey.from_bytes(open(os.path.join(GOLD, "gpu_aes16_vk.bin"), "rb").read())
    ark = api.VerifyingKey.from_ark_bytes(vk.to_ark_bytes())
    proof = open(os.path.join(GOLD, "gpu_aes16_proof.bin"), "rb").read()
    iv, tag, coms, ct = bytes(range(12)), bytes(16), [bytes(32)], bytes(range(1, 18))
    for kt in (bytes(range(16)), bytes(range(32))):
        for fn in (api.verify_gcm_segments, lambda *a, **k: api.verify_gcm_segments_batch(*a, device=False, **k)):
            with pytest.raises(api.ZkAesError, match="not synthesized for this segment's lengths"):
                fn((vk, None, vk), [proof, proof], iv, b"", ct, tag, coms, 1, key_tag=kt)
            assert fn((ark, None, ark), [proof, proof], iv, b"", ct, tag, coms, 1, key_tag=kt) == [False, False]
            with pytest.raises(api.ZkAesError, match="16 or 32"):
                fn((ark, None, ark), [proof, proof], iv, b"", ct, tag, coms, 1, key_tag=kt[:15])
        rec = ((ark, None, ark), [proof, proof], iv, b"", ct, tag, coms, 1)
        assert api.verify_gcm_records_batch([rec, rec], device=False, key_tag=kt) == [[False, False], [False, False]]
        with pytest.raises(api.ZkAesError, match="16 or 32"):
            api.verify_gcm_records_batch([rec], device=False, key_tag=kt[:15])


def test_layout_macros_of_a_tagged_head():
    """trace_layout.h through the preprocessor: its static_asserts hold (it compiles); a head's tag slot 0 lies at its segment trace length, a multiple of 16, the slots
    follow at the block stride, the reveal region begins where they end, and T = 0 leaves every length what it was"""
    src = ('#include "trace_layout.h"\n#include <cstdio>\nint main() { for (int nk = 4; nk <= 8; nk += 2) for (int T = 0; T <= 2; T++) '
           'printf("%d %d %ld %ld %ld %ld %ld\\n", nk, T, (long)TRS_BYTES(nk, TRS_HEAD, 1, 2), (long)TRS_KT(nk, TRS_HEAD, 1, 2), (long)TRS_KT_BYTES(nk, TRS_HEAD, 1, 2, T), '
           '(long)TRS_KT_RV(nk, TRS_HEAD, 1, 2, T), (long)TRS_KT_RV_BYTES(nk, TRS_HEAD, 1, 2, T, 1, 32)); }\n')
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "m.cpp"), "w") as f:
            f.write(src)
        subprocess.check_call(["g++", "-std=c++17", "-I", CSRC, os.path.join(d, "m.cpp"), "-o", os.path.join(d, "m")])
        lines = [list(map(int, ln.split())) for ln in subprocess.check_output([os.path.join(d, "m")], text=True).splitlines()]
    assert len(lines) == 9
    for nk, blocks, seg, kt, with_slots, rv, with_region in lines:
        stride = 112 * (nk + 6) - 48
        assert seg % 16 == 0 and kt == seg and stride % 16 == 0
        assert with_slots == seg + blocks * stride and rv == with_slots and with_region == rv + 16 + 32


def test_segment_keytag_kernels_on_host_under_sanitizers():
    """k_aes_trace_gcm_seg, k_ghash_trace_seg and k_key_tag_trace (csrc/kernels_witness.cuh), k_commit_trace (csrc/kernels_digest.cuh), k_reveal_trace
    (csrc/kernels_reveal.cuh) and k_witness_expand -- the very headers the library compiles for the device -- compiled for the host and run lane by lane under ASan + UBSan
    (tests/gcm_segment_keytag_trace_emu.cpp, a stand-alone program: nothing is loaded into python), over the four head shapes listed there, two proofs per launch"""
    wit, dig, rev = (open(os.path.join(CSRC, "kernels_%s.cuh" % name)).read() for name in ("witness", "digest", "reveal"))
    assert "k_aes_trace_gcm_seg" in wit and "k_ghash_trace_seg" in wit and "k_key_tag_trace" in wit and "k_witness_expand" in wit and "k_commit_trace" in dig and "k_reveal_trace" in rev
    for word in ("atomic", "__shared__", "__syncthreads", "__shfl", "hipLaunch"):                   # one writer per byte needs no atomics; no LDS, barrier or cross-lane operation
        assert word not in wit and word not in dig and word not in rev
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "gcm_segment_keytag_trace_emu")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wno-unknown-pragmas", "-I", CSRC, "-I", os.path.join(ROOT, "tests"),
                               os.path.join(ROOT, "tests", "gcm_segment_keytag_trace_emu.cpp")] + HOST_SOURCES + ["-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=1800)
        assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
        print(out.stdout)
        assert out.stdout.splitlines()[-1] == "total bad 0"
        assert out.stdout.count("unsatisfied 0, instance and slot mismatches 0, rows unsatisfied after one flipped tag bit 1") == 8
        assert out.stdout.count("bytes with two writers 0, guard bytes written 0, alignment bytes written 0, tag slot bytes without their one tag lane 0, bytes elsewhere the tag kernel wrote 0, "
                                "reveal region bytes without their one writer 0, lane faults 0") == 4


def test_host_entry_points_under_sanitizers():
    """tests/gcm_segment_keytag_host_check.cpp with the three host-only sources under -fsanitize=address,undefined: the _kt circuit queries and rows, and the committed
    ECB fixture proof -- whole, truncated at every length, garbage -- a tag one byte short and a commitments array one short through zkaes_verify_gcm_segments_kt and
    zkaes_verify_gcm_segments_batch_kt: never accepted.  A stand-alone program: nothing is loaded into python"""
    cxx = CLANG if os.path.exists(CLANG) else "g++"
    flags = ["-x", "c++", "-O1", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC]
    if cxx == CLANG:
        flags += ["-mllvm", "-asan-globals=0"]        # (as tests/test_fuzz_host.py: this toolchain's ASan trips over its own registration of merged string literals)
    name = "gcm_segment_keytag_host_check"
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, name)
        subprocess.check_call([cxx] + flags + [os.path.join(ROOT, "tests", name + ".cpp")] + HOST_SOURCES + ["-o", exe])
        env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
        out = subprocess.run([exe, GOLD], capture_output=True, text=True, env=env, timeout=900)
        assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
        assert out.stdout.split() == [name, "ok"]
