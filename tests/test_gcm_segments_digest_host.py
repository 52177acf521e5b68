"""Digests on segmented GCM records, on the host: every role's counts against closed forms restated from 9f and 9g, the capacity table over the default
SRS, the flag off as today's circuits, the plan, the record helper against hashlib and the model, the public-input rows against a Python restatement, the refusals, and
the changed and new trace kernels run lane by lane under sanitizers (no GPU, no oracle).

A digest record is nd data segments -- head, mids, the LAST with the record's final Lr bytes -- and one closing tail without data.  Every data segment proves, beside its
GCM statement of 9g, the SHA-256 compressions over its hidden bytes between two public states; the last carries the final padding with the public bit count, so the
record's last state is hashlib's digest of its plaintext.
"""
import hashlib
import os
import subprocess
import tempfile

import numpy as np
import pytest

import gcm_segment_digest_model as model
import gcm_segment_model as seg_model
import sha256_model
from test_cbc_host import CSRC, ROOT
from test_gcm_segments_host import CAPACITY as PLAIN_CAPACITY, _ecb

K_LIMIT = 1 << 22                                                                  # over the default SRS literal (866_944, 513, 4_062_064) the joint matrix binds: |K| <= 2^22
# DESIGN.md 9m's capacity table: the joint non-zeros of every role of an AES-128 digest record at c = 4, measured through circuit_info_gcm_segment(..., digest=True),
# and of the mids of the longer keys, which do not fit
CAPACITY_DIGEST = {("head", 4, 0): 3_583_957, ("head", 4, 13): 3_642_985, ("mid", 4, 0): 3_695_173, ("last", 64, 0): 3_803_162, ("last", 56, 0): 3_800_628, ("tail", 0, 0): 1_495_723}
OVER = {192: 4_256_936, 256: 4_910_331}                                            # the mid at c = 4


@pytest.mark.parametrize("bits", [128, 256])
def test_builder_agrees_with_the_closed_forms(api, bits):
    """rows, instance and witnesses of head (A = 0, 13), mid, last (Lr = 1, 17, 55, 56, 64) and the closing tail at c = 4 against gcm_segment_digest_model.segment_size"""
    ecb = _ecb(api, bits)
    shapes = [("head", 4, 0), ("head", 4, 13), ("mid", 4, 0), ("tail", 0, 0)] + [("last", lr, 0) for lr in (1, 17, 55, 56, 64)]
    for role, units, a in shapes:
        got = api.circuit_info_gcm_segment(role, units, a, bits, digest=True)
        want = model.segment_size(role, units, a, bits, ecb)
        print(bits, role, units, a, "->", int(got["raw_constraints"]), int(got["raw_instance"]), int(got["raw_witness"]), "joint", int(got["joint_nnz"]))
        assert (got["raw_constraints"], got["raw_instance"], got["raw_witness"]) == want
        assert got["constraints"] == got["instance"] + got["witness"]                              # square after padding
    # what the flag adds to a mid is exactly 9f's chain digest over 64 bytes: 512 inputs, one compression over variables
    plain, dg = api.circuit_info_gcm_segment("mid", 4, 0, bits), api.circuit_info_gcm_segment("mid", 4, 0, bits, digest=True)
    rows, wits = sha256_model.digest_size("chain", 64)
    assert (dg["raw_constraints"] - plain["raw_constraints"], dg["raw_instance"] - plain["raw_instance"], dg["raw_witness"] - plain["raw_witness"]) == (rows, 512, wits)
    assert rows == sha256_model.HEAD_ROWS + sha256_model.COMPRESSION_ROWS
    # Lr = 55 is the longest last with one compression, 56 the shortest with two
    assert model.final_digest_size(56)[0] - model.final_digest_size(55)[0] > 20_000


def test_capacity_over_the_default_srs(api):
    """AES-128 at c = 4: head (A = 0, 13), mid, the longest last and the closing tail stay inside |K| <= 2^22; the closing tail is a 2^21 key; the mids of AES-192 and
    -256 at c = 4 do not fit, which is why GCM_SEGMENT_DIGEST_DEFAULT_C has 128-bit keys only"""
    for (role, units, a), want in CAPACITY_DIGEST.items():
        info = api.circuit_info_gcm_segment(role, units, a, 128, digest=True)
        print(role, units, a, "joint non-zeros", int(info["joint_nnz"]), "|H|", int(info["h"]), "|K|", int(info["k"]))
        assert info["joint_nnz"] == want <= K_LIMIT and info["h"] <= 1 << 21
    assert api.circuit_info_gcm_segment("tail", 0, 0, 128, digest=True)["k"] == 1 << 21
    assert max(api.circuit_info_gcm_segment("last", lr, 0, 128, digest=True)["joint_nnz"] for lr in (49, 55, 56, 63, 64)) == CAPACITY_DIGEST[("last", 64, 0)]
    for bits, want in OVER.items():
        info = api.circuit_info_gcm_segment("mid", 4, 0, bits, digest=True)
        assert info["joint_nnz"] == want > K_LIMIT
    assert api.GCM_SEGMENT_DIGEST_DEFAULT_C == {128: 4}
    # the reason the record ends in a last and a closing tail: a data-bearing tail of 64 bytes has no room for even one compression (DESIGN.md 9g's table)
    tail64 = api.circuit_info_gcm_segment("tail", 64, 0, 128)["joint_nnz"]
    one_compression = CAPACITY_DIGEST[("mid", 4, 0)] - PLAIN_CAPACITY[128][("mid", 0)][1]
    assert tail64 == PLAIN_CAPACITY[128][("tail", 0)][1] and tail64 + one_compression > K_LIMIT


@pytest.mark.parametrize("bits", [128, 192, 256])
def test_flag_off_is_todays_circuit(api, bits):
    """with digest=False every query answers what it answered: the closed forms of tests/gcm_segment_model.py and the recorded joint counts of
    tests/test_gcm_segments_host.py's table, element for element through the Python form and the C entry without the flag"""
    import ctypes as C
    ecb = _ecb(api, bits)
    for (role, a), (c, joint_at, joint_over) in PLAIN_CAPACITY[bits].items():
        for cc, joint in ((c, joint_at), (c + 1, joint_over)):
            units = 16 * cc if role == "tail" else cc
            off = api.circuit_info_gcm_segment(role, units, a, bits, digest=False)
            assert off == api.circuit_info_gcm_segment(role, units, a, bits) and off["joint_nnz"] == joint
            assert (off["raw_constraints"], off["raw_instance"], off["raw_witness"]) == seg_model.segment_size(role, units, a, bits, ecb)
            raw = (C.c_uint64 * 12)()
            assert api.lib().zkaes_circuit_info_gcm_seg({"head": 0, "mid": 1, "tail": 2}[role], C.c_uint(bits), C.c_size_t(units), C.c_size_t(a), raw) == 0
            assert list(raw) == list(off.values())
    if bits == 128:
        for which in range(3):
            a, b = api.circuit_matrix_gcm_segment("mid", 1, which), api.circuit_matrix_gcm_segment("mid", 1, which, digest=False)
            assert all(len(x) == len(y) and (x == y).all() for x, y in zip(a, b))
    assert api.gcm_segment_plan(16384, 13, key_bits=bits) == api.gcm_segment_plan(16384, 13, key_bits=bits, digest=False)
    assert api.gcm_segment_header(bytes(12), 2, aad=b"abc") == api.gcm_segment_header(bytes(12), 2, aad=b"abc", h_in=None, total_bits=None)


def test_plan(api):
    want = {65: (2, 1), 119: (2, 55), 120: (2, 56), 128: (2, 64), 145: (3, 17), 16384: (256, 64)}
    for length, (nd, lr) in want.items():
        p = api.gcm_segment_plan(length, 13, digest=True)
        assert (p["nd"], p["last_bytes"]) == (nd, lr) == model.plan(length, 4) and p["n"] == nd + 1 and p["c"] == 4 and p["tail_bytes"] == 0 and p["aad"] == 13
        roles = [s["role"] for s in p["segments"]]
        assert roles == ["head"] + ["mid"] * (nd - 2) + ["last", "tail"]
        assert [s["ctr0"] for s in p["segments"]] == [2 + 4 * s for s in range(nd + 1)]
        assert [s["bytes"] for s in p["segments"]] == [64] * (nd - 1) + [lr, 0] and [s["offset"] for s in p["segments"]] == [64 * s for s in range(nd)] + [length]
    assert api.gcm_segment_plan(16384, 0, digest=True)["n"] == 257                                 # one small proof more than the plain plan's 256
    assert api.gcm_segment_plan(200, 0, c=8, key_bits=256, digest=True)["nd"] == 2
    with pytest.raises(api.ZkAesError, match="lone digest key"):                                   # a record of one segment names the lone key
        api.gcm_segment_plan(64, 0, digest=True)
    for kwargs in (dict(key_bits=192), dict(key_bits=256)):                                        # no default c over the default SRS: c must be passed
        with pytest.raises(api.ZkAesError, match="larger srs"):
            api.gcm_segment_plan(1000, 0, digest=True, **kwargs)
    for bad in (dict(c=3), dict(c=0), dict(reveal=True), dict(key_tag_blocks=1)):
        with pytest.raises(api.ZkAesError):
            api.gcm_segment_plan(1000, 0, digest=True, **bad)
    for length in (0, (1 << 20) + 1):
        with pytest.raises(api.ZkAesError):
            api.gcm_segment_plan(length, 0, digest=True)


@pytest.mark.parametrize("length", [65, 119, 120, 128, 145, 1000])
def test_record_helper(api, length):
    """states[nd] is hashlib's digest of the message -- and of prefix || message from the prefix's chain state --, every state is the model's, the first nd - 1
    accumulators are gcm_boundaries' and the last is the model's accumulator behind the last data block"""
    rs = np.random.RandomState(0xD16 + length)
    msg, key, iv, aad, prefix = rs.bytes(length), rs.bytes(16), rs.bytes(12), rs.bytes(13), rs.bytes(64)
    ys, states = api.gcm_digest_plan(msg, key, iv, aad, 4)
    nd, lr = model.plan(length, 4)
    assert len(ys) == nd and len(states) == nd + 1
    assert states[0] == sha256_model.IV and states[nd] == hashlib.sha256(msg).digest() and states == model.states(msg, 4)
    ct, tag, want_ys = model.boundaries(msg, key, iv, aad, 4)
    assert ys == want_ys and ys[:nd - 1] == api.gcm_boundaries(msg, key, iv, aad, 4) and (ct, tag) == api.gcm_encrypt(msg, key, iv, aad)
    h1 = api.sha256_chain(prefix)
    ys2, states2 = api.gcm_digest_plan(msg, key, iv, aad, 4, h_in=h1, digest_prefix=64)
    assert ys2 == ys and states2[0] == h1 and states2[nd] == hashlib.sha256(prefix + msg).digest() and states2 == model.states(msg, 4, h1, 64)
    # the last state through the public helpers a verifier has: chain over the whole segments, finish over the last one
    assert api.sha256_finish(api.sha256_chain(msg[:64 * (nd - 1)]), 64 * (nd - 1), msg[64 * (nd - 1):]) == states[nd]


def test_public_input_rows(api):
    """zkaes_gcm_segment_digest_public_inputs against the model's restatement: H_in, H_out behind the role's inputs of 9g, a last's total_bits behind them, the tag with
    the closing tail only; their lengths are the compiler's raw_instance - 1"""
    rs = np.random.RandomState(0xD17)
    for length, alen, prefix in ((65, 0, 0), (145, 13, 0), (120, 5, 64)):
        msg, iv, aad = rs.bytes(length), rs.bytes(12), rs.bytes(alen)
        nd, lr = model.plan(length, 4)
        ct, tag, coms, st = rs.bytes(length), rs.bytes(16), [rs.bytes(32) for _ in range(nd)], [rs.bytes(32) for _ in range(nd + 1)]
        key_of, rows = api.gcm_segment_digest_public_inputs(nd + 1, iv, aad, ct, tag, coms, 4, st, digest_prefix=prefix)
        assert key_of == [0] + [1] * (nd - 2) + [2, 3]
        assert rows == [model.public_input(s, length, 4, iv, aad, ct, tag, coms, st, prefix) for s in range(nd + 1)]
        shapes = [("head", 4, alen)] + [("mid", 4, 0)] * (nd - 2) + [("last", lr, 0), ("tail", 0, 0)]
        assert [len(r) for r in rows] == [api.circuit_info_gcm_segment(*sh, digest=True)["raw_instance"] - 1 for sh in shapes]
        for bad in (dict(n=nd), dict(coms=coms[:-1]), dict(st=st[:-1]), dict(prefix=prefix + 1), dict(c=3), dict(ct=ct[:64])):
            with pytest.raises(api.ZkAesError):
                api.gcm_segment_digest_public_inputs(bad.get("n", nd + 1), iv, aad, bad.get("ct", ct), tag, bad.get("coms", coms), bad.get("c", 4), bad.get("st", st), digest_prefix=bad.get("prefix", prefix))


def test_refusals(api):
    # without the flag: role "last" and a tail of 0 bytes stay refused, and the refusals name the digest entries
    with pytest.raises(api.ZkAesError, match="digest"):
        api.circuit_info_gcm_segment("last", 17)
    with pytest.raises(api.ZkAesError, match="_gcm_seg_dg"):
        api.circuit_info_gcm_segment("tail", 0, 0)
    import ctypes as C
    out = (C.c_uint64 * 12)()
    assert api.lib().zkaes_circuit_info_gcm_seg(3, C.c_uint(128), C.c_size_t(17), C.c_size_t(0), out) != 0 and b"_gcm_seg_dg" in api.lib().zkaes_last_error()
    # with it: reveal, key-tag blocks, a head or mid that is no multiple of 64 bytes, a tail with data, a last without bytes -- each names what to use instead
    with pytest.raises(api.ZkAesError, match="reveal segment key without a digest"):
        api.circuit_info_gcm_segment("mid", 4, digest=True, reveal=True)
    with pytest.raises(api.ZkAesError, match="tagged head without a digest"):
        api.circuit_info_gcm_segment("head", 4, digest=True, key_tag_blocks=1)
    for role, units in (("head", 1), ("mid", 3), ("mid", 5)):
        with pytest.raises(api.ZkAesError, match="multiple of 4"):
            api.circuit_info_gcm_segment(role, units, digest=True)
    with pytest.raises(api.ZkAesError, match="units = 0"):
        api.circuit_info_gcm_segment("tail", 7, digest=True)
    for role, units, a in (("last", 0, 0), ("last", 17, 5), ("mid", 4, 5), ("tail", 0, 5), ("body", 4, 0)):
        with pytest.raises(api.ZkAesError):
            api.circuit_info_gcm_segment(role, units, a, digest=True)
    assert api.lib().zkaes_circuit_info_gcm_seg_dg(4, C.c_uint(128), C.c_size_t(4), C.c_size_t(0), out) != 0
    # the header: total_bits goes with h_in, h_in is 32 bytes, and neither goes with a mask
    for bad in (dict(total_bits=8), dict(h_in=bytes(31)), dict(h_in=bytes(32), mask=b"\1"), dict(h_in=bytes(32), total_bits=1 << 64)):
        with pytest.raises(api.ZkAesError):
            api.gcm_segment_header(bytes(12), 2, **bad)
    h = api.gcm_segment_header(bytes(12), 6, aad=b"abcde", h_in=bytes(range(32)), total_bits=8 * 145)
    assert len(h) == 80 + 5 + 32 + 16 and h[85:117] == bytes(range(32)) and h[117:] == (8 * 145).to_bytes(8, "big") + bytes(8)
    # the record helper: c a multiple of 4, more than one segment, a prefix of whole blocks
    rs = np.random.RandomState(0xD18)
    msg, key, iv = rs.bytes(100), rs.bytes(16), rs.bytes(12)
    for bad in (dict(c=3), dict(c=8), dict(digest_prefix=32), dict(h_in=bytes(16))):
        with pytest.raises(api.ZkAesError):
            api.gcm_digest_plan(msg, key, iv, b"", bad.pop("c", 4), **bad)
    for prefix in (32, 1 << 61):                                                                   # the entry itself checks the prefix and names itself
        with pytest.raises(api.ZkAesError, match="zkaes_gcm_digest_plan: digest_prefix"):
            api.gcm_digest_plan(msg, key, iv, b"", 4, digest_prefix=prefix)


def test_segment_digest_kernels_on_host_under_sanitizers():
    """k_aes_trace_gcm_seg and k_ghash_trace_seg (csrc/kernels_witness.cuh), k_commit_trace and the new k_sha256_trace_seg (csrc/kernels_digest.cuh) and k_witness_expand --
    the very headers the library compiles for the device -- compiled for the host and run lane by lane under ASan + UBSan (tests/gcm_segment_digest_trace_emu.cpp, a
    stand-alone program: nothing is loaded into python), over the shapes listed there, two proofs with different total_bits per launch"""
    wit = open(os.path.join(CSRC, "kernels_witness.cuh")).read()
    dig = open(os.path.join(CSRC, "kernels_digest.cuh")).read()
    assert "k_sha256_trace_seg" in dig and "TRS_LAST" in dig and "sha_load_block" in dig
    for word in ("atomic", "__shared__", "__syncthreads", "__shfl", "hipLaunch"):                   # one writer per byte needs no atomics; no LDS, barrier or cross-lane operation
        assert word not in wit and word not in dig
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "gcm_segment_digest_trace_emu")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wno-unknown-pragmas", "-I", CSRC, "-I", os.path.join(ROOT, "tests"),
                               os.path.join(ROOT, "tests", "gcm_segment_digest_trace_emu.cpp")] + [os.path.join(CSRC, f) for f in ("circuit.cpp", "marlin_codec.cpp", "capi_host.cpp")] + ["-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=1800)
        assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
        print(out.stdout)
        assert out.stdout.splitlines()[-1] == "total bad 0"
        assert out.stdout.count("unsatisfied 0, instance mismatches 0,") == 16
        assert out.stdout.count("differ from the plain") == 4 and out.stdout.count("trace 0\n") == 4
