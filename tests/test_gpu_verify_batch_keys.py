"""Batch verification across keys on the GPU: the keyed public-input kernel against a big-integer model, verify_batch_keys(device=True) against the
host back end and the per-proof verifier on proofs of three keys, and the segment-proofs of GCM records -- head, mid and tail keys with rows of three lengths -- through one
batch, plain and under reveal keys.

The segment keys live over the default SRS literal without window tables, as in test_gpu_gcm_segments.py; every key and every proof is made once per module."""
import ctypes as C
import random

import numpy as np
import pytest

from test_gpu_verify_batch import R, model_xhat
from test_verify_batch_host import _damage, per_proof
from test_verify_batch_keys_host import INTERLEAVED, WANT, make_mixed

pytestmark = pytest.mark.gpu

SEED = bytes(range(90, 122))


# ---- the kernel --------------------------------------------------------------------------------------------------------------------------------------------------------
def domain_gen(zko, m):
    if m == 1:
        return 1
    gb = C.create_string_buffer(32)
    zko.lib().zko_api_domain_gen(377, C.c_size_t(m), gb)
    g = zko.fr_unpack(gb.raw)[0]
    assert pow(g, m, R) == 1 and pow(g, m // 2, R) != 1
    return g


def test_keyed_public_input_eval_against_the_integer_model(api, zko):
    """four domains, |X| = 1, 2, 256 and 1024, two row lengths for each of the larger two, twelve rows in interleaved key order in ONE launch: rows all-zero, all-one
    and random, an empty row between two non-empty ones, and betas that are random, in the row's own domain (the indicator branch), in a SUBGROUP of the row's domain
    (g_256^3 under the 1024 key: indicator) and in a larger domain only (g_1024^5 under the 256 key: the fraction path)"""
    rnd = random.Random(0x9B17)
    keys = [(0, 0), (1, 1), (8, 255), (8, 131), (10, 1023), (10, 517)]
    g = {lg: domain_gen(zko, 1 << lg) for lg in (0, 1, 8, 10)}
    rand_row = lambda n: bytes(rnd.randrange(2) for _ in range(n))      # noqa: E731
    plan = [                                             # (key, row, beta)
        (2, rand_row(255), rnd.randrange(R)),
        (0, b"", rnd.randrange(R)),
        (4, bytes([1] * 1023), pow(g[10], 3, R)),        # own domain: indicator
        (1, b"\x01", rnd.randrange(R)),
        (3, rand_row(131), pow(g[10], 5, R)),            # in X_1024, not in X_256: fractions
        (0, b"", 1),                                     # an empty row between two non-empty ones; beta = 1 lies in X = {1}: indicator
        (5, rand_row(517), pow(g[8], 3, R)),             # X_256 is a subgroup of X_1024: indicator
        (1, b"\x00", R - 1),                             # g_2^3 = -1: indicator
        (2, bytes(255), pow(g[8], 3, R)),
        (4, rand_row(1023), rnd.randrange(R)),
        (3, bytes([1] * 131), rnd.randrange(R)),
        (5, bytes(517), rnd.randrange(R)),
    ]
    assert pow(pow(g[10], 5, R), 256, R) != 1 and pow(pow(g[8], 3, R), 1024, R) == 1
    got = zko.fr_unpack(api.public_input_eval_keyed(keys, [p[0] for p in plan], zko.fr_pack([p[2] for p in plan]), [p[1] for p in plan]))
    want = [model_xhat(1 << keys[k][0], g[keys[k][0]], beta, row) for k, row, beta in plan]
    assert got == want
    # twelve rows under ONE key: the existing kernel's answers
    rows = [rand_row(255) for _ in range(10)] + [bytes(255), bytes([1] * 255)]
    betas = zko.fr_pack([rnd.randrange(R) for _ in range(11)] + [pow(g[8], 7, R)])
    assert api.public_input_eval_keyed([(8, 255)], [0] * 12, betas, rows) == api.public_input_eval(8, betas, rows)


def test_keyed_public_input_eval_refuses_rows_that_do_not_fit(api, zko):
    one = zko.fr_pack([5])
    with pytest.raises(api.ZkAesError, match="fewer than 2\\^lg_m bits"):
        api.public_input_eval_keyed([(3, 8)], [0], one, [bytes(8)])
    with pytest.raises(api.ZkAesError, match="lg_m <= 30"):
        api.public_input_eval_keyed([(31, 1)], [0], one, [bytes(1)])
    with pytest.raises(api.ZkAesError, match="key index out of range"):
        api.public_input_eval_keyed([(3, 7)], [1], one, [bytes(7)])


# ---- proofs of three keys ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed(zko, api, vectors):
    return make_mixed(zko, api, vectors)


def agree(api, keys, items, want):
    """device == host back end == the per-proof verifier == want"""
    key_of, proofs, rows = [k for k, _, _ in items], [p for _, p, _ in items], [r for _, _, r in items]
    assert [per_proof(api, keys[k], p, r) for k, p, r in items] == want
    assert api.verify_batch_keys(keys, key_of, proofs, rows, device=False) == want
    assert api.verify_batch_keys(keys, key_of, proofs, rows, device=True) == want


def test_mixed_batch_device_host_and_per_proof_agree(api, mixed):
    keys, items, _, _ = mixed
    agree(api, keys, items, WANT)
    assert api.verify_batch_timings()["sub_batches"] <= 1 + 2 * 4      # one bad proof among nine: 2 ceil(log2 9) further sub-batches
    agree(api, keys, [items[i] for i in INTERLEAVED], [WANT[i] for i in INTERLEAVED])
    assert api.verify_batch_timings()["sub_batches"] <= 1 + 2 * 4
    good = [items[i] for i in INTERLEAVED if WANT[i]]
    agree(api, keys, good, [True] * 8)
    assert api.verify_batch_timings()["sub_batches"] == 1


@pytest.mark.parametrize("kind", ["eval", "random_v", "truncated"])
@pytest.mark.parametrize("pos", [0, 4, 8])
def test_damaged_mixed_batches(api, mixed, kind, pos):
    keys, items, _, _ = mixed
    order = [items[i] for i in INTERLEAVED]
    k, p, r = order[pos]
    order[pos] = (k, _damage(p, kind), r)
    agree(api, keys, order, [WANT[i] and j != pos for j, i in enumerate(INTERLEAVED)])


def test_mislabelled_proof_and_a_row_of_another_length(api, mixed):
    keys, items, _, _ = mixed
    order = [items[i] for i in INTERLEAVED]
    want = [WANT[i] for i in INTERLEAVED]
    order[0] = (1, order[0][1], order[0][2])                              # an xor proof under the add key
    order[2] = (2, order[2][1], order[2][2][:-1])                         # 127 bits: pads to |X| = 128, not the AES key's 256
    want[0] = want[2] = False
    agree(api, keys, order, want)


def test_errors_of_the_call_on_the_device_entry(api, mixed):
    keys, items, _, _ = mixed
    _, p, r = items[0]
    with pytest.raises(api.ZkAesError, match="names key 3 of 3"):
        api.verify_batch_keys(keys, [0, 3], [p, p], [r, r], device=True)
    with pytest.raises(api.ZkAesError, match="at least one verifying key"):
        api.verify_batch_keys([], [0], [p], [r], device=True)


# ---- segmented GCM records -----------------------------------------------------------------------------------------------------------------------------------------------
OPEN_39 = [range(14, 19), 38]                            # across the head / mid boundary, and the record's last byte


def record(seed, length, alen):
    rs = np.random.RandomState(seed)
    return bytes(b | 1 for b in rs.bytes(length)), rs.bytes(16), rs.bytes(12), rs.bytes(alen)


def make_records(api, reveal):
    """the 39-byte record (head, mid, 7-byte tail) and, for plain keys, the 65-byte record of five one-block segments, A = 13 and c = 1: {length: (vks, proofs, iv, aad,
    ct, tag, coms[, mask, revealed])}.  The proving keys are freed once the proofs are made"""
    api.srs_hold(True)
    made = {}

    def get(role, units, aad=0):
        if (role, units) not in made:
            made[(role, units)] = api.synthesize_keys_gcm_segment(role, units, aad, flags=api.KEY_NO_TABLES, reveal=reveal)
        return made[(role, units)]
    try:
        out = {}
        for length in (39,) if reveal else (39, 65):
            ks = [get("head", 1, 13), get("mid", 1), get("tail", length - 16 * ((length - 1) // 16))]
            pks, vks = tuple(k[0] for k in ks), tuple(k[1] for k in ks)
            msg, key, iv, aad = record(0x9C00 + length, length, 13)
            if reveal:
                ct, tag, coms, revealed, proofs = api.encrypt_gcm_segments(msg, key, iv, aad, pks, zk_seed=SEED, mask=OPEN_39)
                out[length] = (vks, proofs, iv, aad, ct, tag, coms, api.reveal_mask(OPEN_39, length), revealed)
            else:
                ct, tag, coms, proofs = api.encrypt_gcm_segments(msg, key, iv, aad, pks, zk_seed=SEED)
                out[length] = (vks, proofs, iv, aad, ct, tag, coms)
        return out
    finally:
        for pk, _ in made.values():
            pk.free()
        api.srs_hold(False)


@pytest.fixture(scope="module")
def plain(api):
    return make_records(api, False)


@pytest.fixture(scope="module")
def revealing(api):
    return make_records(api, True)


def segments_agree(api, rec, want, **change):
    """verify_gcm_segments_batch on the device and on the host == verify_gcm_segments == want, for the record with some of its arguments changed"""
    names = ("vks", "proofs", "iv", "aad", "ct", "tag", "coms", "mask", "revealed")
    a = dict(zip(names, tuple(rec) + (None, None)))
    a.update(change)
    args = (a["vks"], a["proofs"], a["iv"], a["aad"], a["ct"], a["tag"], a["coms"], 1)
    assert api.verify_gcm_segments(*args, mask=a["mask"], revealed=a["revealed"]) == want
    assert api.verify_gcm_segments_batch(*args, mask=a["mask"], revealed=a["revealed"], device=False) == want
    assert api.verify_gcm_segments_batch(*args, mask=a["mask"], revealed=a["revealed"], device=True) == want


def flip(data, byte, bit=0):
    return data[:byte] + bytes([data[byte] ^ (1 << bit)]) + data[byte + 1:]


def test_a_39_byte_record_three_keys_three_row_lengths(api, plain):
    rec = plain[39]
    vks, proofs, coms = rec[0], rec[1], rec[6]
    rows, roles = api.gcm_segment_public_inputs(3, *rec[2:7], 1)
    assert roles == ["head", "mid", "tail"] and [len(r) for r in rows] == [616, 768, 696]     # three keys, three row lengths (each pads to |X| = 1024)
    assert [int.from_bytes(vk.to_ark_bytes()[24:32], "little") for vk in vks] == [1024] * 3 and len({vk.to_ark_bytes()[40:88] for vk in vks}) == 3
    segments_agree(api, rec, [True, True, True])
    assert api.verify_batch_timings()["sub_batches"] == 1
    segments_agree(api, rec, [True, True, False], tag=flip(rec[5], 9, 3))                     # a wrong tag: the tail alone
    segments_agree(api, rec, [False, False, True], coms=[flip(coms[0], 31, 7), coms[1]])      # commitments[0] is the head's output and the mid's input
    segments_agree(api, rec, [False, False, True], proofs=[proofs[1], proofs[0], proofs[2]])  # head and mid proofs exchanged


def test_errors_of_the_segment_batch_are_those_of_the_per_proof_entry(api, plain):
    vks, proofs, iv, aad, ct, tag, coms = plain[39]
    with pytest.raises(api.ZkAesError, match="the record has 3 segments of 1 blocks"):
        api.verify_gcm_segments(vks, proofs[:2], iv, aad, ct, tag, coms, 1)
    for device in (False, True):
        with pytest.raises(api.ZkAesError, match="the record has 3 segments of 1 blocks"):
            api.verify_gcm_segments_batch(vks, proofs[:2], iv, aad, ct, tag, coms, 1, device=device)
        with pytest.raises(api.ZkAesError, match="the tail key was not synthesized for this segment's lengths"):
            api.verify_gcm_segments_batch((vks[0], vks[1], plain[65][0][2]), proofs, iv, aad, ct, tag, coms, 1, device=device)
        with pytest.raises(api.ZkAesError, match="needs the mid key"):
            api.verify_gcm_segments_batch((vks[0], None, vks[2]), proofs, iv, aad, ct, tag, coms, 1, device=device)


def test_a_65_byte_record_of_five_segments(api, plain):
    segments_agree(api, plain[65], [True] * 5)
    assert api.verify_batch_timings()["sub_batches"] == 1


def test_two_records_in_one_batch(api, plain):
    a, b = plain[39], plain[65]
    assert a[0][0] is b[0][0] and a[0][1] is b[0][1] and a[0][2] is not b[0][2]               # one head, one mid, two tails: four keys
    for device in (False, True):
        assert api.verify_gcm_records_batch([a + (1,), b + (1,)], device=device) == [[True] * 3, [True] * 5]
        assert api.verify_batch_timings()["sub_batches"] == 1
    bad = b[:5] + (flip(b[5], 0),) + b[6:]                                                    # the second record's tag
    for device in (False, True):
        assert api.verify_gcm_records_batch([a + (1,), bad + (1,)], device=device) == [[True] * 3, [True] * 4 + [False]]


def test_a_39_byte_record_under_reveal_keys(api, revealing):
    rec = revealing[39]
    revealed = rec[8]
    segments_agree(api, rec, [True, True, True])
    segments_agree(api, rec, [False, True, True], revealed=flip(revealed, 15, 4))             # byte 15 is the head's
    segments_agree(api, rec, [True, False, True], revealed=flip(revealed, 17, 0))             # byte 17 the mid's
    segments_agree(api, rec, [True, True, False], revealed=flip(revealed, 38, 7))             # byte 38 the tail's
    for device in (False, True):
        assert api.verify_gcm_records_batch([rec[:7] + (1,) + rec[7:]], device=device) == [[True, True, True]]
