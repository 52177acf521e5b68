"""What a larger AES key costs the prover, against AES-128 in the same process, and what fits the default universal SRS at each key size.

    python tools/keysize_vs_aes128.py --capacity                                   (host only: no GPU)
    python tools/keysize_vs_aes128.py [--blocks 1] [--reps 5] [--chunks 24] [--out profiles/keysize_witness_ms.json]      (run on the GPU box)

--capacity compiles circuits on the host and prints, for each key size, the largest statement whose index fits the default SRS literal (866_944, 513, 4_062_064):
blocks per proof for ECB, CBC and CTR, message bytes at an empty aad for GCM.  "Fits" is what key synthesis checks: AHPForR1CS::max_degree of the padded constraint
count and the joint matrix's non-zeros is at most that of the literal (|H| <= 2^21 and |K| <= 2^22).

The GPU run records (1) witness_ms and the whole proof's ms from ProvingKey.timings() of lone ECB proofs at 128 / 192 / 256 bits and the same block count, the median
of --reps proofs behind one warm-up, and (2) chunked ECB and CTR blocks/s for each key size over the default SRS at the largest block count that fits, every proof
verified.  Expectation, stated before measuring: a block's gates are dominated by its rounds, so the per-block cost should scale roughly with Nr / 10 (1.2 and 1.4).
Measurement only -- nothing here is a pass/fail threshold except that every proof must verify.  (tools/ctr_vs_ecb.py is the mould.)
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
try:
    import torch  # noqa: F401  -- before libzkaes.so where torch exists (tests/conftest.py: one process, two HIP runtimes)
except ImportError:
    pass
import numpy as np

from aes_zero_knowledge_proof_circuit_amd import api

DEFAULT_SRS = (866_944, 513, 4_062_064)
KEY_BITS = (128, 192, 256)
MODES = {"ecb": api.CIRCUIT_AES, "cbc": api.CIRCUIT_AES_CBC, "ctr": api.CIRCUIT_AES_CTR, "gcm": api.CIRCUIT_AES_GCM}


def pow2(n):
    p = 1
    while p < n:
        p <<= 1
    return p


def ahp_max_degree(nc, nv, nnz):
    """AHPForR1CS::max_degree with zk_bound = 1 (csrc/marlin_host.hpp)"""
    h, k = pow2(max(nc, nv)), pow2(nnz)
    return max(2 * h - 1, 3 * h - 1, h, 3 * k - 3)


def index_sizes(kind, length, key_bits):
    """(padded constraints, joint non-zeros) of a circuit, on the host: the joint matrix is the union of the supports of A, B and C"""
    keys, rows = [], 0
    for which in range(3):
        rowptr, col, _ = api.circuit_matrix(kind, length, which, 0, key_bits=key_bits)
        rows = len(rowptr) - 1
        r = np.repeat(np.arange(rows, dtype=np.int64), np.diff(rowptr.astype(np.int64)))
        keys.append(r * (1 << 32) + col.astype(np.int64))
    return rows, len(np.unique(np.concatenate(keys)))


def fits(kind, length, key_bits, limit):
    n, joint = index_sizes(kind, length, key_bits)
    return ahp_max_degree(n, n, joint) <= limit, n, joint


def capacity():
    limit = ahp_max_degree(*DEFAULT_SRS)
    out = {"srs": list(DEFAULT_SRS), "max_degree": limit, "modes": {}}
    for mode, kind in MODES.items():
        unit = 1 if mode == "gcm" else 16                      # GCM: bytes at A = 0 (whole blocks first, then the bytes of one more, partial block)
        for key_bits in KEY_BITS:
            # the joint count is close to affine in the block count: estimate from one and two blocks, then walk to the boundary
            _, _, j1 = fits(kind, 16, key_bits, limit)
            _, _, j2 = fits(kind, 32, key_bits, limit)
            nb = max(1, ((1 << 22) - j1) // max(j2 - j1, 1) + 1)
            while nb > 1 and not fits(kind, 16 * nb, key_bits, limit)[0]:
                nb -= 1
            while fits(kind, 16 * (nb + 1), key_bits, limit)[0]:
                nb += 1
            length = 16 * nb
            if mode == "gcm":                                   # a further partial block may still fit: the largest byte count inside block nb + 1
                lo, hi = 16 * nb, 16 * (nb + 1)                 # lo fits, hi does not
                while hi - lo > 1:
                    mid = (lo + hi) // 2
                    lo, hi = (mid, hi) if fits(kind, mid, key_bits, limit)[0] else (lo, mid)
                length = lo
            ok, n, joint = fits(kind, length, key_bits, limit)
            assert ok
            _, n_next, joint_next = fits(kind, length + unit, key_bits, limit)
            out["modes"]["%s-%d" % (mode, key_bits)] = {"blocks": (length + 15) // 16, "bytes": length, "constraints": n, "joint_nnz": joint, "h": pow2(n), "k": pow2(joint),
                                                        "next_constraints": n_next, "next_joint_nnz": joint_next}
            print("%s-%d: %d blocks (%d bytes%s): %d constraints (|H| = 2^%d), %d joint non-zeros (|K| = 2^%d); the next size up: %d, %d" %
                  (mode, key_bits, (length + 15) // 16, length, " at A = 0" if unit == 1 else "", n, pow2(n).bit_length() - 1, joint, pow2(joint).bit_length() - 1, n_next, joint_next), flush=True)
    return out


def host_ecb(msg, key):
    return api.ecb_ciphertext(msg, key)


def lone(blocks, reps):
    """median witness_ms and total_ms of lone ECB proofs per key size, keys over an SRS sized for the largest of the three circuits (one SRS for all three)"""
    length = 16 * blocks
    ci = api.circuit_info(api.CIRCUIT_AES, length, key_bits=256)
    srs = (int(ci["constraints"]), int(ci["instance"]), int(ci["nnz_a"] + ci["nnz_b"] + ci["nnz_c"]))
    rs = np.random.RandomState(0x5EED)
    out = {}
    for key_bits in KEY_BITS:
        pk, vk = api.synthesize_keys(length, srs=srs, flags=api.KEY_NO_TABLES, key_bits=key_bits)
        try:
            msg, key = rs.bytes(length), rs.bytes(key_bits // 8)
            ct = host_ecb(msg, key)
            wit, tot = [], []
            for i in range(reps + 1):
                proof = api.encrypt(msg, key, pk, zk_seed=rs.bytes(32))
                assert api.verify_encryption(vk, proof, ct)
                if i:                                            # the first proof warms the context up
                    t = pk.timings()
                    wit.append(t["witness_ms"]); tot.append(t["total_ms"])
            info = pk.info()
            out[str(key_bits)] = {"witness_ms": statistics.median(wit), "total_ms": statistics.median(tot), "witness_ms_all": wit, "total_ms_all": tot,
                                  "constraints": int(info["raw_constraints"]), "h": int(info["h"]), "k": int(info["k"])}
        finally:
            pk.free()
    for key_bits in (192, 256):
        out[str(key_bits)]["witness_ratio_to_128"] = out[str(key_bits)]["witness_ms"] / out["128"]["witness_ms"]
        out[str(key_bits)]["total_ratio_to_128"] = out[str(key_bits)]["total_ms"] / out["128"]["total_ms"]
        out[str(key_bits)]["expected_ratio_nr_over_10"] = (key_bits // 32 + 6) / 10
    return out


def chunked(cap, n_chunks):
    """blocks/s of chunked ECB and CTR per key size over the default SRS, at the largest block count that fits; every proof verified"""
    rs = np.random.RandomState(0xC4A9)
    out = {}
    for mode in ("ecb", "ctr"):
        for key_bits in KEY_BITS:
            nb = cap["modes"]["%s-%d" % (mode, key_bits)]["blocks"]
            chunk = 16 * nb
            pk, vk = api.synthesize_keys(chunk, circuit=MODES[mode], key_bits=key_bits)
            try:
                msg, key, icb, seed = rs.bytes(chunk * n_chunks), rs.bytes(key_bits // 8), rs.bytes(16), rs.bytes(32)
                times = []
                for i in range(2):                              # a warm-up leg, then the timed one
                    t0 = time.perf_counter()
                    if mode == "ecb":
                        proofs = pk.encrypt_chunked(msg, key, zk_seed=seed)
                        dt = time.perf_counter() - t0
                        ct = host_ecb(msg, key)
                        ok = sum(api.verify_encryption(vk, p, ct[chunk * j:chunk * (j + 1)]) for j, p in enumerate(proofs))
                    else:
                        ct, proofs = pk.encrypt_ctr_chunked(msg, key, icb, zk_seed=seed)
                        dt = time.perf_counter() - t0
                        assert ct == api.ctr_crypt(msg, key, icb)
                        ok = sum(api.verify_ctr_chunked(vk, proofs, icb, ct))
                    assert ok == n_chunks, (mode, key_bits, ok)
                    times.append(dt)
                out["%s-%d" % (mode, key_bits)] = {"blocks_per_chunk": nb, "chunks": n_chunks, "contexts": pk.contexts(), "seconds": times[1], "blocks_per_s": nb * n_chunks / times[1],
                                                   "verified": ok}
                print(mode, key_bits, out["%s-%d" % (mode, key_bits)], flush=True)
            finally:
                pk.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--capacity", action="store_true", help="host only: print what fits the default SRS per mode and key size, and stop")
    ap.add_argument("--blocks", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chunks", type=int, default=24)
    ap.add_argument("--skip-chunked", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "keysize_witness_ms.json"))
    args = ap.parse_args()
    if args.capacity:
        print(json.dumps(capacity()))
        return
    res = {"lone_ecb": lone(args.blocks, args.reps), "blocks": args.blocks}
    print(json.dumps(res["lone_ecb"]), flush=True)
    if not args.skip_chunked:                                   # (the capacity search is minutes of host work: only where the chunked legs need it)
        res["capacity"] = capacity()
        res["chunked"] = chunked(res["capacity"], args.chunks)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
