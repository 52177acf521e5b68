"""Chunked proving throughput of AES-128-CBC against AES-128-ECB in ONE process: the same 48-chunk message under a 6-block ECB key and a 6-block CBC key over
the shared universal SRS, legs alternating ECB / CBC for three rounds each after a warm-up of both, every proof verified.

    python tools/cbc_vs_ecb.py [--chunks 48] [--rounds 3] [--out profiles/cbc_vs_ecb.json]      (run on the GPU box)

Writes blocks/s per leg, the CBC / ECB ratio of the medians and ECB's own run-to-run spread.  The comparison is against ECB in the same run, never against a fixed
number: identical |H|, |K|, |X| mean identical transform and MSM op lists, and the extra work of CBC is 768 xor gates per chunk and the serial host chain ahead of the
prover contexts.  Measurement only -- nothing here is a pass/fail threshold except that every proof must verify.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
try:
    import torch  # noqa: F401  -- before libzkaes.so where torch exists (tests/conftest.py: one process, two HIP runtimes)
except ImportError:
    pass
import numpy as np

from aes_zero_knowledge_proof_circuit_amd import api

BLOCKS = 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "cbc_vs_ecb.json"))
    args = ap.parse_args()
    chunk = 16 * BLOCKS
    rs = np.random.RandomState(0x5EED)
    msg, key, iv = rs.bytes(chunk * args.chunks), rs.bytes(16), rs.bytes(16)
    seed = rs.bytes(32)

    t = time.perf_counter()
    pk_e, vk_e = api.synthesize_keys(chunk)
    pk_c, vk_c = api.synthesize_keys(chunk, circuit=api.CIRCUIT_AES_CBC)
    setup_s = time.perf_counter() - t
    ie, ic = pk_e.info(), pk_c.info()
    assert (ie["h"], ie["k"], ie["instance"]) == (ic["h"], ic["k"], ic["instance"]), (ie, ic)
    contexts = pk_e.contexts()
    assert pk_c.contexts() == contexts

    # expected ciphertexts from the host: CBC over the whole message; an ECB block is a one-block CBC message under a zero IV
    ct_c = api.cbc_ciphertext(msg, key, iv)
    ct_e = b"".join(api.cbc_ciphertext(msg[o:o + 16], key, bytes(16)) for o in range(0, len(msg), 16))

    def leg_ecb():
        t0 = time.perf_counter()
        proofs = pk_e.encrypt_chunked(msg, key, zk_seed=seed)
        return time.perf_counter() - t0, proofs

    def leg_cbc():
        t0 = time.perf_counter()
        ct, proofs = pk_c.encrypt_cbc_chunked(msg, key, iv, zk_seed=seed)
        dt = time.perf_counter() - t0
        assert ct == ct_c
        return dt, proofs

    def verify_ecb(proofs):
        return sum(api.verify_encryption(vk_e, p, ct_e[chunk * j:chunk * (j + 1)]) for j, p in enumerate(proofs))

    def verify_cbc(proofs):
        return sum(api.verify_cbc_chunked(vk_c, proofs, iv, ct_c))

    # warm-up: one full leg each (creates every context's workspace, fills the caches a timed leg finds filled)
    for leg, ver in ((leg_ecb, verify_ecb), (leg_cbc, verify_cbc)):
        _, proofs = leg()
        assert ver(proofs) == args.chunks

    blocks = BLOCKS * args.chunks
    legs = {"ecb": [], "cbc": []}
    verified = {"ecb": 0, "cbc": 0}
    for _ in range(args.rounds):
        for name, leg, ver in (("ecb", leg_ecb, verify_ecb), ("cbc", leg_cbc, verify_cbc)):
            dt, proofs = leg()
            legs[name].append(dt)
            verified[name] += ver(proofs)                     # outside the timed region
    t0 = time.perf_counter()
    api.cbc_ciphertext(msg, key, iv)
    host_chain_ms = 1e3 * (time.perf_counter() - t0)

    def rate(dt):
        return blocks / dt

    med = {k: float(np.median([rate(dt) for dt in v])) for k, v in legs.items()}
    ecb_rates = [rate(dt) for dt in legs["ecb"]]
    out = {
        "what": "chunked proving, %d chunks of %d blocks, same message and AES key, ECB and CBC legs alternating in one process after a warm-up leg each" % (args.chunks, BLOCKS),
        "cmd": "python tools/cbc_vs_ecb.py --chunks %d --rounds %d" % (args.chunks, args.rounds),
        "contexts": contexts,
        "window_tables": {"ecb": pk_e.tables_built()[0], "cbc": pk_c.tables_built()[0]},
        "h": int(ic["h"]), "k": int(ic["k"]), "x": int(ic["instance"]),
        "raw_constraints": {"ecb": int(ie["raw_constraints"]), "cbc": int(ic["raw_constraints"])},
        "joint_nnz": {"ecb": int(ie["joint_nnz"]), "cbc": int(ic["joint_nnz"])},
        "blocks_per_leg": blocks,
        "blocks_per_s": {k: [round(rate(dt), 3) for dt in v] for k, v in legs.items()},
        "median_blocks_per_s": {k: round(v, 3) for k, v in med.items()},
        "cbc_over_ecb": round(med["cbc"] / med["ecb"], 4),
        "ecb_spread": round((max(ecb_rates) - min(ecb_rates)) / med["ecb"], 4),
        "ecb_spread_note": "(max - min) / median of the ECB legs' blocks/s: what run-to-run noise looks like in this process",
        "host_chain_ms": round(host_chain_ms, 3),
        "proofs_verified": {k: "%d/%d" % (v, args.chunks * args.rounds) for k, v in verified.items()},
        "key_setup_s": round(setup_s, 2),
    }
    assert all(v == args.chunks * args.rounds for v in verified.values()), out["proofs_verified"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
