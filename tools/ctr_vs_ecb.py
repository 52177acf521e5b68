"""Chunked proving throughput of AES-128-CTR against AES-128-ECB in ONE process: the same 48-chunk message under a 6-block ECB key and a 6-block CTR key over
the shared universal SRS, legs alternating ECB / CTR for three rounds each after a warm-up of both, every proof verified.

    python tools/ctr_vs_ecb.py [--chunks 48] [--rounds 3] [--out profiles/ctr_vs_ecb.json]      (run on the GPU box)

Writes blocks/s per leg, the CTR / ECB ratio of the medians and ECB's own run-to-run spread.  The comparison is against ECB in the same run, never against a fixed
number: identical |H|, |K|, |X| mean identical transform and MSM op lists, and the extra work of CTR is 768 xor gates and five 253-gate incrementers per chunk; nothing
runs serially on the host ahead of the prover contexts.  Measurement only -- nothing here is a pass/fail threshold except that every proof must verify.
(tools/cbc_vs_ecb.py is the same measurement for CBC.)
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
    ap.add_argument("--out", default=os.path.join("profiles", "ctr_vs_ecb.json"))
    args = ap.parse_args()
    chunk = 16 * BLOCKS
    rs = np.random.RandomState(0x5EED)
    msg, key, icb = rs.bytes(chunk * args.chunks), rs.bytes(16), rs.bytes(16)
    seed = rs.bytes(32)

    t = time.perf_counter()
    pk_e, vk_e = api.synthesize_keys(chunk)
    pk_c, vk_c = api.synthesize_keys(chunk, circuit=api.CIRCUIT_AES_CTR)
    setup_s = time.perf_counter() - t
    ie, ic = pk_e.info(), pk_c.info()
    assert (ie["h"], ie["k"], ie["instance"]) == (ic["h"], ic["k"], ic["instance"]), (ie, ic)
    contexts = pk_e.contexts()
    assert pk_c.contexts() == contexts

    # expected ciphertexts from the host: CTR over the whole message; an ECB block is a one-block CBC message under a zero IV
    ct_c = api.ctr_crypt(msg, key, icb)
    ct_e = b"".join(api.cbc_ciphertext(msg[o:o + 16], key, bytes(16)) for o in range(0, len(msg), 16))

    def leg_ecb():
        t0 = time.perf_counter()
        proofs = pk_e.encrypt_chunked(msg, key, zk_seed=seed)
        return time.perf_counter() - t0, proofs

    def leg_ctr():
        t0 = time.perf_counter()
        ct, proofs = pk_c.encrypt_ctr_chunked(msg, key, icb, zk_seed=seed)
        dt = time.perf_counter() - t0
        assert ct == ct_c
        return dt, proofs

    def verify_ecb(proofs):
        return sum(api.verify_encryption(vk_e, p, ct_e[chunk * j:chunk * (j + 1)]) for j, p in enumerate(proofs))

    def verify_ctr(proofs):
        return sum(api.verify_ctr_chunked(vk_c, proofs, icb, ct_c))

    # warm-up: one full leg each (creates every context's workspace, fills the caches a timed leg finds filled)
    for leg, ver in ((leg_ecb, verify_ecb), (leg_ctr, verify_ctr)):
        _, proofs = leg()
        assert ver(proofs) == args.chunks

    blocks = BLOCKS * args.chunks
    legs = {"ecb": [], "ctr": []}
    verified = {"ecb": 0, "ctr": 0}
    for _ in range(args.rounds):
        for name, leg, ver in (("ecb", leg_ecb, verify_ecb), ("ctr", leg_ctr, verify_ctr)):
            dt, proofs = leg()
            legs[name].append(dt)
            verified[name] += ver(proofs)                     # outside the timed region

    def rate(dt):
        return blocks / dt

    med = {k: float(np.median([rate(dt) for dt in v])) for k, v in legs.items()}
    ecb_rates = [rate(dt) for dt in legs["ecb"]]
    out = {
        "what": "chunked proving, %d chunks of %d blocks, same message and AES key, ECB and CTR legs alternating in one process after a warm-up leg each" % (args.chunks, BLOCKS),
        "cmd": "python tools/ctr_vs_ecb.py --chunks %d --rounds %d" % (args.chunks, args.rounds),
        "contexts": contexts,
        "window_tables": {"ecb": pk_e.tables_built()[0], "ctr": pk_c.tables_built()[0]},
        "h": int(ic["h"]), "k": int(ic["k"]), "x": int(ic["instance"]),
        "raw_constraints": {"ecb": int(ie["raw_constraints"]), "ctr": int(ic["raw_constraints"])},
        "joint_nnz": {"ecb": int(ie["joint_nnz"]), "ctr": int(ic["joint_nnz"])},
        "blocks_per_leg": blocks,
        "blocks_per_s": {k: [round(rate(dt), 3) for dt in v] for k, v in legs.items()},
        "median_blocks_per_s": {k: round(v, 3) for k, v in med.items()},
        "ctr_over_ecb": round(med["ctr"] / med["ecb"], 4),
        "ecb_spread": round((max(ecb_rates) - min(ecb_rates)) / med["ecb"], 4),
        "ecb_spread_note": "(max - min) / median of the ECB legs' blocks/s: what run-to-run noise looks like in this process",
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
