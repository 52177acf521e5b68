"""What the two GCM trace kernels cost: witness_ms (trace kernels + k_witness_expand + the two SpMVs + the instance read-back, ProverTimings) of a lone proof under the
(17, 5) GCM key against a 64-byte CTR key -- both have four AES blocks -- in ONE process, after a warm-up proof each, legs alternating, median of five.

    python tools/gcm_witness_ms.py [--rounds 5] [--out profiles/gcm_witness_ms.json]      (run on the GPU box)

Measurement only: no threshold, the comparison is against CTR in the same run.  Both keys sit on SRSs sized for their own circuits, without window tables.  The GCM
circuit is larger (688,557 constraints against CTR's 631,255, |H| = 2^20 for both), so the ratio holds the longer expand and SpMV as well as the GHASH kernel.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
try:
    import torch  # noqa: F401  -- before libzkaes.so where torch exists (tests/conftest.py: one process, two HIP runtimes)
except ImportError:
    pass
import numpy as np

from aes_zero_knowledge_proof_circuit_amd import api


def small_srs(kind, length, alen=0):
    ci = api.circuit_info(kind, length, alen)
    return (int(ci["constraints"]), int(ci["instance"]), int(ci["nnz_a"] + ci["nnz_b"] + ci["nnz_c"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "gcm_witness_ms.json"))
    args = ap.parse_args()
    rs = np.random.RandomState(0x6C3)
    key, iv, aad, icb = rs.bytes(16), rs.bytes(12), rs.bytes(5), rs.bytes(16)
    msg_g, msg_c = rs.bytes(17), rs.bytes(64)
    pk_g, vk_g = api.synthesize_keys_gcm(17, 5, srs=small_srs(api.CIRCUIT_AES_GCM, 17, 5), flags=api.KEY_NO_TABLES)
    pk_c, vk_c = api.synthesize_keys(64, circuit=api.CIRCUIT_AES_CTR, srs=small_srs(api.CIRCUIT_AES_CTR, 64), flags=api.KEY_NO_TABLES)

    def leg_gcm():
        ct, tag, proof = api.encrypt_gcm(msg_g, key, iv, aad, pk_g, zk_seed=bytes(32))
        t = pk_g.timings()
        assert api.verify_encryption_gcm(vk_g, proof, iv, aad, ct, tag)
        return t

    def leg_ctr():
        ct, proof = api.encrypt_ctr(msg_c, key, icb, pk_c, zk_seed=bytes(32))
        t = pk_c.timings()
        assert api.verify_encryption_ctr(vk_c, proof, icb, ct)
        return t

    leg_gcm(), leg_ctr()                                      # warm-up: every context buffer exists, every kernel has been loaded
    runs = {"gcm": [], "ctr": []}
    for _ in range(args.rounds):
        runs["gcm"].append(leg_gcm())
        runs["ctr"].append(leg_ctr())
    med = {k: float(np.median([t["witness_ms"] for t in v])) for k, v in runs.items()}
    ig, ic = pk_g.info(), pk_c.info()
    out = {
        "what": "witness_ms of a lone proof, GCM key (L, A) = (17, 5) against a 64-byte CTR key (four AES blocks each), one process, a warm-up proof each, legs alternating",
        "cmd": "python tools/gcm_witness_ms.py --rounds %d" % args.rounds,
        "raw_constraints": {"gcm": int(ig["raw_constraints"]), "ctr": int(ic["raw_constraints"])},
        "h": {"gcm": int(ig["h"]), "ctr": int(ic["h"])},
        "witness_ms": {k: [round(t["witness_ms"], 4) for t in v] for k, v in runs.items()},
        "median_witness_ms": {k: round(v, 4) for k, v in med.items()},
        "gcm_over_ctr": round(med["gcm"] / med["ctr"], 4),
        "median_total_ms": {k: round(float(np.median([t["total_ms"] for t in v])), 3) for k, v in runs.items()},
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
