"""What a plaintext digest costs: the same 48-chunk ECB job proven with the 4 data + 2 tag block key and with the same key plus digest="chain" (one SHA-256 compression
per 64-byte chunk), in ONE process over the shared default universal SRS, the legs alternating for three rounds after a warm-up leg each, every proof verified (the
tagged ones against ONE tag, the digest ones also against ONE array of states, and the job's digest against hashlib).

    python tools/digest_vs_keytag.py [--chunks 48] [--rounds 3] [--out profiles/digest_vs_keytag.json]      (run on the GPU box)

Writes proofs/s per leg, the ratio to the tagged key without a digest, that leg's own run-to-run spread and the witness_ms of a lone proof per leg.  The yardstick is
the tagged leg of the same run, never a constant.  Both chunks have |H| = 2^20 and |K| = 2^22, but the digest's 512 public bits take |X| from 1024 to 2048, so the two
op lists (ProvingKey.op_lists) are compared and every difference is reported, none assumed away.  Measurement only -- nothing here is a pass/fail threshold except that
every proof must verify.
"""
import argparse
import hashlib
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

LEGS = (("tag_4+2", None), ("digest_4+2", "chain"))                      # name, digest kind: four data blocks and two tag blocks of circuit each
CHUNK = 64


def op_list_differences(a, b):
    """launch by launch: (index, what the first list has, what the second has) wherever the transform or MSM lists differ, a missing launch as None"""
    out = {}
    for kind in ("ntt", "msm"):
        la, lb = a[kind], b[kind]
        diff = [[i, la[i] if i < len(la) else None, lb[i] if i < len(lb) else None] for i in range(max(len(la), len(lb))) if i >= len(la) or i >= len(lb) or la[i] != lb[i]]
        out[kind] = {"launches": [len(la), len(lb)], "differ": diff}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "digest_vs_keytag.json"))
    args = ap.parse_args()
    rs = np.random.RandomState(0x5EED)
    msg, key, seed = rs.bytes(CHUNK * args.chunks), rs.bytes(16), rs.bytes(32)

    t = time.perf_counter()
    keys = {name: api.synthesize_keys(CHUNK, key_tag_blocks=2, digest=kind) for name, kind in LEGS}
    setup_s = time.perf_counter() - t
    infos = {name: keys[name][0].info() for name, _ in LEGS}
    shape = {name: (int(i["h"]), int(i["k"]), int(i["instance"])) for name, i in infos.items()}
    contexts = keys["tag_4+2"][0].contexts()
    ct, tag, want_digest = api.ecb_ciphertext(msg, key), api.key_tag(key, 2), hashlib.sha256(msg).digest()

    ops = {name: keys[name][0].op_lists(msg[:CHUNK], key) for name, _ in LEGS}
    differences = op_list_differences(ops["tag_4+2"], ops["digest_4+2"])

    def leg(name, kind):
        t0 = time.perf_counter()
        if kind:
            _, states, proofs = keys[name][0].encrypt_digest_chunked(msg, key, zk_seed=seed)
        else:
            states, proofs = None, keys[name][0].encrypt_chunked(msg, key, zk_seed=seed)
        return time.perf_counter() - t0, states, proofs

    def verify(name, kind, states, proofs):
        vk = keys[name][1]
        if not kind:
            return sum(api.verify_chunked_tagged(vk, api.CIRCUIT_AES, proofs, ct, tag))
        accepted, digest = api.verify_digest_chunked(vk, api.CIRCUIT_AES, proofs, ct, states, key_tag=tag)
        assert digest == want_digest, "the job's digest is not hashlib's"
        return sum(accepted)

    for name, kind in LEGS:                                                # warm-up: one full leg each (every context's workspace, the caches a timed leg finds filled)
        _, states, proofs = leg(name, kind)
        assert verify(name, kind, states, proofs) == args.chunks
    times = {name: [] for name, _ in LEGS}
    verified = {name: 0 for name, _ in LEGS}
    for _ in range(args.rounds):
        for name, kind in LEGS:
            dt, states, proofs = leg(name, kind)
            times[name].append(dt)
            verified[name] += verify(name, kind, states, proofs)           # outside the timed region
    witness_ms = {}
    for name, kind in LEGS:                                                # one lone proof per leg for the prover's own phase timer
        if kind:
            keys[name][0].encrypt_digest_batch([msg[:CHUNK]], [key], zk_seed=seed)
        else:
            api.encrypt(msg[:CHUNK], key, keys[name][0])
        witness_ms[name] = round(float(keys[name][0].timings()["witness_ms"]), 4)

    proofs_s = {name: [args.chunks / dt for dt in v] for name, v in times.items()}
    med = {name: float(np.median(v)) for name, v in proofs_s.items()}
    base = proofs_s["tag_4+2"]
    out = {
        "what": "chunked ECB proving, %d chunk-proofs of 64 bytes per leg, same AES key, four data blocks + two key-tag blocks per proof, without and with digest=\"chain\" "
                "(one SHA-256 compression per proof); legs alternating in one process after a warm-up leg each" % args.chunks,
        "cmd": "python tools/digest_vs_keytag.py --chunks %d --rounds %d" % (args.chunks, args.rounds),
        "contexts": contexts,
        "window_tables": {name: keys[name][0].tables_built()[0] for name, _ in LEGS},
        "h_k_x": {name: list(shape[name]) for name, _ in LEGS},
        "op_list_differences": differences,
        "raw_constraints": {name: int(i["raw_constraints"]) for name, i in infos.items()},
        "joint_nnz": {name: int(i["joint_nnz"]) for name, i in infos.items()},
        "proofs_per_s": {name: [round(v, 3) for v in vs] for name, vs in proofs_s.items()},
        "median_proofs_per_s": {name: round(v, 3) for name, v in med.items()},
        "proofs_per_s_over_tagged": {name: round(med[name] / med["tag_4+2"], 4) for name in med},
        "tagged_spread": round((max(base) - min(base)) / med["tag_4+2"], 4),
        "tagged_spread_note": "(max - min) / median of the tagged legs' proofs/s: what run-to-run noise looks like in this process",
        "witness_ms_lone_proof": witness_ms,
        "proofs_verified": {name: "%d/%d" % (v, args.chunks * args.rounds) for name, v in verified.items()},
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
