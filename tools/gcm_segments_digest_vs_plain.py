"""What a digest costs on a GCM segment: proofs of the mid key at c = 4 (AES-128) without a digest against the digest mid key at the same c, in ONE process
over the shared default universal SRS, the legs alternating for three rounds after a warm-up leg each, every proof verified against the public input the Python models
give for its header (ciphertext under its ctr0, com_in, com_out, and for the digest leg H_in and the chain state behind the segment's 64 bytes).

    python tools/gcm_segments_digest_vs_plain.py [--proofs 48] [--rounds 3] [--out profiles/gcm_segments_digest.json]      (run on the GPU box)

Writes proofs/s per leg (the median of the rounds), the ratio of the digest leg to the plain leg, each leg's own run-to-run spread, (max - min) / median, and the
witness_ms of each leg's last proof (trace kernels, witness expansion and the two sparse products: the digest leg has one more trace launch).  No threshold is fixed in
advance: the yardstick is the plain leg of the same run, and a difference counts only if it exceeds that leg's spread.  Measurement only -- nothing here is a pass/fail
threshold except that every proof must verify.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
try:
    import torch  # noqa: F401  -- before libzkaes.so where torch exists (tests/conftest.py: one process, two HIP runtimes)
except ImportError:
    pass
import numpy as np

from aes_zero_knowledge_proof_circuit_amd import api
import gcm_segment_digest_model as digest_model
import gcm_segment_model as model
import sha256_model

LEGS = ("mid_plain", "mid_digest")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--proofs", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "gcm_segments_digest.json"))
    args = ap.parse_args()
    n, c = args.proofs, api.GCM_SEGMENT_DIGEST_DEFAULT_C[128]
    assert c == api.GCM_SEGMENT_DEFAULT_C[128]
    rs = np.random.RandomState(0x5EF0)
    seed = rs.bytes(32)
    msgs, keys_, ivs = [rs.bytes(16 * c) for _ in range(n)], [rs.bytes(16) for _ in range(n)], [rs.bytes(12) for _ in range(n)]
    y_ins, s_ins, s_outs, h_ins = ([rs.bytes(16) for _ in range(n)], [rs.bytes(16) for _ in range(n)], [rs.bytes(16) for _ in range(n)], [rs.bytes(32) for _ in range(n)])
    ctr0 = 2 + c
    headers = {"mid_plain": [api.gcm_segment_header(iv, ctr0, y, a, b) for iv, y, a, b in zip(ivs, y_ins, s_ins, s_outs)],
               "mid_digest": [api.gcm_segment_header(iv, ctr0, y, a, b, h_in=h) for iv, y, a, b, h in zip(ivs, y_ins, s_ins, s_outs, h_ins)]}
    publics = {name: [] for name in LEGS}
    for m, k, iv, y, a, b, h in zip(msgs, keys_, ivs, y_ins, s_ins, s_outs, h_ins):                # what each proof must say, from the models
        tr = model.segment_trace("mid", m, k, iv, ctr0, y)
        plain = iv + ctr0.to_bytes(4, "big") + tr["ct"] + model.commitment(k, y, a) + model.commitment(k, tr["ys"][-1].to_bytes(16, "big"), b)
        publics["mid_plain"].append(digest_model.bits(plain))
        publics["mid_digest"].append(digest_model.bits(plain + h + sha256_model.chain(m, h)))

    t = time.perf_counter()
    keys = {"mid_plain": api.synthesize_keys_gcm_segment("mid", c), "mid_digest": api.synthesize_keys_gcm_segment("mid", c, digest=True)}
    setup_s = time.perf_counter() - t
    infos = {name: keys[name][0].info() for name in LEGS}
    contexts = keys["mid_plain"][0].contexts()

    def leg(name):
        t0 = time.perf_counter()
        pk = keys[name][0]
        fn = pk.encrypt_gcm_segment_digest_batch if name == "mid_digest" else pk.encrypt_gcm_segment_batch
        out = fn(msgs, keys_, headers[name], zk_seed=seed)
        return time.perf_counter() - t0, out

    def verify(name, out):
        return sum(keys[name][1].verify(p, pub) for p, pub in zip(out, publics[name]))

    for name in LEGS:                                                      # warm-up: one full leg each (every context's workspace, the caches a timed leg finds filled)
        _, out = leg(name)
        assert verify(name, out) == n
    times = {name: [] for name in LEGS}
    witness_ms = {name: [] for name in LEGS}
    verified = {name: 0 for name in LEGS}
    for _ in range(args.rounds):
        for name in LEGS:
            dt, out = leg(name)
            times[name].append(dt)
            witness_ms[name].append(round(float(keys[name][0].timings()["witness_ms"]), 3))      # the leg's last proof
            verified[name] += verify(name, out)                            # outside the timed region

    proofs_s = {name: [n / dt for dt in v] for name, v in times.items()}
    med = {name: float(np.median(v)) for name, v in proofs_s.items()}
    spread = {name: round((max(v) - min(v)) / med[name], 4) for name, v in proofs_s.items()}
    out = {
        "what": "GCM segment proving, %d mid proofs of %d message bytes at c = %d per leg: the plain mid key against the digest mid key (one SHA-256 compression, 512 more "
                "public input bits); legs alternating in one process after a warm-up leg each" % (n, 16 * c, c),
        "cmd": "python tools/gcm_segments_digest_vs_plain.py --proofs %d --rounds %d" % (n, args.rounds),
        "contexts": contexts,
        "window_tables": {name: keys[name][0].tables_built()[0] for name in LEGS},
        "h_k_x": {name: [int(i["h"]), int(i["k"]), int(i["instance"])] for name, i in infos.items()},
        "raw_constraints": {name: int(i["raw_constraints"]) for name, i in infos.items()},
        "joint_nnz": {name: int(i["joint_nnz"]) for name, i in infos.items()},
        "proofs_per_s": {name: [round(v, 3) for v in vs] for name, vs in proofs_s.items()},
        "median_proofs_per_s": {name: round(v, 3) for name, v in med.items()},
        "digest_over_plain": round(med["mid_digest"] / med["mid_plain"], 4),
        "spread": spread,
        "spread_note": "(max - min) / median of a leg's proofs/s over the rounds: what run-to-run noise looks like in this process",
        "witness_ms": witness_ms,
        "witness_ms_note": "witness_ms of the last proof of every timed leg, a throughput call over all contexts: a figure, not a bound",
        "proofs_verified": {name: "%d/%d" % (v, n * args.rounds) for name, v in verified.items()},
        "key_setup_s": round(setup_s, 2),
    }
    assert all(v == n * args.rounds for v in verified.values()), out["proofs_verified"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
