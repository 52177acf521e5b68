"""What a GCM segment costs: proofs of the mid key at the default c (four data blocks, GHASH from a hidden Y_in, two boundary commitments) against records of the lone
(64, 0) GCM key (four data blocks, H, J_0, five multiplications, the tag), in ONE process over the shared default universal SRS, the legs alternating for three rounds
after a warm-up leg each, every proof verified -- the lone records with verify_encryption_gcm, the mid proofs against the public input the Python model gives for
their headers (ciphertext under ctr0, both commitments).

    python tools/gcm_segments_vs_gcm.py [--proofs 48] [--rounds 3] [--out profiles/gcm_segments.json]      (run on the GPU box)

Writes proofs/s per leg, the ratio to the lone key, that leg's own run-to-run spread and the witness_ms of a lone proof per leg.  The yardstick is the lone leg of the
same run, never a constant.  A mid proof and a lone record cover the same 64 message bytes, so proofs/s is also bytes/s.  Measurement only -- nothing here is a
pass/fail threshold except that every proof must verify.
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
import gcm_segment_model as model

LEGS = ("lone_64_0", "mid_c4")


def bits(data):
    return bytes((b >> i) & 1 for b in data for i in range(8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--proofs", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "gcm_segments.json"))
    args = ap.parse_args()
    n, c = args.proofs, api.GCM_SEGMENT_DEFAULT_C[128]
    rs = np.random.RandomState(0x5EED)
    seed = rs.bytes(32)
    msgs, keys_, ivs = [rs.bytes(16 * c) for _ in range(n)], [rs.bytes(16) for _ in range(n)], [rs.bytes(12) for _ in range(n)]
    y_ins, salts = [rs.bytes(16) for _ in range(n)], [(rs.bytes(16), rs.bytes(16)) for _ in range(n)]
    ctr0s = [2 + c * (1 + i % 250) for i in range(n)]
    headers = [api.gcm_segment_header(iv, ctr0, y, s[0], s[1]) for iv, ctr0, y, s in zip(ivs, ctr0s, y_ins, salts)]
    publics = []
    for m, k, iv, ctr0, y, s in zip(msgs, keys_, ivs, ctr0s, y_ins, salts):                     # what each mid proof must say, from the model
        tr = model.segment_trace("mid", m, k, iv, ctr0, y)
        publics.append(bits(iv + ctr0.to_bytes(4, "big") + tr["ct"] + model.commitment(k, y, s[0]) + model.commitment(k, tr["ys"][-1].to_bytes(16, "big"), s[1])))

    t = time.perf_counter()
    keys = {"lone_64_0": api.synthesize_keys_gcm(16 * c, 0), "mid_c4": api.synthesize_keys_gcm_segment("mid", c)}
    setup_s = time.perf_counter() - t
    infos = {name: keys[name][0].info() for name in LEGS}
    contexts = keys["lone_64_0"][0].contexts()

    def leg(name):
        t0 = time.perf_counter()
        if name == "lone_64_0":
            out = keys[name][0].encrypt_gcm_batch(msgs, keys_, ivs, [b""] * n, zk_seed=seed)
        else:
            out = keys[name][0].encrypt_gcm_segment_batch(msgs, keys_, headers, zk_seed=seed)
        return time.perf_counter() - t0, out

    def verify(name, out):
        vk = keys[name][1]
        if name == "lone_64_0":
            cts, tags, proofs = out
            return sum(api.verify_encryption_gcm(vk, p, iv, b"", ct, tag) for p, iv, ct, tag in zip(proofs, ivs, cts, tags))
        return sum(vk.verify(p, pub) for p, pub in zip(out, publics))

    for name in LEGS:                                                      # warm-up: one full leg each (every context's workspace, the caches a timed leg finds filled)
        _, out = leg(name)
        assert verify(name, out) == n
    times = {name: [] for name in LEGS}
    verified = {name: 0 for name in LEGS}
    for _ in range(args.rounds):
        for name in LEGS:
            dt, out = leg(name)
            times[name].append(dt)
            verified[name] += verify(name, out)                            # outside the timed region
    witness_ms = {}
    api.encrypt_gcm(msgs[0], keys_[0], ivs[0], b"", keys["lone_64_0"][0], zk_seed=seed)         # one lone proof per leg for the prover's own phase timer
    witness_ms["lone_64_0"] = round(float(keys["lone_64_0"][0].timings()["witness_ms"]), 4)
    keys["mid_c4"][0].encrypt_gcm_segment_batch(msgs[:1], keys_[:1], headers[:1], zk_seed=seed)
    witness_ms["mid_c4"] = round(float(keys["mid_c4"][0].timings()["witness_ms"]), 4)

    proofs_s = {name: [n / dt for dt in v] for name, v in times.items()}
    med = {name: float(np.median(v)) for name, v in proofs_s.items()}
    base = proofs_s["lone_64_0"]
    out = {
        "what": "GCM proving, %d proofs of 64 message bytes per leg: records of the lone (64, 0) key against proofs of the mid segment key at c = %d (Y_in hidden, two "
                "boundary commitments); legs alternating in one process after a warm-up leg each" % (n, c),
        "cmd": "python tools/gcm_segments_vs_gcm.py --proofs %d --rounds %d" % (n, args.rounds),
        "contexts": contexts,
        "window_tables": {name: keys[name][0].tables_built()[0] for name in LEGS},
        "h_k_x": {name: [int(i["h"]), int(i["k"]), int(i["instance"])] for name, i in infos.items()},
        "raw_constraints": {name: int(i["raw_constraints"]) for name, i in infos.items()},
        "joint_nnz": {name: int(i["joint_nnz"]) for name, i in infos.items()},
        "proofs_per_s": {name: [round(v, 3) for v in vs] for name, vs in proofs_s.items()},
        "median_proofs_per_s": {name: round(v, 3) for name, v in med.items()},
        "proofs_per_s_over_lone": {name: round(med[name] / med["lone_64_0"], 4) for name in med},
        "lone_spread": round((max(base) - min(base)) / med["lone_64_0"], 4),
        "lone_spread_note": "(max - min) / median of the lone legs' proofs/s: what run-to-run noise looks like in this process",
        "witness_ms_lone_proof": witness_ms,
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
