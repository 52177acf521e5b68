"""What a key tag costs on a GCM segment head: proofs of the head key at the default c (A = 13) with key_tag_blocks = 0 against the head key at the same c with
key_tag_blocks = 1, in ONE process over the shared default universal SRS, the legs alternating for three rounds after a warm-up leg each, every proof verified against
the public input the Python models give for its header (ciphertext under ctr0 = 2, com_out, and for the tagged leg the key's tag).

    python tools/gcm_segments_keytag_vs_plain.py [--proofs 48] [--rounds 3] [--out profiles/gcm_segments_keytag.json]      (run on the GPU box)

Writes proofs/s per leg (the median of the rounds), the ratio of the tagged leg to the plain leg and each leg's own run-to-run spread, (max - min) / median.  No
threshold is fixed in advance: the yardstick is the T = 0 leg of the same run and its own spread, never a constant.  Measurement only -- nothing here is a pass/fail
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
import gcm_segment_keytag_model as keytag_model
import gcm_segment_model as model
import gcm_segment_reveal_model as reveal_model

LEGS = ("head_t0", "head_t1")
AAD = 13


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--proofs", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "gcm_segments_keytag.json"))
    args = ap.parse_args()
    n, c = args.proofs, api.GCM_SEGMENT_DEFAULT_C[128]
    assert c == api.GCM_SEGMENT_KEYTAG_DEFAULT_C[1][128]
    rs = np.random.RandomState(0x5EEF)
    seed = rs.bytes(32)
    msgs, keys_, ivs = [rs.bytes(16 * c) for _ in range(n)], [rs.bytes(16) for _ in range(n)], [rs.bytes(12) for _ in range(n)]
    aads, salts = [rs.bytes(AAD) for _ in range(n)], [rs.bytes(16) for _ in range(n)]
    headers = [api.gcm_segment_header(iv, 2, salt_out=s, aad=a) for iv, s, a in zip(ivs, salts, aads)]
    publics = {name: [] for name in LEGS}
    for m, k, iv, a, s in zip(msgs, keys_, ivs, aads, salts):                                   # what each proof must say, from the models
        tr = model.segment_trace("head", m, k, iv, 2, aad=a)
        plain = reveal_model.bits(iv + (2).to_bytes(4, "big") + a + tr["ct"] + model.commitment(k, tr["ys"][-1].to_bytes(16, "big"), s))
        publics["head_t0"].append(plain)
        publics["head_t1"].append(plain + reveal_model.bits(keytag_model.key_tag(k, 1)))

    t = time.perf_counter()
    keys = {"head_t0": api.synthesize_keys_gcm_segment("head", c, AAD), "head_t1": api.synthesize_keys_gcm_segment("head", c, AAD, key_tag_blocks=1)}
    setup_s = time.perf_counter() - t
    infos = {name: keys[name][0].info() for name in LEGS}
    contexts = keys["head_t0"][0].contexts()

    def leg(name):
        t0 = time.perf_counter()
        out = keys[name][0].encrypt_gcm_segment_batch(msgs, keys_, headers, zk_seed=seed)        # the same entry for both legs: the tag's witness comes from the key
        return time.perf_counter() - t0, out

    def verify(name, out):
        return sum(keys[name][1].verify(p, pub) for p, pub in zip(out, publics[name]))

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

    proofs_s = {name: [n / dt for dt in v] for name, v in times.items()}
    med = {name: float(np.median(v)) for name, v in proofs_s.items()}
    spread = {name: round((max(v) - min(v)) / med[name], 4) for name, v in proofs_s.items()}
    out = {
        "what": "GCM segment proving, %d head proofs of %d message bytes at c = %d, A = %d per leg: the plain head key (T = 0) against the tagged head key (T = 1); legs "
                "alternating in one process after a warm-up leg each" % (n, 16 * c, c, AAD),
        "cmd": "python tools/gcm_segments_keytag_vs_plain.py --proofs %d --rounds %d" % (n, args.rounds),
        "contexts": contexts,
        "window_tables": {name: keys[name][0].tables_built()[0] for name in LEGS},
        "h_k_x": {name: [int(i["h"]), int(i["k"]), int(i["instance"])] for name, i in infos.items()},
        "raw_constraints": {name: int(i["raw_constraints"]) for name, i in infos.items()},
        "joint_nnz": {name: int(i["joint_nnz"]) for name, i in infos.items()},
        "proofs_per_s": {name: [round(v, 3) for v in vs] for name, vs in proofs_s.items()},
        "median_proofs_per_s": {name: round(v, 3) for name, v in med.items()},
        "keytag_over_plain": round(med["head_t1"] / med["head_t0"], 4),
        "spread": spread,
        "spread_note": "(max - min) / median of a leg's proofs/s over the rounds: what run-to-run noise looks like in this process",
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
