"""What selective disclosure costs: the same 48-chunk ECB job proven with the plain ECB-128 64-byte key and with the same key plus reveal=True (half of the bytes masked
in), in ONE process over the shared default universal SRS, the legs alternating for three rounds after a warm-up leg each, every proof verified (the reveal ones against
ONE mask and ONE array of revealed bytes over the whole job).

    python tools/reveal_vs_ecb.py [--chunks 48] [--rounds 3] [--out profiles/reveal_vs_ecb.json]      (run on the GPU box)

Writes proofs/s per round and leg, the ratio of the medians, each leg's own run-to-run spread, the witness_ms of a lone proof per leg and the op-list difference.  The
yardstick is the plain leg of the same run, never a constant.  Both chunks have |H| = 2^20 and |K| = 2^22, but the 9 L reveal bits take |X| from 1024 to 2048, so the two
op lists (ProvingKey.op_lists) are compared and every difference is reported, none assumed away.  Measurement only -- nothing here is a pass/fail threshold except that
every proof must verify.
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

LEGS = (("ecb_64", False), ("ecb_64_reveal", True))                     # name, reveal flag: four data blocks of circuit each
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
    ap.add_argument("--contexts", type=int, default=12)
    ap.add_argument("--out", default=os.path.join("profiles", "reveal_vs_ecb.json"))
    args = ap.parse_args()
    rs = np.random.RandomState(0x5EED)
    msg, key, seed = rs.bytes(CHUNK * args.chunks), rs.bytes(16), rs.bytes(32)
    mask = api.reveal_mask(range(0, len(msg), 2), len(msg))                # half of the bytes masked in
    revealed = api.reveal_bytes(msg, mask)

    t = time.perf_counter()
    keys = {name: api.synthesize_keys(CHUNK, reveal=rv) for name, rv in LEGS}
    setup_s = time.perf_counter() - t
    for pk, _ in keys.values():
        pk.set_contexts(args.contexts)
    infos = {name: keys[name][0].info() for name, _ in LEGS}
    shape = {name: (int(i["h"]), int(i["k"]), int(i["instance"])) for name, i in infos.items()}
    ct = api.ecb_ciphertext(msg, key)

    ops = {name: keys[name][0].op_lists(msg[:CHUNK], key) for name, _ in LEGS}
    differences = op_list_differences(ops["ecb_64"], ops["ecb_64_reveal"])

    def leg(name, rv):
        t0 = time.perf_counter()
        if rv:
            _, _, rev, proofs = keys[name][0].encrypt_reveal_chunked(msg, key, mask, zk_seed=seed)
            assert rev == revealed
        else:
            proofs = keys[name][0].encrypt_chunked(msg, key, zk_seed=seed)
        return time.perf_counter() - t0, proofs

    def verify(name, rv, proofs):
        vk = keys[name][1]
        if rv:
            return sum(api.verify_reveal_chunked(vk, api.CIRCUIT_AES, proofs, ct, mask, revealed))
        return sum(api.verify_encryption(vk, p, ct[CHUNK * j:CHUNK * (j + 1)]) for j, p in enumerate(proofs))

    for name, rv in LEGS:                                                  # warm-up: one full leg each (every context's workspace, the caches a timed leg finds filled)
        _, proofs = leg(name, rv)
        assert verify(name, rv, proofs) == args.chunks
    times = {name: [] for name, _ in LEGS}
    verified = {name: 0 for name, _ in LEGS}
    for _ in range(args.rounds):
        for name, rv in LEGS:
            dt, proofs = leg(name, rv)
            times[name].append(dt)
            verified[name] += verify(name, rv, proofs)                     # outside the timed region
    witness_ms = {}
    for name, rv in LEGS:                                                  # one lone proof per leg for the prover's own phase timer
        if rv:
            keys[name][0].encrypt_reveal_batch([msg[:CHUNK]], [key], [mask[:CHUNK // 8]], zk_seed=seed)
        else:
            api.encrypt(msg[:CHUNK], key, keys[name][0])
        witness_ms[name] = round(float(keys[name][0].timings()["witness_ms"]), 4)

    proofs_s = {name: [args.chunks / dt for dt in v] for name, v in times.items()}
    med = {name: float(np.median(v)) for name, v in proofs_s.items()}
    out = {
        "what": "chunked ECB-128 proving, %d chunk-proofs of 64 bytes per leg, same AES key, four data blocks per proof, without and with reveal=True (every second byte "
                "masked in); legs alternating in one process after a warm-up leg each" % args.chunks,
        "cmd": "python tools/reveal_vs_ecb.py --chunks %d --rounds %d --contexts %d" % (args.chunks, args.rounds, args.contexts),
        "contexts": {name: keys[name][0].contexts() for name, _ in LEGS},
        "window_tables": {name: keys[name][0].tables_built()[0] for name, _ in LEGS},
        "h_k_x": {name: list(shape[name]) for name, _ in LEGS},
        "op_list_differences": differences,
        "raw_constraints": {name: int(i["raw_constraints"]) for name, i in infos.items()},
        "joint_nnz": {name: int(i["joint_nnz"]) for name, i in infos.items()},
        "proofs_per_s": {name: [round(v, 3) for v in vs] for name, vs in proofs_s.items()},
        "median_proofs_per_s": {name: round(v, 3) for name, v in med.items()},
        "ratio_of_medians_reveal_over_plain": round(med["ecb_64_reveal"] / med["ecb_64"], 4),
        "spread": {name: round((max(v) - min(v)) / med[name], 4) for name, v in proofs_s.items()},
        "spread_note": "(max - min) / median of each leg's own proofs/s: what run-to-run noise looks like in this process",
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
