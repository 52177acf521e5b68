"""What a key tag costs: the same 48-chunk ECB job proven with the untagged 6-block key, the 5 data + 1 tag block key and the 4 data + 2 tag block key, in ONE process
over the shared default universal SRS, the legs alternating for three rounds after a warm-up leg each, every proof verified (the tagged ones against ONE tag).

    python tools/keytag_vs_ecb.py [--chunks 48] [--rounds 3] [--out profiles/keytag_vs_ecb.json]      (run on the GPU box)

Writes proofs/s and data blocks/s per leg, the ratios to ECB, ECB's own run-to-run spread and the witness_ms of a lone proof per leg.  The yardstick is the ECB leg of
the same run, never a constant.  All three chunks have |H| = 2^20, |K| = 2^22, |X| = 1024, and the tool asserts that their transform and MSM op lists are equal
(ProvingKey.op_lists), so proofs/s is expected inside ECB's spread and data blocks/s at 5/6 and 4/6 of it; a tag block adds one lane per proof to the trace kernels,
microseconds of witness_ms.  Measurement only -- nothing here is a pass/fail threshold except the op-list equality and that every proof must verify.
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

LEGS = (("ecb_6+0", 6, 0), ("tag_5+1", 5, 1), ("tag_4+2", 4, 2))           # name, data blocks, tag blocks: six AES blocks of circuit each


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "keytag_vs_ecb.json"))
    args = ap.parse_args()
    rs = np.random.RandomState(0x5EED)
    whole, key, seed = rs.bytes(96 * args.chunks), rs.bytes(16), rs.bytes(32)

    t = time.perf_counter()
    keys = {name: api.synthesize_keys(16 * data, key_tag_blocks=tags) for name, data, tags in LEGS}
    setup_s = time.perf_counter() - t
    infos = {name: keys[name][0].info() for name, _, _ in LEGS}
    shape = {name: (int(i["h"]), int(i["k"]), int(i["instance"])) for name, i in infos.items()}
    assert len(set(shape.values())) == 1, shape
    contexts = keys["ecb_6+0"][0].contexts()
    msgs = {name: whole[:16 * data * args.chunks] for name, data, _ in LEGS}
    cts = {name: api.ecb_ciphertext(msgs[name], key) for name, _, _ in LEGS}
    tags_of = {name: (api.key_tag(key, tags) if tags else None) for name, _, tags in LEGS}

    # the op lists of one proof on the throughput path: equal sizes and kinds, launch by launch
    ops = {name: keys[name][0].op_lists(msgs[name][:16 * data], key) for name, data, _ in LEGS}
    for name, _, _ in LEGS[1:]:
        assert ops[name]["ntt"] == ops["ecb_6+0"]["ntt"] and ops[name]["msm"] == ops["ecb_6+0"]["msm"], (name, "op lists differ from ECB's")

    def leg(name):
        t0 = time.perf_counter()
        proofs = keys[name][0].encrypt_chunked(msgs[name], key, zk_seed=seed)
        return time.perf_counter() - t0, proofs

    def verify(name, data, tags, proofs):
        vk, chunk = keys[name][1], 16 * data
        if tags:
            return sum(api.verify_chunked_tagged(vk, api.CIRCUIT_AES, proofs, cts[name], tags_of[name]))
        return sum(api.verify_encryption(vk, p, cts[name][chunk * j:chunk * (j + 1)]) for j, p in enumerate(proofs))

    for name, data, tags in LEGS:                                          # warm-up: one full leg each (every context's workspace, the caches a timed leg finds filled)
        _, proofs = leg(name)
        assert verify(name, data, tags, proofs) == args.chunks
    times = {name: [] for name, _, _ in LEGS}
    verified = {name: 0 for name, _, _ in LEGS}
    for _ in range(args.rounds):
        for name, data, tags in LEGS:
            dt, proofs = leg(name)
            times[name].append(dt)
            verified[name] += verify(name, data, tags, proofs)             # outside the timed region
    witness_ms = {}
    for name, data, _ in LEGS:                                             # one lone proof per leg for the prover's own phase timer
        api.encrypt(msgs[name][:16 * data], key, keys[name][0])
        witness_ms[name] = round(float(keys[name][0].timings()["witness_ms"]), 4)

    proofs_s = {name: [args.chunks / dt for dt in v] for name, v in times.items()}
    med = {name: float(np.median(v)) for name, v in proofs_s.items()}
    data_of = {name: data for name, data, _ in LEGS}
    ecb = proofs_s["ecb_6+0"]
    out = {
        "what": "chunked ECB proving, %d chunk-proofs per leg, same AES key, six AES blocks of circuit per proof: 6 data, 5 data + 1 key-tag, 4 data + 2 key-tag; legs alternating "
                "in one process after a warm-up leg each" % args.chunks,
        "cmd": "python tools/keytag_vs_ecb.py --chunks %d --rounds %d" % (args.chunks, args.rounds),
        "contexts": contexts,
        "window_tables": {name: keys[name][0].tables_built()[0] for name, _, _ in LEGS},
        "h": shape["ecb_6+0"][0], "k": shape["ecb_6+0"][1], "x": shape["ecb_6+0"][2],
        "op_lists_equal": True,
        "raw_constraints": {name: int(i["raw_constraints"]) for name, i in infos.items()},
        "joint_nnz": {name: int(i["joint_nnz"]) for name, i in infos.items()},
        "proofs_per_s": {name: [round(v, 3) for v in vs] for name, vs in proofs_s.items()},
        "median_proofs_per_s": {name: round(v, 3) for name, v in med.items()},
        "median_data_blocks_per_s": {name: round(med[name] * data_of[name], 3) for name in med},
        "proofs_per_s_over_ecb": {name: round(med[name] / med["ecb_6+0"], 4) for name in med},
        "data_blocks_per_s_over_ecb": {name: round(med[name] * data_of[name] / (med["ecb_6+0"] * 6), 4) for name in med},
        "ecb_spread": round((max(ecb) - min(ecb)) / med["ecb_6+0"], 4),
        "ecb_spread_note": "(max - min) / median of the ECB legs' proofs/s: what run-to-run noise looks like in this process",
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
