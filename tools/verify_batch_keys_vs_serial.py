"""Batch verification across keys against the per-proof verifier in ONE process: the segment-proofs of one GCM record -- one head, n - 2 mid and one tail proof under
three keys -- checked by four legs that alternate for three rounds after a warm-up of each:

  serial        verify_gcm_segments, one proof at a time on one host core: the code path before the multi-key batch, and the baseline;
  three_batches three single-key verify_batch calls on the device (head, mid, tail), rows from gcm_segment_public_inputs;
  host_keys     verify_gcm_segments_batch(device=False): ONE multi-key batch on the host;
  device_keys   verify_gcm_segments_batch(device=True): ONE multi-key batch on the device.

    python tools/verify_batch_keys_vs_serial.py [--bytes 1024 16384] [--rounds 3] [--out profiles/verify_batch_keys_vs_serial.json]      (run on the GPU box)

The record is AES-128-GCM at the default c (4 blocks, 64 bytes per segment) with 13 bytes of aad; a length that is a multiple of 64 keeps one tail key for every size.
Writes ms per record and per proof per leg, the ratios of the medians against the serial leg of the same run (never against a fixed number), and the multi-key legs'
split between parse / decompress / transcripts / x^ / MSM / pairing (zkaes_verify_batch_timings).  Measurement only -- nothing here is a pass/fail threshold except that
every leg must accept every proof.
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

STAGES = ("parse_ms", "decompress_ms", "transcripts_ms", "xhat_ms", "msm_ms", "pairing_ms")
AAD = 13


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, nargs="+", default=[1024])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tables", action="store_true", help="proving keys with window tables (faster proving, tens of GB per key)")
    ap.add_argument("--out", default=os.path.join("profiles", "verify_batch_keys_vs_serial.json"))
    args = ap.parse_args()
    c = api.GCM_SEGMENT_DEFAULT_C[128]
    seg = 16 * c
    if any(b % seg or b < 3 * seg for b in args.bytes):
        raise SystemExit("--bytes: multiples of %d, at least %d (head, mid and tail)" % (seg, 3 * seg))
    rs = np.random.RandomState(0x5EED)
    key, iv, aad, seed = rs.bytes(16), rs.bytes(12), rs.bytes(AAD), rs.bytes(32)

    flags = 0 if args.tables else api.KEY_NO_TABLES
    t = time.perf_counter()
    api.srs_hold(True)
    ks = [api.synthesize_keys_gcm_segment("head", c, AAD, flags=flags), api.synthesize_keys_gcm_segment("mid", c, flags=flags), api.synthesize_keys_gcm_segment("tail", seg, flags=flags)]
    api.srs_hold(False)
    pks, vks = tuple(k[0] for k in ks), tuple(k[1] for k in ks)
    setup_s = time.perf_counter() - t
    records, prove_s = {}, {}
    for length in args.bytes:
        msg = rs.bytes(length)
        t = time.perf_counter()
        ct, tag, coms, proofs = api.encrypt_gcm_segments(msg, key, iv, aad, pks, zk_seed=seed)
        prove_s[str(length)] = round(time.perf_counter() - t, 2)
        records[length] = (proofs, ct, tag, coms)
    for pk in pks:
        pk.free()                                              # the verifier legs hold verifying keys alone

    results = {}
    for length in args.bytes:
        proofs, ct, tag, coms = records[length]
        n = len(proofs)
        rows, roles = api.gcm_segment_public_inputs(n, iv, aad, ct, tag, coms, c)
        groups = [(vks[i], [p for p, r in zip(proofs, roles) if r == role], [row for row, r in zip(rows, roles) if r == role]) for i, role in enumerate(("head", "mid", "tail"))]

        def leg_serial():
            t0 = time.perf_counter()
            ok = sum(api.verify_gcm_segments(vks, proofs, iv, aad, ct, tag, coms, c))
            return time.perf_counter() - t0, ok, None

        def leg_three():
            t0 = time.perf_counter()
            ok = sum(sum(api.verify_batch(vk, ps, rws, device=True)) for vk, ps, rws in groups)
            return time.perf_counter() - t0, ok, None

        def leg_keys(device):
            t0 = time.perf_counter()
            ok = sum(api.verify_gcm_segments_batch(vks, proofs, iv, aad, ct, tag, coms, c, device=device))
            return time.perf_counter() - t0, ok, api.verify_batch_timings()

        legs_def = (("serial", leg_serial), ("three_batches", leg_three), ("host_keys", lambda: leg_keys(False)), ("device_keys", lambda: leg_keys(True)))
        for name, leg in legs_def:                             # warm-up: one full leg each
            assert leg()[1] == n, name
        legs = {name: [] for name, _ in legs_def}
        splits = {"host_keys": [], "device_keys": []}
        for _ in range(args.rounds):
            for name, leg in legs_def:
                dt, ok, split = leg()
                assert ok == n, (name, ok, n)
                legs[name].append(dt)
                if split is not None:
                    splits[name].append(split)
        med = {k: float(np.median(v)) for k, v in legs.items()}
        serial_ms = [1e3 * dt for dt in legs["serial"]]

        def split_median(name):
            d = {s: round(float(np.median([x[s] for x in splits[name]])), 3) for s in STAGES + ("total_ms",)}
            d["sub_batches"] = int(np.median([x["sub_batches"] for x in splits[name]]))
            return d
        results[str(length)] = {
            "segments": n,
            "ms_per_record": {k: [round(1e3 * dt, 3) for dt in v] for k, v in legs.items()},
            "median_ms_per_record": {k: round(1e3 * v, 3) for k, v in med.items()},
            "median_ms_per_proof": {k: round(1e3 * v / n, 4) for k, v in med.items()},
            "serial_over_three_batches": round(med["serial"] / med["three_batches"], 3),
            "serial_over_host_keys": round(med["serial"] / med["host_keys"], 3),
            "serial_over_device_keys": round(med["serial"] / med["device_keys"], 3),
            "three_batches_over_device_keys": round(med["three_batches"] / med["device_keys"], 3),
            "serial_spread": round((max(serial_ms) - min(serial_ms)) / float(np.median(serial_ms)), 4),
            "device_keys_split_ms_per_record": split_median("device_keys"),
            "host_keys_split_ms_per_record": split_median("host_keys"),
        }
    out = {
        "what": "verification of the segment-proofs of one AES-128-GCM record (c = %d, %d bytes of aad; head, mid and tail keys over the default SRS): verify_gcm_segments one proof at a "
                "time, three single-key device batches, the host multi-key batch and the device multi-key batch, legs alternating in one process after a warm-up leg each" % (c, AAD),
        "cmd": "python tools/verify_batch_keys_vs_serial.py --bytes %s --rounds %d%s" % (" ".join(str(b) for b in args.bytes), args.rounds, " --tables" if args.tables else ""),
        "rounds": args.rounds,
        "bytes": results,
        "serial_spread_note": "(max - min) / median of the serial legs' ms per record: what run-to-run noise looks like in this process",
        "key_setup_s": round(setup_s, 2),
        "prove_s": prove_s,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
