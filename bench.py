#!/usr/bin/env python3
"""bench.py -- AES-ECB blocks proven per second (Marlin) on N x MI355X.

Default workload = BASELINE.json configs[2], the one the >=100x target is quoted on: ONE 4096-block (64 KiB) ECB message per GPU, proven as
682 chunk-proofs of 6 blocks + 1 of 4 with one proving key per chunk size (ECB blocks are independent, src/lib.rs:194; 6 blocks is the most
that fits |H| = 2^20, |K| = 2^22 and the reference's SRS literal).  The --steps timed steps SLICE that one message: step i proves the i-th
contiguous share of its chunk-proofs, witness generation -> serialized proof, SRS / index / circuit tables resident in HBM beforehand (the
region criterion times in the reference: benches/benchmark_encrypt.rs:45-47).  value = blocks of the whole message(s) / timed region.
The slices are issued through a 2-deep software pipeline (slice i+1 is submitted while slice i drains, as a streaming caller of the library would do), so
the chip does not idle between steps; the timed region is still exactly the --steps slices between two barriers.
Warm-up steps have the shape of the timed steps (the same slices through the same pipeline, over a separate message of the same length; the first covers
every prover context), so a warm-up step costs about what a timed step does.  Every timed proof is verified afterwards on the host (accept rate must be 100 %) together
with the reference's negative case (a wrong ciphertext must be rejected).
The timed proofs draw their prover randomness from one fixed 32-byte job seed (proof i: the job-global chunk index i, zkaes_encrypt_chunked_seeded_at), so that
the same arguments give the same proof bytes on every run and every build: `--dump-outputs DIR` writes the proofs of the last timed step there.

A plain run does only what the headline needs: set-up, warm-up, the timed steps, verification, the result line.  `--full` adds everything
measured beside it: the per-box integer-rate calibration, clock / power telemetry of the timed region, the one-context probe and the library's op
lists, the roofline and SRS reports, the `alt` and `latency_ms` legs, the `big` leg (child process) and the CPU-oracle baseline.

modes (all one process per GPU, torch.distributed over RCCL):
  headline (default at 1 GPU)   every rank proves its own --blocks message (default 4096)    -> "scaling": "weak", no data-path collective
  strong   (default at N > 1)   ONE --blocks message sharded over the ranks: rank r proves the contiguous chunk range split_chunks(n, r, world), the
                                proofs are all-gathered (the job's one exchange, inside the timed region) and rank 0 verifies every one.  Default size =
                                8192 blocks per rank, i.e. at 8 GPUs exactly BASELINE configs[3]'s 65,536-block (1 MiB) message (~130 s timed at every N;
                                "scaling": "weak" because the per-GPU share is what stays fixed).  An explicit --blocks fixes the whole job -> "strong".
  batch                         --proofs independent single-block proofs on one SRS (configs[4]), sharded the same way -> "scaling": "strong"

    python bench.py --gpus 1 --steps 4 --warmup 1
    python bench.py --gpus 1 --steps 4 --warmup 1 --full --dump-outputs bench_outputs/
    python bench.py --gpus 8                      # starts 8 ranks itself (re-executes under torch.distributed.run, rank r on GPU r)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...   # what the driver does
"""
import argparse
import json
import os
import sys
import threading
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
# one hardware queue per prover context (ROCclr default: 4 for all streams of the process); must be in the environment before the first HIP call,
# which under torchrun is torch's, not libzkaes' (csrc/runtime.hip sets the same default when the library is loaded first)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")

HBM_PEAK_GBS = 8000.0   # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
MADS_PER_ADD = 2649.0   # v_mad_u64_u32 per bucket addition of k_accumulate<EdwardsLaw> (7 Fq products x 378 + 3; disassembly of the gfx950 code object)
CIRCUIT_MODEL_NOTE = ("R1CS of the restated ark-r1cs-std 0.3.1 gadget semantics: 629,856 constraints / 3,002,900 non-zeros at 64 bytes; the reference's own SRS literal "
                      "(src/lib.rs:141) records 866,944 / 4,062,064 for that size and no variant of the source-less simpleworks shift/rotate calls reproduces it "
                      "(tools/circuit_variants.py, DESIGN.md section 2a) -- at the literal's density a 2^20 domain holds 4 blocks per chunk-proof, not 6: the `alt` object of this line is "
                      "that configuration MEASURED in this run (after the timed region); integration/check_on_cargo_box.sh is the run that settles which one is right")
ALT_CHUNK = 4            # blocks per chunk-proof that fit |H| = 2^20 at the density of the reference's SRS literal
LATENCY_BYTES = (16, 32, 64)   # the reference's own criterion shape: ONE encrypt() per message size (benches/benchmark.rs:8-10, benches/benchmark_encrypt.rs:39-49)

from aes_zero_knowledge_proof_circuit_amd import sharding  # noqa: E402
from tools import gpu_telemetry  # noqa: E402   (shader clock / socket power / temperature sampled beside the timed region: what the box was doing)

synthetic = sharding.synthetic_bytes


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2] if len(xs) % 2 else 0.5 * (xs[len(xs) // 2 - 1] + xs[len(xs) // 2])


def cpu_baseline(samples_small=0, samples_chunk=3, chunk_blocks=6, budget_s=300.0):
    """The CPU oracle (oracle/, a C restatement of the same algorithm; NOT arkworks) timed on this box's host cores, SRS + index prebuilt
    outside the timed part like the GPU side: `samples_chunk` proofs at the bench's own chunk size (the MEDIAN is the reported value; criterion reports a median-like
    estimate of its samples too, benches/benchmark_encrypt.rs:39-49) and optionally `samples_small` one-block chunk-proofs."""
    from oracle import zko
    nthreads = int(zko.lib().zko_api_num_threads())
    out = {"unit": "blocks/s", "cores": nthreads, "kind": "port", "by_chunk": {}}
    t_begin = time.perf_counter()
    for blocks, samples in ((1, samples_small), (chunk_blocks, samples_chunk)):
        if samples <= 0 or (blocks != 1 and time.perf_counter() - t_begin > budget_s):
            continue
        t0 = time.perf_counter()
        cs, _ = zko.synth_aes(bytes(16 * blocks), bytes(16))
        ix = zko.Index(cs)                       # setup (SRS + index), outside the timed region like the GPU side
        t_index = time.perf_counter() - t0
        times = []
        for i in range(samples):
            msg, key = synthetic(16 * blocks, 0x5EED + 1 + i), synthetic(16, 0x5EED)
            t0 = time.perf_counter()
            cs, _ = zko.synth_aes(msg, key)
            ix.prove(cs)
            times.append(time.perf_counter() - t0)
            if time.perf_counter() - t_begin > budget_s:
                break
        med, best = median(times), min(times)
        out["by_chunk"][str(blocks)] = {"blocks_per_s": round(blocks / med, 5), "median_s": round(med, 2), "best_s": round(best, 2), "samples_s": [round(t, 2) for t in times],
                                        "index_s": round(t_index, 1), "h": int(ix.info()["h"]), "k": int(ix.info()["k"])}
        del ix
    best_chunk = max(out["by_chunk"], key=lambda b: out["by_chunk"][b]["blocks_per_s"])
    out["value"] = out["by_chunk"][best_chunk]["blocks_per_s"]
    bc = out["by_chunk"][best_chunk]
    out["sample"] = "median of %d sample%s of one %s-block chunk-proof (%s s; %.1f s median, %.1f s best)%s" % (
        len(bc["samples_s"]), "" if len(bc["samples_s"]) == 1 else "s", best_chunk, ", ".join("%.1f" % t for t in bc["samples_s"]), bc["median_s"], bc["best_s"],
        "".join("; %s-block chunk: %s blocks/s" % (b, v["blocks_per_s"]) for b, v in out["by_chunk"].items() if b != best_chunk))
    out["threads_effective"] = "MSM: windows x point-slices tasks (all %d threads); NTT / polynomial loops: OpenMP static; synthesis + transcript: 1 thread" % nthreads
    return out


class _stdout_to_stderr:
    """file descriptor 1 -> stderr for the duration (native libraries that print on stdout); Python's own sys.stdout is flushed either side"""
    def __enter__(self):
        sys.stdout.flush()
        self.saved = os.dup(1)
        os.dup2(2, 1)
        return self

    def __exit__(self, *exc):
        sys.stdout.flush()
        os.dup2(self.saved, 1)
        os.close(self.saved)
        return False


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(dirname, proofs, indices):
    """--dump-outputs: the proofs of one timed step as DIR/proofs.npy (float32 [n, longest proof]: byte values 0..255, -1 past the end of a shorter proof) and
    DIR/proof_index.npy (float64: the job-global chunk index of each row).  Beyond 64 MB in all, a fixed seeded sample of the rows is written."""
    import numpy as np
    assert len(proofs) == len(indices), (len(proofs), len(indices))
    width = max((len(p) for p in proofs), default=0)
    rows = np.arange(len(proofs))
    max_rows = DUMP_LIMIT_BYTES // (4 * max(width, 1) + 8)
    if len(rows) > max_rows:
        rows = np.sort(np.random.RandomState(0x5EED).choice(len(rows), max_rows, replace=False))
    arr = np.full((len(rows), width), -1.0, dtype=np.float32)
    for j, i in enumerate(rows):
        arr[j, :len(proofs[i])] = np.frombuffer(proofs[i], dtype=np.uint8)
    np.save(os.path.join(dirname, "proofs.npy"), arr)
    np.save(os.path.join(dirname, "proof_index.npy"), np.asarray(indices, dtype=np.float64)[rows])


def even_slices(lo, hi, parts):
    """`parts` contiguous shares of [lo, hi), sizes differing by at most one"""
    return [tuple(lo + x for x in sharding.split_chunks(hi - lo, i, parts)) for i in range(parts)]


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--mode", choices=["headline", "strong", "batch"], default=None, help="default: headline on one rank, strong on several")
    ap.add_argument("--blocks", type=int, default=None, help="ECB blocks of the message (headline: per rank, default 4096; strong: whole job, default 8192 per rank = 65536 at 8 ranks)")
    ap.add_argument("--proofs", type=int, default=1024, help="batch mode: independent single-block proofs (whole job)")
    ap.add_argument("--chunk", type=int, default=6, help="blocks per chunk-proof (6 = the most that fits |H|=2^20, |K|=2^22 and the reference's SRS literal)")
    ap.add_argument("--contexts", type=int, default=12, help="chunk-proofs in flight per GPU (separate HIP streams; 8, 12 and 16 measure the same, profiles/r03_knobs.txt -- 12 holds ~56 GB of workspaces)")
    ap.add_argument("--pipeline", type=int, default=2, help="timed slices in flight (1 = strictly one after the other: the chip drains at every step boundary)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-chunk-samples", type=int, default=3, help="CPU-oracle samples at the bench's chunk size, ~60 s each; the median is reported (0 = one-block samples only)")
    ap.add_argument("--serial-probe", type=int, default=2, help="chunk-proofs proven one at a time after the timed region for un-overlapped kernel durations (0 = off)")
    ap.add_argument("--alt-proofs", type=int, default=64, help="one rank, headline mode: chunk-proofs of the %d-block alt leg measured after the timed region (0 = off)" % ALT_CHUNK)
    ap.add_argument("--latency-samples", type=int, default=5, help="one rank, headline mode: lone encrypt() calls timed per message size of the latency leg (0 = off)")
    ap.add_argument("--no-tables", action="store_true", help="synthesize the keys without the fixed-base window tables of the SRS (ZKAES_KEY_NO_TABLES: 2.4 GB instead of 31.4 GB per process; "
                                                             "~9 %% fewer proofs per second) -- for rehearsals of many ranks on one GPU")
    ap.add_argument("--big-chunk", type=int, default=28, help="one rank, headline mode: blocks per chunk-proof of the `big` leg -- the same prover over a universal SRS FOUR TIMES the reference's "
                                                              "literal, where 28 blocks fill |H| = 2^22 to 99.9 %% and |K| = 2^24 to 98 %% (6 fill 2^20 / 2^22 to 88 / 87 %%); measured in a child process after "
                                                              "everything else, reported beside `value`, never inside it (0 = off)")
    ap.add_argument("--big-proofs", type=int, default=16, help="chunk-proofs of the big leg")
    ap.add_argument("--big-contexts", type=int, default=4, help="prover contexts of the big leg (~19 GB each at 28 blocks)")
    ap.add_argument("--big-only", action="store_true", help=argparse.SUPPRESS)       # the child process of the big leg
    ap.add_argument("--calibrate-s", type=float, default=0.5, help="seconds of the per-box integer-rate calibration before and after the timed region (0 = off)")
    ap.add_argument("--cpu-small-samples", type=int, default=0, help="CPU-oracle samples of a one-block chunk-proof (~17 s each + 20 s of setup; off by default: the run stays under 400 s)")
    ap.add_argument("--full", action="store_true", help="also measure everything beside the headline (calibration, telemetry, one-context probe, roofline, SRS report, alt / latency / big "
                                                        "legs, CPU baseline); the options above that tune those legs take effect only with --full")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write the proofs of the last timed step to DIR/*.npy (float32 byte values; rank 0)")
    return ap



def big_leg(args, api):
    """The `big` leg (runs in a process of its own: bench.py --big-only): chunk-proofs of --big-chunk blocks over a universal SRS sized for them.  The reference hard-codes
    generate_universal_srs(866_944, 513, 4_062_064) (src/lib.rs:141), under which our R1CS model fits 6 blocks per proof and fills the radix-2 domains to 88 %; a deployment that
    proves long ECB messages is free to run a larger universal setup ONCE -- zkaes_synthesize_keys_ex takes the literals -- and then 28 blocks fill |H| = 2^22 to 99.9 % and
    |K| = 2^24 to 98.3 %: the same 4 x domain work for 28 blocks instead of 24, and four times fewer per-proof fixed costs.  NOT the reference's configuration: reported beside it."""
    B, nproofs, nctx = args.big_chunk, max(1, args.big_proofs), max(1, args.big_contexts)
    out = {"chunk_blocks": B, "unit": "blocks/s"}
    try:
        from oracle import zko   # checker only: byte-level AES for the expected ciphertext
        api.set_device(0)
        info = api.circuit_info(api.CIRCUIT_AES, 16 * B)
        h = 1
        while h < int(info["constraints"]):
            h <<= 1
        lits = (h, 513, 4 * h)                                   # |K| = 4 |H| holds the joint non-zeros (3.94 per constraint) at every size tried; synthesis fails loudly if not
        need = 13 * (3 * 4 * h) * 192 + nctx * 30 * 4 * h * 32 + (16 << 30)
        free_b, total_b = api.mem_info()
        out.update({"srs_literals": list(lits), "h": h, "k": 4 * h, "device_free_GB_before": round(free_b / 2**30, 1)})
        if free_b < need:
            out["skipped"] = "needs ~%d GB of free device memory (window tables of the larger SRS + %d contexts)" % (need >> 30, nctx)
            return out
        api.set_default_contexts(nctx)                              # what key synthesis reserves beside the tables
        t0 = time.perf_counter()
        pk, vk = api.synthesize_keys(16 * B, srs=lits)
        out["key_setup_s"] = round(time.perf_counter() - t0, 2)
        pk.set_contexts(nctx)
        key = synthetic(16, 0x5EED)
        msg = synthetic(16 * B * nproofs, 0x5EED + 2828)
        pk.encrypt_chunked(msg[:16 * B * min(nctx, nproofs)], key)  # warm-up: the contexts' workspaces
        t0 = time.perf_counter()
        proofs = pk.encrypt_chunked(msg, key)
        dt = time.perf_counter() - t0
        ct = zko.aes_encrypt(msg, key)
        with ThreadPoolExecutor(max_workers=min(32, os.cpu_count() or 4)) as pool:
            ok = sum(pool.map(lambda j: bool(api.verify_encryption(vk, proofs[j], ct[16 * B * j:16 * B * (j + 1)])), range(len(proofs))))
        bad = bytearray(ct[:16 * B]); bad[3] ^= 1
        # after the timing: the SAME path (window tables, multi-proof call) against the committed CPU-oracle fixture of this size, byte for byte (data under tests/golden/:
        # the oracle's 28-block proof over these SRS literals, 33 minutes of 8 cores; tests/golden/make_oracle_aes96.py 448)
        fx_path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tests", "golden", "oracle_aes%d.json" % (16 * B))
        if os.path.exists(fx_path):
            fx = json.load(open(fx_path))
            if fx.get("srs_literals") == list(lits):
                got = pk.encrypt_chunked(bytes.fromhex(fx["message"]), bytes.fromhex(fx["key"]), zk_seed=api.PARITY)
                out["proof_bytes_equal_oracle_fixture"] = bool(len(got) == 1 and got[0].hex() == fx["proof"])
        si, pi = pk.srs_info(), pk.info()
        f1, _ = api.mem_info()
        out.update({"value": round(B * len(proofs) / dt, 4), "proofs": len(proofs), "proofs_verified": "%d/%d" % (ok, len(proofs)), "ms_per_proof_in_flight": round(1e3 * dt / len(proofs), 1),
                    "wrong_ciphertext_rejected": not api.verify_encryption(vk, proofs[0], bytes(bad)), "contexts": nctx, "window_tables": bool(pk.tables_built()[0]),
                    "universal_srs_GB": round(si["bytes"] / 2**30, 1), "constraints": int(pi["constraints"]), "joint_nnz": int(pi["joint_nnz"]),
                    "domain_fill": {"H": round(int(pi["constraints"]) / h, 4), "K": round(int(pi["joint_nnz"]) / (4 * h), 4)}, "device_GB_in_use": round((total_b - f1) / 2**30, 1),
                    "note": "same prover, same kernels; universal SRS literals (%d, 513, %d) instead of the reference's (866944, 513, 4062064): NOT the reference's configuration" % (lits[0], lits[2])})
        pk.free()
    except Exception as e:                                          # noqa: BLE001 -- a leg beside the headline: it reports, it does not take the line down
        out["error"] = str(e)[:300]
    return out


def run(args, api, dist_env=None):
    """the rank path.  `api` = aes_zero_knowledge_proof_circuit_amd.api (the CPU tests drive this exact function with a stub prover)."""
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    import torch
    import torch.distributed as dist
    use_dist = world > 1 or "RANK" in os.environ            # under torchrun the RCCL group is created (and exercised) even for one rank
    # rehearsal hooks for a one-GPU box (not used by the driver): ZKAES_BENCH_BACKEND=gloo + ZKAES_BENCH_ONE_GPU=1 run N ranks on device 0
    backend = os.environ.get("ZKAES_BENCH_BACKEND", "nccl")
    device_ordinal = 0 if os.environ.get("ZKAES_BENCH_ONE_GPU") else local_rank      # (the CPU share below still goes by the true local rank)
    have_cuda = torch.cuda.is_available()
    if use_dist and not dist.is_initialized():
        if backend == "nccl":
            torch.cuda.set_device(device_ordinal)
            # this image's RCCL (2.26.6) prints a five-line version banner on STDOUT when its first communicator comes up; the contract is ONE JSON line on stdout, so the
            # group is created -- and its communicator forced into being by a first barrier -- with file descriptor 1 pointing at stderr
            with _stdout_to_stderr():
                dist.init_process_group("nccl", device_id=torch.device("cuda", device_ordinal))
                dist.barrier()
        else:
            dist.init_process_group(backend)
    coll_device = "cuda" if (use_dist and backend == "nccl") else None
    if api.device_count() <= 0:
        raise SystemExit("bench.py needs a HIP device: libzkaes has no CPU fallback")
    api.set_device(device_ordinal)

    affinity = sharding.bind_rank_cpus(local_rank, int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))) if world > 1 else None

    mode = args.mode or ("headline" if world == 1 else "strong")
    chunk = 1 if mode == "batch" else args.chunk
    STRONG_BLOCKS_PER_RANK = 8192                            # x 8 ranks = BASELINE configs[3]'s 65,536-block message
    total_blocks = args.proofs if mode == "batch" else (args.blocks or (STRONG_BLOCKS_PER_RANK * world if mode == "strong" else 4096))
    scaling = "weak" if (mode == "headline" or (mode == "strong" and not args.blocks)) else "strong"
    n_full, rem = divmod(total_blocks, chunk)
    n_chunks = n_full + (1 if rem else 0)                    # chunk-proof i < n_full has `chunk` blocks, the last one (if rem) has `rem`
    # ---- this rank's share of the chunk-proof list
    if mode == "headline":
        lo, hi = 0, n_chunks                                 # weak scaling: every rank its own whole message
        key = synthetic(16, 0x5EED)
        msg = synthetic(16 * total_blocks, 0x5EED + 1 + rank)
        keys16 = None
    else:
        lo, hi = sharding.split_chunks(n_chunks, rank, world)   # strong scaling: contiguous chunk range of ONE job
        key = synthetic(16, 0x5EED)
        msg = synthetic(16 * total_blocks, 0x5EED + 1)
        keys16 = synthetic(16 * total_blocks, 0x5EED + 2) if mode == "batch" else None   # batch: one key per proof
    # prover randomness of the timed proofs: one seed per job (headline: every rank its own job), proof i of the job at index i -- reproducible, and no two proofs of
    # a job share blinding factors
    job_seed = synthetic(32, 0x5EED + 3 + (rank if mode == "headline" else 0))
    if args.dump_outputs and rank == 0:
        os.makedirs(args.dump_outputs, exist_ok=True)          # (a bad path fails here, before any GPU work)
    contexts = max(1, args.contexts)
    t_setup = time.perf_counter()
    chunk_bytes = 16 * chunk
    need_full = min(hi, n_full) > lo or args.warmup > 0 or args.serial_probe > 0
    need_rem = bool(rem) and hi == n_chunks and hi > lo
    pk = vk = pk_rem = vk_rem = None
    key_flags = {"flags": api.KEY_NO_TABLES} if args.no_tables else {}
    key_setup_s = []
    if need_full:
        tk = time.perf_counter()
        pk, vk = api.synthesize_keys(chunk_bytes, **key_flags)
        key_setup_s.append(round(time.perf_counter() - tk, 2))
    if need_rem:                                              # (the second key over the same universal SRS: shares its powers and window tables)
        tk = time.perf_counter()
        pk_rem, vk_rem = api.synthesize_keys(16 * rem, **key_flags)
        key_setup_s.append(round(time.perf_counter() - tk, 2))
    for k_ in (pk, pk_rem):
        if k_ is not None and hasattr(k_, "set_contexts"):
            k_.set_contexts(contexts)                         # proofs in flight per multi-proof call on this key (zkaes_pk_set_contexts)
    setup_s = time.perf_counter() - t_setup
    info = (pk or pk_rem).info()

    def barrier():
        if use_dist:
            dist.barrier()
        if have_cuda:
            torch.cuda.synchronize()

    def prove_range(a, b, source=None, source_keys=None, seed=job_seed):
        """chunk-proofs [a, b) of this job -> list of proof bytes (the remainder chunk, if inside the range, is proven alongside on its own key).
        source / source_keys: another message (and batch keys) of the job's length instead, without the remainder chunk; seed None = a fresh OS seed per call"""
        m = source if source is not None else msg
        out_full, out_rem = [], []
        fa, fb = a, min(b, n_full)

        def run_rem():
            api.set_device(device_ordinal)                    # HIP's current device is per thread (libzkaes re-selects the key's device itself, too)
            out_rem.extend(pk_rem.encrypt_chunked(m[16 * chunk * n_full:16 * total_blocks], key, zk_seed=seed, first_proof_index=n_full))
        t = None
        if rem and b == n_chunks and b > a and source is None:
            t = threading.Thread(target=run_rem)
            t.start()
        if fb > fa:
            if mode == "batch":
                ks = source_keys if source_keys is not None else keys16
                out_full = pk.encrypt_batch([m[16 * i:16 * i + 16] for i in range(fa, fb)], [ks[16 * i:16 * i + 16] for i in range(fa, fb)], zk_seed=seed, first_proof_index=fa)
            else:
                out_full = pk.encrypt_chunked(m[chunk_bytes * fa:chunk_bytes * fb], key, zk_seed=seed, first_proof_index=fa)
        if t:
            t.join()
        return out_full + out_rem

    # ---- per-box calibration of the integer roof (the same kernel read 5.02 ... 5.54 ms per launch on five boxes): the isolated Fq product stream and the hot
    # loop over an L2-resident table, ~0.5 s, before anything is timed; repeated right after the timed region (a warm chip clocks lower)
    calibration = None
    if args.full and rank == 0 and args.calibrate_s > 0 and hasattr(api, "int_rate_bench"):
        try:
            calibration = {"before": api.int_rate_bench(args.calibrate_s)}
        except Exception as e:                                      # noqa: BLE001 -- the bench line says so instead of dying on a diagnostic
            calibration = {"error": str(e)[:200]}

    # ---- warm-up steps shaped like the timed ones: warm-up step j proves the chunk range of timed step j (mod --steps) of a separate message of the job's length,
    # through the same pipeline; the first covers at least `contexts` chunk-proofs (allocates every context's workspace outside the timed region)
    slices = even_slices(lo, hi, args.steps)
    warm_n = min(contexts, max(1, n_full))
    warm_msg = synthetic(16 * total_blocks, 0x5EED + 7777 + rank)
    warm_keys = synthetic(16 * total_blocks, 0x5EED + 7778) if mode == "batch" else None
    warm_slices = [slices[j % len(slices)] for j in range(args.warmup)]
    if warm_slices and min(warm_slices[0][1], n_full) - warm_slices[0][0] < warm_n:
        warm_slices[0] = (0, warm_n)

    def warm_slice(ab):
        api.set_device(device_ordinal)
        prove_range(*ab, source=warm_msg, source_keys=warm_keys, seed=None)
    with ThreadPoolExecutor(max_workers=max(1, args.pipeline)) as ex:
        list(ex.map(warm_slice, warm_slices))
    if need_rem and args.warmup > 0:
        pk_rem.encrypt_chunked(synthetic(16 * rem, 0x5EED + 7779), key)

    api.msm_stats(reset=True)
    phase = dict(witness_ms=0.0, round1_ms=0.0, round2_ms=0.0, round3_ms=0.0, open_ms=0.0, total_ms=0.0)
    proofs = []
    last_step = []                                                           # the proofs of the last timed step (--dump-outputs)
    telemetry = gpu_telemetry.Sampler(device_ordinal, 0.5) if (args.full and rank == 0) else None
    barrier()
    if telemetry:
        telemetry.__enter__()
    t0 = time.perf_counter()
    def timed_slice(ab):
        api.set_device(device_ordinal)
        r = prove_range(*ab)
        t = pk.timings() if (pk is not None and ab[1] > ab[0]) else None      # wall times of ONE chunk-proof of the step (sampled; several are in flight concurrently)
        return r, t
    with ThreadPoolExecutor(max_workers=max(1, args.pipeline)) as ex:        # slice i+1 starts while slice i drains: both queue on the same prover contexts
        for r, t in ex.map(timed_slice, slices):
            proofs.extend(r)
            last_step = r
            if t:
                for k, v in t.items():
                    phase[k] += v
    gathered = None
    if mode != "headline":
        gathered = sharding.gather_proofs(proofs, device=coll_device)    # the job's one exchange: ~855 B per chunk-proof to every rank
    barrier()
    elapsed = time.perf_counter() - t0
    if telemetry:
        telemetry.__exit__(None, None, None)
    stats = api.msm_stats()
    if calibration is not None and "before" in calibration:
        try:
            calibration["after"] = api.int_rate_bench(args.calibrate_s)
        except Exception as e:                                      # noqa: BLE001
            calibration["after_error"] = str(e)[:200]
    mem_after_timed = None
    if args.full and rank == 0 and hasattr(api, "mem_info"):
        try:
            f_, t_ = api.mem_info()
            mem_after_timed = t_ - f_                           # device bytes in use right after the timed region: the SRS + this rank's keys and prover contexts
        except Exception:
            pass

    # ---- un-overlapped kernel durations: a few chunk-proofs one at a time (outside the timed region; cross-check for the rocprof one-context profile)
    serial = oplists = None
    if args.full and args.serial_probe > 0 and rank == 0 and pk is not None and mode != "batch":
        pk.set_contexts(1)
        api.msm_stats(reset=True)
        ts = time.perf_counter()
        pk.encrypt_chunked(warm_msg[:chunk_bytes * min(args.serial_probe, warm_n)], key)
        t_serial = time.perf_counter() - ts
        s1 = api.msm_stats()
        pk.set_contexts(contexts)
        # the library's ACTUAL op lists of one chunk-proof on the path the timed region uses (zkaes_pk_op_lists: one proof with the op recorder open) -- SURVEY.md 8(d)
        if hasattr(pk, "op_lists"):
            oplists = pk.op_lists(warm_msg[:chunk_bytes], key, throughput_path=True)
        if s1["launches"]:
            serial = {"proofs": min(args.serial_probe, warm_n), "ms_per_proof": round(1e3 * t_serial / min(args.serial_probe, warm_n), 2),
                      "avg_launch_ms": round(s1["accumulate_ms"] / s1["launches"], 4), "launches": s1["launches"],
                      "algorithmic_bytes_per_launch": round(128.0 * s1["points"] / s1["launches"]), "pairs_per_launch": round(s1["pairs"] / s1["launches"]),
                      "achieved_GBs": round(128.0 * s1["points"] / 1e9 / (s1["accumulate_ms"] / 1e3), 2),
                      "int_multiplier_frac_vs_round3_reference_peak": round(MADS_PER_ADD * s1["pairs"] / 1e12 / (s1["accumulate_ms"] / 1e3) / 28.1, 4)}

    from oracle import zko   # checker only: byte-level AES for the expected ciphertext
    pool = ThreadPoolExecutor(max_workers=min(32, os.cpu_count() or 4))        # ctypes releases the GIL inside zkaes_verify_encryption

    # ---- two more MEASURED legs of the one-GPU headline run, after the timed region (they are reported beside `value`, never inside it):
    #   alt        the same prover at ALT_CHUNK blocks per chunk-proof -- what fits |H| = 2^20 if the reference's SRS literal, not our R1CS model, has the true density
    #   latency_ms ONE encrypt() per message size, keys resident: the reference's own criterion shape (benches/benchmark_encrypt.rs:45-47)
    alt = latency = None
    extra_keys = []                                             # every further proving key of the two legs below (released before the big leg)
    if args.full and world == 1 and mode == "headline" and rank == 0 and (args.alt_proofs > 0 or args.latency_samples > 0):
        small_keys = {}

        def key_for(nbytes):
            if nbytes == chunk_bytes and pk is not None:
                return pk, vk
            if rem and nbytes == 16 * rem and pk_rem is not None:
                return pk_rem, vk_rem
            if nbytes not in small_keys:
                small_keys[nbytes] = api.synthesize_keys(nbytes)
                extra_keys.append(small_keys[nbytes][0])
            return small_keys[nbytes]

        # (latency leg first: the 16- and 32-byte keys are synthesized while the device still has room for their window tables -- the library skips the tables of a key
        #  when the default number of contexts could not be created beside them -- and are released before the alt leg creates its contexts on the 4-block key)
        if args.latency_samples > 0:
            latency, lat_ok = {}, True
            for nbytes in LATENCY_BYTES:
                lpk, lvk = key_for(nbytes)
                lmsg = synthetic(nbytes, 0x5EED + 9000 + nbytes)
                api.encrypt(lmsg, key, lpk)                                                         # warm-up: lanes + workspaces of a lone call
                ts = []
                for _ in range(args.latency_samples):
                    tl = time.perf_counter()
                    lp = api.encrypt(lmsg, key, lpk)
                    ts.append(time.perf_counter() - tl)
                lat_ok = lat_ok and bool(api.verify_encryption(lvk, lp, zko.aes_encrypt(lmsg, key)))
                latency[str(nbytes)] = round(1e3 * sorted(ts)[len(ts) // 2], 2)
                latency.setdefault("min", {})[str(nbytes)] = round(1e3 * min(ts), 2)
                latency.setdefault("window_tables", {})[str(nbytes)] = bool(lpk.tables_built()[0])      # (skipped by the library when the device is short of memory)
            latency["samples"] = args.latency_samples
            latency["verified"] = lat_ok
        small_keys.clear()
        if args.alt_proofs > 0 and chunk != ALT_CHUNK:
            apk, avk = key_for(16 * ALT_CHUNK)
            amsg = synthetic(16 * ALT_CHUNK * args.alt_proofs, 0x5EED + 4242)
            apk.encrypt_chunked(amsg[:16 * ALT_CHUNK * min(contexts, args.alt_proofs)], key)          # warm-up: this key's prover contexts
            ta = time.perf_counter()
            aproofs = apk.encrypt_chunked(amsg, key)
            ta = time.perf_counter() - ta
            act = zko.aes_encrypt(amsg, key)
            aok = sum(pool.map(lambda j: bool(api.verify_encryption(avk, aproofs[j], act[16 * ALT_CHUNK * j:16 * ALT_CHUNK * (j + 1)])), range(len(aproofs))))
            ainfo = apk.info()
            alt = {"chunk_blocks": ALT_CHUNK, "value": round(ALT_CHUNK * len(aproofs) / ta, 4), "unit": "blocks/s", "proofs": len(aproofs), "proofs_verified": "%d/%d" % (aok, len(aproofs)),
                   "elapsed_s": round(ta, 3), "h": int(ainfo["h"]), "k": int(ainfo["k"]),
                   "note": "measured in this run after the timed region, same contexts; the headline value is what this prover does at %d blocks per chunk-proof" % chunk}

    # ---- acceptance: every timed proof must verify (host), the wrong-ciphertext negative must be rejected

    def chunk_ct(i, ct_all):
        return ct_all[chunk_bytes * i:chunk_bytes * (i + 1)] if i < n_full else ct_all[chunk_bytes * n_full:]

    def check(job):
        i, p, ct_all = job
        k = vk if i < n_full else vk_rem
        return bool(api.verify_encryption(k, p, chunk_ct(i, ct_all)))

    accepted = total = 0
    rejected_wrong = 1
    if mode == "headline":
        ct = zko.aes_encrypt(msg, key)
        jobs = [(lo + j, p, ct) for j, p in enumerate(proofs)]
        accepted, total = sum(pool.map(check, jobs)), len(jobs)
    elif rank == 0:
        if mode == "batch":
            ct = b"".join(zko.aes_encrypt(msg[16 * i:16 * i + 16], keys16[16 * i:16 * i + 16]) for i in range(total_blocks))
        else:
            ct = zko.aes_encrypt(msg, key)
        def vk_only(nbytes):       # rank 0 verifies chunk sizes it did not prove itself: a key without the window tables is enough to get the verifying key
            flags = getattr(api, "KEY_NO_TABLES", None)
            return api.synthesize_keys(nbytes, flags=flags)[1] if flags is not None else api.synthesize_keys(nbytes)[1]
        if vk is None:
            vk = vk_only(chunk_bytes)
        if rem and vk_rem is None:
            vk_rem = vk_only(16 * rem)
        jobs = [(i, p, ct) for i, p in enumerate(gathered)]
        accepted, total = sum(pool.map(check, jobs)), len(jobs)
        if total != n_chunks:
            accepted = -1                                       # a proof went missing in the gather
    if (mode == "headline" or rank == 0) and (proofs or gathered):
        first_i = lo if mode == "headline" else 0
        first_p = proofs[0] if mode == "headline" else gathered[0]
        bad = bytearray(chunk_ct(first_i, ct)); bad[1] ^= 1; bad[-1] ^= 1
        rejected_wrong = int(not api.verify_encryption(vk if first_i < n_full else vk_rem, first_p, bytes(bad)))
    elapsed, acc_sum, tot_sum, neg_sum = sharding.reduce_report(elapsed, accepted, total, rejected_wrong, device=coll_device)
    affinity_by_rank = sharding.gather_affinities(affinity, device=coll_device) if world > 1 else None

    out = None
    if rank == 0:
        job_blocks = total_blocks * (world if mode == "headline" else 1)
        value = job_blocks / elapsed
        workload = {
            "headline": "%d-block (%d B) ECB message per GPU as %d chunk-proofs of %d block(s)%s, sliced over the %d timed steps" % (total_blocks, 16 * total_blocks, n_full, chunk, (" + 1 of %d" % rem) if rem else "", args.steps),
            "strong": "ONE %d-block (%d B) ECB message%s as %d chunk-proofs of %d block(s)%s, chunk ranges sharded over %d rank(s), proofs all-gathered, rank 0 verifies all" % (
                total_blocks, 16 * total_blocks, " (BASELINE configs[3])" if total_blocks == 65536 else (" (%d blocks per rank: configs[3]'s per-GPU share)" % STRONG_BLOCKS_PER_RANK if not args.blocks else ""),
                n_full, chunk, (" + 1 of %d" % rem) if rem else "", world),
            "batch": "%d independent single-block proofs on one SRS (own key each), sharded over %d rank(s), proofs all-gathered, rank 0 verifies all" % (total_blocks, world),
        }[mode] + "; BLS12-377 Marlin, |H|=%d |K|=%d, universal SRS literals (866944,513,4062064)" % (info["h"], info["k"])
        out = {
            "metric": "AES-ECB blocks proven/sec (Marlin), proof verifies", "value": round(value, 4), "unit": "blocks/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(1e3 * elapsed / args.steps, 2),
            "higher_is_better": True, "scaling": scaling, "vs_baseline": None,
            "dtype": "u32 limbs (253-bit Fr / 377-bit Fq modular integers)",
            "data": "synthetic (numpy MT19937 bytes, seed 0x5EED; key fixed, message per rank)" if mode == "headline" else "synthetic (numpy MT19937 bytes, seed 0x5EED; one job shared by all ranks)",
            "config": {"workload": workload, "mode": mode, "blocks_total": job_blocks, "chunk_blocks": chunk, "proofs_total": n_chunks * (world if mode == "headline" else 1),
                       "proofs_per_step_per_gpu": round((hi - lo) / args.steps, 2), "contexts_per_gpu": contexts, "window_tables": not args.no_tables,
                       "parallelism": "independent chunk-proofs per rank, no data-path collective" if mode == "headline" else "chunk range per rank + one all-gather of proof bytes",
                       "circuit_model": CIRCUIT_MODEL_NOTE},
            "proofs_verified": "%d/%d" % (acc_sum, tot_sum), "wrong_ciphertext_rejected": bool(neg_sum == world),
            "setup_s": round(setup_s, 2), "key_setup_s": key_setup_s, "cpu_affinity": affinity, "cpu_affinity_by_rank": affinity_by_rank,
            "phase_ms_last_proof_avg": {k: round(v / args.steps, 2) for k, v in phase.items()},
        }
        if acc_sum != tot_sum or neg_sum != world or tot_sum != out["config"]["proofs_total"]:
            out["error"] = "verification failure"
        if args.full:
            srs_report = None
            if hasattr(pk or pk_rem, "srs_info"):
                si = (pk or pk_rem).srs_info()
                srs_report = {"universal_srs_bytes": si["bytes"], "copies": si["copies"], "points_per_copy": si["points_per_copy"], "keys_sharing_now": si["keys_sharing"],
                              "first_key_srs_build_s": round(si["srs_build_s"], 2), "lagrange_bytes": si["lagrange_bytes"],
                              "note": "ONE universal SRS (powers_of_g[0..=max_degree] + 12 window-table copies) per process and device, shared by every key (src/lib.rs:139-141); "
                                      "key_setup_s = wall seconds of synthesize_keys per key, in creation order -- the second key only indexes its circuit"}
                srs_report["device_bytes_in_use_after_timed_region"] = mem_after_timed
            # roofline of the dominant kernel (MSM bucket accumulation, kernels_msm.hip k_accumulate): algorithmic bytes per launch =
            # 128 B per point (96 B affine base + 32 B scalar) x points in the launch, divided by the kernel's CHIP time per launch.
            # HIP events on the kernel's own stream bracket every launch of the timed region, but 16 prover contexts overlap their launches (launch_overlap =
            # sum of in-situ durations / wall ~ 1.9), so an in-situ duration is stretched by whatever shares the chip with it and summing them counts the chip
            # twice (round 2's line did that).  Chip time = the un-overlapped duration: the one-context probe right after the timed region (same key, same
            # kernel, same launch shapes; this is what the one-context rocprof summary under profiles/ must agree with).  Self-check: launches per step x chip
            # time per launch must fit into a step.
            acc_ms, pts, launches = stats["accumulate_ms"], stats["points"], stats["launches"]
            in_situ_ms = acc_ms / max(launches, 1)
            overlap = acc_ms / (1e3 * elapsed) if elapsed > 0 else 0.0
            if serial:
                chip_ms, bytes_per_launch, chip_src = serial["avg_launch_ms"], serial["algorithmic_bytes_per_launch"], "one_context_probe (un-overlapped HIP-event duration, %d launches)" % serial["launches"]
                pairs_per_launch = serial["pairs_per_launch"]
            else:
                chip_ms, bytes_per_launch = in_situ_ms / max(1.0, overlap), 128.0 * pts / max(launches, 1)
                chip_src = "in-situ duration / launch_overlap (no one-context probe in this mode)"
                pairs_per_launch = stats["pairs"] / max(launches, 1)
            achieved = (bytes_per_launch / 1e9) / (chip_ms / 1e3) if chip_ms > 0 else 0.0
            kernel_ms_per_step = launches / max(args.steps, 1) * chip_ms
            traffic = traffic_src = None
            for name in ("r06_pmc_k_accumulate_tables.json", "r05_pmc_k_accumulate_tables.json", "r04_pmc_k_accumulate_tables.json", "r03_pmc_k_accumulate_tables.json", "r02_pmc_k_accumulate_tables.json"):
                try:
                    pmc = json.load(open(os.path.join(ROOT, "profiles", name)))
                    traffic = round(pmc["hbm_bytes_per_point_window"] * pairs_per_launch)
                    traffic_src = ("separate PMC run of the isolated kernel (profiles/%s, measured at commit %s: rocprofv3 --pmc bytes per (point, window) gather), scaled by this run's pairs per launch -- "
                                   "not counters of this run" % (name, pmc.get("measured_at_commit", "unrecorded (rounds 2-5 did not stamp their PMC files)")))
                    break
                except Exception:
                    pass
            try:
                copy_gbs = round(api.stream_copy_bench(1 << 30, 20), 1)
            except Exception:
                copy_gbs = None
            # ---- whole-proof algorithmic bytes: bytes = W + S + T + M from the library's ACTUAL op lists of one chunk-proof (zkaes_pk_op_lists), not a literal:
            #   W = 16 c + 16 + 32 V (message + key in, z written once);  S = 36 (nnzA + nnzB) + 36 (nnzA + nnzB + nnzC) + 32 V + 64 N (the two SpMVs + round 2's t pass);
            #   T = sum over transforms of 64 n_i (one read + one write);  M = sum over MSMs of 128 m_j (96 B affine base + 32 B scalar, each read once)
            proof_roof = None
            if oplists:
                V, N, (na, nb_, nc) = oplists["variables"], oplists["constraints"], oplists["nnz"]
                ntt_sizes = {}
                for n_i, cnt in oplists["ntt"]:
                    ntt_sizes[n_i] = ntt_sizes.get(n_i, 0) + cnt
                msm_by_kind = {}
                for m_j, kind in oplists["msm"]:
                    msm_by_kind.setdefault(kind, []).append(m_j)
                Wb = 16 * oplists["blocks"] + 16 + 32 * V
                Sb = 36 * (na + nb_) + 36 * (na + nb_ + nc) + 32 * V + 64 * N
                Tb = sum(64 * n_i * cnt for n_i, cnt in ntt_sizes.items())
                Mb = sum(128 * m_j for ms_ in msm_by_kind.values() for m_j in ms_)
                total_b = Wb + Sb + Tb + Mb
                proofs_per_s = (n_chunks * (world if mode == "headline" else 1)) / elapsed
                # (the remainder chunk-proof, if any, is counted at the full chunk's bytes: same |H|, |K|, same launches)
                proof_roof = {"W": Wb, "S": Sb, "T": Tb, "M": Mb, "bytes": total_b, "unit": "B per %d-block chunk-proof" % oplists["blocks"],
                              "ntt_list": {"transforms_by_size": {str(k_): v_ for k_, v_ in sorted(ntt_sizes.items())}, "launches": len(oplists["ntt"]),
                                           "transforms": sum(ntt_sizes.values())},
                              "msm_list": {kind: {"count": len(v_), "points": sum(v_), "sizes": sorted(v_, reverse=True)} for kind, v_ in sorted(msm_by_kind.items())},
                              "k_accumulate_launches_per_proof": len(msm_by_kind.get("buckets", [])) + len(msm_by_kind.get("second_bases", [])),
                              "path": oplists["path"], "h": oplists["h"], "k": oplists["k"],
                              "proofs_per_s": round(proofs_per_s / max(world, 1), 3), "achieved_GBs": round(total_b * proofs_per_s / max(world, 1) / 1e9, 2),
                              "frac": round(total_b * proofs_per_s / max(world, 1) / 1e9 / HBM_PEAK_GBS, 6),
                              "source": "zkaes_pk_op_lists: one chunk-proof proven with the library's op recorder open (every ntt / msm launch appends its size); per GPU",
                              "not_counted": "the <= 3-term hiding MSMs and blinding products (host comb tables), Fiat-Shamir, the streaming polynomial kernels between the transforms"}
            mads = MADS_PER_ADD * stats["pairs"] / 1e12
            mads_per_launch = MADS_PER_ADD * pairs_per_launch / 1e12
            # the integer roof, calibrated on THIS box (zkaes_int_rate_bench right after the timed region, chip warm; `before` = cold, ahead of the warm-up)
            PEAK_REF = 28.1          # T v_mad_u64_u32/s: round 3's measurement on one box (tools/ubench/rates.hip), what rounds 3-5 divided by
            cal = (calibration or {}).get("after") or (calibration or {}).get("before")
            peak_box = round(cal["mad_per_s"] / 1e12, 2) if cal else None
            peak = peak_box or PEAK_REF
            mad_rate = mads_per_launch / (chip_ms / 1e3) if chip_ms > 0 else 0.0
            add_rate = pairs_per_launch / (chip_ms / 1e3) if chip_ms > 0 else 0.0
            hot_loop = None
            if cal:
                hot_loop = {"additions_per_s": round(add_rate / 1e9, 3), "additions_per_s_gathers_from_L2_this_box": round(cal["hot_loop_l2_additions_per_s"] / 1e9, 3), "unit": "G bucket additions/s",
                            "frac": round(add_rate / cal["hot_loop_l2_additions_per_s"], 4), "shader_cycles_per_addition_per_simd": round(cal["hot_loop_cycles_per_addition_per_wave"] / 3.0),
                            "sclk_mhz_of_the_l2_resident_loop": round(cal["hot_loop_l2_sclk_mhz"]),
                            "note": "k_accumulate's own loop (te_madd_hot, same launch shape) over a table that stays in L2, timed on this box after the timed region: what the kernel would do if its gathers were free. "
                                    "The loop costs the same ~13,380 shader cycles per addition per SIMD either way (3,349 VALU instructions x 4 cycles = 13,396: the SIMD issues back to back at three waves, "
                                    "profiles/r06_accumulate_4waves.md); the gap to frac 1.0 is shader clock the chip gives back while ~1.9 TB/s of random 192-byte gathers are live, plus uneven bucket sizes"}
            out.update({
                "alt": alt, "latency_ms": latency,
                "srs": srs_report,
                "telemetry": dict(telemetry.summary(), window="the timed region, sampled from a side thread (tools/gpu_telemetry.py)") if telemetry else None,
                "roofline": {"bound": "hbm", "kernel": "k_accumulate (Pippenger bucket accumulation)", "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                             "frac": round(achieved / HBM_PEAK_GBS, 6), "traffic": traffic, "traffic_source": traffic_src,
                             "peak_measured_stream_copy": copy_gbs,
                             "avg_launch_ms": round(chip_ms, 4), "avg_launch_ms_source": chip_src, "algorithmic_bytes_per_launch": round(bytes_per_launch),
                             "launches": launches, "kernel_ms_per_step": round(kernel_ms_per_step, 1), "kernel_share_of_step": round(kernel_ms_per_step / (1e3 * elapsed / args.steps), 3) if elapsed > 0 else None,
                             "avg_launch_ms_in_situ": round(in_situ_ms, 4), "launch_overlap": round(overlap, 3),
                             "one_context_probe": serial, "proof": proof_roof,
                             "int_multiplier": {"unit": "T v_mad_u64_u32/s", "achieved": round(mad_rate, 2), "peak": peak, "peak_this_box": peak_box, "peak_reference_round3_box": PEAK_REF,
                                                "frac": round(mad_rate / peak, 4), "frac_vs_round3_reference_peak": round(mad_rate / PEAK_REF, 4), "frac_of_wall": round(mads / elapsed / peak, 4),
                                                "calibration": calibration, "hot_loop": hot_loop,
                                                "note": "the kernel's real roof: 2649 v_mad_u64_u32 per bucket addition (7 Fq products x 378 on the curve's twisted Edwards model; round 2's XYZZ mixed add needed 3416), one addition per "
                                                        "(point, window) pair; peak = rate of the same Fq product stream in isolation MEASURED ON THIS BOX in this run (zkaes_int_rate_bench, four waves per SIMD; rounds 3-5 divided by one "
                                                        "box's 28.1). frac uses the same chip time per launch as roofline.frac; frac_of_wall = all multiplies of the timed region / whole timed region."},
                             "note": "integer-ALU bound (7 Fq limb products with their Montgomery reductions = 2649 v_mad_u64_u32 per bucket addition); HBM fraction of O(1%) is the expected regime (BASELINE.md §3); traffic is ~23x the "
                                     "algorithmic bytes by construction: every one of the 13 windows gathers its own 192-byte (64-byte aligned) precomputed copy of the base + a 4-byte index (2,548 B per point against 128 B), "
                                     "~1.7 TB/s, not the limiter"},
            })
            if kernel_ms_per_step > 1e3 * elapsed / args.steps * 1.02:
                out["roofline"]["inconsistent"] = "kernel chip time per step exceeds the step itself"
            if (alt and alt["proofs_verified"] != "%d/%d" % (alt["proofs"], alt["proofs"])) or (latency and not latency["verified"]):
                out["error"] = "verification failure (alt / latency leg)"
        if args.full and world == 1 and mode == "headline" and args.big_chunk > 0 and not use_dist and have_cuda:
            # the big leg needs the device to itself (126 GB of tables for its own SRS): this process lets go of its keys first, the leg runs in a child process
            # (a failure there cannot take this line down) and comes back as one JSON object
            import subprocess
            for k_ in [pk, pk_rem] + extra_keys:
                if k_ is not None and hasattr(k_, "free"):
                    k_.free()
            try:
                cmd = [sys.executable, os.path.abspath(__file__), "--big-only", "--big-chunk", str(args.big_chunk), "--big-proofs", str(args.big_proofs), "--big-contexts", str(args.big_contexts)]
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=420)
                lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
                out["big"] = json.loads(lines[-1]) if lines else {"error": "no output (rc %d): %s" % (r.returncode, (r.stderr or "")[-300:])}
            except Exception as e:                                  # noqa: BLE001
                out["big"] = {"error": str(e)[:300]}
        if args.full and world == 1 and not args.no_cpu_baseline:
            cb = cpu_baseline(samples_small=args.cpu_small_samples, samples_chunk=args.cpu_chunk_samples, chunk_blocks=chunk if chunk > 1 else 6, budget_s=100.0 * max(1, args.cpu_chunk_samples))
            out["cpu_baseline"] = cb
            out["speedup_vs_cpu_baseline"] = round(value / cb["value"], 2)
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, last_step, list(range(*slices[-1])))      # (a step's proofs come back in chunk order, the remainder chunk last)
        print(json.dumps(out), flush=True)
    if use_dist:
        dist.barrier()
        if dist_env is None:
            dist.destroy_process_group()
    return out


def launch_ranks(argv, n):
    """`python bench.py --gpus N` without a launcher: re-execute under torch.distributed.run with N ranks on this node (rank r binds GPU r in run()).
    The driver's own `python -m torch.distributed.run ... bench.py --gpus N` sets WORLD_SIZE and never comes through here."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")       # the host driver only supports dmabuf IPC (RCCL across processes)
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // n)))      # (rank r also binds itself to the r-th share of the CPU set: sharding.bind_rank_cpus)
    return subprocess.call(cmd, env=env)


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    args = build_parser().parse_args(argv)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(launch_ranks(argv, args.gpus))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus != world and int(os.environ.get("RANK", "0")) == 0:
        print("bench.py: --gpus %d but %d rank(s) were launched; n_gpus reports the ranks that joined" % (args.gpus, world), file=sys.stderr)
    from aes_zero_knowledge_proof_circuit_amd import api
    if args.big_only:
        print(json.dumps(big_leg(args, api)), flush=True)
        return
    run(args, api)


if __name__ == "__main__":
    main()
