"""CPU test of the N > 1 path: two gloo ranks shard chunk-proofs, reduce the report the way bench.py does."""
import json
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from aes_zero_knowledge_proof_circuit_amd import sharding  # noqa: E402


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _spawn(fn, first, rest, nprocs):
    """mp.spawn(fn, args=(first, <rendezvous port>) + rest): the port comes from _free_port(), which can lose a race for it (another process binds it between the probe
    and the store's listen, or the previous test's sockets linger); a rendezvous failure is retried once on a fresh port -- anything else is raised as it is."""
    for attempt in range(2):
        port = _free_port()
        try:
            mp.spawn(fn, args=(first, port) + tuple(rest), nprocs=nprocs, join=True)
            return
        except Exception as e:      # noqa: BLE001
            msg = str(e)
            if attempt == 0 and any(k in msg for k in ("Address already in use", "EADDRINUSE", "Connection refused", "Connection reset", "timed out", "TCPStore", "connect()")):
                continue
            raise


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from oracle import zko   # the checker stands in for the GPU prover here: byte-level ECB of this rank's message
    n_chunks, blocks = sharding.plan(10, 4)
    key, msg = sharding.rank_message(rank, blocks)
    ct = zko.aes_encrypt(msg, key)
    accepted = sum(1 for i in range(n_chunks) if len(ct[64 * i:64 * i + 64]) == 64)
    elapsed = 1.0 + rank          # rank 1 is the slow one
    e, a, t, neg = sharding.reduce_report(elapsed, accepted, n_chunks, 1)
    lo, hi = sharding.split_chunks(7, rank, world)
    out[rank] = (e, a, t, neg, blocks, key, msg[:4], (lo, hi))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_report_reduction():
    world, port = 2, _free_port()
    mgr = mp.Manager()
    out = mgr.dict()
    _spawn(_worker, world, (out, ), world)
    r0, r1 = out[0], out[1]
    assert r0[0] == r1[0] == 2.0                      # max over ranks
    assert (r0[1], r0[2], r0[3]) == (6, 6, 2)          # 3 chunk-proofs per rank, both negatives rejected
    assert r0[4] == 12                                 # 10 blocks rounded up to 3 chunks of 4
    assert r0[5] == r1[5] and r0[6] != r1[6]           # shared key, per-rank message
    assert r0[7] == (0, 4) and r1[7] == (4, 7)         # contiguous split of 7 chunks
    assert sharding.aggregate_value(2, 12, 3, 2.0) == 36.0


# ---- bench.py's own rank path (bench.run) on two gloo ranks with a stub prover: strong scaling = ONE job sharded by chunk range, proofs
# all-gathered, rank 0 verifies every one (BASELINE configs[3] / [4]); weak scaling = every rank its own message (configs[2])
class _StubKey:
    def __init__(self, nbytes, log):
        self.nbytes, self.log, self.seeds = nbytes, log, []

    def info(self):
        return {"raw_instance": 8 * self.nbytes + 1, "h": 1 << 20, "k": 1 << 22}

    def timings(self):
        return dict(witness_ms=0.0, round1_ms=0.0, round2_ms=0.0, round3_ms=0.0, open_ms=0.0, total_ms=0.0)

    def tables_built(self):
        return True, 0

    def set_contexts(self, n):
        self.log.append(("contexts", "key%d" % self.nbytes, n))

    def srs_info(self):
        return dict(max_degree=12582909, points_per_copy=12582910, copies=13, bytes=13 * 12582910 * 192, keys_sharing=2, lagrange_bytes=2 * 192 << 20, srs_build_s=3.0, setup_s=4.0)

    def op_lists(self, message, key, throughput_path=True):
        assert len(message) == self.nbytes
        h, k = 1 << 20, 1 << 22
        return {"h": h, "k": k, "x": 1024, "variables": 900000, "constraints": 900000, "nnz": [10, 20, 30], "blocks": self.nbytes // 16, "path": "throughput" if throughput_path else "lone",
                "ntt": [[1024, 1], [h, 3], [h, 10], [k, 1]], "msm": [[h, "class_sum"], [3 * h, "buckets"], [h - 1, "buckets"], [h - 1, "second_bases"], [k - 1, "buckets"]]}

    @staticmethod
    def make(ct):
        import hashlib
        return (hashlib.sha256(bytes(ct)).digest() * 27)[:855]          # a "proof" is a digest of the ciphertext it attests

    def encrypt_chunked(self, message, key, zk_seed=None, first_proof_index=0):
        from oracle import zko
        n = self.nbytes
        assert len(message) % n == 0
        self.log.append(("chunked", n, len(message) // n))
        self.seeds.append((zk_seed, first_proof_index))
        return [self.make(zko.aes_encrypt(message[i:i + n], key)) for i in range(0, len(message), n)]

    def encrypt_batch(self, messages, keys, zk_seed=None, first_proof_index=0):
        from oracle import zko
        self.log.append(("batch", self.nbytes, len(messages)))
        self.seeds.append((zk_seed, first_proof_index))
        return [self.make(zko.aes_encrypt(m, k)) for m, k in zip(messages, keys)]


class _StubApi:
    """stands in for aes_zero_knowledge_proof_circuit_amd.api (no GPU here): same calls bench.run makes, proofs are ciphertext digests"""

    def __init__(self):
        self.log, self.keys = [], []

    def device_count(self):
        return 1

    def set_device(self, _):
        pass

    def synthesize_keys(self, nbytes):
        k = _StubKey(nbytes, self.log)
        self.keys.append(k)
        return k, k

    def msm_stats(self, reset=False):
        return dict(accumulate_ms=0.0, total_ms=0.0, points=0, launches=0, pairs=0)

    def verify_encryption(self, vk, proof, ct):
        return len(ct) == vk.nbytes and proof == _StubKey.make(ct)

    def encrypt(self, message, key, pk):
        from oracle import zko
        assert len(message) == pk.nbytes
        self.log.append(("lone", pk.nbytes, 1))
        return _StubKey.make(zko.aes_encrypt(message, key))

    def stream_copy_bench(self, *a):
        raise RuntimeError("no device")

    def mem_info(self):
        return 100 << 30, 288 << 30


def _bench_worker(rank, world, port, argv, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), ZKAES_BENCH_BACKEND="gloo")
    import contextlib
    import io
    import bench
    api = _StubApi()
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = bench.run(bench.build_parser().parse_args(argv), api)
    timed = [e for e in api.log]
    out[rank] = (res, timed, buf.getvalue())


def _run_bench(argv, world=2):
    port = _free_port()
    out = mp.Manager().dict()
    _spawn(_bench_worker, world, (argv, out, ), world)
    return out


def test_bench_strong_mode_two_ranks_gathers_and_verifies_every_proof():
    out = _run_bench(["--gpus", "2", "--mode", "strong", "--blocks", "64", "--chunk", "6", "--steps", "2", "--warmup", "1", "--contexts", "3", "--no-cpu-baseline", "--full"])
    res, log0, printed = out[0]
    assert out[1][0] is None and out[1][2] == ""               # only rank 0 reports
    assert json.loads(printed)["value"] == res["value"]         # ONE JSON line
    assert res["scaling"] == "strong" and res["n_gpus"] == 2 and "error" not in res
    assert res["proofs_verified"] == "11/11" and res["wrong_ciphertext_rejected"] is True     # 10 chunks of 6 blocks + 1 of 4, all on rank 0 after the gather
    assert res["config"]["blocks_total"] == 64 and res["config"]["proofs_total"] == 11
    # rank 0 proved chunks [0, 6) in two timed steps, rank 1 chunks [6, 11) = four 96-byte chunks + the 64-byte remainder (own key)
    timed0 = [e for e in log0 if e[0] == "chunked"][1:]          # drop the warm-up call
    assert [e for e in timed0 if e[1] == 96][:2] == [("chunked", 96, 3), ("chunked", 96, 3)]
    log1 = out[1][1]
    assert sum(e[2] for e in log1 if e[1] == 96) - 3 == 4 and ("chunked", 64, 1) in log1      # 3 = warm-up (contexts) chunk-proofs
    # the contexts are set per key through the C-ABI setter (no environment round-trip), dropped to 1 for the one-context probe and restored
    assert [e[2] for e in log0 if e[0] == "contexts" and e[1] == "key96"] == [3, 1, 3] and "ZKAES_CONTEXTS" not in open(os.path.join(ROOT, "bench.py")).read()
    # whole-proof roofline from the library's op lists (W + S + T + M), here the stub's canned lists
    pr, h, k = res["roofline"]["proof"], 1 << 20, 1 << 22
    assert pr["T"] == 64 * (1024 + 13 * h + k) and pr["M"] == 128 * (h + 3 * h + 2 * (h - 1) + (k - 1)) and pr["W"] == 16 * 6 + 16 + 32 * 900000
    assert pr["S"] == 36 * 30 + 36 * 60 + 32 * 900000 + 64 * 900000 and pr["bytes"] == pr["W"] + pr["S"] + pr["T"] + pr["M"]
    assert pr["k_accumulate_launches_per_proof"] == 4 and pr["ntt_list"]["transforms"] == 15 and pr["ntt_list"]["launches"] == 4
    assert abs(pr["frac"] - pr["achieved_GBs"] / 8000.0) < 1e-6 and pr["msm_list"]["class_sum"]["count"] == 1
    assert res["srs"]["copies"] == 13 and res["srs"]["keys_sharing_now"] == 2 and len(res["key_setup_s"]) == 1          # rank 0 holds the full-chunk key only


def test_bench_batch_mode_two_ranks():
    out = _run_bench(["--gpus", "2", "--mode", "batch", "--proofs", "9", "--steps", "2", "--warmup", "0", "--no-cpu-baseline"])
    res = out[0][0]
    assert res["scaling"] == "strong" and res["proofs_verified"] == "9/9" and "error" not in res
    assert sum(e[2] for e in out[0][1] if e[0] == "batch") == 5 and sum(e[2] for e in out[1][1] if e[0] == "batch") == 4


def test_bench_headline_mode_two_ranks_is_weak_scaling():
    out = _run_bench(["--gpus", "2", "--mode", "headline", "--blocks", "10", "--chunk", "4", "--steps", "3", "--warmup", "1", "--contexts", "2", "--no-cpu-baseline"])
    res = out[0][0]
    assert res["scaling"] == "weak" and res["proofs_verified"] == "6/6" and "error" not in res       # 2 ranks x (2 chunks of 4 + 1 of 2)
    assert res["config"]["blocks_total"] == 20
    assert abs(res["value"] * res["ms_per_step"] * 3 / 1e3 - 20) < 0.5                               # value = all ranks' blocks / timed region (ms_per_step is rounded)


def test_bench_default_on_several_ranks_is_the_sharded_configs3_message():
    """no --mode / --blocks on N > 1 ranks: ONE message of 8192 blocks per rank (65,536 at 8 ranks = BASELINE configs[3]) sharded by chunk range, proofs
    all-gathered, rank 0 verifies all; the per-GPU share is fixed, so the line says "weak" """
    out = _run_bench(["--gpus", "2", "--steps", "2", "--warmup", "0", "--contexts", "2", "--no-cpu-baseline", "--serial-probe", "0"])
    res = out[0][0]
    assert res["config"]["mode"] == "strong" and res["scaling"] == "weak" and res["n_gpus"] == 2 and "error" not in res
    assert res["config"]["blocks_total"] == 2 * 8192 and res["config"]["proofs_total"] == 2731 and res["proofs_verified"] == "2731/2731"
    n0 = sum(e[2] for e in out[0][1] if e[0] == "chunked" and e[1] == 96)
    n1 = sum(e[2] for e in out[1][1] if e[0] == "chunked" and e[1] == 96)
    assert (n0, n1) == (1366, 1364) and ("chunked", 64, 1) in out[1][1]          # 2730 full chunks + the 4-block remainder on the last rank


def test_bench_default_on_eight_ranks_is_configs3_itself():
    """8 gloo ranks, no --mode / --blocks: BASELINE configs[3] -- ONE 65,536-block (1 MiB) message as 10,922 chunk-proofs of 6 blocks + 1 of 4, contiguous
    chunk ranges per rank, one all-gather, rank 0 verifies all 10,923 in chunk order; every rank pinned to its own eighth of the CPU set (reference loop: src/lib.rs:194)"""
    out = _run_bench(["--gpus", "8", "--steps", "2", "--warmup", "0", "--contexts", "2", "--no-cpu-baseline", "--serial-probe", "0"], world=8)
    res = out[0][0]
    assert all(out[r][0] is None for r in range(1, 8))
    assert res["config"]["mode"] == "strong" and res["scaling"] == "weak" and res["n_gpus"] == 8 and "error" not in res
    assert res["config"]["blocks_total"] == 65536 and res["config"]["proofs_total"] == 10923 and res["proofs_verified"] == "10923/10923"
    assert "BASELINE configs[3]" in res["config"]["workload"]
    shares = [sum(e[2] for e in out[r][1] if e[0] == "chunked" and e[1] == 96) for r in range(8)]
    assert shares == [1366, 1366, 1366, 1365, 1365, 1365, 1365, 1364] and ("chunked", 64, 1) in out[7][1]      # 10,922 full chunks + the 4-block remainder on the last rank
    ncpu = len(os.sched_getaffinity(0))
    if ncpu >= 8:
        assert res["cpu_affinity"]["local_rank"] == 0 and res["cpu_affinity"]["cpus"] in (ncpu // 8, ncpu // 8 + 1)


def test_rank_cpu_shares_are_contiguous_and_disjoint():
    cpus = list(range(3, 131))                                    # 128 CPUs the process may run on, not starting at 0
    shares = [sharding.rank_cpu_share(cpus, r, 8) for r in range(8)]
    assert [len(s) for s in shares] == [16] * 8 and sorted(sum(shares, [])) == cpus
    assert shares[0] == list(range(3, 19)) and shares[7][-1] == 130
    assert [len(sharding.rank_cpu_share(range(10), r, 4)) for r in range(4)] == [3, 3, 2, 2]
    assert sharding.rank_cpu_share([5], 1, 2) == [] and sharding.bind_rank_cpus(0, 1) is None


def test_bench_one_rank_reports_the_measured_alt_and_latency_legs():
    """the one-GPU headline line carries `alt` (the same prover at 4 blocks per chunk-proof, measured after the timed region, every proof verified) and
    `latency_ms` (ONE encrypt() per 16 / 32 / 64-byte message: benches/benchmark_encrypt.rs:45-47) -- driven here with the stub prover"""
    import contextlib
    import io
    import bench
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        os.environ.pop(k, None)
    api = _StubApi()
    argv = ["--blocks", "40", "--steps", "2", "--warmup", "1", "--contexts", "3", "--no-cpu-baseline", "--serial-probe", "0", "--alt-proofs", "5", "--latency-samples", "2", "--full"]
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = bench.run(bench.build_parser().parse_args(argv), api)
    line = json.loads(buf.getvalue())
    assert "error" not in res and res["proofs_verified"] == "7/7" and line["alt"] == res["alt"]
    assert res["alt"]["chunk_blocks"] == 4 and res["alt"]["proofs_verified"] == "5/5" and res["alt"]["value"] > 0
    assert set(res["latency_ms"]) == {"16", "32", "64", "min", "window_tables", "samples", "verified"} and res["latency_ms"]["verified"] is True
    assert set(res["latency_ms"]["min"]) == {"16", "32", "64"} and res["latency_ms"]["window_tables"] == {"16": True, "32": True, "64": True}
    assert [e for e in api.log if e[0] == "lone"] == [("lone", n, 1) for n in (16, 32, 64) for _ in range(3)]     # one warm-up + two timed calls per size
    assert ("chunked", 64, 5) in api.log                                                                          # the timed alt call: five 4-block chunk-proofs
    src = open(bench.__file__).read()
    assert "blocks/s on this code" not in src                   # no measurement is quoted as a literal


def test_bench_plain_run_is_lean_and_dumps_its_last_step(tmp_path):
    """without --full a one-rank run does the headline only: no calibration, probe, legs, roofline or CPU baseline.  The timed proofs draw from ONE job seed at
    job-global chunk indices, and --dump-outputs writes the last timed step's proofs; a second run with the same arguments writes the same arrays"""
    import contextlib
    import io
    import numpy as np
    import bench
    from oracle import zko
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        os.environ.pop(k, None)
    dumps = []
    for run_i in range(2):
        api = _StubApi()
        d = tmp_path / ("run%d" % run_i)
        argv = ["--blocks", "40", "--steps", "3", "--warmup", "2", "--contexts", "3", "--dump-outputs", str(d)]
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            res = bench.run(bench.build_parser().parse_args(argv), api)
        assert json.loads(buf.getvalue()) == res and "error" not in res and res["proofs_verified"] == "7/7"        # 6 chunks of 6 blocks + 1 of 4
        assert res["steps"] == 3 and res["ms_per_step"] > 0 and res["metric"] and res["unit"] == "blocks/s" and res["higher_is_better"] is True and res["dtype"]
        assert not {"alt", "latency_ms", "roofline", "srs", "telemetry", "big", "cpu_baseline"} & set(res)
        assert [e for e in api.log if e[0] in ("lone", "contexts")] == [("contexts", "key96", 3), ("contexts", "key64", 3)]      # no one-context probe, no latency leg
        k96, k64 = api.keys
        timed = [s_ for s_ in k96.seeds + k64.seeds if s_[0] is not None]
        assert [i for _, i in timed] == [0, 3, 5, 6] and len({s_ for s_, _ in timed}) == 1 and len(timed[0][0]) == 32     # slices [0, 3) [3, 5) [5, 7)
        # warm-up steps have the timed steps' shape (slices [0, 3) and [3, 5) of a separate message; the remainder key gets its own single proof), fresh OS seeds
        assert sorted(i for s_, i in k96.seeds if s_ is None) == [0, 3] and [i for s_, i in k64.seeds if s_ is None] == [0]
        assert sorted([e for e in api.log if e[0] == "chunked"][:3]) == [("chunked", 64, 1), ("chunked", 96, 2), ("chunked", 96, 3)]     # (two in flight)
        proofs, index = np.load(d / "proofs.npy"), np.load(d / "proof_index.npy")
        assert proofs.dtype == np.float32 and index.dtype == np.float64 and proofs.shape == (2, 855) and index.tolist() == [5.0, 6.0]
        msg, key = bench.synthetic(16 * 40, 0x5EED + 1), bench.synthetic(16, 0x5EED)
        want = [_StubKey.make(zko.aes_encrypt(msg[96 * 5:96 * 6], key)), _StubKey.make(zko.aes_encrypt(msg[96 * 6:], key))]
        assert [bytes(r.astype(np.uint8)) for r in proofs] == want
        dumps.append((proofs, index))
    assert all(np.array_equal(a, b) for a, b in zip(*dumps))


def test_bench_dump_pads_short_proofs_and_samples_beyond_the_limit(tmp_path, monkeypatch):
    import numpy as np
    import bench
    proofs = [bytes([i]) * (10 - i % 2) for i in range(8)]
    bench.dump_outputs(str(tmp_path), proofs, list(range(100, 108)))
    got = np.load(tmp_path / "proofs.npy")
    assert got.shape == (8, 10) and got[1, 9] == -1 and got[2, 9] == 2 and np.load(tmp_path / "proof_index.npy").tolist() == list(range(100, 108))
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 3 * (4 * 10 + 8))
    bench.dump_outputs(str(tmp_path), proofs, list(range(100, 108)))
    got, idx = np.load(tmp_path / "proofs.npy"), np.load(tmp_path / "proof_index.npy")
    assert got.shape == (3, 10) and idx.tolist() == sorted(idx.tolist()) and all(got[j, 0] == idx[j] - 100 for j in range(3))
    assert got.nbytes + idx.nbytes <= bench.DUMP_LIMIT_BYTES


def test_bench_gpus_flag_launches_the_ranks_itself(monkeypatch):
    """`python bench.py --gpus N` without a launcher re-executes under torch.distributed.run with N ranks (the driver's own torchrun command sets
    WORLD_SIZE and is left alone)"""
    import bench
    calls = []
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr("subprocess.call", lambda cmd, env=None: calls.append((cmd, env)) or 0)
    with pytest.raises(SystemExit) as e:
        bench.main(["--gpus", "4", "--steps", "2"])
    assert e.value.code == 0 and len(calls) == 1
    cmd, env = calls[0]
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"] and cmd[cmd.index("--nproc-per-node") + 1] == "4"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[-4:] == ["--gpus", "4", "--steps", "2"] and cmd[-5].endswith("bench.py")
    assert env["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def _gather_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    mine = [bytes([7]) * (855 - i) for i in range(3 if rank == 0 else 0)]                          # rank 1 contributes nothing
    out[rank] = sharding.gather_proofs(mine)
    dist.destroy_process_group()


def test_gather_proofs_uneven_shares():
    port = _free_port()
    out = mp.Manager().dict()
    _spawn(_gather_worker, 2, (out, ), 2)
    assert out[0] == out[1] == [b"\x07" * 855, b"\x07" * 854, b"\x07" * 853]


def test_plan_edges():
    assert sharding.plan(1, 1) == (1, 1)
    assert sharding.plan(64, 4) == (16, 64)
    assert sharding.plan(65, 4) == (17, 68)
    with pytest.raises(ValueError):
        sharding.plan(0, 4)
    assert [sharding.split_chunks(5, r, 8) for r in range(8)] == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 5), (5, 5), (5, 5)]


# ---- ONE MSM sharded by point range: all-gather of per-rank partial sums + host-side EC add (second row) ----------------
def _msm_inputs(cid, n, seed):
    import ctypes as C
    import numpy as np
    from oracle import zko
    rs = np.random.RandomState(seed)
    gen = b"".join((int.from_bytes(rs.bytes(32), "little") % zko.FR[cid]).to_bytes(32, "little") for _ in range(n))
    bases = C.create_string_buffer(96 * n)
    zko.lib().zko_api_fixed_base(cid, gen, C.c_size_t(n), bases)
    scalars = b"".join((int.from_bytes(rs.bytes(32), "little") % zko.FR[cid]).to_bytes(32, "little") for _ in range(n))
    return bases.raw, scalars


def _oracle_msm(cid):
    import ctypes as C
    from oracle import zko

    def run(bases, scalars):
        out = C.create_string_buffer(96)
        inf = zko.lib().zko_api_msm(cid, bytes(bases), bytes(scalars), C.c_size_t(len(scalars) // 32), out)
        return out.raw, bool(inf)
    return run


def _msm_worker(rank, world, port, cid, n, use_gpu, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    bases, scalars = _msm_inputs(cid, n, 4000 + n)
    out[rank] = sharding.msm_sharded(cid, bases, scalars, local_msm=None if use_gpu else _oracle_msm(cid))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("cid,n", [(377, 301), (381, 64), (377, 1)])
def test_point_range_sharded_msm_two_ranks(cid, n):
    """per-rank partials come from the oracle here (no GPU); the exchange + zkaes_g1_sum fold is the product code under test"""
    world, port = 2, _free_port()
    out = mp.Manager().dict()
    _spawn(_msm_worker, world, (cid, n, False, out, ), world)
    bases, scalars = _msm_inputs(cid, n, 4000 + n)
    ref = _oracle_msm(cid)(bases, scalars)
    assert out[0] == out[1] == ref


def test_g1_sum_edges():
    from aes_zero_knowledge_proof_circuit_amd import api
    from oracle import zko
    bases, _ = _msm_inputs(377, 2, 9)
    p, q = bases[:96], bases[96:]
    (px, py), = zko.pt_unpack(p)
    neg_p = zko.pt_pack([(px, (-py) % zko.Q377)])
    assert api.g1_sum(377, [])[1] is True
    assert api.g1_sum(377, [(p, False)]) == (p, False)
    assert api.g1_sum(377, [(p, False), (neg_p, False)])[1] is True                     # P + (-P)
    assert api.g1_sum(377, [(p, True), (q, False)]) == (q, False)                      # flagged infinity is skipped
    two_p = _oracle_msm(377)(p, zko.fr_pack([2]))
    assert api.g1_sum(377, [(p, False), (p, False)]) == two_p                          # P + P takes the doubling branch
    assert api.g1_sum(377, [(p, False), (q, False)]) == _oracle_msm(377)(p + q, zko.fr_pack([1, 1]))


@pytest.mark.gpu
def test_point_range_sharded_msm_two_gpu_processes():
    """both ranks run the HIP Pippenger on their slice through the C ABI (sharing GPU 0 on a one-GPU box), then all-gather + fold"""
    world, port, cid, n = 2, _free_port(), 377, 5000
    out = mp.Manager().dict()
    _spawn(_msm_worker, world, (cid, n, True, out, ), world)
    bases, scalars = _msm_inputs(cid, n, 4000 + n)
    assert out[0] == out[1] == _oracle_msm(cid)(bases, scalars)


def _msm_device_worker(rank, world, port, cid, n, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dev = rank if world > 1 else 0                  # one GPU per rank (RCCL refuses two ranks on one device)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", dev))
    if world > 1:
        from aes_zero_knowledge_proof_circuit_amd import api
        api.set_device(dev)
    bases, scalars = _msm_inputs(cid, n, 4000 + n)
    out[rank] = sharding.msm_sharded_device(cid, bases, scalars, torch.device("cuda", dev))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize("cid,n", [(377, 5000), (381, 333)])
def test_point_range_sharded_msm_device_resident_exchange_rccl(cid, n):
    """the device-resident variant: window sums stay in HBM, torch.distributed.all_gather_into_tensor over RCCL, per-window fold on the device.
    One rank here (a one-GPU box; RCCL refuses two ranks on one device) -- the collective and both C-ABI calls still run."""
    port = _free_port()
    out = mp.Manager().dict()
    _spawn(_msm_device_worker, 1, (cid, n, out, ), 1)
    bases, scalars = _msm_inputs(cid, n, 4000 + n)
    assert out[0] == _oracle_msm(cid)(bases, scalars)


@pytest.mark.gpu
def test_point_range_sharded_msm_device_resident_exchange_two_gpus():
    """the same over TWO RCCL ranks on two GPUs (skipped on a one-GPU box): rank-major rows of the all-gather, stream ordering between libzkaes and RCCL"""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    cid, n, port = 377, 5000, _free_port()
    out = mp.Manager().dict()
    _spawn(_msm_device_worker, 2, (cid, n, out, ), 2)
    bases, scalars = _msm_inputs(cid, n, 4000 + n)
    assert out[0] == out[1] == _oracle_msm(cid)(bases, scalars)


@pytest.mark.gpu
def test_window_sum_fold_of_two_slices_equals_the_whole_msm():
    """the fold itself with world = 2 on one GPU (no process group): slice A and slice B -> rows 0 and 1 of one device buffer -> per-window sum"""
    from aes_zero_knowledge_proof_circuit_amd import api
    cid, n = 377, 4097
    bases, scalars = _msm_inputs(cid, n, 77)
    c, nwin, nbytes = api.msm_sharded_plan(cid, n)
    assert nbytes == nwin * 192 and (253 + 1 + c - 1) // c == nwin
    buf = torch.zeros((2, nbytes), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    cut = 1500
    api.msm_window_sums_dev(cid, bases[:96 * cut], scalars[:32 * cut], n, buf[0].data_ptr(), nbytes)
    api.msm_window_sums_dev(cid, bases[96 * cut:], scalars[32 * cut:], n, buf[1].data_ptr(), nbytes)
    assert api.msm_fold_window_sums_dev(cid, buf.data_ptr(), 2, n) == _oracle_msm(cid)(bases, scalars)
    # an empty share is the point at infinity in every window
    api.msm_window_sums_dev(cid, b"", b"", n, buf[1].data_ptr(), nbytes)
    api.msm_window_sums_dev(cid, bases, scalars, n, buf[0].data_ptr(), nbytes)
    assert api.msm_fold_window_sums_dev(cid, buf.data_ptr(), 2, n) == _oracle_msm(cid)(bases, scalars)
    with pytest.raises(api.ZkAesError, match="too small"):
        api.msm_window_sums_dev(cid, bases, scalars, n, buf[0].data_ptr(), 100)


# ---- the same sharding on the PROVER'S OWN path: a key's SRS on the twisted Edwards model with window tables, one partial sum per rank
def _srs_msm_case(n, off, seed):
    """scalars (Montgomery bytes) over powers_of_g[off .. off + n) and the expected sum from the (public, test_rng-derived) trapdoor: (sum s_i beta^(off + i)) g,
    computed with Python big integers (tools/curve_math.py) -- independent of every kernel and of the C oracle"""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import curve_math as cm
    from oracle import zko
    rs = np.random.RandomState(seed)
    vals = [int.from_bytes(rs.bytes(32), "little") % zko.FR[377] for _ in range(n)]
    vals[0], vals[1] = 0, zko.FR[377] - 1
    beta, g, _, _ = cm.ark_kzg10_setup_points()
    acc, pw = 0, pow(beta, off, zko.FR[377])
    for v in vals:
        acc = (acc + v * pw) % zko.FR[377]
        pw = pw * beta % zko.FR[377]
    return zko.fr_pack(vals), cm.ec_mul(acc, g, cm.Q377)


@pytest.mark.gpu
def test_srs_path_sharded_msm_fold_of_two_slices_equals_the_trapdoor_product():
    """zkaes_pk_msm_partial_dev on two slices of one MSM over the 16-byte key's SRS (Edwards tables, ONE bucket set -> one XYZZ point per slice, left in device memory)
    + zkaes_msm_fold_partials_dev == (sum s_i beta^i) g; an empty share is the point at infinity; a range beyond the committer key is refused"""
    from aes_zero_knowledge_proof_circuit_amd import api
    from oracle import zko
    pk, _ = api.synthesize_keys(16)
    built, nbytes = pk.tables_built()
    assert built and nbytes > (1 << 30)
    n, off, cut = 520_003, 12_345, 200_000
    scalars, want = _srs_msm_case(n, off, 11)
    buf = torch.zeros((2, 192), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    pk.msm_partial_dev(scalars[:32 * cut], off, buf[0].data_ptr())
    pk.msm_partial_dev(scalars[32 * cut:], off + cut, buf[1].data_ptr())
    got, inf = api.msm_fold_partials_dev(377, buf.data_ptr(), 2)
    assert not inf and zko.pt_unpack(got)[0] == want
    pk.msm_partial_dev(scalars, off, buf[0].data_ptr())
    pk.msm_partial_dev(b"", 0, buf[1].data_ptr())
    got, inf = api.msm_fold_partials_dev(377, buf.data_ptr(), 2)
    assert not inf and zko.pt_unpack(got)[0] == want
    with pytest.raises(api.ZkAesError, match="exceeds the committer key"):
        pk.msm_partial_dev(scalars, 1 << 22, buf[0].data_ptr())
    with pytest.raises(api.ZkAesError, match="too small"):
        pk.msm_partial_dev(scalars, off, buf[0].data_ptr(), 100)
    nt_pk, _ = api.synthesize_keys(16, flags=api.KEY_NO_TABLES)
    assert nt_pk.tables_built() == (False, 0)
    with pytest.raises(api.ZkAesError, match="no window tables"):
        nt_pk.msm_partial_dev(scalars[:3200], 0, buf[0].data_ptr())


def _srs_msm_device_worker(rank, world, port, n, off, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dev = rank if world > 1 else 0
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", dev))
    from aes_zero_knowledge_proof_circuit_amd import api
    api.set_device(dev)
    pk, _ = api.synthesize_keys(16)
    scalars, _ = _srs_msm_case(n, off, 12)
    out[rank] = sharding.msm_sharded_srs_device(pk, scalars, torch.device("cuda", dev), offset=off)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
def test_srs_path_sharded_msm_through_rccl():
    """sharding.msm_sharded_srs_device end to end: partial sums in HBM, all_gather_into_tensor over RCCL, device fold -- on as many ranks as the box has GPUs
    (one here; RCCL refuses two ranks on one device)"""
    from oracle import zko
    world = 2 if torch.cuda.device_count() >= 2 else 1
    n, off, port = 500_500, 7, _free_port()
    out = mp.Manager().dict()
    _spawn(_srs_msm_device_worker, world, (n, off, out, ), world)
    _, want = _srs_msm_case(n, off, 12)
    for r in range(world):
        got, inf = out[r]
        assert not inf and zko.pt_unpack(got)[0] == want


@pytest.mark.gpu
def test_bench_two_ranks_real_prover_on_one_gpu():
    """the N > 1 launch path with the REAL prover inside the driver's GPU suite.  `python bench.py --gpus 2` starts its two ranks itself (launch_ranks ->
    torch.distributed.run); with ZKAES_BENCH_ONE_GPU=1 both ranks prove on device 0 and ZKAES_BENCH_BACKEND=gloo carries the collectives (RCCL needs one GPU per rank),
    so a one-GPU box exercises everything but xGMI: bind_rank_cpus per rank, the remainder key (4 blocks) on the last rank beside its 6-block key, the chunk-range split of
    ONE 100-block message (src/lib.rs:194 is the loop that shards), the all-gather of the proofs and rank 0 verifying all 17.  2-8 real GPUs stay unmeasured here."""
    import subprocess
    import time
    env = dict(os.environ, ZKAES_BENCH_ONE_GPU="1", ZKAES_BENCH_BACKEND="gloo")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--blocks", "100", "--steps", "2", "--warmup", "1", "--contexts", "4", "--no-cpu-baseline", "--alt-proofs", "0",
           "--latency-samples", "0", "--full"]
    t0 = time.perf_counter()
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    took = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]                       # ONE JSON line, from rank 0
    res = json.loads(lines[0])
    assert "error" not in res and res["n_gpus"] == 2 and res["scaling"] == "strong" and res["config"]["mode"] == "strong"
    assert res["proofs_verified"] == "17/17" and res["wrong_ciphertext_rejected"] is True and res["config"]["proofs_total"] == 17 and res["value"] > 0
    aff = res["cpu_affinity_by_rank"]
    assert len(aff) == 2 and all(a and a["cpus"] >= 1 for a in aff) and [a["local_rank"] for a in aff] == [0, 1]
    assert aff[0]["last"] < aff[1]["first"]                        # two disjoint, contiguous CPU shares
    assert res["roofline"]["launches"] > 0 and res["roofline"]["proof"]["k_accumulate_launches_per_proof"] == 10
    assert took < 240, took                                         # (90 s on an idle box: two key sets + 17 proofs)


@pytest.mark.gpu
def test_bench_eight_ranks_real_prover_on_one_gpu():
    """the 8-rank launch path with the REAL prover (round 5 drove eight ranks only with a stub).  `python bench.py --gpus 8` starts its eight ranks itself;
    ZKAES_BENCH_ONE_GPU=1 puts them all on device 0, gloo carries the collectives, --no-tables keeps a rank at ~10 GB (no window tables: 2.4 GB of SRS per process).
    Exercised: the 8-way rendezvous, eight disjoint CPU shares, an UNEVEN split of ONE 196-block message (33 chunk-proofs over 8 ranks: 5 + 7 x 4) with the 4-block remainder
    key on the last rank, the all-gather, rank 0 verifying all 33 proofs (src/lib.rs:194 is the loop that shards).  The host CPU time of the whole job goes to
    gpurun_out/r06_bench_gpus8_one_gpu_rehearsal.json (busy cores per rank).  2-8 real GPUs stay unmeasured: this is a rehearsal of the launch path, not a scaling number."""
    import resource
    import subprocess
    import time
    env = dict(os.environ, ZKAES_BENCH_ONE_GPU="1", ZKAES_BENCH_BACKEND="gloo")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--blocks", "196", "--steps", "2", "--warmup", "1", "--contexts", "1", "--no-cpu-baseline", "--alt-proofs", "0",
           "--latency-samples", "0", "--no-tables", "--calibrate-s", "0"]
    ru0 = resource.getrusage(resource.RUSAGE_CHILDREN)
    t0 = time.perf_counter()
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    took = time.perf_counter() - t0
    ru1 = resource.getrusage(resource.RUSAGE_CHILDREN)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]                       # ONE JSON line, from rank 0
    res = json.loads(lines[0])
    assert "error" not in res and res["n_gpus"] == 8 and res["scaling"] == "strong" and res["config"]["mode"] == "strong"
    assert res["proofs_verified"] == "33/33" and res["wrong_ciphertext_rejected"] is True and res["config"]["proofs_total"] == 33 and res["value"] > 0
    assert res["config"]["window_tables"] is False
    aff = res["cpu_affinity_by_rank"]
    assert len(aff) == 8 and all(a and a["cpus"] >= 1 for a in aff) and [a["local_rank"] for a in aff] == list(range(8))
    assert all(aff[i]["last"] < aff[i + 1]["first"] for i in range(7))          # eight disjoint, contiguous CPU shares
    cpu_s = (ru1.ru_utime + ru1.ru_stime) - (ru0.ru_utime + ru0.ru_stime)
    res["host"] = {"wall_s": round(took, 1), "cpu_s_all_ranks_and_launcher": round(cpu_s, 1), "busy_cores_per_rank_over_the_whole_run": round(cpu_s / took / 8, 2),
                   "note": "getrusage(RUSAGE_CHILDREN) around `python bench.py --gpus 8` (eight ranks on ONE GPU over gloo): imports, key synthesis, warm-up, 33 proofs, verification by rank 0"}
    try:
        os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
        json.dump(res, open(os.path.join(ROOT, "gpurun_out", "r06_bench_gpus8_one_gpu_rehearsal.json"), "w"))
    except OSError:
        pass
    assert took < 400, took
