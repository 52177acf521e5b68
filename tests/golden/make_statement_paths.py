#!/usr/bin/env python3
"""Run ON THE GPU BOX, at the commit whose behaviour is to be pinned: make every call of tests/statement_paths.py and record the answers (the SHA-256 of every proof,
every returned ciphertext, tag, state and commitment) with that commit's hash into tests/golden/statement_paths.json, or into the file named last.

    python tests/golden/make_statement_paths.py <hash of the recording commit> [output file]

tests/test_gpu_statement_paths.py replays the calls on a later tree and asserts equality: the file must come from the commit BEFORE a change to the statement layer,
never from the code under test.
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from aes_zero_knowledge_proof_circuit_amd import api  # noqa: E402
import statement_paths  # noqa: E402

if len(sys.argv) not in (2, 3):
    sys.exit(__doc__)
record = {"recorded_at_commit": sys.argv[1], "zk_seed": statement_paths.SEED.hex(), "first_proof_index": statement_paths.FIRST_INDEX, "entries": {}}
for name in statement_paths.NAMES:
    t0 = time.perf_counter()
    record["entries"][name] = statement_paths.run(api, name)
    print("%-28s %.1f s" % (name, time.perf_counter() - t0), flush=True)
text = json.dumps(record, indent=1, sort_keys=True)
assert "false" not in text, "a proof of the recording commit was rejected"
out = sys.argv[2] if len(sys.argv) == 3 else os.path.join(ROOT, "tests", "golden", "statement_paths.json")
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as f:
    f.write(text + "\n")
print("wrote", len(text), "bytes")
