"""Every host statement path against the answers of the commit before the statement layer was collapsed (tests/golden/statement_paths.json, recorded on an MI355X by
tests/golden/make_statement_paths.py at the commit the file names).  Proofs are deterministic per (seed, index), so the SHA-256 of every proof and every returned
ciphertext, tag, state and commitment must be the same bytes: the prover's lone, batch, chunked and segment forms of every mode make the statements they made before, and
the verifiers still accept them.  The calls, their shapes and why those are the smallest that reach every branch: tests/statement_paths.py.
"""
import json
import os

import pytest

import statement_paths

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "statement_paths.json")) as f:
        record = json.load(f)
    assert len(record["recorded_at_commit"]) == 40 and sorted(record["entries"]) == sorted(statement_paths.NAMES)
    assert record["zk_seed"] == statement_paths.SEED.hex() and record["first_proof_index"] == statement_paths.FIRST_INDEX
    return record["entries"]


@pytest.mark.parametrize("name", statement_paths.NAMES)
def test_statement_path(api, recorded, name):
    got = json.loads(json.dumps(statement_paths.run(api, name)))            # through JSON, as the recording went: tuples are lists, keys are strings
    assert sorted(got) == ["parity", "seeded"]
    for label in got:
        assert got[label] == recorded[name][label], (name, label)
