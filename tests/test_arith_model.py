"""The big-integer model of tests/arith_model.py against the HOST branch of every probe of csrc/arith_probe.cuh (tests/arith_probe_host.cpp, a stand-alone program built with
-fsanitize=address,undefined; nothing is loaded into python).  This validates the model and the operand lists before a GPU sees them, and makes a later failure of
tests/test_gpu_arith.py three-way: model, host branch, device branch.  Every operation with a host body is covered: everything except the four-lanes-per-point forms."""
import ctypes as C
import os
import struct
import subprocess

import pytest

import arith_model as am
from aes_zero_knowledge_proof_circuit_amd.api import ARITH_OPS, ARITH_QUAD_OPS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aes_zero_knowledge_proof_circuit_amd", "csrc")
HOST_OPS = sorted(n for n in ARITH_OPS if n not in ARITH_QUAD_OPS and n != am.HOT)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("arith_probe")
    exe = str(d / "arith_probe_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                           os.path.join(ROOT, "tests", "arith_probe_host.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")

    def run(records):
        """records: [(name, case word lists)] -> [output word lists] per record, all in ONE run of the program"""
        with open(d / "cases.bin", "wb") as f:
            for name, ins in records:
                f.write(struct.pack("<II", ARITH_OPS[name][0], len(ins)) + am.pack(ins))
        out = subprocess.run([exe, str(d / "cases.bin"), str(d / "out.bin")], capture_output=True, text=True, env=env, timeout=900)
        assert out.returncode == 0 and out.stdout.split() == ["arith_probe_host", "ok", str(len(records))], (out.stdout + out.stderr)[-4000:]
        buf, res, o = open(d / "out.bin", "rb").read(), [], 0
        for name, ins in records:
            nout = ARITH_OPS[name][2]
            res.append(am.unpack(buf[o:o + 4 * nout * len(ins)], nout))
            o += 4 * nout * len(ins)
        assert o == len(buf)
        return res
    run.exe = exe
    return run


@pytest.fixture(scope="module")
def host_outputs(probe):
    """every host operation on its whole case list, one run of the program"""
    return dict(zip(HOST_OPS, probe([(n, am.cases(n)) for n in HOST_OPS])))


def test_the_compiled_table_is_the_one_api_py_names(probe):
    out = subprocess.run([probe.exe, "--list"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0
    compiled = {int(i): (int(nin), int(nout), int(quad)) for i, nin, nout, quad in (ln.split() for ln in out.stdout.splitlines())}
    named = {op: (nin, nout, int(name in ARITH_QUAD_OPS)) for name, (op, nin, nout) in ARITH_OPS.items()}
    assert compiled == named and len(named) == len(ARITH_OPS)


@pytest.mark.parametrize("name", HOST_OPS)
def test_host_branch_equals_the_model(host_outputs, name):
    am.check(name, am.cases(name), host_outputs[name])


def test_hot_addition_chains_on_the_host(probe):
    """seven te_madd_hot in a row with mixed signs, checked as points after every step; for a positive digit the same bytes as te_madd of the same record"""
    prev = None
    for step in range(7):
        ins = am.hot_step_cases(step, prev)
        plain = [(c, x) for c, x in enumerate(am.hot_as_madd(ins)) if x is not None]
        prev, madd = probe([(am.HOT, ins), ("te377.te_madd", [x for _, x in plain])])
        am.hot_step_check(step, prev)
        assert plain and all(prev[c][:56] == m for (c, _), m in zip(plain, madd)), "te_madd_hot differs from te_madd at step %d" % step


def test_the_python_reference_of_the_top_limb_estimate_stays_inside_its_bounds():
    """reduce_by_top_limb in integers alone, on the listed boundary values and the pseudo-random ones: below 1.003 p (BLS12-377 Fr) and 1.018 p (BLS12-381 Fr)"""
    for f, bound1000 in (("fr377x29", 1003), ("fr381x29", 1018)):
        R = am.X29[f]
        worst = max(am.reduce_by_top_limb_model(R, R.val(x)) for x in am.cases(f + ".reduce_by_top_limb"))
        print(f, "worst remainder / p = %.6f" % (worst / R.p))
        assert worst * 1000 < bound1000 * R.p


def test_entry_point_refuses_bad_arguments_before_it_touches_a_device(api):
    """an unknown op, no cases, more than 2^16 cases, a ragged case buffer: refused with a message (validated before anything is allocated, so this needs no GPU)"""
    one = am.pack(am.cases("fr377.neg")[:1])
    out = C.create_string_buffer(32)
    for op, buf, n, what in ((15, one, 1, "unknown op"), (-1, one, 1, "unknown op"), (225, one, 1, "unknown op"), (3, one, 0, "n_cases"), (3, one, (1 << 16) + 1, "n_cases"),
                             (3, None, 1, "null")):
        assert api.lib().zkaes_arith_probe(op, buf, C.c_size_t(n), out) == 1
        assert what in api.lib().zkaes_last_error().decode()
    assert api.lib().zkaes_arith_probe(3, one, C.c_size_t(1), None) == 1
    with pytest.raises(api.ZkAesError):
        api.arith_probe("fr377.neg", b"")
    with pytest.raises(api.ZkAesError):
        api.arith_probe("fr377.neg", one[:-4])
