"""The Fp28 products of csrc/ff28.cuh -- row-wise lower half, carry-seeded column chains for the upper half, plain and zipped -- against the exact integer (a b + M p) / R':
tests/ff28_columns_host_check.cpp, a stand-alone program with its own big-integer arithmetic, built with -fsanitize=address,undefined (no GPU, no HIP)."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aes_zero_knowledge_proof_circuit_amd", "csrc")


def test_products_equal_the_exact_integer_limb_for_limb():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "t")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                               os.path.join(ROOT, "tests", "ff28_columns_host_check.cpp"), "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        lines = out.stdout.splitlines()
        assert len(lines) == 2 and lines[0].startswith("fq377x28 ") and lines[1].startswith("fq381x28 ") and all(l.endswith(" 0 bad") for l in lines), out.stdout
        assert all(int(l.split()[1]) > 6000 for l in lines), out.stdout          # the operand lists ran: 2,000 random pairs through three products each, and the edges
