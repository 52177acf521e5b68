"""The device code of the witness trace lives in three headers that the host emulators (tests/*_trace_emu.cpp) include directly behind tests/lane_emu.h.  Checked here,
without a GPU: each header stands on its own, and nothing goes back to cutting kernel text out of a translation unit."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aes_zero_knowledge_proof_circuit_amd", "csrc")
TESTS = os.path.join(ROOT, "tests")
HEADERS = ("kernels_witness.cuh", "kernels_digest.cuh", "kernels_reveal.cuh")
TRACE_UNITS = ("kernels_witness.hip", "kernels_digest.hip", "kernels_reveal.hip")
# Two older models read tuning constants and one branch condition of the MSM and the polynomial layer from their translation units, and one test walks the whole package
# for a forbidden word.  None of them touches the trace kernels; they are named here so that a new reader of a .hip file has to be added on purpose.
READERS_OF_OTHER_UNITS = {"msm_model.py": "kernels_msm.hip", "test_gpu_poly.py": "kernels_poly.hip", "test_capi.py": ".hip"}
HIP_LITERAL = re.compile(r"""["'][^"'\n]*\.hip["']""")


@pytest.mark.parametrize("header", HEADERS)
def test_header_compiles_on_its_own_behind_the_lane_shim(header):
    """lane_emu.h, then the one header: everything else it needs it includes itself (<cstdint>, <cstddef>, trace_layout.h), and it names no runtime header"""
    text = open(os.path.join(CSRC, header)).read()
    includes = set(re.findall(r"^#include\s+(\S+)", text, re.M))
    assert includes <= {"<cstdint>", "<cstddef>", '"trace_layout.h"', '"kernels_witness.cuh"', '"kernels_digest.cuh"'}, includes
    for word in ("atomic", "__shared__", "__syncthreads", "__shfl", "hipLaunch"):
        assert word not in text
    unit = '#include "lane_emu.h"\n#include "%s"\n' % header
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wno-unknown-pragmas", "-I", CSRC, "-I", TESTS, "-x", "c++", "-"], input=unit, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-4000:]


def test_each_header_has_one_translation_unit():
    """every __global__ keeps a single definition in the library: a header is included by exactly one file of csrc/, the .hip file of the same name"""
    for header in HEADERS:
        users = sorted(f for f in os.listdir(CSRC) if os.path.isfile(os.path.join(CSRC, f)) and '#include "%s"' % header in open(os.path.join(CSRC, f)).read())
        assert users == [header.replace(".cuh", ".hip")], (header, users)


def test_no_test_opens_a_trace_translation_unit():
    """no file under tests/ names a .hip file in a string literal -- the way a path to open is spelled -- except the three listed readers of other units, each only its own"""
    me = os.path.basename(__file__)
    found = {}
    for dirpath, dirs, files in os.walk(TESTS):
        dirs[:] = [d for d in dirs if d not in ("__pycache__", "golden")]
        for f in files:
            if f == me or not f.endswith((".py", ".cpp", ".h", ".hpp", ".sh")):
                continue
            text = open(os.path.join(dirpath, f), errors="replace").read()
            hits = HIP_LITERAL.findall(text)
            if hits:
                found[f] = hits
            for unit in TRACE_UNITS:
                assert '"%s"' % unit not in text and "'%s'" % unit not in text, (f, unit)
    assert set(found) <= set(READERS_OF_OTHER_UNITS), found
    for f, hits in found.items():
        assert all(h.strip("\"'").endswith(READERS_OF_OTHER_UNITS[f]) for h in hits), (f, hits)
        assert not any(unit in h for h in hits for unit in TRACE_UNITS), (f, hits)


def test_the_extract_file_is_gone_everywhere():
    name = ("kern" + "_extract").encode()                     # (spelled in two halves so that this file does not hold the string either)
    skip_dirs = {".git", "__pycache__", ".pytest_cache", "build", "_ref"}
    for dirpath, dirs, files in os.walk(ROOT):
        dirs[:] = [d for d in dirs if d not in skip_dirs]
        for f in files:
            if f.endswith((".so", ".o", ".a", ".pyc")):
                continue
            with open(os.path.join(dirpath, f), "rb") as fh:
                assert name not in fh.read(), os.path.join(dirpath, f)
