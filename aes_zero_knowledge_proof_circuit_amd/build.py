"""Build libzkaes.so (HIP kernels for gfx950 + host library) in-tree with hipcc.

    python -m aes_zero_knowledge_proof_circuit_amd.build [--force]

hipcc cross-compiles gfx950 without a GPU.  Objects are cached under csrc/build/ keyed by source mtime.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "libzkaes.so")
OBJ = os.path.join(CSRC, "build")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HIP_SOURCES = ["runtime.hip", "kernels_ntt.hip", "kernels_msm.hip", "kernels_poly.hip", "kernels_witness.hip", "kernels_digest.hip", "kernels_reveal.hip", "kernels_verify.hip", "capi_kernels.hip", "capi_probe.hip"]
CXX_SOURCES = ["circuit.cpp", "marlin.cpp", "marlin_codec.cpp", "capi.cpp", "capi_host.cpp"]
HOST_ONLY_SOURCES = ["circuit.cpp", "marlin_codec.cpp", "capi_host.cpp"]      # no device code path: what the stand-alone sanitizer programs of tests/ link against
HEADERS = ["ff.cuh", "ff28.cuh", "ff29.cuh", "ec.cuh", "ec28.cuh", "te28.cuh", "gpu.hpp", "hip_util.hpp", "consts32.h", "trace_layout.h", "circuit.hpp", "marlin.hpp", "marlin_host.hpp", "capi_common.hpp", "pairing.hpp", "transcript.hpp", "arith_probe.cuh", "fq_sqrt.cuh", "verify_batch.hpp", "statement.hpp",
           "kernels_witness.cuh", "kernels_digest.cuh", "kernels_reveal.cuh",      # the trace kernels' device code (each included by the .hip file of its name)
           os.path.join("..", "..", "include", "zkaes.h")]
COMMON = ["-O3", "-std=c++17", "-fPIC", "-I", CSRC, "-Wno-unused-result"]
if os.environ.get("ZK_EXTRA_DEFINES"):      # e.g. "-DZKAES_MEASURE" (knock-in hooks of the measurement builds) for A/B builds on the GPU box
    COMMON += os.environ["ZK_EXTRA_DEFINES"].split()


def _newer(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _compile(src):
    obj = os.path.join(OBJ, src + ".o")
    deps = [os.path.join(CSRC, src)] + [os.path.join(CSRC, h) for h in HEADERS]
    if not _newer(obj, deps):
        return obj
    if src.endswith(".hip"):
        cmd = [HIPCC, "--offload-arch=gfx950", "-x", "hip"] + COMMON + ["-c", os.path.join(CSRC, src), "-o", obj]
    else:
        cmd = [HIPCC, "-x", "c++"] + COMMON + ["-c", os.path.join(CSRC, src), "-o", obj]
    subprocess.check_call(cmd)
    return obj


def build(force=False):
    os.makedirs(OBJ, exist_ok=True)
    if force:
        for f in os.listdir(OBJ):
            os.remove(os.path.join(OBJ, f))
    with ThreadPoolExecutor(max_workers=8) as ex:
        objs = list(ex.map(_compile, HIP_SOURCES + CXX_SOURCES))
    if force or _newer(OUT, objs):
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", OUT] + objs)
    return OUT


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
