"""In-tree native builds (explicit compiler invocations; outputs under simdjson_amd/lib/, build/ and oracle/_ref/).

    libsjgpu.so            hipcc --offload-arch=gfx950   HIP kernels + C-ABI (include/sjgpu*.h)   [product]
    libsjcorpus.so         gcc                           synthetic corpora                         [tooling]
    oracle/_ref/libsimdjson_mi355x.so  g++ against the reference's public headers: the simdjson::implementation
                           plug-in shim.  Needs the reference at BUILD time only.
    oracle/_ref/*.so       make -C oracle                CPU checkers                              [tests]
    oracle/_ref/tests/*    g++                           test programs that link the reference (plugin_test, the reference's
                           own test programs): test infrastructure, git-ignored, never under simdjson_amd/.
    Everything built from the reference lies under oracle/_ref/, by the recipes under oracle/ (Makefile, ref_build.py):
    it is built where the reference's sources are and kept, prebuilt, where they are not (a checkout that carries
    oracle/_ref/ but not the reference runs the tests that need it).  oracle/_ref/tests/STAMP.json records the hashes of the sources the test programs were built from, and
    tests refuse a stale binary; build/tests/STAMP.json does the same for libsjgpu.so.

Run `python -m simdjson_amd.build` or call build_all(); each target is rebuilt only when a source
is newer than its output.
"""
import hashlib
import json
import os
import shutil
import subprocess
import sys

from . import _paths

HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
GFX_ARCH = "gfx950"


def _stale(out, srcs):
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    return any(os.path.getmtime(s) > t for s in srcs if os.path.exists(s))


def _run(cmd, cwd=None):
    print("[build]", " ".join(cmd), flush=True)
    subprocess.run(cmd, check=True, cwd=cwd)


def _csrc(*names):
    return [os.path.join(_paths.CSRC_DIR, n) for n in names]


def build_corpus(force=False):
    srcs = _csrc("corpus.c")
    if force or _stale(_paths.LIB_CORPUS, srcs):
        os.makedirs(_paths.LIB_DIR, exist_ok=True)
        _run(["gcc", "-O2", "-std=c99", "-fopenmp", "-fPIC", "-shared", *srcs, "-o", _paths.LIB_CORPUS])
    return _paths.LIB_CORPUS


SJGPU_SOURCES = ("sjgpu_kernels.hip", "sjgpu_fused.hip", "sjgpu_small.hip", "sjgpu_finish.hip", "sjgpu_strings.hip", "sjgpu_string_stream.hip", "sjgpu_tape.hip", "sjgpu_tape_many.hip", "sjgpu_query.hip", "sjgpu_cast.hip", "sjgpu_cast_strings.hip", "sjgpu_dict.hip", "sjgpu_pivot.hip", "sjgpu_json.hip", "sjgpu_json_wide.hip", "sjgpu_write.hip",
                 "sjgpu_mgpu.hip", "sjgpu_comm.hip", "sjgpu_capi.hip", "sjgpu_capi_host.hip", "sjgpu_capi_stage2.hip", "stage1_finish.cpp")
SJGPU_HEADERS = ("sj_block.h", "sj_number.h", "sj_number_in_string.h", "sj_tape_rules.h", "sj_string_stream.h", "sj_xcarry.h", "sj_pow5_table.inc", "sj_dtoa.h", "sj_pow10_table.inc", "sj_json_text.h", "sj_json_walk.h", "sj_write_table.h", "sj_nested_table.h", "sj_query_program.h", "sj_path_program.h", "sj_cell_kinds.h", "sjgpu_internal.h", "sjgpu_device.h", "sjgpu_ctx.h")


def sjgpu_source_stamp():
    """sha256 over everything libsjgpu.so is compiled from (names and bytes): what build/tests/STAMP.json records under "libsjgpu.so" when the
    library is built, and what the tests compare with -- a prebuilt library that travelled with OTHER sources is found out by content, not by mtime."""
    h = hashlib.sha256()
    for f in [*_csrc(*SJGPU_SOURCES), *_csrc(*SJGPU_HEADERS), os.path.join(_paths.INCLUDE_DIR, "sjgpu.h"), os.path.join(_paths.INCLUDE_DIR, "sjgpu_stream.h"),
              os.path.join(_paths.INCLUDE_DIR, "sjgpu_query.h"), os.path.join(_paths.INCLUDE_DIR, "sjgpu_paths.h"), os.path.join(_paths.INCLUDE_DIR, "sjgpu_rows.h"),
              os.path.join(_paths.INCLUDE_DIR, "sjgpu_lists.h"), os.path.join(_paths.INCLUDE_DIR, "sjgpu_cast.h"), os.path.join(_paths.INCLUDE_DIR, "sjgpu_cast_strings.h"), os.path.join(_paths.INCLUDE_DIR, "sjgpu_fields.h"), os.path.join(_paths.INCLUDE_DIR, "sjgpu_dict.h"), os.path.join(_paths.INCLUDE_DIR, "sjgpu_pivot.h"),
              os.path.join(_paths.INCLUDE_DIR, "sjgpu_json.h"), os.path.join(_paths.INCLUDE_DIR, "sjgpu_json_wide.h"), os.path.join(_paths.INCLUDE_DIR, "sjgpu_pretty.h"), os.path.join(_paths.INCLUDE_DIR, "sjgpu_write.h"), os.path.join(_paths.INCLUDE_DIR, "sjgpu_nested.h"), os.path.join(_paths.INCLUDE_DIR, "sjgpu_debug.h")]:
        h.update(os.path.relpath(f, _paths.REPO_ROOT).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()


def sjgpu_is_current():
    path = os.path.join(TEST_BIN_DIR, "STAMP.json")
    out = os.path.join(_paths.LIB_DIR, "libsjgpu.so")
    return os.path.exists(path) and os.path.exists(out) and json.load(open(path)).get("libsjgpu.so") == sjgpu_source_stamp()


def build_sjgpu(force=False):
    out = os.path.join(_paths.LIB_DIR, "libsjgpu.so")  # always the in-tree default, never an SJGPU_LIB override
    srcs = _csrc(*SJGPU_SOURCES)
    if force or not sjgpu_is_current():
        os.makedirs(_paths.LIB_DIR, exist_ok=True)
        _run([HIPCC, f"--offload-arch={GFX_ARCH}", "-O3", "-std=c++17", "-fPIC", "-shared", "-pthread",
              "-I", _paths.INCLUDE_DIR, "-I", _paths.CSRC_DIR, *srcs, "-o", out, "-ldl"])  # RCCL is opened by sjgpu_comm_* on first use, not linked
        os.makedirs(TEST_BIN_DIR, exist_ok=True)
        path = os.path.join(TEST_BIN_DIR, "STAMP.json")
        d = json.load(open(path)) if os.path.exists(path) else {}
        d["libsjgpu.so"] = sjgpu_source_stamp()
        json.dump(d, open(path, "w"), indent=1, sort_keys=True)
    return out


TEST_BIN_DIR = os.path.join(_paths.REPO_ROOT, "build", "tests")  # our own test infrastructure (libsjgpu's stamp, the RCCL loop-back)

# the recipes that compile against the reference live beside its other checkers, under oracle/ (outputs: oracle/_ref/)
sys.path.insert(0, _paths.ORACLE_DIR)
from ref_build import (INTREE_TESTS, REF_TEST_BIN_DIR, REFERENCE_TESTS, binary_is_current, build_intree, build_plugin,  # noqa: E402,F401
                       build_plugin_test, build_reference_tests, source_stamp)


def build_oracle():
    _run(["make", "-s", "-C", _paths.ORACLE_DIR, f"REFERENCE={_paths.REFERENCE_DIR}"])


LOOPBACK_SRC = os.path.join(_paths.REPO_ROOT, "tests", "stubs", "rccl_loopback.cpp")
LIB_LOOPBACK_HIP = os.path.join(TEST_BIN_DIR, "librccl_loopback_hip.so")


def build_rccl_loopback(force=False):
    """tests/stubs/rccl_loopback.cpp against the real HIP / RCCL headers -> build/tests/librccl_loopback_hip.so: the stand-in for librccl
    whose ranks are threads of one process (test infrastructure: SJGPU_RCCL_LIB points libsjgpu's dlopen at it in tests/test_gpu_comm.py, so
    sjgpu_comm_gather_indices runs with a world of two and three on a one-GPU box).  Host code only; hipcc supplies the include paths."""
    if force or _stale(LIB_LOOPBACK_HIP, [LOOPBACK_SRC]):
        os.makedirs(TEST_BIN_DIR, exist_ok=True)
        _run([HIPCC, "-std=c++17", "-O2", "-fPIC", "-shared", LOOPBACK_SRC, "-o", LIB_LOOPBACK_HIP, "-lpthread"])
    return LIB_LOOPBACK_HIP


SAN_DIR = os.path.join(_paths.REPO_ROOT, "build", "san")


def build_sanitizers(force=False):
    """AddressSanitizer / ThreadSanitizer builds of the host side (scripts/sanitize.sh build: libsjgpu's host code, the plug-in, plugin_test) ->
    build/san/*, which travel to the GPU box where tests/test_plugin.py::test_sanitizers_over_the_host_shim runs them.  Needs the reference; rebuilt
    when the library's or the plug-in's sources changed (the stamp in build/tests/STAMP.json); a failure leaves the test skipped, not the build broken."""
    hdr = os.path.join(_paths.REFERENCE_DIR, "include", "simdjson.h")
    bins = [os.path.join(SAN_DIR, f"plugin_test_{s}") for s in ("address", "thread")]
    if not os.path.exists(hdr):
        return bins if all(os.path.exists(b) for b in bins) else None
    want = hashlib.sha256((sjgpu_source_stamp() + source_stamp()).encode()).hexdigest()
    path = os.path.join(TEST_BIN_DIR, "STAMP.json")
    d = json.load(open(path)) if os.path.exists(path) else {}
    if not force and d.get("san") == want and all(os.path.exists(b) for b in bins):
        return bins
    try:
        _run(["bash", os.path.join(_paths.REPO_ROOT, "scripts", "sanitize.sh"), "build"])
    except subprocess.CalledProcessError as e:
        print("[build] sanitizer builds failed:", e, flush=True)
        return None
    d = json.load(open(path)) if os.path.exists(path) else {}
    d["san"] = want
    os.makedirs(TEST_BIN_DIR, exist_ok=True)
    json.dump(d, open(path, "w"), indent=1, sort_keys=True)
    return bins


def build_all(force=False):
    build_corpus(force)
    build_sjgpu(force)
    build_oracle()
    build_rccl_loopback(force)
    build_plugin(force)
    build_plugin_test(force)
    build_reference_tests(force)
    build_intree(force)
    build_sanitizers(force)


if __name__ == "__main__":
    build_all(force="--force" in sys.argv)
