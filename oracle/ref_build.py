"""Builds against the reference (test infrastructure, never the product path): every output lies under oracle/_ref/.

    libsimdjson_mi355x.so  g++ against the reference's public headers: the simdjson::implementation plug-in shim
    tests/plugin_test      tests/plugin/plugin_test.cpp: the unmodified reference library + the shim
    tests/ref_*            the reference's own test programs, linked with the shim + an activator TU
    tests/intree_*         the reference's own test programs against a patched scratch copy of it (intree/)

Each target is built where the reference's sources are and kept, prebuilt, where they are not: a checkout that carries
oracle/_ref/ but not the reference runs the tests that need these.  oracle/_ref/tests/STAMP.json records the hashes of our
sources each test program was built from, and tests refuse a stale binary.  Called through simdjson_amd.build.build_all();
the reference object and the C-ABI wrapper of the reference (libsjref.so) come from the Makefile beside this file.
"""
import hashlib
import json
import os
import shutil
import subprocess

from simdjson_amd import _paths


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


def build_plugin(force=False):
    """simdjson::implementation shim; skipped (prebuilt kept) when the reference headers are absent."""
    srcs = _csrc("plugin/mi355x_implementation.cpp")
    hdr = os.path.join(_paths.REFERENCE_DIR, "include", "simdjson.h")
    if not os.path.exists(hdr) or not all(os.path.exists(s) for s in srcs):
        return _paths.LIB_PLUGIN if os.path.exists(_paths.LIB_PLUGIN) else None
    deps = srcs + _csrc("plugin/mi355x_implementation.h") + [os.path.join(_paths.INCLUDE_DIR, "sjgpu.h")]
    if force or _stale(_paths.LIB_PLUGIN, deps):
        os.makedirs(_paths.ORACLE_OUT, exist_ok=True)
        _run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DSIMDJSON_THREADS_ENABLED=1",
              "-I", os.path.join(_paths.REFERENCE_DIR, "include"), "-I", _paths.INCLUDE_DIR, "-I", _paths.CSRC_DIR,
              *srcs, "-o", _paths.LIB_PLUGIN, f"-L{_paths.LIB_DIR}", "-lsjgpu", "-Wl,-rpath,$ORIGIN/../../simdjson_amd/lib"])
    return _paths.LIB_PLUGIN


REF_TEST_BIN_DIR = os.path.join(_paths.ORACLE_OUT, "tests")            # test programs that link the reference
_RPATH = ["-Wl,-rpath,$ORIGIN/../../../simdjson_amd/lib", "-Wl,-rpath,$ORIGIN/.."]  # libsjgpu / libsjcorpus, and the plug-in in oracle/_ref/
_REF_LINK = [f"-L{_paths.LIB_DIR}", f"-L{_paths.ORACLE_OUT}"]


def _stamp_sources():
    """Everything of OURS a prebuilt test binary embeds (libsjgpu.so / the plug-in .so are linked dynamically)."""
    plug = os.path.join(_paths.REPO_ROOT, "tests", "plugin")
    files = [os.path.join(_paths.INCLUDE_DIR, "sjgpu.h"), *_csrc("plugin/mi355x_implementation.h", "plugin/intree/simdjson_mi355x.patch")]
    files += sorted(os.path.join(plug, f) for f in os.listdir(plug) if f.endswith((".cpp", ".h")))
    return files


def source_stamp():
    h = hashlib.sha256()
    for f in _stamp_sources():
        h.update(os.path.relpath(f, _paths.REPO_ROOT).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()


def _write_stamp(name):
    path = os.path.join(REF_TEST_BIN_DIR, "STAMP.json")
    d = json.load(open(path)) if os.path.exists(path) else {}
    d[name] = source_stamp()
    json.dump(d, open(path, "w"), indent=1, sort_keys=True)


def binary_is_current(name):
    """True iff oracle/_ref/tests/<name> exists and was built from the sources as they are now."""
    path = os.path.join(REF_TEST_BIN_DIR, "STAMP.json")
    if not (os.path.exists(path) and os.path.exists(os.path.join(REF_TEST_BIN_DIR, name))):
        return False
    return json.load(open(path)).get(name) == source_stamp()


def build_plugin_test(force=False):
    """tests/plugin/plugin_test.cpp -> oracle/_ref/tests/plugin_test: unmodified reference library + our shim.
    Needs the reference (headers + oracle/_ref/simdjson_ref.o) to build; kept prebuilt where the reference is absent."""
    out = os.path.join(REF_TEST_BIN_DIR, "plugin_test")
    src = os.path.join(_paths.REPO_ROOT, "tests", "plugin", "plugin_test.cpp")
    ref_obj = os.path.join(_paths.ORACLE_OUT, "simdjson_ref.o")
    hdr = os.path.join(_paths.REFERENCE_DIR, "include", "simdjson.h")
    if not (os.path.exists(hdr) and os.path.exists(ref_obj) and os.path.exists(_paths.LIB_PLUGIN)):
        return out if os.path.exists(out) else None
    if force or not binary_is_current("plugin_test") or _stale(out, [src, ref_obj, _paths.LIB_PLUGIN, _paths.LIB_CORPUS]):
        os.makedirs(REF_TEST_BIN_DIR, exist_ok=True)
        _run(["g++", "-O2", "-std=c++17", "-DSIMDJSON_THREADS_ENABLED=1", "-I", os.path.join(_paths.REFERENCE_DIR, "include"),
              "-I", os.path.join(_paths.CSRC_DIR, "plugin"), "-I", _paths.INCLUDE_DIR, src, ref_obj, "-o", out,
              *_REF_LINK, "-lsimdjson_mi355x", "-lsjgpu", "-lsjcorpus", "-lpthread", *_RPATH])
        _write_stamp("plugin_test")
    return out


REFERENCE_TESTS = {  # reference test programs that need no external data files
    "ref_unicode_tests": "tests/unicode_tests.cpp",
    "ref_dom_document_stream_tests": "tests/dom/document_stream_tests.cpp",
    "ref_dom_document_stream_fuzz_tests": "tests/dom/document_stream_fuzz_tests.cpp",
    "ref_ondemand_document_stream_tests": "tests/ondemand/ondemand_document_stream_tests.cpp",
    "ref_ondemand_document_stream_fuzz_tests": "tests/ondemand/ondemand_document_stream_fuzz_tests.cpp",
}


def build_reference_tests(force=False):
    """The reference's OWN test programs, compiled in place from the reference's tests/ and linked with the
    mi355x plug-in + an activator TU, so they exercise our backend unmodified.  Outputs oracle/_ref/tests/ref_*."""
    ref = _paths.REFERENCE_DIR
    ref_obj = os.path.join(_paths.ORACLE_OUT, "simdjson_ref.o")
    act = os.path.join(_paths.REPO_ROOT, "tests", "plugin", "activate_mi355x.cpp")
    built = []
    for name, rel in REFERENCE_TESTS.items():
        out = os.path.join(REF_TEST_BIN_DIR, name)
        src = os.path.join(ref, rel)
        if not (os.path.exists(src) and os.path.exists(ref_obj) and os.path.exists(_paths.LIB_PLUGIN)):
            if os.path.exists(out):
                built.append(out)
            continue
        if force or not binary_is_current(name) or _stale(out, [src, act, ref_obj, _paths.LIB_PLUGIN]):
            os.makedirs(REF_TEST_BIN_DIR, exist_ok=True)
            _run(["g++", "-O1", "-std=c++17", "-w", "-DSIMDJSON_THREADS_ENABLED=1", "-I", os.path.join(ref, "include"), "-I", os.path.join(ref, "tests"),
                  "-I", os.path.join(ref, "tests", "dom"), "-I", os.path.join(ref, "tests", "ondemand"),
                  "-I", os.path.join(_paths.CSRC_DIR, "plugin"), "-I", _paths.INCLUDE_DIR,
                  # data files come from the committed fixtures, relative to the checkout (the tests run the programs from its root)
                  '-DSIMDJSON_BENCHMARK_DATA_DIR="tests/golden/jsonexamples/"',
                  src, act, ref_obj, "-o", out, *_REF_LINK, "-lsimdjson_mi355x", "-lsjgpu", "-lpthread",
                  *_RPATH])
            _write_stamp(name)
        built.append(out)
    return built


INTREE_DIR = os.path.join(_paths.ORACLE_OUT, "intree")
INTREE_PATCH = os.path.join(_paths.CSRC_DIR, "plugin", "intree", "simdjson_mi355x.patch")
INTREE_TESTS = {"intree_basictests": "tests/dom/basictests.cpp", "intree_errortests": "tests/dom/errortests.cpp",
                # parse_many with the stream registered by document_stream::start() (the patch's second half): windows cut out of look-ahead spans
                "intree_document_stream_tests": "tests/dom/document_stream_tests.cpp", "intree_document_stream_fuzz_tests": "tests/dom/document_stream_fuzz_tests.cpp",
                # iterate_many: On-Demand's document_stream::start() registers its buffer the same way (round 4)
                "intree_ondemand_document_stream_tests": "tests/ondemand/ondemand_document_stream_tests.cpp",
                "intree_ondemand_document_stream_fuzz_tests": "tests/ondemand/ondemand_document_stream_fuzz_tests.cpp"}


def build_intree(force=False):
    """In-tree registration: a SCRATCH copy of the reference's src/ and include/ under oracle/_ref/intree/
    (git-ignored, never committed) gets simdjson_mi355x.patch -- an `mi355x` entry in the compile-time kernel list of
    src/implementation.cpp -- and is compiled with -DSIMDJSON_IMPLEMENTATION_MI355X=1; the reference's own basictests /
    errortests are then built against THAT library, so `-a mi355x` and SIMDJSON_FORCE_IMPLEMENTATION=mi355x select the
    backend by name, without any activation code in the program.  Outputs oracle/_ref/tests/intree_*."""
    ref = _paths.REFERENCE_DIR
    if not (os.path.exists(os.path.join(ref, "src", "simdjson.cpp")) and os.path.exists(_paths.LIB_PLUGIN)):
        return [os.path.join(REF_TEST_BIN_DIR, n) for n in INTREE_TESTS if os.path.exists(os.path.join(REF_TEST_BIN_DIR, n))]
    tree = os.path.join(INTREE_DIR, "simdjson")
    obj = os.path.join(INTREE_DIR, "simdjson_mi355x.o")
    if force or _stale(obj, [INTREE_PATCH, os.path.join(ref, "src", "implementation.cpp")]):
        shutil.rmtree(tree, ignore_errors=True)
        os.makedirs(tree, exist_ok=True)
        for sub in ("src", "include"):
            shutil.copytree(os.path.join(ref, sub), os.path.join(tree, sub))
        for dirpath, _, files in os.walk(tree):  # the reference tree is read-only; the scratch copy must not be
            os.chmod(dirpath, 0o755)
            for f in files:
                os.chmod(os.path.join(dirpath, f), 0o644)
        _run(["patch", "-p1", "-s", "-i", INTREE_PATCH], cwd=tree)
        _run(["g++", "-O2", "-std=c++17", "-DSIMDJSON_THREADS_ENABLED=1", "-DSIMDJSON_IMPLEMENTATION_MI355X=1", "-I", os.path.join(tree, "include"),
              "-I", os.path.join(tree, "src"), "-c", os.path.join(tree, "src", "simdjson.cpp"), "-o", obj])
    built = []
    for name, rel in INTREE_TESTS.items():
        out = os.path.join(REF_TEST_BIN_DIR, name)
        src = os.path.join(ref, rel)
        if force or not binary_is_current(name) or _stale(out, [src, obj, _paths.LIB_PLUGIN]):
            os.makedirs(REF_TEST_BIN_DIR, exist_ok=True)
            _run(["g++", "-O1", "-std=c++17", "-w", "-DSIMDJSON_THREADS_ENABLED=1", "-DSIMDJSON_IMPLEMENTATION_MI355X=1", "-I", os.path.join(tree, "include"),
                  "-I", os.path.join(ref, "tests"), "-I", os.path.join(ref, "tests", "dom"), "-I", os.path.join(ref, "tests", "ondemand"),
                  '-DSIMDJSON_BENCHMARK_DATA_DIR="tests/golden/jsonexamples/"', src, obj, "-o", out,
                  *_REF_LINK, "-lsimdjson_mi355x", "-lsjgpu", "-lpthread", *_RPATH])
            _write_stamp(name)
        built.append(out)
    return built
