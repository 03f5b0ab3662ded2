"""CPU tier: the helpers under the *_many calls of simdjson_amd/capi.py that need no device -- the capacity retry (_to_capacity) against fake calls, the
marshalling of a list of bytes (_blob) -- and that importing capi does not import torch."""
import ctypes
import gc
import subprocess
import sys

import numpy as np

from simdjson_amd import _paths, capi

OVERFLOW = capi.SJGPU_E_OVERFLOW


def fake(*answers):
    """a `call` that answers in turn (rc, needed) and notes the capacities it was given"""
    caps, left = [], list(answers)

    def call(cap):
        caps.append(cap)
        rc, needed = left.pop(0)
        return rc, needed, ("outputs for", cap)
    return call, caps


def test_overflow_is_the_header_s_code():
    with open(_paths.REPO_ROOT + "/include/sjgpu.h") as f:
        assert "#define SJGPU_E_OVERFLOW  (%d)" % OVERFLOW in f.read()


def test_success_at_the_first_call_is_one_call():
    call, caps = fake((0, 7))
    assert capi._to_capacity(call, 100) == (0, 7, ("outputs for", 100)) and caps == [100]


def test_overflow_then_success_is_two_calls_the_second_at_the_reported_capacity():
    call, caps = fake((OVERFLOW, 123), (0, 123))
    assert capi._to_capacity(call, 5) == (0, 123, ("outputs for", 123)) and caps == [5, 123]


def test_overflow_twice_is_two_calls_and_the_second_code_comes_back():
    call, caps = fake((OVERFLOW, 123), (OVERFLOW, 456), (0, 456))
    assert capi._to_capacity(call, 5) == (OVERFLOW, 456, ("outputs for", 123)) and caps == [5, 123]


def test_any_other_code_at_the_first_call_is_one_call():
    for rc in (-4, -1, capi.CAPACITY, 3):
        call, caps = fake((rc, 9), (0, 9))
        assert capi._to_capacity(call, 5) == (rc, 9, ("outputs for", 5)) and caps == [5]


def test_a_capacity_of_zero_reaches_the_call_as_zero():
    call, caps = fake((OVERFLOW, 3), (0, 3))
    assert capi._to_capacity(call, 0) == (0, 3, ("outputs for", 3)) and caps == [0, 3]


def test_blob_of_nothing():
    chars, lens, count = capi._blob([])
    assert chars is not None and lens is None and count == 0


def test_blob_joins_the_bytes_and_counts_their_lengths():
    chars, lens, count = capi._blob([b"", b"/a"])
    assert count == 2
    assert ctypes.string_at(chars, 2) == b"/a"
    assert list(ctypes.cast(lens, ctypes.POINTER(ctypes.c_uint32))[:2]) == [0, 2]


def test_blob_s_pointers_keep_what_they_point_into():
    items = [bytes([65 + k]) * (k + 1) for k in range(40)]  # built here: nothing else holds the joined bytes or the lengths
    chars, lens, count = capi._blob(items)
    del items
    gc.collect()
    churn = [np.full(64, 0xEE, np.uint8).tobytes() for _ in range(1000)]  # what a freed block would be handed out to
    want = b"".join(bytes([65 + k]) * (k + 1) for k in range(40))
    assert count == 40 and ctypes.string_at(chars, len(want)) == want
    assert list(ctypes.cast(lens, ctypes.POINTER(ctypes.c_uint32))[:40]) == list(range(1, 41))
    assert chars._objects is not None and lens._objects is not None  # ctypes' own record of what a pointer keeps alive
    del churn


def test_importing_capi_does_not_import_torch():
    code = "import sys; sys.path.insert(0, %r); from simdjson_amd import capi; assert 'torch' not in sys.modules; capi.ResidentStream; print('ok')" % _paths.REPO_ROOT
    done = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert done.returncode == 0 and done.stdout.strip() == "ok", done.stderr
