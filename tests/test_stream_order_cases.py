"""CPU tier: what tests/test_gpu_stream_order.py takes for granted before it spends time on a device.

1. The decoys (tests/stream_order.py) are what they claim to be.  For every document the GPU table uses the oracle says of the decoy: the same length, the
   same structural list, the same stage-1 flags; parsed whole or document by document the same tape word count and string bytes; and ANOTHER tape -- a call
   that read the decoy cannot have produced the real answer (a document without a value outside its strings differs in its string bytes).
2. The table is complete: every public method of capi.DomParserImplementation (and of capi.Comm) that takes a `stream` is a key of the GPU module's TABLE or
   of its EXEMPT, which gives a reason.  A new entry point without an ordering test fails here."""
import inspect

import numpy as np
import pytest

import cast_model
import checkers
import stream_order as so
import test_gpu_stream_order as gpu
from simdjson_amd import capi
from test_casts_emu import random_cells


@pytest.fixture(scope="module")
def orc():
    return checkers.Oracle()


@pytest.mark.parametrize("name", sorted(gpu.documents()))
def test_a_decoy_keeps_the_structure_and_changes_the_values(orc, name):
    a = gpu.documents()[name]
    d = so.decoy_document(a)
    assert len(d) == len(a) and d.dtype == np.uint8
    changed = a != d
    assert changed.sum() > len(a) // 10, "the decoy changes too little to be told from the document"
    fixed = np.isin(a, np.frombuffer(b'{}[]:,"\\ \n\r\t', np.uint8))
    assert not (changed & fixed).any() and np.array_equal(d[fixed], a[fixed]), "a structural byte, a quote, a backslash or a blank moved"
    assert not (changed & (a >= 0x80)).any(), "a byte of a multi-byte character changed"
    idx, flags = orc.scan(a)
    didx, dflags = orc.scan(d)
    assert flags == dflags == 0 and np.array_equal(idx, didx), "the structural list or the flags"
    assert orc.validate_utf8(d) and orc.minify(d)[0] == 0 and not np.array_equal(orc.minify(d)[1], orc.minify(a)[1])
    if name.startswith("amazon"):
        begins = gpu.line_begins(a)
        spans = list(zip(begins, begins[1:] + [len(a)]))
        assert len(spans) > 1000
    else:
        spans = [(0, len(a))]
    inside, _ = so.string_masks(a)
    differ = 0
    for b, e in spans:
        ec, tape, sbuf = orc.dom_parse(a[b:e])
        dc, dtape, dsbuf = orc.dom_parse(d[b:e])
        assert ec == dc == 0, (name, b, ec, dc)
        assert len(tape) == len(dtape) and len(sbuf) == len(dsbuf), (name, b, "tape words or string bytes")
        # another tape -- unless the document has no value outside its strings (the line of column names in front of the amazon records): a tape holds
        # where a string lies, not what it says, and then the string bytes are what differs
        outside = ~inside[b:e]
        if np.array_equal(a[b:e][outside], d[b:e][outside]):
            assert not np.array_equal(sbuf, dsbuf), (name, b, "neither tape nor strings differ")
        else:
            assert not np.array_equal(tape, dtape), (name, b, "the decoy has the document's tape")
            differ += 1
    assert differ >= len(spans) - 1, f"{len(spans) - differ} documents of {name} have the tape of their decoy"


def test_the_one_bit_decoys(orc):
    """the UTF-8 verdict and the quote parity do not depend on values: their decoys differ in one byte, and the oracle gives the other answer"""
    a = gpu.documents()["twitter_like"]
    broken, flipped = so.break_utf8(a), so.flip_parity(a)
    assert (broken != a).sum() == 1 and (flipped != a).sum() == 1
    assert orc.validate_utf8(a) and not orc.validate_utf8(broken)
    assert orc.scan(a)[1] & capi.F_UNCLOSED_STRING == 0 and orc.scan(flipped)[1] & capi.F_UNCLOSED_STRING == 1


def test_the_decoy_of_cells_changes_the_census_and_the_casts():
    tags, values = random_cells(np.random.default_rng(95), gpu.N_CELLS, gpu.K_CELLS)
    decoy = so.decoy_cells(values)
    assert (decoy != values).all()
    assert not np.array_equal(cast_model.kinds(tags, values), cast_model.kinds(tags, decoy))
    for first in (0, 2):
        getters = [1 + (first + k) % 7 for k in range(gpu.K_CELLS)]
        assert not np.array_equal(cast_model.cast(tags, values, getters)[0], cast_model.cast(tags, decoy, getters)[0])


def test_the_hand_offs_of_shards_and_ranges(orc):
    """what the GPU cases pass as in_string / n_before / out_before comes from the oracle, and is not trivial: the shard begins inside a string"""
    a = gpu.documents()["twitter_like"]
    assert len(a) > gpu.RANGE + (512 << 10)
    cut, in_string, want_list, want_min = gpu.shard_of(orc, a)
    idx, _ = orc.scan(a)
    assert in_string == 1 and np.array_equal(want_list[:-3], idx[idx >= cut] - cut)
    whole = orc.minify(a)[1]
    assert np.array_equal(whole[len(whole) - len(want_min):], want_min)
    in_string, n_before, out_before, whole2 = gpu.range_handoff(orc, a)
    assert n_before == int((idx < gpu.RANGE).sum()) and 0 < out_before < len(whole) and np.array_equal(whole, whole2)


def stream_takers(cls, prefix=""):
    return {prefix + name for name, fn in inspect.getmembers(cls, inspect.isfunction)
            if not name.startswith("_") and "stream" in inspect.signature(fn).parameters}


def test_every_method_that_takes_a_stream_is_probed_or_exempt():
    takers = stream_takers(capi.DomParserImplementation) | stream_takers(capi.Comm, "Comm.")
    covered, exempt = set(gpu.TABLE), set(gpu.EXEMPT)
    assert not covered & exempt
    assert takers == covered | exempt, f"no ordering test for {sorted(takers - covered - exempt)}; no such method: {sorted((covered | exempt) - takers)}"
    assert exempt == {"Comm.gather_indices", "result"} and all(len(reason) > 20 for reason in gpu.EXEMPT.values())
    assert len(covered) >= 26
