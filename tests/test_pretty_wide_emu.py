"""CPU tier: cells as indented JSON text, breadth first -- the gfx950 kernel sources of sjgpu_json_wide.hip, their PRETTY instantiations, with the narrow count of
sjgpu_json.hip, k_rows_locate of sjgpu_query.hip and the scans of sjgpu_finish.hip, compiled as C++ against tests/host/emu -- run the launches of
sjgpu_prettify_cells_wide_device (tests/host/test_pretty_wide_emu.cpp) and are compared byte for byte with tests/pretty_model.py and, through it, with
tests/golden/pretty.json.  The tests of tests/test_pretty_emu.py, imported: pytest collects them here and gives them THIS module's `emu`, the wide call's driver --
the two calls have one contract, so they have one set of cases.  Behind them the cases of tests/json_wide_cases.py that only a call with one lane per tape word can
get wrong.  The driver also runs built with -fsanitize=address,undefined, as a program of its own."""
import numpy as np
import pytest

import json_text_cases
import json_wide_cases
import pretty_cases
import test_pretty_emu
from test_json_emu import EXACT, ONE_SHORT, parsed_stream
from test_pretty_emu import (fixture_rows, orc, test_a_flat_container_of_more_children_than_a_workgroup, test_a_total_beyond_32_bits,  # noqa: F401
                             test_broken_sub_tapes, test_every_kind_of_root, test_nesting_on_both_sides_of_the_spill_and_the_hand_off,
                             test_rows_at_the_wave_and_workgroup_edges, test_strings_of_every_length_and_byte, test_the_capacities, test_the_chains_in_one_row,
                             test_the_fixture_rows)

KERNEL_TUS = ("sjgpu_json_wide", "sjgpu_json", "sjgpu_query", "sjgpu_finish")
DRIVER = "test_pretty_wide_emu"


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return test_pretty_emu.runner(test_pretty_emu.build(tmp_path_factory.mktemp("pretty_wide_emu"), DRIVER, KERNEL_TUS))


# ---- what one lane per tape word can get wrong -------------------------------------------------------------------------------------------------------------------
def test_the_same_container_twice_and_a_container_beside_its_own_child(emu, orc):
    """the child's text is NOT a piece of its parent's: as a root it starts from indent 0"""
    stream = parsed_stream(orc, [json_wide_cases.NESTED_DOCUMENT])
    row = json_wide_cases.overlapping_row(stream)
    offsets, chars, status = emu(stream, row)
    texts = json_text_cases.split(offsets, chars)
    assert not status.any() and texts[0] == texts[1] == texts[3] and texts[2].startswith(b"[\n    1,\n    {\n        \"b\": [") and texts[2] not in texts[0]
    emu(stream, row, ONE_SHORT)


@pytest.mark.parametrize("words", json_wide_cases.SHARE_EDGE_WORDS)
def test_documents_at_the_edges_of_the_shares(emu, orc, words):
    """roots of 63 / 64 / 65, 255 / 256 / 257 and 511 / 512 / 513 words, once at slot 0 and once behind a scalar's slot, which moves every edge by one; and the same
    words below 15 arrays, where the container is flat and every word's newline stands BEHIND it"""
    for doc in (json_wide_cases.document_of_words(words), b"[" * 15 + json_wide_cases.document_of_words(words) + b"]" * 15):
        stream = parsed_stream(orc, [doc, b"[]"])
        root = json_text_cases.root_row(*stream)
        offsets, chars, status = emu(stream, root)
        assert not status.any()
        shifted = (np.concatenate([np.array([ord("t")], np.uint8), root[0], root[0]]), np.concatenate([np.array([1], np.uint64), root[1], root[1]]))
        emu(stream, shifted)


def test_an_object_whose_fields_cross_two_workgroups(emu, orc):
    doc = json_wide_cases.wide_object(300)
    stream = parsed_stream(orc, [doc])
    offsets, chars, status = emu(stream, json_text_cases.root_row(*stream))
    assert not status.any() and chars.startswith(b'{\n    "k0": "v0",\n    "k1": 1,\n    "k2": true,\n    "k3": {\n        "x": []\n    },\n') and chars.endswith(b"\n}\n")


@pytest.mark.parametrize("slot", json_wide_cases.BORDER_SLOTS)
def test_a_number_whose_second_word_looks_like_a_tag_at_a_share_border(emu, orc, slot):
    """the second word of an `l` with 0x7B / 0x5D / 0x6C on top ({ ] l): it is no opening word in front of a closing one, and no head"""
    for value in json_wide_cases.TAG_LIKE_INTEGERS:
        stream = parsed_stream(orc, [json_wide_cases.number_at_slot(slot, value)])
        offsets, chars, status = emu(stream, json_text_cases.root_row(*stream))
        assert not status.any() and b"[\n        %d\n    ]\n]\n" % value in chars


def test_empty_containers_as_first_middle_and_last_children(emu, orc):
    docs = json_wide_cases.EMPTY_CONTAINER_DOCUMENTS + [b"[" * 15 + d + b"]" * 15 for d in json_wide_cases.EMPTY_CONTAINER_DOCUMENTS]
    stream = parsed_stream(orc, docs)
    for capacity in (EXACT, ONE_SHORT):
        offsets, chars, status = emu(stream, json_text_cases.root_row(*stream), capacity)
    texts = json_text_cases.split(offsets, chars)
    assert not status.any() and texts[6] == b"{}\n" and texts[7] == b"[]\n" and texts[3] == b"[\n    {}\n]\n"


def test_the_driver_runs_clean_under_the_sanitizers(tmp_path, orc, fixture_rows):
    """the narrow test's calls and the new cases, through the stand-alone driver built with -fsanitize=address,undefined"""
    calls = test_pretty_emu.sanitizer_calls(orc, fixture_rows)
    nested = parsed_stream(orc, [json_wide_cases.NESTED_DOCUMENT])
    calls.append((nested, json_wide_cases.overlapping_row(nested), EXACT))
    for doc in (json_wide_cases.document_of_words(257), json_wide_cases.wide_object(300), json_wide_cases.number_at_slot(256, json_wide_cases.TAG_LIKE_INTEGERS[0]),
                b"[" * 15 + json_wide_cases.document_of_words(257) + b"]" * 15):
        stream = parsed_stream(orc, [doc])
        calls.append((stream, json_text_cases.root_row(*stream), EXACT))
    empties = parsed_stream(orc, json_wide_cases.EMPTY_CONTAINER_DOCUMENTS)
    calls.append((empties, json_text_cases.root_row(*empties), ONE_SHORT))
    test_pretty_emu.run_under_the_sanitizers(test_pretty_emu.build(tmp_path, DRIVER, KERNEL_TUS, test_pretty_emu.SANITIZE), calls)


def test_the_range_refusal(emu, orc):
    """65 537 roots over one array of 32 767 ones: status complete (the narrow PRETTY count's), offsets and characters untouched (the driver checks the poison)"""
    import subprocess
    from test_json_emu import blob_of, records_of
    stream, row = json_wide_cases.range_refusal(orc, parsed_stream)
    p = subprocess.run([emu.exe], input=blob_of(stream, row, EXACT), capture_output=True, timeout=1500)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
    (code, total, offsets, status, chars), = records_of(p.stdout, [len(row[0])])
    assert code == -8 and total == 0 and chars == b"" and not status.any() and len(status) == 65537 and (offsets == 0x5A5A5A5A).all()
