"""GPU tier (-m gpu): the entry point of include/sjgpu_pivot.h on a caller's stream with inputs that arrive late -- the probe of tests/test_gpu_stream_order.py
(its world, side stream and delay, imported) over cases of their own, as tests/test_gpu_dict_order.py does for the dictionary's.  They belong in that module's
TABLE, under the name of the binding in simdjson_amd/pivot.py, once it may be edited.  The call only enqueues: the gate must still be closed when it returns.
The decoys are valid inputs of the same shape -- the same offsets, statuses and tags, other codes, other words, another map -- so a read that came too early
gives another table, never a wild address."""
import numpy as np
import pytest

import pivot_cases
import pivot_model
import stream_order as so
from simdjson_amd import pivot
from test_gpu_stream_order import delay, probe, side, world  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def pivot_fields_device(W):
    """8 449 rows of up to a dozen fields over 40 codes, through a map that merges and drops, and with the NULL map"""
    import torch
    p, cases = W.parser(), []
    rng = np.random.default_rng(97)
    groups, rows = 40, 8449
    for name, columns, column_map in (("map", 23, rng.integers(-2, 25, groups).astype(np.int32)), ("identity", groups, None)):
        c = pivot_cases.records(rng, rows, groups, columns, column_map)
        n = c["fields"]
        decoy_codes = ((c["codes"].astype(np.int64) + 7) % groups).astype(np.int32)
        d_offsets, d_status, d_tags = so.Late(c["offsets"]), so.Late(c["status"], pad=1), so.Late(c["tags"], pad=1)
        d_codes, d_values = so.Late(c["codes"], decoy_codes, pad=1), so.Late(c["values"], so.decoy_cells(c["values"]), pad=1)
        d_map = None if column_map is None else so.Late(column_map, column_map[::-1].copy())
        want = pivot_model.pivot(c["offsets"], c["status"], c["codes"], c["values"], c["tags"], n, column_map, groups, columns)
        early = pivot_model.pivot(c["offsets"], c["status"], decoy_codes, so.decoy_cells(c["values"]), c["tags"], n, None if column_map is None else column_map[::-1], groups,
                                  columns)
        assert not np.array_equal(want[0], early[0]) and not np.array_equal(want[1], early[1])
        out_values, out_tags = so.poisoned(columns * rows, torch.int64), so.poisoned(columns * rows, torch.uint8)

        def check(ret, kept, note, want=want, columns=columns):
            assert ret == 0, (ret, note)
            assert np.array_equal(kept[1].reshape(columns, rows), want[0]), f"the tags {note}"
            assert np.array_equal(kept[0].reshape(columns, rows), want[1]), f"the cells {note}"
        inputs = [d_offsets, d_status, d_codes, d_values, d_tags] + ([] if d_map is None else [d_map])
        cases.append(so.Case(f"pivot_fields_device[{name}]", inputs, [out_values, out_tags],
                             lambda st, d_offsets=d_offsets, d_status=d_status, d_codes=d_codes, d_values=d_values, d_tags=d_tags, d_map=d_map, n=n, columns=columns,
                             out_values=out_values, out_tags=out_tags: pivot.pivot_fields_device(p, d_offsets.ptr, d_status.ptr, rows, d_codes.ptr, d_values.ptr, d_tags.ptr, n,
                                                                                                  d_map.ptr if d_map else 0, groups, columns, out_values.data_ptr(),
                                                                                                  out_tags.data_ptr(), st), check, only_enqueues=True))
    return cases


CASES = {"pivot_fields_device": pivot_fields_device}


@pytest.mark.parametrize("entry", list(CASES))
def test_entry_point_with_late_inputs(world, side, delay, entry):  # noqa: F811
    for case in CASES[entry](world):
        probe(case, side, delay)
