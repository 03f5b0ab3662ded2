"""GPU tier (-m gpu): the two entry points of include/sjgpu_dict.h on a caller's stream with inputs that arrive late -- the probe of tests/test_gpu_stream_order.py
(its world, side stream and delay, imported) over two cases of their own.  They belong in that module's TABLE, under the names of the bindings in
simdjson_amd/dictionary.py, once it may be edited.  The encode is modelled on gather_strings_device's case: it waits for the stream, so its inputs must be real by
the time it reads them; the census by code only enqueues: the gate must still be closed when it returns."""
import numpy as np
import pytest

import cast_model
import dictionary_model
import stream_order as so
import test_gpu_query
from simdjson_amd import dictionary
from test_gpu_stream_order import delay, probe, side, world  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def dictionary_encode_device(W):
    """the strings under /2 of every amazon record.  The decoy row is the real one read backwards: the same strings, another first-occurrence order -- codes made
    from it are other codes -- over the decoy document's string buffer"""
    import torch
    A, p = W.amazon, W.parser()
    tags, values = (x[0] for x in test_gpu_query.model(A.T, [b"/2"]))
    n = len(tags)
    want = dictionary_model.encode(tags, values, A.T.sbuf)
    G = len(want[1])
    assert G > 10 and not np.array_equal(dictionary_model.encode(tags[::-1], values[::-1], A.T.sbuf)[0], want[0])
    row_values, row_tags = so.Late(values, values[::-1].copy(), pad=1), so.Late(tags, tags[::-1].copy(), pad=1)
    codes, dict_values, dict_tags = so.poisoned(n, torch.int32), so.poisoned(G, torch.int64), so.poisoned(G, torch.uint8)
    first, counts = so.poisoned(G, torch.int32), so.poisoned(G, torch.int32)

    def check(ret, kept, note):
        assert ret == (0, G), (ret, G, note)
        assert np.array_equal(kept[0].view(np.int32), want[0]), f"the codes {note}"
        assert np.array_equal(kept[3], want[1]) and np.array_equal(kept[1], want[2]) and np.array_equal(kept[4], want[3]), f"the dictionary {note}"
        assert (kept[2] == ord('"')).all(), f"the dictionary's tags {note}"
    return [so.Case("dictionary_encode_device", [A.sbuf, row_values, row_tags], [codes, dict_values, dict_tags, first, counts],
                    lambda st: dictionary.dictionary_encode_device(p, A.sbuf.ptr, len(A.T.sbuf), row_values.ptr, row_tags.ptr, n, codes.data_ptr(), dict_values.data_ptr(),
                                                                   dict_tags.data_ptr(), first.data_ptr(), counts.data_ptr(), G, st), check)]


def kinds_by_code_device(W):
    """cells of every kind under 40 codes (LDS) and under 600 (global atomics); the decoy codes are the next group's, the decoy words change every integer's sign"""
    import torch
    p, cases = W.parser(), []
    rng = np.random.default_rng(96)
    n = 8449
    tags = rng.choice(np.frombuffer(b'{["ludtfn\x11\x13\x14\x16\x00', np.uint8), n)
    values = rng.integers(0, 1 << 62, n, dtype=np.uint64)
    d_values, d_tags = so.Late(values, so.decoy_cells(values)), so.Late(tags)
    for groups in (40, 600):
        codes = rng.integers(-1, groups, n).astype(np.int32)
        d_codes = so.Late(codes, ((codes + 2) % (groups + 1) - 1).astype(np.int32))
        want = dictionary_model.kinds_by_code(codes, tags, values, groups)
        assert not np.array_equal(want, dictionary_model.kinds_by_code(((codes + 2) % (groups + 1) - 1), tags, so.decoy_cells(values), groups))
        assert np.array_equal(want.sum(axis=0, dtype=np.uint64), cast_model.kinds(tags[codes >= 0][None, :], values[codes >= 0][None, :])[0])
        kinds = so.poisoned(groups * 16, torch.int32)

        def check(ret, kept, note, want=want, groups=groups):
            assert ret == 0, (ret, note)
            assert np.array_equal(kept[0].reshape(groups, 16), want), f"the census by code {note}"
        cases.append(so.Case(f"kinds_by_code_device[{groups}]", [d_codes, d_values, d_tags], [kinds],
                             lambda st, d_codes=d_codes, kinds=kinds, groups=groups: dictionary.kinds_by_code_device(p, d_codes.ptr, d_values.ptr, d_tags.ptr, n, groups,
                                                                                                                       kinds.data_ptr(), st), check, only_enqueues=True))
    return cases


CASES = {"dictionary_encode_device": dictionary_encode_device, "kinds_by_code_device": kinds_by_code_device}


@pytest.mark.parametrize("entry", list(CASES))
def test_entry_point_with_late_inputs(world, side, delay, entry):  # noqa: F811
    for case in CASES[entry](world):
        probe(case, side, delay)
