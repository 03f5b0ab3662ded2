"""The hand-made inputs of sjgpu_pivot_fields_device that the CPU tier (tests/test_pivot_emu.py) and the GPU tier (tests/test_gpu_pivot.py) both run against
tests/pivot_model.py.  A case is a dict: offsets uint32[rows + 1], status uint8[rows], codes int32[fields], values uint64[fields], tags uint8[fields], fields,
map (int32[groups] or None), groups, columns."""
import numpy as np

ROWS = (0, 1, 63, 64, 65, 255, 256, 257, 1025)
COLUMNS = (0, 1, 2, 64, 65, 300)
TAGS = np.frombuffer(b'{["ludtfn', np.uint8)


def case(offsets, status, codes, fields=None, column_map=None, groups=0, columns=0, seed=0):
    rng = np.random.default_rng(seed)
    n = len(codes)
    return {"offsets": np.asarray(offsets, np.uint32), "status": np.asarray(status, np.uint8), "codes": np.asarray(codes, np.int32),
            "values": rng.integers(1, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + np.uint64(1), "tags": rng.choice(TAGS, n), "fields": n if fields is None else fields,
            "map": None if column_map is None else np.asarray(column_map, np.int32), "groups": groups, "columns": columns}


def records(rng, rows, groups, columns, column_map=None, max_fields=12, empty_every=7, stray=True):
    """rows of 0 .. max_fields slots with codes in [0, groups) -- every empty_every-th row without a field, every eleventh with a status, and (stray) a code of -1,
    groups or beyond now and then; many rows repeat a code"""
    counts = rng.integers(0, max_fields + 1, rows)
    counts[::empty_every] = 0
    status = np.zeros(rows, np.uint8)
    status[5::11] = np.array([17, 19, 20, 22], np.uint8)[np.arange(len(status[5::11])) % 4]
    counts[status != 0] = 0  # (a root with a status has no field)
    offsets = np.concatenate([[0], np.cumsum(counts)])
    n = int(offsets[-1])
    codes = rng.integers(0, max(groups, 1), n).astype(np.int32)
    if stray and n:
        at = rng.integers(0, n, max(n // 9, 1))
        codes[at] = rng.choice(np.array([-1, -2147483648, groups, groups + 1, 2147483647], np.int64), len(at)).astype(np.int32)
    return case(offsets, status, codes, None, column_map, groups, columns, seed=int(rng.integers(1 << 30)))


def shapes():
    """every ROWS x COLUMNS: groups a little above the columns (codes without a column), the NULL map"""
    out = []
    for rows in ROWS:
        for columns in COLUMNS:
            rng = np.random.default_rng(1000 * rows + columns)
            out.append(records(rng, rows, columns + 3, columns, None, max_fields=min(2 * columns + 2, 12)))
    return out


def special():
    rng = np.random.default_rng(77)
    out = {}
    # rows without fields: none at all (fields == 0), and only the odd rows
    out["no fields at all"] = case(np.zeros(258, np.uint32), np.zeros(257, np.uint8), [], None, None, 4, 5)
    out["no fields, no codes known"] = case(np.zeros(66, np.uint32), np.array([0, 17] * 32 + [0], np.uint8), [], None, None, 0, 3)
    # every slot of a row on one column: the first wins, identity and through a map that sends all codes there
    counts = rng.integers(1, 40, 130)
    offsets = np.concatenate([[0], np.cumsum(counts)])
    out["every slot on one column"] = case(offsets, np.zeros(130, np.uint8), np.full(int(offsets[-1]), 2, np.int32), None, None, 3, 4, seed=1)
    out["every code mapped to one column"] = case(offsets, np.zeros(130, np.uint8), rng.integers(0, 9, int(offsets[-1])), None, np.full(9, 1, np.int32), 9, 2, seed=2)
    # one row of 70 000 slots over 300 codes, between two short rows
    out["one row of 70 000 slots"] = case([0, 2, 70002, 70005], [0, 0, 0], np.concatenate([[7, 7], rng.integers(0, 300, 70000), [299, 0, 299]]), None, None, 300, 300, seed=3)
    # a map with -1, with `columns` and beyond, with two and three codes on one column
    column_map = np.array([0, -1, 1, 1, 5, 6, 2, 2, 2, -2147483648, 2147483647, 4, 3, 0], np.int32)  # columns = 5: 5, 6 and the extremes map nowhere
    out["a map that merges and drops"] = records(rng, 300, len(column_map), 5, column_map)
    out["a map onto more columns than codes"] = records(rng, 129, 3, 70, np.array([69, 0, 33], np.int32))
    out["groups cut the dictionary short"] = records(rng, 200, 4, 9, np.arange(4, dtype=np.int32)[::-1].copy())
    # statuses 17, 19, 20, 22 in every column
    out["statuses"] = case([0, 1, 1, 1, 1, 1, 2], [0, 17, 19, 20, 22, 0], [0, 1], None, None, 2, 3, seed=4)
    # a slice that runs backwards and one that ends beyond `fields`: 20s, nothing of them read; their neighbours are served
    out["a slice that runs backwards"] = case([0, 3, 2, 4, 6], [0, 0, 0, 0], [0, 1, 2, 0, 1, 1], None, None, 3, 3, seed=5)
    out["a slice that ends beyond fields"] = case([0, 3, 9, 4, 0xFFFFFFFF], [0, 0, 0, 0], [0, 1, 2, 0], None, None, 3, 3, seed=6)
    out["offsets beyond a fields of 0"] = case([5, 9, 9], [0, 0], [], None, None, 3, 2, seed=7)
    return out
