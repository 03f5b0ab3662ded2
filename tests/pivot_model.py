"""A numpy model of sjgpu_pivot_fields_device (include/sjgpu_pivot.h), written from the contract alone: the fields of every row -- offsets, statuses, the codes of
the keys, the value cells -- into one column per code, the first field of a row that maps to a column wins.  And what the tests need around it: the fold rule of
the reference's key_equals_case_insensitive, the long format of a set of records by Python's json (duplicate keys kept), and the answers element::at_key gives,
rendered as tests/golden/pivot.json renders them.  tests/test_pivot_model.py pins all of it against the fixture."""
import json
import os

import numpy as np

NO_SUCH_FIELD, INCORRECT_TYPE = 20, 17
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pivot.json")


def pivot(offsets, status, codes, values, tags, fields, column_of_code, groups, columns):
    """-> (tags uint8[columns, rows], values uint64[columns, rows]); column_of_code None: column = code.  `fields` is the call's argument: the arrays may be shorter
    than a broken offset claims, and then nothing of that row is read"""
    rows = len(status)
    out_tags = np.full((columns, rows), NO_SUCH_FIELD, np.uint8)
    out_values = np.zeros((columns, rows), np.uint64)
    for r in range(rows):
        if status[r]:
            out_tags[:, r] = status[r]
            continue
        lo, hi = int(offsets[r]), int(offsets[r + 1])
        if lo > hi or hi > fields:
            continue
        taken = set()
        for i in range(lo, hi):
            code = int(codes[i])
            if code < 0 or code >= groups:
                continue
            column = code if column_of_code is None else int(column_of_code[code])
            if column < 0 or column >= columns or column in taken:
                continue
            taken.add(column)
            out_tags[column, r], out_values[column, r] = tags[i], values[i]
    return out_tags, out_values


def fold_class(key):
    """two keys are one key for at_key_case_insensitive when this is equal: the length, and the bytes up to the first NUL with A-Z lowered (strncasecmp stops at a
    NUL; bytes >= 0x80 are not folded)"""
    head = key.split(b"\0", 1)[0]
    return len(key), bytes(b + 32 if 65 <= b <= 90 else b for b in head)


class Obj(list):
    """an object as its (key, value) pairs in the document's order, duplicates included"""


def parse(record):
    return json.loads(record.decode("utf-8"), object_pairs_hook=Obj)


def minify(v):
    """simdjson::minify of a value without control characters"""
    if isinstance(v, Obj):
        return "{" + ",".join(json.dumps(k, ensure_ascii=False) + ":" + minify(x) for k, x in v) + "}"
    if isinstance(v, list):
        return "[" + ",".join(minify(x) for x in v) + "]"
    if isinstance(v, str):
        return json.dumps(v, ensure_ascii=False)
    return "true" if v is True else "false" if v is False else "null" if v is None else repr(v)


def long_format(records):
    """-> (offsets uint32[rows + 1], status uint8[rows], keys: list of bytes per slot, texts: list of minified values per slot), as
    sjgpu_object_fields_from_cells_device lists the fields of the records' roots"""
    offsets, status, keys, texts = [0], [], [], []
    for record in records:
        root = parse(record)
        if isinstance(root, Obj):
            status.append(0)
            for k, v in root:
                keys.append(k.encode("utf-8"))
                texts.append(minify(v))
        else:
            status.append(INCORRECT_TYPE)
        offsets.append(len(keys))
    return np.array(offsets, np.uint32), np.array(status, np.uint8), keys, texts


def encode(keys):
    """-> (codes int32[slots], dictionary: the distinct keys in order of first occurrence)"""
    seen = {}
    return np.array([seen.setdefault(k, len(seen)) for k in keys], np.int32), list(seen)


def column_map(dictionary, keys, fold):
    """one column per listed key -> (column_of_code int32[len(dictionary)], column behind each listed key): a code maps to the column of the first listed key that
    equals it (fold: that is in its class), or to -1"""
    same = fold_class if fold else bytes
    column_of_class, pick = {}, []
    for k in keys:
        pick.append(column_of_class.setdefault(same(k), len(column_of_class)))
    return np.array([column_of_class.get(same(k), -1) for k in dictionary], np.int32), pick


def answers(records, keys, fold):
    """what at_key (fold: at_key_case_insensitive) answers for every record and listed key, through the model of the pivot: [record][key] "E <code>" | "V <text>" """
    offsets, status, slot_keys, texts = long_format(records)
    codes, dictionary = encode(slot_keys)
    column_of_code, pick = column_map(dictionary, keys, fold)
    columns = max(pick) + 1 if pick else 0
    tags, values = pivot(offsets, status, codes, np.arange(len(texts), dtype=np.uint64), np.zeros(len(texts), np.uint8), len(texts),
                         column_of_code if len(dictionary) else None, len(dictionary), columns)
    return [[("V " + texts[int(values[c, r])]) if tags[c, r] == 0 else "E %d" % tags[c, r] for c in pick] for r in range(len(records))]


def fixture():
    """-> [(records: list of bytes, keys: list of bytes, at_key answers [record][key], at_key_case_insensitive answers)]"""
    g = json.load(open(GOLDEN))
    text = g["answers"]
    return [([bytes.fromhex(r) for r in s["records"]], [bytes.fromhex(k) for k in s["keys"]], [[text[a] for a in row] for row in s["at_key"]],
             [[text[a] for a in row] for row in s["at_key_ci"]]) for s in g["sets"]]
