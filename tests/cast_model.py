"""A numpy model of sjgpu_cast_cells_device and sjgpu_cell_kinds_device (include/sjgpu_cast.h): what dom::element::get<T> answers for every cell of K rows,
written from the reference's rules (dom/element-inl.h:219-334; a failed result forwards its code, :60-83) as whole-row masks -- it shares no code with
the kernels.  tests/test_cast_model.py pins it against tests/golden/casts.json (made from the real reference)."""
import numpy as np

INT64, UINT64, DOUBLE, BOOL, STRING, ARRAY, OBJECT = 1, 2, 3, 4, 5, 6, 7
GETTER_NAMES = ["int64", "uint64", "double", "bool", "string", "array", "object"]  # the order of the fixture's answers: getter g is GETTER_NAMES[g - 1]
INCORRECT_TYPE, NUMBER_OUT_OF_RANGE = 17, 18
KIND_TAGS = b'{["ludtfn'
KIND_CODES = (17, 19, 20, 22)
TOP = np.uint64(1 << 63)


def cast_row(tags, values, getter):
    """one row -> (value_out uint64[n], code uint8[n])"""
    tags = np.asarray(tags, np.uint8)
    values = np.asarray(values, np.uint64)
    is_ = {c: tags == ord(c) for c in '{["ludtfn'}
    ok = np.zeros(len(tags), bool)
    out = values.copy()
    code = np.full(len(tags), INCORRECT_TYPE, np.uint8)
    if getter == INT64:
        ok = is_["l"] | (is_["u"] & (values < TOP))
        code[is_["u"]] = NUMBER_OUT_OF_RANGE
    elif getter == UINT64:
        ok = is_["u"] | (is_["l"] & (values < TOP))
        code[is_["l"]] = NUMBER_OUT_OF_RANGE
    elif getter == DOUBLE:
        ok = is_["d"] | is_["l"] | is_["u"]
        out = np.where(is_["l"], values.view(np.int64).astype(np.float64).view(np.uint64), out)  # the host's casts: round to nearest even
        out = np.where(is_["u"], values.astype(np.float64).view(np.uint64), out)
    elif getter == BOOL:
        ok = is_["t"] | is_["f"]
        out = is_["t"].astype(np.uint64)
    elif getter in (STRING, ARRAY, OBJECT):
        ok = is_['"[{'[getter - STRING]]
    else:
        raise ValueError(getter)
    held = (tags >= 1) & (tags <= 33)  # a code the cell already held
    code[ok] = 0
    code[held] = tags[held]
    out = np.where(code == 0, out, np.uint64(0))
    return out, code


def cast(tags, values, getters):
    """tags uint8[K, n], values uint64[K, n], K getters -> (value_out uint64[K, n], code uint8[K, n], valid uint64[K, ceil(n / 64)], counts uint32[K, 4])"""
    tags = np.asarray(tags, np.uint8)
    values = np.asarray(values, np.uint64)
    K, n = tags.shape
    W = (n + 63) // 64
    value_out, code = np.zeros((K, n), np.uint64), np.zeros((K, n), np.uint8)
    valid, counts = np.zeros((K, W), np.uint64), np.zeros((K, 4), np.uint32)
    for k in range(K):
        value_out[k], code[k] = cast_row(tags[k], values[k], getters[k])
        bits = np.zeros(W * 64, np.uint8)
        bits[:n] = code[k] == 0
        valid[k] = np.packbits(bits, bitorder="little").view(np.uint64)
        counts[k] = [(code[k] == 0).sum(), (tags[k] == ord("n")).sum(), (code[k] == NUMBER_OUT_OF_RANGE).sum(), ((tags[k] >= 1) & (tags[k] <= 33)).sum()]
    return value_out, code, valid, counts


def kinds(tags, values):
    """-> uint32[K, 16]: the census of every row"""
    tags = np.asarray(tags, np.uint8)
    values = np.asarray(values, np.uint64)
    out = np.zeros((tags.shape[0], 16), np.uint32)
    for k in range(tags.shape[0]):
        for s, c in enumerate(KIND_TAGS):
            out[k, s] = (tags[k] == c).sum()
        out[k, 9] = ((tags[k] == ord("l")) & (values[k] >= TOP)).sum()
        for s, c in enumerate(KIND_CODES):
            out[k, 10 + s] = (tags[k] == c).sum()
        out[k, 14] = tags.shape[1] - int(out[k, :9].sum()) - int(out[k, 10:14].sum())
    return out


def infer_getters(kinds_rows):
    """the getter a loader would pick per row from its census, 0 = leave the row as cells (the rule of include/sjgpu_cast.h's users, simdjson_amd/capi.py)"""
    picked = []
    for row in np.asarray(kinds_rows).reshape(-1, 16).tolist():
        obj, arr, string, l, u, d, t, f = row[:8]
        negative, other = row[9], row[14]
        elements = obj + arr + string + l + u + d + t + f + other
        numbers = l + u + d
        if elements == 0:
            g = 0
        elif t + f == elements:
            g = BOOL
        elif string == elements:
            g = STRING
        elif arr == elements:
            g = ARRAY
        elif obj == elements:
            g = OBJECT
        elif numbers == elements:
            g = DOUBLE if d or (u and negative) else UINT64 if u else INT64
        else:
            g = 0
        picked.append(g)
    return picked
