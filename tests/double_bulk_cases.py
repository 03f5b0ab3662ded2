"""Shared by tests/test_double_bulk_cases.py (CPU tier, where every value below is pinned) and tests/test_gpu_doubles.py (GPU tier, where the device compilation of
simdjson_amd/csrc/sj_dtoa.h, sj_number.h and sj_number_in_string.h meets them): the groups of json_text_cases.double_groups() -- made by rule, a few thousand doubles
each -- as what every printer and parser of doubles in the library takes and must give.  Per group: the bits, the texts (json_text_model.double_text, whose digest
per group tests/golden/json_text.json holds from the real reference), the documents made of the texts -- an array, an NDJSON stream, an array of quoted texts, an
object -- the prettified array, and the tapes the documents parse to.  Plain Python, no GPU."""
import functools

import numpy as np

import json_text_cases
import json_text_model

SIGN = 1 << 63
GROUPS = ["powers_of_two", "powers_of_ten", "random", "subnormal_powers_of_two", "tag_lookalikes"]
SIGNED_GROUPS = ["powers_of_two", "subnormal_powers_of_two"]  # every double of these is positive: a "-" in front of its text is the double with the sign bit set
LANE_PER_WORD_GROUPS = ["tag_lookalikes", "random"]
INTEGER_PREFIXES = [[b"7"], [b"7", b"-8"], [b"7", b"-8", b"9"]]  # two tape words each: the doubles move by 2, 4 and 6 words
LITERAL_PREFIXES = [[b"null"], [b"null", b"true"], [b"null", b"true", b"false"]]  # one tape word each: the doubles move by 1, 2 and 3 words, to the other parity too
R, D, OPEN, CLOSE = (ord(c) << 56 for c in "rd[]")


class Group:
    """one group: bits, texts and everything made of them"""

    def __init__(self, name, bits, negated=False):
        assert not negated or not any(b & SIGN for b in bits)
        self.name, self.n = name + (", negated" if negated else ""), len(bits)
        self.bits = [b | SIGN for b in bits] if negated else list(bits)
        self.texts = [(b"-" if negated else b"") + json_text_model.double_text(b) for b in bits]
        self.words = np.array(self.bits, np.uint64)
        self.array = array_document(self.texts)
        self.ndjson = b"".join(t + b"\n" for t in self.texts)
        self.quoted = b"[" + b",".join(b'"' + t + b'"' for t in self.texts) + b"]"
        self.object = b"{" + b",".join(b'"k%d":' % i + t for i, t in enumerate(self.texts)) + b"}"
        self.pretty = pretty_array(self.texts)
        self.loose_pretty = b"".join(t + b"\n" for t in self.texts)  # a scalar cell prettified: its text and a newline

    def cells(self):
        """one row of loose `d` cells -> (tags, values)"""
        return np.full(self.n, ord("d"), np.uint8), self.words.copy()

    def array_tape(self):
        return array_tape(self.words)

    def scalar_tapes(self):
        return scalar_tapes(self.words)


def array_document(texts, prefix=()):
    return b"[" + b",".join(list(prefix) + list(texts)) + b"]"


def pretty_array(texts, prefix=()):
    """simdjson::prettify of array_document: four blanks per level, a newline behind the element"""
    return b"[\n" + b",\n".join(b"    " + t for t in list(prefix) + list(texts)) + b"\n]\n"


def array_tape(words):
    """the tape of [t0,t1,...]: the root word with the tape's length, [ with its count (24 bits, saturating) and the index behind ], `d` and the bits per element, ] with the index of [, the root
    word that ends the tape"""
    n = len(words)
    body = np.empty(2 * n, np.uint64)
    body[0::2], body[1::2] = np.uint64(D), words
    head = [R | (2 * n + 4), OPEN | (min(n, 0xFFFFFF) << 32) | (2 * n + 3)]
    return np.concatenate([np.array(head, np.uint64), body, np.array([CLOSE | 1, R], np.uint64)])


def scalar_tapes(words):
    """the tapes of the documents t0, t1, ... back to back, four words each: the root word with that length, `d`, the bits, the root word that ends the tape"""
    out = np.empty((len(words), 4), np.uint64)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = np.uint64(R | 4), np.uint64(D), words, np.uint64(R)
    return out.reshape(-1)


@functools.lru_cache(maxsize=None)
def group(name, negated=False):
    return Group(name, json_text_cases.double_groups()[name], negated)
