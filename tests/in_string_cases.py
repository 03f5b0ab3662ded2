"""Cells and string buffers for the tests of sjgpu_cast_string_cells_device, shared by the CPU tier (tests/test_cast_strings_emu.py) and the GPU tier
(tests/test_gpu_cast_strings.py): a synthetic string buffer laid out as the parser lays its own out, words that point into it and past it, and random rows
whose tags cover all 256 bytes."""
import struct

import numpy as np

import in_string_model

# contents that need an escape in a document (the model stands alone for these: tests/test_in_string_model.py) and a few of each length around the window
ESCAPED = [b'12"', b"1\\", b"12\x01", b'"12', b"1\t", b"12\x00"]
SHORT = [b"505874924095815700", b"-7", b"3.25", b"1e3", b"12345678901234567", b"0.1", b"17.5e-3", b"99999999999999999999", b"1" * 31 + b"x", b"1" * 32, b"2" * 33,
         b"0." + b"3" * 30, b"0." + b"3" * 31, b"1.5" + b" " * 29, b"1.5" + b" " * 30, b"1e" + b"0" * 29 + b"5", b"1e" + b"0" * 30 + b"5", b"x" * 40]
EDGE_WORDS = np.array([0, 1, (1 << 64) - 1, (1 << 63) - 1, 1 << 63, (1 << 63) + 1, 1 << 53, (1 << 53) + 1, 18446744073709550592, 0x3FF8000000000000, 0x7FEFFFFFFFFFFFFF,
                       0x5A5A5A5A5A5A5A5A], np.uint64)


def pool():
    return [c for c, _ in in_string_model.load_fixture()] + ESCAPED + SHORT


def string_buffer(contents):
    """the contents as the parser stores strings: a 4-byte length, the bytes, a NUL -- the first record's bytes begin at offset 4, and the LAST record's last byte
    is the buffer's last byte (its NUL is cut off).  -> (buffer bytes, the word (length << 32) | offset of every content)"""
    out, words = bytearray(), []
    for c in contents:
        out += struct.pack("<I", len(c))
        words.append((len(c) << 32) | len(out))
        out += c + b"\0"
    del out[-1]
    return bytes(out), words


def outside_words(string_bytes):
    """words of string cells that point outside a buffer of string_bytes bytes, by one byte and by far"""
    return [(1 << 32) | string_bytes, (2 << 32) | (string_bytes - 1), (5 << 32) | 0xFFFFFFFF, (0xFFFFFFFF << 32) | 4, (0xFFFFFFFF << 32) | 0xFFFFFFFF, (string_bytes << 32) | 1]


def random_cells(rng, n, K, words, string_bytes):
    """tags over all 256 bytes (strings most often, then the other tags and the codes), string words from `words` and from outside, other words from the edges"""
    common = np.frombuffer(b'{[ludtfn' + bytes([17, 19, 20, 22]), np.uint8)
    r = rng.random((K, n))
    tags = np.where(r < 0.55, np.uint8(0x22), np.where(r < 0.85, common[rng.integers(0, len(common), (K, n))], rng.integers(0, 256, (K, n)).astype(np.uint8))).astype(np.uint8)
    flat = tags.reshape(-1)
    flat[: min(256, flat.size)] = np.arange(min(256, flat.size), dtype=np.uint8)  # every byte at least once where there is room
    inside, outside = np.array(words, np.uint64), np.array(outside_words(string_bytes), np.uint64)
    strings = np.where(rng.random((K, n)) < 0.97, inside[rng.integers(0, len(inside), (K, n))], outside[rng.integers(0, len(outside), (K, n))])
    values = np.where(tags == 0x22, strings, EDGE_WORDS[rng.integers(0, len(EDGE_WORDS), (K, n))])
    return tags, values


def halfway(digits, odd):
    """an integer of `digits` digits exactly half way between two neighbouring doubles; odd: the double below has an odd significand (the tie goes up)"""
    e = (10 ** digits - 1).bit_length() - 53
    m = ((10 ** digits - 1) >> e) - 11
    m -= (m & 1) != int(odd)
    return (2 * m + 1) << (e - 1)


def long_decimals():
    """numbers of 25 and of 800 digits, every one valid and for the exact road: ties in both directions, their neighbours, a fraction, an exponent"""
    out = []
    for odd in (False, True):
        mid = halfway(25, odd)
        out += [str(mid + d).encode() for d in (-1, 0, 1)] + [b"-" + str(mid).encode(), str(mid).encode() + b".000", str(mid).encode() + b"e-30"]
        wide = halfway(800, odd)  # (800 digits as a fraction or under an exponent: as an integer it is beyond every double)
        out += [b"0." + str(wide + d).encode() for d in (-1, 0, 1)] + [b"-0." + str(wide).encode(), str(wide).encode() + b"E-900", str(wide).encode() + b"e-492"]
        # a tie among the subnormals, where the doubles are the multiples of 2^-1074: an odd multiple of 2^-1075, about 765 significant digits, and its neighbours
        j = (1 << 40) + 2 + int(odd)
        tie = (2 * j + 1) * 5 ** 1075
        out += [b"0." + str(tie + d).rjust(1075, "0").encode() for d in (-1, 0, 1)]
    assert all(len(c) > 32 or in_string_model.significant_digits(c) > 19 for c in out)
    return out


def cycled(K, first=0):
    """the six getter bytes in turn"""
    return [in_string_model.ALL_GETTERS[(first + k) % 6] for k in range(K)]
