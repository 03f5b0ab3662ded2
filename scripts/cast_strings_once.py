"""One measurement of sjgpu_cast_string_cells_device (numbers held in strings) beside two calls that were here before it, on the same rows, by the protocol of
scripts/pretty_text_once.py: one process, warmed, the calls alternating, events on the stream, median of --reps, and the outputs compared before anything is timed
-- the int64 of every cell must be the number the generator wrote.

Rows of 18-digit numeric strings from two sources: ONE dense array document `["505874924095815700", ...]` of --dense rows each (1 M and 16 M by default: the strings
lie back to back, 21 bytes apart in the source and 23 in the string buffer), and a STREAM of documents of about 350 bytes with one `id_str` field each, --stream
documents (1 M and 4 M by default; 16 M documents of 350 bytes are more bytes than the 32-bit offsets of a stream call serve), the strings as far apart as a column
picked out of records lies.  Per row: the new call under GETS_INT64 and under GETS_DOUBLE; sjgpu_cast_cells_device on the same row (GET_STRING: elementwise, the same
traffic under every getter); sjgpu_gather_strings_device on the same row at its exact capacity -- the only road there was for such a column, before the copy to
the host.  Then the share of cells the exact road decides on a row of --doubles strings that hold 17-digit doubles (repr of random floats).
Writes --out (profiles/cast_strings.txt) and prints the same JSON line."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from simdjson_amd import build, capi  # noqa: E402

HEAD = b'{"created_at":"Sun Aug 31 00:29:15 +0000 2014","id_str":"'
TAIL = b'","source":"web","truncated":false,"lang":"ja","favorite_count":0,"retweet_count":12,"text":"'


def digits_of(ids):
    """uint64[n] of 18 digits each -> uint8[n, 18], the decimal text"""
    powers = (10 ** np.arange(17, -1, -1)).astype(np.uint64)
    out = np.empty((len(ids), 18), np.uint8)
    for at in range(0, len(ids), 1 << 20):  # (a million rows at a time: the quotients are 144 bytes per row)
        out[at: at + (1 << 20)] = (ids[at: at + (1 << 20), None] // powers) % np.uint64(10) + np.uint64(48)
    return out


def dense_document(ids):
    rows = np.empty((len(ids), 21), np.uint8)
    rows[:, 0], rows[:, 19], rows[:, 20] = 0x22, 0x22, 0x2C
    rows[:, 1:19] = digits_of(ids)
    flat = np.concatenate([np.frombuffer(b"[", np.uint8), rows.reshape(-1)])
    flat[-1] = 0x5D
    return flat


def stream_of_documents(ids, width=350):
    filler = width - len(HEAD) - 18 - len(TAIL) - 3
    row = np.frombuffer(HEAD + b"0" * 18 + TAIL + b"x" * filler + b'"}\n', np.uint8)
    assert len(row) == width
    rows = np.tile(row, (len(ids), 1))
    rows[:, len(HEAD): len(HEAD) + 18] = digits_of(ids)
    return rows.reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dense", type=int, nargs="*", default=[1 << 20, 16 << 20])
    ap.add_argument("--stream", type=int, nargs="*", default=[1 << 20, 4 << 20])
    ap.add_argument("--doubles", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "cast_strings.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this script measures, it does not fall back")
    build.build_sjgpu()
    rng = np.random.default_rng(7)

    def note(what):
        print(f"[cast_strings_once] {what}", file=sys.stderr, flush=True)

    def timed(fn, s):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def stats(t):
        return {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4), "runs": len(t)}

    def measure(named, s):
        for _ in range(args.warmup):
            for fn in named.values():
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name in named}
        for _ in range(args.reps):  # alternating: what the clock and the neighbours do hits all alike
            for name, fn in named.items():
                times[name].append(timed(fn, s))
        return {name + "_ms": stats(t) for name, t in times.items()}

    def cells_of(p, S, dense, n):
        """the row of string cells: the elements of the dense array, the id_str of every document of the stream"""
        values, tags = torch.empty(n, dtype=torch.int64, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
        if dense:
            offsets, status = torch.empty(2, dtype=torch.int32, device="cuda"), torch.empty(1, dtype=torch.uint8, device="cuda")
            rc, rows = p.at_paths_wide_device(*S.args(), [b"$[*]"], offsets.data_ptr(), status.data_ptr(), values.data_ptr(), tags.data_ptr(), n, S.stream)
            assert (rc, rows) == (0, n), (rc, rows)
        else:
            assert p.at_pointers_device(*S.args(), [b"/id_str"], values.data_ptr(), tags.data_ptr(), S.stream) == 0
        S.synchronize()
        assert bool((tags == 0x22).all().item())
        return values, tags

    class Leg:
        """the calls over one row, outputs allocated once"""

        def __init__(self, p, S, values, tags, n):
            self.p, self.S, self.values, self.tags, self.n = p, S, values, tags, n
            self.out = torch.empty(n, dtype=torch.int64, device="cuda")
            self.codes = torch.empty(n, dtype=torch.uint8, device="cuda")
            self.valid = torch.empty((n + 63) // 64, dtype=torch.int64, device="cuda")
            self.counts = torch.empty(8, dtype=torch.int32, device="cuda")
            self.soff = torch.empty(n + 1, dtype=torch.int32, device="cuda")
            rc, self.bytes = p.gather_strings_device(S.sbuf.data_ptr(), S.sb, values.data_ptr(), tags.data_ptr(), n, self.soff.data_ptr(), 0, 0, S.stream)
            assert rc == capi.SJGPU_E_OVERFLOW and self.bytes > 0, (rc, self.bytes)
            self.chars = torch.empty(self.bytes, dtype=torch.uint8, device="cuda")

        def in_string(self, getter):
            rc = capi.cast_string_cells_device(self.p, self.S.sbuf.data_ptr(), self.S.sb, self.values.data_ptr(), self.tags.data_ptr(), self.n, [getter], self.out.data_ptr(),
                                               self.codes.data_ptr(), self.valid.data_ptr(), self.counts.data_ptr(), self.S.stream)
            assert rc == 0, rc

        def cast(self):
            rc = self.p.cast_cells_device(self.values.data_ptr(), self.tags.data_ptr(), self.n, [capi.GET_STRING], self.out.data_ptr(), self.codes.data_ptr(), self.valid.data_ptr(),
                                          self.counts.data_ptr(), self.S.stream)
            assert rc == 0, rc

        def gather(self):
            rc, total = self.p.gather_strings_device(self.S.sbuf.data_ptr(), self.S.sb, self.values.data_ptr(), self.tags.data_ptr(), self.n, self.soff.data_ptr(),
                                                     self.chars.data_ptr(), self.bytes, self.S.stream)
            assert (rc, total) == (0, self.bytes), (rc, total)

    out = {"reps": args.reps, "legs": {}}
    for dense, sizes in ((True, args.dense), (False, args.stream)):
        for n in sizes:
            ids = rng.integers(10 ** 17, 9 * 10 ** 17, n, dtype=np.uint64)
            host = dense_document(ids) if dense else stream_of_documents(ids)
            p = capi.DomParserImplementation(len(host) + 64)
            S = capi.ResidentStream(p, host, doc_cap=1 if dense else n)
            assert (S.code, S.docs) == (0, 1 if dense else n), (S.code, S.docs)
            values, tags = cells_of(p, S, dense, n)
            leg = Leg(p, S, values, tags, n)
            leg.in_string(capi.GETS_INT64)
            S.synchronize()
            assert np.array_equal(leg.out.cpu().numpy().view(np.uint64), ids) and leg.counts.cpu().numpy().tolist() == [n, 0, 0, 0, 0, 0, 0, 0], "the values are not the generator's"
            leg.in_string(capi.GETS_DOUBLE)
            S.synchronize()
            assert np.array_equal(leg.out.cpu().numpy().view(np.float64), ids.astype(np.float64)) and int(leg.counts[5].item()) == 0
            entry = {"rows": n, "source_bytes": int(len(host)), "string_buffer_bytes": int(S.sb), "gathered_bytes": int(leg.bytes)}
            entry.update(measure({"in_string_int64": lambda: leg.in_string(capi.GETS_INT64), "in_string_double": lambda: leg.in_string(capi.GETS_DOUBLE), "cast_cells": leg.cast,
                                  "gather_strings": leg.gather}, S.stream))
            for name in ("in_string_int64", "in_string_double"):
                entry[name + "_over_cast"] = round(entry[name + "_ms"]["median"] / entry["cast_cells_ms"]["median"], 2)
                entry[name + "_over_gather"] = round(entry[name + "_ms"]["median"] / entry["gather_strings_ms"]["median"], 2)
                entry[name + "_ns_per_cell"] = round(entry[name + "_ms"]["median"] * 1e6 / n, 3)
            out["legs"][("dense_" if dense else "stream_") + str(n)] = entry
            note(f"{'dense' if dense else 'stream'} {n}: {entry}")
            del leg, values, tags, S
            p.close()
            torch.cuda.empty_cache()
    # the share of cells the exact road decides on a row of 17-digit doubles
    floats = (rng.standard_normal(args.doubles) * 10.0 ** rng.integers(-8, 9, args.doubles)).tolist()
    host = np.frombuffer(("[" + ",".join('"' + repr(x) + '"' for x in floats) + "]").encode(), np.uint8)
    p = capi.DomParserImplementation(len(host) + 64)
    S = capi.ResidentStream(p, host, doc_cap=1)
    assert (S.code, S.docs) == (0, 1)
    values, tags = cells_of(p, S, True, args.doubles)
    leg = Leg(p, S, values, tags, args.doubles)
    leg.in_string(capi.GETS_DOUBLE)
    S.synchronize()
    counts = leg.counts.cpu().numpy().tolist()
    assert np.array_equal(leg.out.cpu().numpy().view(np.float64), np.array(floats)) and counts[0] == args.doubles, counts
    entry = {"rows": args.doubles, "exact_road_cells": counts[5], "exact_road_share": counts[5] / args.doubles}
    entry.update(measure({"in_string_double": lambda: leg.in_string(capi.GETS_DOUBLE), "cast_cells": leg.cast}, S.stream))
    out["doubles_17_digits"] = entry
    note(f"doubles: {entry}")
    p.close()
    line = json.dumps(out)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
