"""One measurement of the JSON text call (sjgpu_serialize_cells_device) beside the mover it should be compared with, in the manner of scripts/dictionary_once.py.

Builds one twitter-like document of --mib MiB (simdjson_amd/csrc/corpus.c: `{"statuses": [ ... ]}`) and one amazon-like NDJSON stream of --nd-mib MiB, their tapes
(sjgpu_stage2_many_device), and the rows:
  (a) `$.statuses[*].user.entities` of the document   small containers, one per status (the synthetic statuses keep their entities under the user)
  (b) `$.statuses[*]`                              whole records: nearly all of the document's bytes leave as text
  (c) the root of every record of the NDJSON stream (sjgpu_at_pointers_device with the empty pointer), beside sjgpu_minify_device over the SAME source bytes in the
      same process: the same order of output bytes, by a mover near its roofline.  c_over_minify is the yardstick
  (d) a column of --doubles doubles, `$[*]` of an array of seeded random ones: scalar cells, served from the cell, two conversions each
Everything is timed in one process, warmed, alternating, with events on the stream, median of --reps; the call waits for the stream (the total is read back) and runs
at the exact capacity, found by a call with room for nothing.  Before anything is timed the outputs are compared: every text of a sample of (a), (b) and (c) parses
with Python's json to what the source says there, and (d)'s texts read back as the doubles they were made from.
Writes --out (profiles/json_text.txt) and prints the same JSON line."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from simdjson_amd import build, capi, corpus, json_text  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--nd-mib", type=int, default=256)
    ap.add_argument("--doubles", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "json_text.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this script measures, it does not fall back")
    build.build_sjgpu()
    host, statuses = corpus.twitter_like(args.mib << 20, 7)
    nd_host, lines = corpus.amazon_ndjson(args.nd_mib << 20, 7)
    rng = np.random.default_rng(7)
    numbers = (rng.standard_normal(args.doubles) * 10.0 ** rng.integers(-8, 9, args.doubles)).tolist()
    d_host = np.frombuffer(("[" + ",".join(repr(x) for x in numbers) + "]").encode(), np.uint8)
    p = capi.DomParserImplementation(max(len(host), len(nd_host), len(d_host)) + 64)
    D = capi.ResidentStream(p, host, doc_cap=1)
    N = capi.ResidentStream(p, nd_host, doc_cap=lines)
    F = capi.ResidentStream(p, d_host, doc_cap=1)
    assert (D.code, D.docs, N.code, N.docs, F.code, F.docs) == (0, 1, 0, lines, 0, 1), (D.code, D.docs, N.code, N.docs, F.code, F.docs)
    s = D.stream

    def rows_of(S, path, cap):
        offsets, status = torch.empty(2, dtype=torch.int32, device="cuda"), torch.empty(1, dtype=torch.uint8, device="cuda")
        values, tags = torch.empty(cap, dtype=torch.int64, device="cuda"), torch.empty(cap, dtype=torch.uint8, device="cuda")
        rc, rows = p.at_paths_wide_device(*S.args(), [path], offsets.data_ptr(), status.data_ptr(), values.data_ptr(), tags.data_ptr(), cap, s)
        assert rc == 0 and 0 < rows <= cap, (path, rc, rows)
        return values, tags, rows

    class Serialize:
        """one row's texts at their exact capacity"""

        def __init__(self, S, row):
            self.S, (self.values, self.tags, self.n) = S, row
            self.offsets, self.status = torch.empty(self.n + 1, dtype=torch.int32, device="cuda"), torch.empty(self.n, dtype=torch.uint8, device="cuda")
            rc, self.bytes = json_text.serialize_cells_device(p, *S.args(), self.values.data_ptr(), self.tags.data_ptr(), self.n, self.offsets.data_ptr(), self.status.data_ptr(), 0, 0, s)
            assert rc == -5 and self.bytes > 0, (rc, self.bytes)
            self.chars = torch.empty(self.bytes, dtype=torch.uint8, device="cuda")

        def __call__(self):
            rc, total = json_text.serialize_cells_device(p, *self.S.args(), self.values.data_ptr(), self.tags.data_ptr(), self.n, self.offsets.data_ptr(), self.status.data_ptr(),
                                                         self.chars.data_ptr(), self.bytes, s)
            assert (rc, total) == (0, self.bytes), (rc, total)

        def texts(self, which):
            at, chars = self.offsets.cpu().numpy().view(np.uint32), self.chars.cpu().numpy()
            return [chars[int(at[r]): int(at[r + 1])].tobytes() for r in which]

    nd_values, nd_tags = torch.empty(lines, dtype=torch.int64, device="cuda"), torch.empty(lines, dtype=torch.uint8, device="cuda")
    assert p.at_pointers_device(*N.args(), [b""], nd_values.data_ptr(), nd_tags.data_ptr(), s) == 0
    runs = {"a": Serialize(D, rows_of(D, b"$.statuses[*].user.entities", statuses)), "b": Serialize(D, rows_of(D, b"$.statuses[*]", statuses)),
            "c": Serialize(N, (nd_values, nd_tags, lines)), "d": Serialize(F, rows_of(F, b"$[*]", args.doubles))}
    minified = torch.empty(len(nd_host) + 64, dtype=torch.uint8, device="cuda")

    def run_minify():
        assert p.minify_device(N.buf.data_ptr(), len(nd_host), minified.data_ptr(), s) == 0

    for fn in runs.values():
        fn()
    run_minify()
    _, _, minified_bytes = p.result(s)
    torch.cuda.synchronize()
    for e in runs.values():
        assert not bool(e.status.any().item()), "a cell was refused"
    source = json.loads(host.tobytes())["statuses"]
    sample = np.random.default_rng(1).integers(0, statuses, 200).tolist()
    for r, text in zip(sample, runs["a"].texts(sample)):
        assert json.loads(text) == source[r]["user"]["entities"], "(a): a text is not its status's entities"
    for r, text in zip(sample, runs["b"].texts(sample)):
        assert json.loads(text) == source[r], "(b): a text is not its status"
    nd_lines = nd_host.tobytes().split(b"\n")
    nd_sample = np.random.default_rng(2).integers(0, lines, 2000).tolist()
    for r, text in zip(nd_sample, runs["c"].texts(nd_sample)):
        assert json.loads(text) == json.loads(nd_lines[r]), "(c): a text is not its record"
    for r, text in zip(sample, runs["d"].texts(sample)):
        assert float(text) == numbers[r], "(d): a text does not read back as its double"

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    named = {"a_entities_ms": runs["a"], "b_statuses_ms": runs["b"], "c_ndjson_roots_ms": runs["c"], "c_minify_same_bytes_ms": run_minify, "d_doubles_ms": runs["d"]}
    for _ in range(args.warmup):
        for fn in named.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in named}
    for _ in range(args.reps):  # alternating: what the clock and the neighbours do hits all alike
        for name, fn in named.items():
            times[name].append(timed(fn))
    out = {"mib": round(len(host) / 2 ** 20, 1), "nd_mib": round(len(nd_host) / 2 ** 20, 1), "rows": {k: int(e.n) for k, e in runs.items()},
           "bytes": {k: int(e.bytes) for k, e in runs.items()}, "minified_bytes": int(minified_bytes), "reps": args.reps}
    for name, t in times.items():
        out[name] = {"median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3)}
    med = {name: statistics.median(t) for name, t in times.items()}
    out["c_over_minify"] = round(med["c_ndjson_roots_ms"] / med["c_minify_same_bytes_ms"], 1)
    out["gb_per_s_out"] = {k: round(runs[k].bytes / med[name] / 1e6, 2) for k, name in (("a", "a_entities_ms"), ("b", "b_statuses_ms"), ("c", "c_ndjson_roots_ms"), ("d", "d_doubles_ms"))}
    out["ns_per_cell"] = {k: round(1e6 * med[name] / runs[k].n, 1) for k, name in (("a", "a_entities_ms"), ("b", "b_statuses_ms"), ("c", "c_ndjson_roots_ms"), ("d", "d_doubles_ms"))}
    p.close()
    line = json.dumps(out)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
