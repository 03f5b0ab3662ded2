"""One measurement of the nested writer (sjgpu_write_nested_device) beside a copy of the same bytes, in the manner of scripts/write_records_once.py.

Legs:
  (a) the write step of writer.project_rows_many over the twitter-like document of --doc-mib MiB: rows $.statuses[*]; the id, the hashtag index pairs as list<int64>
      ($.user.entities.hashtags[*].indices[*]), the coordinates as list<double> ($.coordinates[*]) and the metadata's values as list<string> ($.metadata.*) -- the
      generated corpus has no hashtag texts and no mentions; these are the lists it has --, the fields as the query and cast calls left them, only the writer timed
  (b) --rows rows of one list<int64> of 0 .. 8 elements
  (c) --long-rows rows of lists of about 64 doubles: rows far longer than 112 bytes, so 256 of them never fit the window (at some 1.3 KB a row 32 of them do not
      either: "group_rows_of_the_iterations" says which groups the split build would take, 0 for the direct road)
  (d) --long-rows rows of lists of 12 .. 20 doubles: some 330 bytes a row, where groups of 64 rows fit the window and 128 do not
Yardstick, not the code under test: per leg a device-to-device copy of the same number of output bytes, timed in the same process.
--variant NAME=PATH adds the same legs through another build of the library (build/ab/, e.g. the one WITH the split the product compiles out:
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -pthread -DSJGPU_NESTED_SPLIT -I include -I simdjson_amd/csrc <build.SJGPU_SOURCES> -o build/ab/libsjgpu_nested_split.so -ldl),
loaded under its own copy of simdjson_amd.capi as scripts/lib_ab.py loads its variants; its output is compared byte for byte with the product's.
Everything is timed in one process, warmed, alternating, with events on the stream, median of --reps with min and max; the call waits for the stream (the total is read
back) and runs at the exact capacity, found by a call with room for nothing.  Before anything is timed the outputs are compared with tests/nested_write_model.py: a
sample of rows of every leg, row by row; and the road every iteration of the fill takes is counted from the offsets (tests/nested_write_cases.group_rows).
Writes --out (profiles/nested_write.txt) and prints the same JSON line."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from simdjson_amd import build, capi, corpus, writer  # noqa: E402
import nested_write_cases as cases  # noqa: E402
import nested_write_model as model  # noqa: E402
from lib_ab import capi_for  # noqa: E402

NAMES = ("values", "valid", "offsets", "chars", "list_offsets", "list_valid")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--long-rows", type=int, default=1 << 16)
    ap.add_argument("--doc-mib", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--variant", action="append", default=[])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nested_write.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this script measures, it does not fall back")
    build.build_sjgpu()
    doc_host, statuses = corpus.twitter_like(args.doc_mib << 20, 7)
    p = capi.DomParserImplementation(len(doc_host) + 64)
    parsers = {"product": p}
    for spec in args.variant:
        name, path = spec.split("=", 1)
        parsers[name] = capi_for(path, name).DomParserImplementation(1 << 20)
    s = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(7)

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def ragged(n, low, high, values):
        lengths = rng.integers(low, high + 1, n)
        offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
        m = int(offsets[-1])
        valid = np.frombuffer(np.packbits(np.arange((m + 63) // 64 * 64) % 11 != 0, bitorder="little").tobytes(), np.int64)
        return offsets, m, values(m), valid
    # the legs as tables of tensors (what writer.write_nested takes)
    S = capi.ResidentStream(p, doc_host)
    assert (S.code, S.docs) == (0, 1), (S.code, S.docs)
    fields_a = [(b"/id", capi.GET_UINT64, b"id"), (b"$.user.entities.hashtags[*].indices[*]", capi.GET_INT64, b"indices"), (b"$.coordinates[*]", capi.GET_DOUBLE, b"coordinates"),
                (b"$.metadata.*", capi.GET_STRING, b"metadata")]
    table_a, rows_a, keep = writer._row_fields(p, S, b"$.statuses[*]", fields_a)
    assert rows_a == statuses, (rows_a, statuses)
    o, m, v, valid = ragged(args.rows, 0, 8, lambda m: rng.integers(-(1 << 62), 1 << 62, m))
    table_b = [{"key": b"v", "kind": capi.COL_INT64, "values": dev(v), "valid": dev(valid), "list_offsets": dev(o), "elements": m}]
    o, m, v, valid = ragged(args.long_rows, 56, 72, lambda m: (rng.standard_normal(m) * 10.0 ** rng.integers(-8, 9, m)).view(np.int64))
    table_c = [{"key": b"d", "kind": capi.COL_DOUBLE, "values": dev(v), "valid": dev(valid), "list_offsets": dev(o), "elements": m}]
    o, m, v, valid = ragged(args.long_rows, 12, 20, lambda m: (rng.standard_normal(m) * 10.0 ** rng.integers(-8, 9, m)).view(np.int64))
    table_d = [{"key": b"d", "kind": capi.COL_DOUBLE, "values": dev(v), "valid": dev(valid), "list_offsets": dev(o), "elements": m}]
    tables = {"a": (table_a, rows_a), "b": (table_b, args.rows), "c": (table_c, args.long_rows), "d": (table_d, args.long_rows)}
    torch.cuda.synchronize()

    def host_arrays(table, n):
        """the table as tests/nested_write_model.py takes it"""
        out = []
        for f in table:
            a = {"key": f["key"], "kind": f["kind"], "chars_bytes": int(f.get("chars_bytes", 0)), "elements": int(f.get("elements", 0))}
            for name in NAMES:
                t = f.get(name)
                a[name] = None if t is None else t.cpu().numpy().view({"values": np.uint64, "valid": np.uint64, "list_valid": np.uint64, "chars": np.uint8}.get(name, np.uint32))
            out.append(a)
        return {"n": n, "fields": out}

    class Write:
        """one table's rows at their exact capacity, through one build of the library"""

        def __init__(self, q, leg):
            table, self.n = tables[leg]
            self.q, self.fields = q, writer._field_addresses(table)
            self.offsets, self.status = torch.empty(self.n + 1, dtype=torch.int32, device="cuda"), torch.empty(self.n, dtype=torch.uint8, device="cuda")
            self.counts = torch.empty(6, dtype=torch.int64, device="cuda")
            rc, self.bytes = writer.write_nested_device(q, self.fields, self.n, capi.WRITE_NEWLINE, self.offsets.data_ptr(), self.status.data_ptr(), 0, 0, self.counts.data_ptr(), s)
            assert rc == -5 and self.bytes > 0, (rc, self.bytes)
            self.chars = torch.empty(self.bytes, dtype=torch.uint8, device="cuda")

        def __call__(self):
            rc, total = writer.write_nested_device(self.q, self.fields, self.n, capi.WRITE_NEWLINE, self.offsets.data_ptr(), self.status.data_ptr(), self.chars.data_ptr(), self.bytes,
                                                   self.counts.data_ptr(), s)
            assert (rc, total) == (0, self.bytes), (rc, total)

    legs = ("a", "b", "c", "d")
    runs = {(name, leg): Write(q, leg) for name, q in parsers.items() for leg in legs}
    for fn in runs.values():
        fn()
    torch.cuda.synchronize()
    # the outputs first: a sample of rows against the model, the variants against the product byte for byte; and which road the fill's iterations take
    roads = {}
    for leg in legs:
        e = runs[("product", leg)]
        assert not bool(e.status.any().item()), "a row was refused"
        at, chars = e.offsets.cpu().numpy().view(np.uint32), e.chars.cpu().numpy()
        arrays = host_arrays(*tables[leg])
        for r in np.random.default_rng(3).integers(0, e.n, 2000).tolist() + [0, e.n - 1]:
            code, text = model.row_text(arrays["fields"], r, capi.WRITE_NEWLINE)[:2]
            assert code == 0 and chars[int(at[r]): int(at[r + 1])].tobytes() == text, (leg, r, text)
        for name in parsers:
            assert torch.equal(runs[(name, leg)].chars, e.chars) and torch.equal(runs[(name, leg)].offsets, e.offsets), f"({leg}): {name} writes something else"
        edges = at[np.minimum(np.arange(0, (e.n + 255) // 256 * 256 + 1, 32), e.n)].astype(np.int64).reshape(-1)
        took = {}
        for i in range(0, len(edges) - 8, 8):
            g = _group(edges[i: i + 9])
            took[g] = took.get(g, 0) + 1
        roads[leg] = {str(k): v for k, v in sorted(took.items())}
    copies = {leg: (torch.empty(runs[("product", leg)].bytes, dtype=torch.uint8, device="cuda"), runs[("product", leg)].chars) for leg in legs}

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    named = {f"{leg}_{name}_ms": fn for (name, leg), fn in runs.items()}
    for leg, (dst, src) in copies.items():
        named[f"{leg}_copy_same_bytes_ms"] = (lambda dst=dst, src=src: dst.copy_(src))
    for _ in range(args.warmup):
        for fn in named.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in named}
    for _ in range(args.reps):  # alternating: what the clock and the neighbours do hits all alike
        for name, fn in named.items():
            times[name].append(timed(fn))
    out = {"rows": {leg: int(tables[leg][1]) for leg in legs}, "bytes": {leg: int(runs[("product", leg)].bytes) for leg in legs},
           "group_rows_of_the_iterations": roads, "doc_mib": round(len(doc_host) / 2 ** 20, 1), "reps": args.reps, "variants": list(parsers)}
    for name, t in times.items():
        out[name] = {"median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3)}
    med = {name: statistics.median(t) for name, t in times.items()}
    out["gb_per_s_out"] = {f"{leg}_{name}": round(runs[(name, leg)].bytes / med[f"{leg}_{name}_ms"] / 1e6, 1) for (name, leg) in runs}
    out["over_copy"] = {f"{leg}_{name}": round(med[f"{leg}_{name}_ms"] / med[f"{leg}_copy_same_bytes_ms"], 1) for (name, leg) in runs}
    del keep
    for q in parsers.values():
        q.close()
    line = json.dumps(out)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    print(line, flush=True)


def _group(e):
    """cases.group_rows over the nine edges of one iteration"""
    for size, step in ((256, 8), (128, 4), (64, 2), (32, 1)):
        if all(int(e[j + step]) - int(e[j]) <= cases.WINDOW for j in range(0, 8, step)):
            return size
    return 0


if __name__ == "__main__":
    main()
