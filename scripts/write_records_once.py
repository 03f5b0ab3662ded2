"""One measurement of the record writer (sjgpu_write_records_device) beside the movers it should be compared with, in the manner of scripts/json_text_once.py.

Legs:
  (a) --rows rows x 4 columns: an int64, a double, a bool and a short string (SJGPU_COL_STRING), every seventh cell invalid
  (b) the write step of writer.project_many over an amazon-like NDJSON stream of --nd-mib MiB: asin and price as string cells, rating as a double, the review count
      as an int64 -- the columns as sjgpu_at_pointers_device and sjgpu_cast_cells_device left them, only the writer timed
  (c) --rows rows of one double column
Yardsticks, none of them the code under test: per leg a device-to-device copy of the same number of output bytes, timed in the same process (the mover the staged fill
tries to approach); for (c), sjgpu_serialize_cells_device over the same doubles as scalar cells (leg (d) of profiles/json_text.txt), in the same process.
--variant NAME=PATH adds the same legs through another build of the library (build/ab/, e.g. one compiled with -DSJGPU_WRITE_DIRECT_ONLY:
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -pthread -DSJGPU_WRITE_DIRECT_ONLY -I include -I simdjson_amd/csrc <build.SJGPU_SOURCES> -o build/ab/libsjgpu_write_direct.so -ldl),
loaded under its own copy of simdjson_amd.capi as scripts/lib_ab.py loads its variants; its output is compared byte for byte with the product's.
Everything is timed in one process, warmed, alternating, with events on the stream, median of --reps with min and max; the call waits for the stream (the total is read
back) and runs at the exact capacity, found by a call with room for nothing.  Before anything is timed the outputs are compared with tests/write_records_model.py: a
sample of rows of every leg, row by row.
Writes --out (profiles/write_records.txt) and prints the same JSON line."""
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
from simdjson_amd import build, capi, corpus, json_text, writer  # noqa: E402
import write_records_model as model  # noqa: E402
from lib_ab import capi_for  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--nd-mib", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--variant", action="append", default=[])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "write_records.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this script measures, it does not fall back")
    build.build_sjgpu()
    n = args.rows
    nd_host, lines = corpus.amazon_ndjson(args.nd_mib << 20, 7)
    p = capi.DomParserImplementation(len(nd_host) + 64)
    parsers = {"product": p}
    for spec in args.variant:
        name, path = spec.split("=", 1)
        parsers[name] = capi_for(path, name).DomParserImplementation(1 << 20)
    s = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(7)
    W = (n + 63) // 64

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ints = rng.integers(-(1 << 62), 1 << 62, n)
    doubles = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 9, n)
    bools = rng.integers(0, 2, n)
    lengths = rng.integers(4, 17, n)
    s_offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    s_chars = rng.integers(0x61, 0x7B, int(s_offsets[-1])).astype(np.uint8)
    valid = np.frombuffer(np.packbits(np.arange(W * 64) % 7 != 0, bitorder="little").tobytes(), np.int64)
    hosts = {"a": {"n": n, "columns": [
        {"key": b"id", "kind": capi.COL_INT64, "values": ints.view(np.uint64), "valid": valid.view(np.uint64), "offsets": None, "chars": None, "chars_bytes": 0},
        {"key": b"score", "kind": capi.COL_DOUBLE, "values": doubles.view(np.uint64), "valid": np.roll(valid, 1).view(np.uint64), "offsets": None, "chars": None, "chars_bytes": 0},
        {"key": b"ok", "kind": capi.COL_BOOL, "values": bools.astype(np.uint64), "valid": None, "offsets": None, "chars": None, "chars_bytes": 0},
        {"key": b"name", "kind": capi.COL_STRING, "values": None, "valid": None, "offsets": s_offsets.view(np.uint32), "chars": s_chars, "chars_bytes": len(s_chars)}]}}
    hosts["c"] = {"n": n, "columns": [dict(hosts["a"]["columns"][1], valid=None)]}
    # (b): the columns project_many hands to the writer
    N = capi.ResidentStream(p, nd_host, doc_cap=lines)
    assert (N.code, N.docs) == (0, lines), (N.code, N.docs)
    fields = [(b"/0", capi.GET_STRING, b"asin"), (b"/5", capi.GET_DOUBLE, b"rating"), (b"/7", capi.GET_INT64, b"reviews"), (b"/8", capi.GET_STRING, b"price")]
    K, Wb = len(fields), (lines + 63) // 64
    values, tags = torch.empty((K, lines), dtype=torch.int64, device="cuda"), torch.empty((K, lines), dtype=torch.uint8, device="cuda")
    assert p.at_pointers_device(*N.args(), [f[0] for f in fields], values.data_ptr(), tags.data_ptr(), s) == 0
    cast, codes = torch.empty((K, lines), dtype=torch.int64, device="cuda"), torch.empty((K, lines), dtype=torch.uint8, device="cuda")
    b_valid, cast_counts = torch.empty((K, Wb), dtype=torch.int64, device="cuda"), torch.empty((K, 4), dtype=torch.int32, device="cuda")
    assert p.cast_cells_device(values.data_ptr(), tags.data_ptr(), lines, [f[1] for f in fields], cast.data_ptr(), codes.data_ptr(), b_valid.data_ptr(), cast_counts.data_ptr(), s) == 0
    torch.cuda.synchronize()
    sbuf_host = N.sbuf[: N.sb].cpu().numpy()
    hosts["b"] = {"n": lines, "columns": [
        {"key": f[2], "kind": capi.COL_STRING_CELLS if f[1] == capi.GET_STRING else f[1], "values": cast[k].cpu().numpy().view(np.uint64),
         "valid": b_valid[k].cpu().numpy().view(np.uint64), "offsets": None, "chars": sbuf_host if f[1] == capi.GET_STRING else None,
         "chars_bytes": N.sb if f[1] == capi.GET_STRING else 0} for k, f in enumerate(fields)]}

    keep = []

    def table_of(h, leg):
        cols = []
        for k, c in enumerate(h["columns"]):
            d = {"key": c["key"], "kind": c["kind"], "chars_bytes": c["chars_bytes"]}
            for name in ("values", "valid", "offsets"):
                if c[name] is not None:
                    t = cast[k] if (leg == "b" and name == "values") else b_valid[k] if (leg == "b" and name == "valid") else dev(c[name].view(np.int64 if name != "offsets" else np.int32))
                    keep.append(t)
                    d[name] = t.data_ptr()
            if c["chars"] is not None:
                t = N.sbuf if leg == "b" else dev(c["chars"])
                keep.append(t)
                d["chars"] = t.data_ptr()
            cols.append(d)
        return cols
    tables = {leg: table_of(h, leg) for leg, h in hosts.items()}

    class Write:
        """one table's records at their exact capacity, through one build of the library"""

        def __init__(self, q, leg):
            self.q, self.cols, self.n = q, tables[leg], hosts[leg]["n"]
            self.offsets, self.status = torch.empty(self.n + 1, dtype=torch.int32, device="cuda"), torch.empty(self.n, dtype=torch.uint8, device="cuda")
            self.counts = torch.empty(4, dtype=torch.int64, device="cuda")
            rc, self.bytes = writer.write_records_device(q, self.cols, self.n, capi.WRITE_NEWLINE, self.offsets.data_ptr(), self.status.data_ptr(), 0, 0, self.counts.data_ptr(), s)
            assert rc == -5 and self.bytes > 0, (rc, self.bytes)
            self.chars = torch.empty(self.bytes, dtype=torch.uint8, device="cuda")

        def __call__(self):
            rc, total = writer.write_records_device(self.q, self.cols, self.n, capi.WRITE_NEWLINE, self.offsets.data_ptr(), self.status.data_ptr(), self.chars.data_ptr(), self.bytes,
                                                    self.counts.data_ptr(), s)
            assert (rc, total) == (0, self.bytes), (rc, total)

    runs = {(name, leg): Write(q, leg) for name, q in parsers.items() for leg in ("a", "b", "c")}
    for fn in runs.values():
        fn()
    torch.cuda.synchronize()
    # the outputs first: a sample of rows against the model, the variants against the product byte for byte
    for leg in ("a", "b", "c"):
        e = runs[("product", leg)]
        assert not bool(e.status.any().item()), "a row was refused"
        at, chars = e.offsets.cpu().numpy().view(np.uint32), e.chars.cpu().numpy()
        for r in np.random.default_rng(3).integers(0, e.n, 3000).tolist() + [0, e.n - 1]:
            code, text, _, _ = model.row_text(hosts[leg]["columns"], r, capi.WRITE_NEWLINE)
            assert code == 0 and chars[int(at[r]): int(at[r + 1])].tobytes() == text, (leg, r, text)
        for name in parsers:
            assert torch.equal(runs[(name, leg)].chars, e.chars) and torch.equal(runs[(name, leg)].offsets, e.offsets), f"({leg}): {name} writes something else"
    # the yardsticks
    copies = {leg: (torch.empty(runs[("product", leg)].bytes, dtype=torch.uint8, device="cuda"), runs[("product", leg)].chars) for leg in ("a", "b", "c")}
    d_tags = torch.full((n,), ord("d"), dtype=torch.uint8, device="cuda")
    d_values = dev(doubles.view(np.int64))
    dummy_tape, dummy_table = torch.zeros(8, dtype=torch.int64, device="cuda"), torch.zeros(8, dtype=torch.int32, device="cuda")
    ser_offsets, ser_status = torch.empty(n + 1, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    ser_args = (dummy_tape.data_ptr(), 0, dummy_tape.data_ptr(), 0, dummy_table.data_ptr(), 0, d_values.data_ptr(), d_tags.data_ptr(), n, ser_offsets.data_ptr(), ser_status.data_ptr())
    rc, ser_bytes = json_text.serialize_cells_device(p, *ser_args, 0, 0, s)
    assert rc == -5 and ser_bytes > 0, (rc, ser_bytes)
    ser_chars = torch.empty(ser_bytes, dtype=torch.uint8, device="cuda")

    def run_serialize():
        rc, total = json_text.serialize_cells_device(p, *ser_args, ser_chars.data_ptr(), ser_bytes, s)
        assert (rc, total) == (0, ser_bytes), (rc, total)

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
    named["c_serialize_cells_ms"] = run_serialize
    for _ in range(args.warmup):
        for fn in named.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in named}
    for _ in range(args.reps):  # alternating: what the clock and the neighbours do hits all alike
        for name, fn in named.items():
            times[name].append(timed(fn))
    out = {"rows": {leg: int(hosts[leg]["n"]) for leg in ("a", "b", "c")}, "bytes": {leg: int(runs[("product", leg)].bytes) for leg in ("a", "b", "c")},
           "serialize_cells_bytes": int(ser_bytes), "nd_mib": round(len(nd_host) / 2 ** 20, 1), "reps": args.reps, "variants": list(parsers)}
    for name, t in times.items():
        out[name] = {"median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3)}
    med = {name: statistics.median(t) for name, t in times.items()}
    out["gb_per_s_out"] = {f"{leg}_{name}": round(runs[(name, leg)].bytes / med[f"{leg}_{name}_ms"] / 1e6, 1) for (name, leg) in runs}
    out["over_copy"] = {f"{leg}_{name}": round(med[f"{leg}_{name}_ms"] / med[f"{leg}_copy_same_bytes_ms"], 1) for (name, leg) in runs}
    for q in parsers.values():
        q.close()
    line = json.dumps(out)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
