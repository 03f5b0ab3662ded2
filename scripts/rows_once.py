"""One measurement of at_pointer rooted at cells (sjgpu_at_pointers_from_cells_device) beside the call it extends, in the manner of scripts/query_once.py.

Builds one twitter-like document of --mib MiB (simdjson_amd/csrc/corpus.c: `{"statuses": [ ... ]}`), its tapes (sjgpu_stage2_many_device, one document) and
the rows of `$.statuses[*]` (sjgpu_at_paths_wide_device, once), and the SAME records as a stream of documents -- the document's bytes between the brackets of
`statuses`, the commas between the records blanked -- with its tapes.  Then times in one process, warmed, alternating, with events on the stream, median of --reps:
  (a) sjgpu_at_pointers_from_cells_device, 8 pointers over the rows of `$.statuses[*]` of the document    the new call
  (b) sjgpu_at_pointers_device, the same 8 pointers over the records as a stream of documents             the yardstick
The two walk the same records with the same pointers: what (a) has more than (b) is the locate step (one lane per root: the document search -- of depth 0
here, one document -- and the comparison of the cell with its tape word) and the read of the root cells.  Both calls only enqueue their walk: the second
event is recorded behind it, so a figure is the walk's, the table check's and the call's.  Before anything is timed the two outputs are compared: tags equal,
numbers equal, strings of equal length.
Writes --out (profiles/rows.txt) and prints the same JSON line.  For k_rows_locate's share run it once more under `rocprofv3 --kernel-trace --stats` with
--reps 3 (tracing slows the host: the timings of that run are not the ones to quote)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from simdjson_amd import build, capi, corpus  # noqa: E402

POINTERS = [b"/id", b"/text", b"/user/id", b"/user/name", b"/user/followers_count", b"/retweet_count", b"/coordinates/1", b"/user/entities/hashtags/0/indices/0"]
HEADER, TRAILER = b'{\n  "statuses": [\n', b'\n  ],\n  "search_metadata": { "count": 100, "since_id": 0 }\n}\n'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "rows.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this script measures, it does not fall back")
    build.build_sjgpu()
    host, statuses = corpus.twitter_like(args.mib << 20, 7)
    raw = host.tobytes()
    assert raw.startswith(HEADER) and raw.endswith(TRAILER)
    records = np.frombuffer(raw[len(HEADER): len(raw) - len(TRAILER)].replace(b"\n    },\n", b"\n    } \n"), np.uint8)  # (no raw newline inside a string: the pattern is a record's end)
    del raw
    p = capi.DomParserImplementation(len(host) + 64)
    D = capi.ResidentStream(p, host, doc_cap=1)
    S = capi.ResidentStream(p, records, doc_cap=statuses + 1)
    assert (D.code, D.docs, S.code, S.docs) == (0, 1, 0, statuses), (D.code, D.docs, S.code, S.docs, statuses)
    s = D.stream
    K = len(POINTERS)
    # the rows of $.statuses[*]: every record's cell, in order
    offsets = torch.empty(2, dtype=torch.int32, device="cuda")
    status = torch.empty(1, dtype=torch.uint8, device="cuda")
    root_values = torch.empty(statuses, dtype=torch.int64, device="cuda")
    root_tags = torch.empty(statuses, dtype=torch.uint8, device="cuda")
    rc, rows = p.at_paths_wide_device(*D.args(), [b"$.statuses[*]"], offsets.data_ptr(), status.data_ptr(), root_values.data_ptr(), root_tags.data_ptr(), statuses, s)
    assert (rc, rows) == (0, statuses), (rc, rows)
    out_a = torch.empty((K, rows), dtype=torch.int64, device="cuda"), torch.empty((K, rows), dtype=torch.uint8, device="cuda")
    out_b = torch.empty((K, rows), dtype=torch.int64, device="cuda"), torch.empty((K, rows), dtype=torch.uint8, device="cuda")

    def run_rows():
        rc = p.at_pointers_from_cells_device(*D.args(), root_values.data_ptr(), root_tags.data_ptr(), rows, POINTERS, out_a[0].data_ptr(), out_a[1].data_ptr(), s)
        assert rc == 0, rc

    def run_stream():
        rc = p.at_pointers_device(*S.args(), POINTERS, out_b[0].data_ptr(), out_b[1].data_ptr(), s)
        assert rc == 0, rc

    run_rows()
    run_stream()
    torch.cuda.synchronize()
    ta, tb = out_a[1].cpu().numpy(), out_b[1].cpu().numpy()
    va, vb = out_a[0].cpu().numpy().view(np.uint64), out_b[0].cpu().numpy().view(np.uint64)
    assert np.array_equal(ta, tb), "the two roads disagree on a tag"
    numbers = np.isin(ta, [ord(c) for c in "ludtfn"]) | (ta < 34)
    strings = ta == ord('"')
    assert np.array_equal(va[numbers], vb[numbers]) and np.array_equal(va[strings] >> 32, vb[strings] >> 32), "the two roads disagree on a value"
    hits = [int((ta[k] >= 34).sum()) for k in range(K)]
    assert all(h == rows for h in hits[:7]) and 0 < hits[7] < rows, hits  # seven fields every record has, and one that only some have

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    runs = {"a_rows_8_ms": run_rows, "b_stream_8_ms": run_stream}
    for _ in range(args.warmup):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in runs}
    for _ in range(args.reps):  # alternating: what the clock and the neighbours do hits both alike
        for name, fn in runs.items():
            times[name].append(timed(fn))
    out = {"mib": round(len(host) / 2 ** 20, 1), "records": int(rows), "document_tape_words": int(D.tw), "stream_tape_words": int(S.tw), "pointers": K, "hits": hits,
           "reps": args.reps}
    for name, t in times.items():
        out[name] = {"median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3)}
    out["a_over_b"] = round(statistics.median(times["a_rows_8_ms"]) / statistics.median(times["b_stream_8_ms"]), 3)
    p.close()
    line = json.dumps(out)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
