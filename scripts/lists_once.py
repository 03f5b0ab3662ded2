"""One measurement of at_path_with_wildcard rooted at cells (sjgpu_at_paths_from_cells_device) beside the call it extends, in the manner of scripts/rows_once.py.

Builds one twitter-like document of --mib MiB (simdjson_amd/csrc/corpus.c: `{"statuses": [ ... ]}`), its tapes (sjgpu_stage2_many_device, one document) and
the rows of `$.statuses[*]` (sjgpu_at_paths_wide_device, once), and the SAME records as a stream of documents -- the document's bytes between the brackets of
`statuses`, the commas between the records blanked -- with its tapes.  Then times in one process, warmed, alternating, with events on the stream, median of --reps:
  (a) sjgpu_at_paths_from_cells_device, 4 paths over the rows of `$.statuses[*]` of the document    the new call
  (b) sjgpu_at_paths_device, the same 4 paths over the records as a stream of documents             the yardstick
The paths: two lists, one list of lists, one without a wildcard.  The two calls do the same walks over the same records, twice each (count, fill), with the same
scan between them; what (a) has more than (b) is the locate step (one lane per root) and the read of the root cells and their verdicts.  Both calls wait for the
stream (the total is read back) and run at the exact capacity, found by a call with room for nothing.  Before anything is timed the two outputs are compared:
statuses and offsets equal, tags equal, numbers equal.
Writes --out (profiles/lists.txt) and prints the same JSON line.  For the kernels' shares run it once more under `rocprofv3 --kernel-trace --stats` with
--reps 3 (tracing slows the host: the timings of that run are not the ones to quote)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from simdjson_amd import build, capi, corpus  # noqa: E402

PATHS = [b"$.coordinates[*]", b"$.user.entities.hashtags[*]", b"$.user.entities.hashtags[*].indices[*]", b"$.user.id"]
HEADER, TRAILER = b'{\n  "statuses": [\n', b'\n  ],\n  "search_metadata": { "count": 100, "since_id": 0 }\n}\n'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "lists.txt"))
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
    K = len(PATHS)
    # the rows of $.statuses[*]: every record's cell, in order
    offsets = torch.empty(2, dtype=torch.int32, device="cuda")
    status = torch.empty(1, dtype=torch.uint8, device="cuda")
    root_values = torch.empty(statuses, dtype=torch.int64, device="cuda")
    root_tags = torch.empty(statuses, dtype=torch.uint8, device="cuda")
    rc, rows = p.at_paths_wide_device(*D.args(), [b"$.statuses[*]"], offsets.data_ptr(), status.data_ptr(), root_values.data_ptr(), root_tags.data_ptr(), statuses, s)
    assert (rc, rows) == (0, statuses), (rc, rows)
    cells = K * rows
    out_a = [torch.empty(cells + 1, dtype=torch.int32, device="cuda"), torch.empty(cells, dtype=torch.uint8, device="cuda"), None, None]
    out_b = [torch.empty(cells + 1, dtype=torch.int32, device="cuda"), torch.empty(cells, dtype=torch.uint8, device="cuda"), None, None]
    # the exact capacity: a call with room for nothing says what is needed
    rc, matches = p.at_paths_from_cells_device(*D.args(), root_values.data_ptr(), root_tags.data_ptr(), rows, PATHS, out_a[0].data_ptr(), out_a[1].data_ptr(), 0, 0, 0, s)
    assert rc == -5 and matches > rows, (rc, matches)
    for out in (out_a, out_b):
        out[2], out[3] = torch.empty(matches, dtype=torch.int64, device="cuda"), torch.empty(matches, dtype=torch.uint8, device="cuda")

    def run_lists():
        rc, m = p.at_paths_from_cells_device(*D.args(), root_values.data_ptr(), root_tags.data_ptr(), rows, PATHS, out_a[0].data_ptr(), out_a[1].data_ptr(), out_a[2].data_ptr(),
                                             out_a[3].data_ptr(), matches, s)
        assert (rc, m) == (0, matches), (rc, m)

    def run_stream():
        rc, m = p.at_paths_device(*S.args(), PATHS, out_b[0].data_ptr(), out_b[1].data_ptr(), out_b[2].data_ptr(), out_b[3].data_ptr(), matches, s)
        assert (rc, m) == (0, matches), (rc, m)

    run_lists()
    run_stream()
    torch.cuda.synchronize()
    assert np.array_equal(out_a[0].cpu().numpy(), out_b[0].cpu().numpy()), "the two roads disagree on an offset"
    assert np.array_equal(out_a[1].cpu().numpy(), out_b[1].cpu().numpy()), "the two roads disagree on a status"
    ta, tb = out_a[3].cpu().numpy(), out_b[3].cpu().numpy()
    va, vb = out_a[2].cpu().numpy().view(np.uint64), out_b[2].cpu().numpy().view(np.uint64)
    assert np.array_equal(ta, tb), "the two roads disagree on a tag"
    numbers = np.isin(ta, [ord(c) for c in "ludtfn"])
    assert np.array_equal(va[numbers], vb[numbers]), "the two roads disagree on a value"
    per_path = np.diff(out_a[0].cpu().numpy().view(np.uint32)[:: rows].astype(np.int64)).tolist()
    assert per_path[0] == 2 * rows and per_path[2] == 2 * per_path[1] > 0 and per_path[3] == rows, per_path

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    runs = {"a_lists_4_ms": run_lists, "b_stream_4_ms": run_stream}
    for _ in range(args.warmup):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in runs}
    for _ in range(args.reps):  # alternating: what the clock and the neighbours do hits both alike
        for name, fn in runs.items():
            times[name].append(timed(fn))
    out = {"mib": round(len(host) / 2 ** 20, 1), "records": int(rows), "document_tape_words": int(D.tw), "stream_tape_words": int(S.tw), "paths": K, "matches": per_path,
           "reps": args.reps}
    for name, t in times.items():
        out[name] = {"median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3)}
    out["a_over_b"] = round(statistics.median(times["a_lists_4_ms"]) / statistics.median(times["b_stream_4_ms"]), 3)
    p.close()
    line = json.dumps(out)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
