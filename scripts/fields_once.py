"""One measurement of the map column (sjgpu_object_fields_from_cells_device) beside the parent's way to the values alone and beside the sizes, in the manner of
scripts/lists_once.py.

Builds one twitter-like document of --mib MiB (simdjson_amd/csrc/corpus.c: `{"statuses": [ ... ]}`), its tapes (sjgpu_stage2_many_device, one document) and the
roots `$.statuses[*].user` (sjgpu_at_paths_wide_device, once).  Then times in one process, warmed, alternating, with events on the stream, median of --reps:
  (a) sjgpu_object_fields_from_cells_device over the roots                                  the new call: keys and values, ONE walk (the count reads a word)
  (b) sjgpu_at_paths_from_cells_device, the single path `$.*`, over the same roots          the values alone, TWO walks (count, fill)
  (c) sjgpu_cell_sizes_device over the same roots                                           no walk; only enqueued, so the clock runs until its kernels end
(a) and (b) wait for the stream (the total is read back) and run at the exact capacity, found by a call with room for nothing.  Before anything is timed the
outputs are compared: offsets equal, value tags and values equal, the sizes equal to the offsets' differences.
Writes --out (profiles/fields.txt) and prints the same JSON line."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from simdjson_amd import build, capi, corpus  # noqa: E402

ROOTS = b"$.statuses[*].user"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "fields.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this script measures, it does not fall back")
    build.build_sjgpu()
    host, statuses = corpus.twitter_like(args.mib << 20, 7)
    p = capi.DomParserImplementation(len(host) + 64)
    D = capi.ResidentStream(p, host, doc_cap=1)
    assert (D.code, D.docs) == (0, 1), (D.code, D.docs)
    s = D.stream
    row_offsets = torch.empty(2, dtype=torch.int32, device="cuda")
    row_status = torch.empty(1, dtype=torch.uint8, device="cuda")
    root_values = torch.empty(statuses, dtype=torch.int64, device="cuda")
    root_tags = torch.empty(statuses, dtype=torch.uint8, device="cuda")
    rc, rows = p.at_paths_wide_device(*D.args(), [ROOTS], row_offsets.data_ptr(), row_status.data_ptr(), root_values.data_ptr(), root_tags.data_ptr(), statuses, s)
    assert rc == 0 and 0 < rows <= statuses, (rc, rows)
    roots = (root_values.data_ptr(), root_tags.data_ptr(), rows)
    offsets_a, status_a = torch.empty(rows + 1, dtype=torch.int32, device="cuda"), torch.empty(rows, dtype=torch.uint8, device="cuda")
    offsets_b, status_b = torch.empty(rows + 1, dtype=torch.int32, device="cuda"), torch.empty(rows, dtype=torch.uint8, device="cuda")
    sizes, codes = torch.empty(rows, dtype=torch.int32, device="cuda"), torch.empty(rows, dtype=torch.uint8, device="cuda")
    # the exact capacity: a call with room for nothing says what is needed
    rc, fields = p.object_fields_from_cells_device(*D.args(), *roots, offsets_a.data_ptr(), status_a.data_ptr(), 0, 0, 0, 0, 0, s)
    assert rc == -5 and fields > rows, (rc, fields)
    key_values, values_a, values_b = (torch.empty(fields, dtype=torch.int64, device="cuda") for _ in range(3))
    key_tags, tags_a, tags_b = (torch.empty(fields, dtype=torch.uint8, device="cuda") for _ in range(3))

    def run_fields():
        rc, n = p.object_fields_from_cells_device(*D.args(), *roots, offsets_a.data_ptr(), status_a.data_ptr(), key_values.data_ptr(), key_tags.data_ptr(), values_a.data_ptr(),
                                                  tags_a.data_ptr(), fields, s)
        assert (rc, n) == (0, fields), (rc, n)

    def run_values():
        rc, n = p.at_paths_from_cells_device(*D.args(), *roots, [b"$.*"], offsets_b.data_ptr(), status_b.data_ptr(), values_b.data_ptr(), tags_b.data_ptr(), fields, s)
        assert (rc, n) == (0, fields), (rc, n)

    def run_sizes():
        rc = p.cell_sizes_device(D.tape.data_ptr(), D.tw, D.table.data_ptr(), D.docs, *roots, sizes.data_ptr(), codes.data_ptr(), s)
        assert rc == 0, rc

    run_fields()
    run_values()
    run_sizes()
    torch.cuda.synchronize()
    oa = offsets_a.cpu().numpy().view(np.uint32)
    assert np.array_equal(oa, offsets_b.cpu().numpy().view(np.uint32)), "the two roads disagree on an offset"
    assert not status_a.cpu().numpy().any() and not status_b.cpu().numpy().any() and not codes.cpu().numpy().any(), "a root that is no object"
    assert np.array_equal(tags_a.cpu().numpy(), tags_b.cpu().numpy()) and np.array_equal(values_a.cpu().numpy(), values_b.cpu().numpy()), "the two roads disagree on a value"
    assert (key_tags.cpu().numpy() == ord('"')).all() and np.array_equal(sizes.cpu().numpy().view(np.uint32), np.diff(oa)), "keys or sizes"

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    runs = {"a_fields_ms": run_fields, "b_values_by_path_ms": run_values, "c_sizes_ms": run_sizes}
    for _ in range(args.warmup):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in runs}
    for _ in range(args.reps):  # alternating: what the clock and the neighbours do hits all alike
        for name, fn in runs.items():
            times[name].append(timed(fn))
    out = {"mib": round(len(host) / 2 ** 20, 1), "roots": int(rows), "document_tape_words": int(D.tw), "fields": int(fields), "reps": args.reps}
    for name, t in times.items():
        out[name] = {"median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3)}
    out["a_over_b"] = round(statistics.median(times["a_fields_ms"]) / statistics.median(times["b_values_by_path_ms"]), 3)
    p.close()
    line = json.dumps(out)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
