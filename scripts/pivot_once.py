"""One measurement of sjgpu_pivot_fields_device beside the only road the library had to the same table, in the manner of scripts/dictionary_once.py and on its
inputs.

Builds one twitter-like document of --mib MiB (simdjson_amd/csrc/corpus.c: `{"statuses": [ ... ]}`), its tapes (sjgpu_stage2_many_device, one document) and, for
each of two sets of records -- `$.statuses[*].user` (flat records of scalars) and `$.statuses[*]` (records with nested values) --, the rows
(sjgpu_at_paths_wide_device), their fields (sjgpu_object_fields_from_cells_device) and the dictionary of the keys (sjgpu_dictionary_encode_device): what BOTH
roads need, timed on their own.  Then, for the table of all G learned keys:
  pivot     ONE sjgpu_pivot_fields_device call, identity map
  fill      the same call with fields = 0: the fill as it is, and a scatter whose lanes leave behind their offsets
  scatter   pivot - fill (the call enqueues both kernels; no event can be put between them from outside)
  pivot_map the call with a map (the identity, as device memory): what the map's extra load costs
  pointers  sjgpu_at_pointers_from_cells_device for `/` + each key, in chunks of 64: G walks over every object
Everything is timed in one process, warmed, alternating, with events on the stream, median of --reps.  Before anything is timed the two tables are compared
cell for cell.  The bytes: the pivot's are counted from its contract (9 per cell filled, 13 per slot read, 5 per row, 9 per slot stored); the pointers' are an
estimate from below -- per key and row the key words, value words and string lengths (20 bytes a field) up to the first match, or of all fields where there
is none -- which leaves out the key bytes compared and everything the call reads to find its roots.
Writes --out (profiles/pivot.txt) and prints the same JSON lines."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from simdjson_amd import build, capi, corpus, dictionary, pivot  # noqa: E402

ROW_PATHS = {"users": b"$.statuses[*].user", "statuses": b"$.statuses[*]"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "pivot.txt"))
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
    sbuf = (D.sbuf.data_ptr(), D.sb)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    for name, row_path in ROW_PATHS.items():
        offsets1, status1 = torch.empty(2, dtype=torch.int32, device="cuda"), torch.empty(1, dtype=torch.uint8, device="cuda")
        root_values, root_tags = torch.empty(statuses, dtype=torch.int64, device="cuda"), torch.empty(statuses, dtype=torch.uint8, device="cuda")
        rc, rows = p.at_paths_wide_device(*D.args(), [row_path], offsets1.data_ptr(), status1.data_ptr(), root_values.data_ptr(), root_tags.data_ptr(), statuses, s)
        assert rc == 0 and 0 < rows <= statuses, (row_path, rc, rows)
        roots = (root_values.data_ptr(), root_tags.data_ptr(), rows)
        f_offsets, f_status = torch.empty(rows + 1, dtype=torch.int32, device="cuda"), torch.empty(rows, dtype=torch.uint8, device="cuda")
        rc, fields = p.object_fields_from_cells_device(*D.args(), *roots, f_offsets.data_ptr(), f_status.data_ptr(), 0, 0, 0, 0, 0, s)
        assert rc == -5 and fields > rows, (rc, fields)
        key_values, values = (torch.empty(fields, dtype=torch.int64, device="cuda") for _ in range(2))
        key_tags, tags = (torch.empty(fields, dtype=torch.uint8, device="cuda") for _ in range(2))

        def run_fields():
            rc, n = p.object_fields_from_cells_device(*D.args(), *roots, f_offsets.data_ptr(), f_status.data_ptr(), key_values.data_ptr(), key_tags.data_ptr(), values.data_ptr(),
                                                      tags.data_ptr(), fields, s)
            assert (rc, n) == (0, fields), (rc, n)

        run_fields()
        codes = torch.empty(fields, dtype=torch.int32, device="cuda")
        rc, G = dictionary.dictionary_encode_device(p, *sbuf, key_values.data_ptr(), key_tags.data_ptr(), fields, codes.data_ptr(), 0, 0, 0, 0, 0, s)
        assert rc == -5 and G > 0, (rc, G)
        dict_values, dict_tags = torch.empty(G, dtype=torch.int64, device="cuda"), torch.empty(G, dtype=torch.uint8, device="cuda")
        first, counts = (torch.empty(G, dtype=torch.int32, device="cuda") for _ in range(2))

        def run_encode():
            rc, distinct = dictionary.dictionary_encode_device(p, *sbuf, key_values.data_ptr(), key_tags.data_ptr(), fields, codes.data_ptr(), dict_values.data_ptr(),
                                                               dict_tags.data_ptr(), first.data_ptr(), counts.data_ptr(), G, s)
            assert (rc, distinct) == (0, G), (rc, distinct)

        run_encode()
        d_at = torch.empty(G + 1, dtype=torch.int32, device="cuda")
        d_chars = torch.empty(64 * G, dtype=torch.uint8, device="cuda")
        rc, d_bytes = p.gather_strings_device(*sbuf, dict_values.data_ptr(), dict_tags.data_ptr(), G, d_at.data_ptr(), d_chars.data_ptr(), 64 * G, s)
        assert rc == 0, rc
        at, chars = d_at.cpu().numpy().tolist(), d_chars.cpu().numpy().tobytes()
        keys = [chars[at[j]: at[j + 1]] for j in range(G)]
        pointers = [b"/" + k.replace(b"~", b"~0").replace(b"/", b"~1") for k in keys]
        table_values, walk_values = (torch.empty((G, rows), dtype=torch.int64, device="cuda") for _ in range(2))
        table_tags, walk_tags = (torch.empty((G, rows), dtype=torch.uint8, device="cuda") for _ in range(2))
        identity = torch.arange(G, dtype=torch.int32, device="cuda")

        def run_pivot(n=fields, column_map=0):
            rc = pivot.pivot_fields_device(p, f_offsets.data_ptr(), f_status.data_ptr(), rows, codes.data_ptr(), values.data_ptr(), tags.data_ptr(), n, column_map, G, G,
                                           table_values.data_ptr(), table_tags.data_ptr(), s)
            assert rc == 0, rc

        def run_pointers():
            for k0 in range(0, G, 64):
                rc = p.at_pointers_from_cells_device(*D.args(), *roots, pointers[k0: k0 + 64], walk_values[k0].data_ptr(), walk_tags[k0].data_ptr(), s)
                assert rc == 0, rc

        run_pointers()
        for column_map in (identity.data_ptr(), 0):
            table_values.fill_(-1)
            table_tags.fill_(0x5A)
            run_pivot(column_map=column_map)
            torch.cuda.synchronize()
            assert torch.equal(table_values, walk_values) and torch.equal(table_tags, walk_tags), "the pivoted table is not the pointers' table"
        runs = {"fields_ms": run_fields, "encode_ms": run_encode, "pivot_ms": run_pivot, "fill_ms": lambda: run_pivot(n=0), "pivot_map_ms": lambda: run_pivot(column_map=identity.data_ptr()),
                "pointers_ms": run_pointers}
        for _ in range(args.warmup):
            for fn in runs.values():
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in runs}
        for _ in range(args.reps):  # alternating: what the clock and the neighbours do hits all alike
            for k, fn in runs.items():
                times[k].append(timed(fn))
        # the bytes: from the contract for the pivot, from below for the pointers
        h_codes, h_offsets = codes.cpu().numpy().astype(np.int64), f_offsets.cpu().numpy().view(np.uint32).astype(np.int64)
        per_row = np.diff(h_offsets)
        row_of = np.repeat(np.arange(rows, dtype=np.int64), per_row)
        position = np.arange(fields, dtype=np.int64) - h_offsets[row_of]
        _, first_slot = np.unique(row_of * G + h_codes, return_index=True)  # the first slot of every (row, key) there is
        found_steps = int((position[first_slot] + 1).sum())
        present = np.bincount(row_of[first_slot], minlength=rows)
        absent_steps = int((per_row * (G - present)).sum())
        stored = int(len(first_slot))  # (every code has a column: every slot is stored, the duplicates too)
        out = {"records": name, "mib": round(len(host) / 2 ** 20, 1), "rows": int(rows), "fields": int(fields), "fields_per_row": round(fields / rows, 2), "G": int(G),
               "cells": int(G * rows), "reps": args.reps, "scatter_shape": "a: one lane per row, slots from last to first (the only one built)"}
        for k, t in times.items():
            out[k] = {"median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3)}
        med = {k: statistics.median(t) for k, t in times.items()}
        out["scatter_ms_pivot_minus_fill"] = round(med["pivot_ms"] - med["fill_ms"], 3)
        out["pivot_bytes"] = {"fill_written": 9 * G * rows, "scatter_read": 13 * fields + 5 * rows, "scatter_written": 9 * fields, "cells_that_keep_a_field": stored}
        out["pointers_bytes_at_least"] = {"walked": 20 * (found_steps + absent_steps), "written": 9 * G * rows, "walk_steps": found_steps + absent_steps}
        out["pointers_over_pivot"] = round(med["pointers_ms"] / med["pivot_ms"], 2)
        out["pivot_GBps"] = round((9 * G * rows + 13 * fields + 5 * rows + 9 * fields) / med["pivot_ms"] / 1e6, 1)
        line = json.dumps(out)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        print(line, flush=True)
    p.close()


if __name__ == "__main__":
    main()
