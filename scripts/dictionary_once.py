"""One measurement of the dictionary calls (sjgpu_dictionary_encode_device, sjgpu_cell_kinds_by_code_device) beside what a user did without them, in the manner of
scripts/fields_once.py.

Builds one twitter-like document of --mib MiB (simdjson_amd/csrc/corpus.c: `{"statuses": [ ... ]}`), its tapes (sjgpu_stage2_many_device, one document), the rows
of three paths (sjgpu_at_paths_wide_device) and the key and value rows of the users' fields (sjgpu_object_fields_from_cells_device).  The synthetic document has
neither `lang` nor `screen_name`; the three columns are chosen for what they stand for, and their distinct counts are reported:
  (a) the encode of `$.statuses[*].metadata.iso_language_code`      a categorical column: few distinct values
  (b) the encode of the key row of `$.statuses[*].user`             the keys of every user: millions of cells, a handful of distinct keys
  (c) the encode of `$.statuses[*].user.name`                       nearly all distinct, long strings
  (c2) the encode of `$.statuses[*].created_at`                     short strings, as distinct as the generator makes them
  (d) the census by code over (b)'s value row
  (e) what gives (b)'s answer without the call: sjgpu_gather_strings_device over the key row, the offsets and characters copied to the host, a Python dict
      (wall clock, --host-reps runs: it is host work)
Everything else is timed in one process, warmed, alternating, with events on the stream, median of --reps; the encodes wait for the stream (the total is read
back) and run at the exact capacity, found by a call with room for nothing.  Before anything is timed the outputs are compared: (b)'s dictionary and counts with
(e)'s dict, every code with the string it stands for on a sample, (d) with the sums of a census of the whole value row.
Writes --out (profiles/dictionary.txt) and prints the same JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from simdjson_amd import build, capi, corpus, dictionary  # noqa: E402

COLUMNS = {"a": b"$.statuses[*].metadata.iso_language_code", "c": b"$.statuses[*].user.name", "c2": b"$.statuses[*].created_at"}
USERS = b"$.statuses[*].user"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "dictionary.txt"))
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

    def rows_of(path):
        offsets, status = torch.empty(2, dtype=torch.int32, device="cuda"), torch.empty(1, dtype=torch.uint8, device="cuda")
        values, tags = torch.empty(statuses, dtype=torch.int64, device="cuda"), torch.empty(statuses, dtype=torch.uint8, device="cuda")
        rc, rows = p.at_paths_wide_device(*D.args(), [path], offsets.data_ptr(), status.data_ptr(), values.data_ptr(), tags.data_ptr(), statuses, s)
        assert rc == 0 and 0 < rows <= statuses, (path, rc, rows)
        return values, tags, rows

    rows = {name: rows_of(path) for name, path in COLUMNS.items()}
    root_values, root_tags, users = rows_of(USERS)
    roots = (root_values.data_ptr(), root_tags.data_ptr(), users)
    f_offsets, f_status = torch.empty(users + 1, dtype=torch.int32, device="cuda"), torch.empty(users, dtype=torch.uint8, device="cuda")
    rc, fields = p.object_fields_from_cells_device(*D.args(), *roots, f_offsets.data_ptr(), f_status.data_ptr(), 0, 0, 0, 0, 0, s)
    assert rc == -5 and fields > users, (rc, fields)
    key_values, values = (torch.empty(fields, dtype=torch.int64, device="cuda") for _ in range(2))
    key_tags, tags = (torch.empty(fields, dtype=torch.uint8, device="cuda") for _ in range(2))
    rc, n = p.object_fields_from_cells_device(*D.args(), *roots, f_offsets.data_ptr(), f_status.data_ptr(), key_values.data_ptr(), key_tags.data_ptr(), values.data_ptr(),
                                              tags.data_ptr(), fields, s)
    assert (rc, n) == (0, fields), (rc, n)
    rows["b"] = (key_values, key_tags, fields)

    class Encode:
        """one row's encode at its exact capacity"""

        def __init__(self, row):
            self.values, self.tags, self.n = row
            self.codes = torch.empty(self.n, dtype=torch.int32, device="cuda")
            rc, self.distinct = dictionary.dictionary_encode_device(p, *sbuf, self.values.data_ptr(), self.tags.data_ptr(), self.n, self.codes.data_ptr(), 0, 0, 0, 0, 0, s)
            assert rc in (0, -5), rc
            cap = max(self.distinct, 1)
            self.dict_values, self.dict_tags = torch.empty(cap, dtype=torch.int64, device="cuda"), torch.empty(cap, dtype=torch.uint8, device="cuda")
            self.first, self.counts = (torch.empty(cap, dtype=torch.int32, device="cuda") for _ in range(2))

        def __call__(self):
            rc, distinct = dictionary.dictionary_encode_device(p, *sbuf, self.values.data_ptr(), self.tags.data_ptr(), self.n, self.codes.data_ptr(), self.dict_values.data_ptr(),
                                                               self.dict_tags.data_ptr(), self.first.data_ptr(), self.counts.data_ptr(), self.distinct, s)
            assert (rc, distinct) == (0, self.distinct), (rc, distinct)

    encodes = {name: Encode(rows[name]) for name in ("a", "b", "c", "c2")}
    B = encodes["b"]
    kinds = torch.empty(max(B.distinct, 1) * 16, dtype=torch.int32, device="cuda")

    def run_census():
        rc = dictionary.kinds_by_code_device(p, B.codes.data_ptr(), values.data_ptr(), tags.data_ptr(), fields, B.distinct, kinds.data_ptr(), s)
        assert rc == 0, rc

    key_offsets = torch.empty(fields + 1, dtype=torch.int32, device="cuda")
    rc, key_bytes = p.gather_strings_device(*sbuf, key_values.data_ptr(), key_tags.data_ptr(), fields, key_offsets.data_ptr(), 0, 0, s)
    assert rc == -5, rc
    key_chars = torch.empty(key_bytes, dtype=torch.uint8, device="cuda")

    def run_host():
        """-> {key: [first, count]} in order of first appearance, the parent's way"""
        rc, total = p.gather_strings_device(*sbuf, key_values.data_ptr(), key_tags.data_ptr(), fields, key_offsets.data_ptr(), key_chars.data_ptr(), key_bytes, s)
        assert (rc, total) == (0, key_bytes), (rc, total)
        at, chars = key_offsets.cpu().numpy().tolist(), key_chars.cpu().numpy().tobytes()
        seen = {}
        for i in range(fields):
            k = chars[at[i]: at[i + 1]]
            e = seen.get(k)
            if e is None:
                seen[k] = [i, 1]
            else:
                e[1] += 1
        return seen

    for e in encodes.values():
        e()
    run_census()
    seen = run_host()
    torch.cuda.synchronize()
    d_at = torch.empty(B.distinct + 1, dtype=torch.int32, device="cuda")
    d_chars = torch.empty(max(key_bytes, 1), dtype=torch.uint8, device="cuda")
    rc, d_bytes = p.gather_strings_device(*sbuf, B.dict_values.data_ptr(), B.dict_tags.data_ptr(), B.distinct, d_at.data_ptr(), d_chars.data_ptr(), key_bytes, s)
    assert rc == 0, rc
    at, chars = d_at.cpu().numpy().tolist(), d_chars.cpu().numpy().tobytes()
    assert [chars[at[j]: at[j + 1]] for j in range(B.distinct)] == list(seen), "the dictionary is not the dict's keys in order"
    assert B.first[: B.distinct].cpu().tolist() == [v[0] for v in seen.values()] and B.counts[: B.distinct].cpu().tolist() == [v[1] for v in seen.values()], "first / counts"
    codes = B.codes.cpu().numpy()
    k_at, k_chars = key_offsets.cpu().numpy().tolist(), key_chars.cpu().numpy().tobytes()
    order = list(seen)
    for i in np.random.default_rng(1).integers(0, fields, 20000).tolist():
        assert order[codes[i]] == k_chars[k_at[i]: k_at[i + 1]], "a code does not stand for its cell's string"
    whole = torch.empty(16, dtype=torch.int32, device="cuda")
    assert p.cell_kinds_device(values.data_ptr(), tags.data_ptr(), fields, 1, whole.data_ptr(), s) == 0
    torch.cuda.synchronize()
    assert kinds[: B.distinct * 16].view(B.distinct, 16).sum(dim=0).cpu().tolist() == whole.cpu().tolist(), "the census by code does not sum to the census"
    for e in encodes.values():
        assert int(e.counts[: e.distinct].sum().item()) == int((e.codes >= 0).sum().item()) and int(e.codes.max().item()) == e.distinct - 1

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    runs = {"a_few_distinct_ms": encodes["a"], "b_user_keys_ms": encodes["b"], "c_nearly_distinct_ms": encodes["c"], "c2_short_strings_ms": encodes["c2"], "d_census_by_code_ms": run_census}
    for _ in range(args.warmup):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in runs}
    for _ in range(args.reps):  # alternating: what the clock and the neighbours do hits all alike
        for name, fn in runs.items():
            times[name].append(timed(fn))
    host_ms = []
    for _ in range(args.host_reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run_host()
        host_ms.append((time.perf_counter() - t0) * 1e3)
    out = {"mib": round(len(host) / 2 ** 20, 1), "rows": {k: int(e.n) for k, e in encodes.items()}, "distinct": {k: int(e.distinct) for k, e in encodes.items()},
           "key_bytes": int(key_bytes), "reps": args.reps}
    for name, t in times.items():
        out[name] = {"median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3)}
    out["e_gather_copy_python_dict_ms"] = {"median": round(statistics.median(host_ms), 1), "min": round(min(host_ms), 1), "max": round(max(host_ms), 1), "reps": args.host_reps}
    med = {name: statistics.median(t) for name, t in times.items()}
    out["e_over_b"] = round(statistics.median(host_ms) / med["b_user_keys_ms"], 1)
    out["ns_per_cell"] = {k: round(1e6 * med[name] / encodes[k].n, 3) for k, name in (("a", "a_few_distinct_ms"), ("b", "b_user_keys_ms"), ("c", "c_nearly_distinct_ms"),
                                                                                     ("c2", "c2_short_strings_ms"))}
    p.close()
    line = json.dumps(out)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
