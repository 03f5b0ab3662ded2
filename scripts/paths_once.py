"""One measurement of the paths over device tapes (sjgpu_at_paths_device) beside the pointers they generalise.

Builds the amazon-like NDJSON stream of --mib MiB of scripts/query_once.py (every record an array of nine scalars), runs stage 1 and
sjgpu_stage2_many_device once, and times in one process, warmed, alternating, with events on the stream, median of --reps:
  (a) sjgpu_at_pointers_device, /0 .. /7         the yardstick: eight typed columns, eight of the nine values of every record
  (b) sjgpu_at_paths_device, $[*]                one ragged column: all nine values of every record (count + scan + fill)
  (c) sjgpu_at_paths_device, $[*] and $[2]       the same beside a path without a wildcard
and, on a twitter-like SINGLE document of --twitter-mib MiB:
  (d) sjgpu_at_paths_device, $.statuses[*].user.id   one cell: the whole walk is one lane's work -- the bound the header states, as a number
(a) only enqueues its walk; (b) .. (d) read their total back and return when the column is complete.  Prints one JSON line.  For the split into
count, scan and fill run it once more under `rocprofv3 --kernel-trace --stats` with --reps 3 (tracing slows the host: the timings of that run are
not the ones to quote)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from simdjson_amd import build, capi, corpus  # noqa: E402


def resident(host, doc_cap):
    """a host buffer's tapes (one per document) on the device, with a parser of its own"""
    R = capi.ResidentStream(capi.DomParserImplementation(len(host) + 64), host, doc_cap=doc_cap)
    assert R.code == 0, R.code
    return R


def paths_run(torch, R, paths):
    """-> a function that runs sjgpu_at_paths_device into outputs of the size a first call asked for, and the matches"""
    cells = len(paths) * R.docs
    offsets = torch.empty(cells + 1, dtype=torch.int32, device="cuda")
    status = torch.empty(cells, dtype=torch.uint8, device="cuda")
    args = (*R.args(), paths, offsets.data_ptr(), status.data_ptr())
    rc, matches = R.p.at_paths_device(*args, 0, 0, 0, R.stream)
    assert rc in (0, capi.SJGPU_E_OVERFLOW), rc
    values = torch.empty(max(matches, 1), dtype=torch.int64, device="cuda")
    tags = torch.empty(max(matches, 1), dtype=torch.uint8, device="cuda")

    def run():
        rc, m = R.p.at_paths_device(*args, values.data_ptr(), tags.data_ptr(), matches, R.stream)
        assert (rc, m) == (0, matches), (rc, m)
    run.keep = (offsets, status, values, tags)
    return run, matches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--twitter-mib", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this script measures, it does not fall back")
    build.build_sjgpu()
    host, lines = corpus.amazon_ndjson(args.mib << 20, 7)
    R = resident(host, lines + 1)
    assert R.docs == lines, (R.docs, lines)
    top = [b"/%d" % k for k in range(8)]
    values = torch.empty((8, R.docs), dtype=torch.int64, device="cuda")
    tags = torch.empty((8, R.docs), dtype=torch.uint8, device="cuda")

    def run_pointers():
        rc = R.p.at_pointers_device(*R.args(), top, values.data_ptr(), tags.data_ptr(), R.stream)
        assert rc == 0, rc

    run_all, all_matches = paths_run(torch, R, [b"$[*]"])
    run_both, both_matches = paths_run(torch, R, [b"$[*]", b"$[2]"])
    assert all_matches == 9 * R.docs and both_matches == 10 * R.docs, (all_matches, both_matches, R.docs)
    thost, statuses = corpus.twitter_like(args.twitter_mib << 20, 7)
    W = resident(thost, 1)
    assert W.docs == 1
    run_ids, id_matches = paths_run(torch, W, [b"$.statuses[*].user.id"])
    assert 0 < id_matches <= statuses, (id_matches, statuses)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    runs = {"a_pointers_8_ms": run_pointers, "b_paths_all_ms": run_all, "c_paths_all_and_one_ms": run_both, "d_twitter_user_ids_ms": run_ids}
    for _ in range(args.warmup):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in runs}
    for _ in range(args.reps):  # alternating: what the clock and the neighbours do hits all four alike
        for name, fn in runs.items():
            times[name].append(timed(fn))
    out = {"mib": round(len(host) / 2 ** 20, 1), "records": int(R.docs), "tape_words": int(R.tw), "matches_all": int(all_matches), "twitter_mib": round(len(thost) / 2 ** 20, 1),
           "twitter_tape_words": int(W.tw), "twitter_statuses": int(statuses), "twitter_matches": int(id_matches), "reps": args.reps}
    for name, t in times.items():
        out[name] = {"median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3)}
    base = statistics.median(times["a_pointers_8_ms"])
    for name in ("b_paths_all_ms", "c_paths_all_and_one_ms"):
        out[name.replace("_ms", "_over_a")] = round(statistics.median(times[name]) / base, 3)
    R.p.close()
    W.p.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
