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

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from simdjson_amd import build, capi, corpus  # noqa: E402


class Resident:
    """a host buffer's stage 1 and its tapes (one per document), everything on the device"""

    def __init__(self, torch, host, doc_cap):
        self.p = p = capi.DomParserImplementation(len(host) + 64)
        self.s = s = torch.cuda.current_stream().cuda_stream
        self.buf = torch.from_numpy(np.concatenate([host, np.zeros(64, np.uint8)])).cuda()
        self.idx = torch.zeros(len(host) + 16, dtype=torch.int32, device="cuda")
        assert p.stage1_device(self.buf.data_ptr(), len(host), self.idx.data_ptr(), len(host) + 3, s) == 0
        n, flags, _ = p.result(s)
        assert flags == 0, flags
        sbuf_cap = 5 * (len(host) // 3) + 256
        self.sbuf = torch.empty(sbuf_cap, dtype=torch.uint8, device="cuda")
        tape_cap = min(4 * n, len(host) + 3 * doc_cap) + 8
        self.tape = torch.empty(tape_cap, dtype=torch.int64, device="cuda")
        self.table = torch.empty((doc_cap + 1) * 4, dtype=torch.int32, device="cuda")
        code, self.docs, self.tw, self.sb = p.stage2_many_device(self.buf.data_ptr(), len(host), self.idx.data_ptr(), n, self.tape.data_ptr(), tape_cap, self.sbuf.data_ptr(),
                                                                 sbuf_cap, self.table.data_ptr(), doc_cap + 1, stream=s)
        assert code == 0, code
        self.torch = torch

    def paths(self, paths):
        """-> a function that runs sjgpu_at_paths_device into outputs of the size a first call asked for, and the matches"""
        torch, p = self.torch, self.p
        cells = len(paths) * self.docs
        offsets = torch.empty(cells + 1, dtype=torch.int32, device="cuda")
        status = torch.empty(cells, dtype=torch.uint8, device="cuda")
        args = (self.tape.data_ptr(), self.tw, self.sbuf.data_ptr(), self.sb, self.table.data_ptr(), self.docs, paths, offsets.data_ptr(), status.data_ptr())
        rc, matches = p.at_paths_device(*args, 0, 0, 0, self.s)
        assert rc in (0, -5), rc
        values = torch.empty(max(matches, 1), dtype=torch.int64, device="cuda")
        tags = torch.empty(max(matches, 1), dtype=torch.uint8, device="cuda")

        def run():
            rc, m = p.at_paths_device(*args, values.data_ptr(), tags.data_ptr(), matches, self.s)
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
    R = Resident(torch, host, lines + 1)
    assert R.docs == lines, (R.docs, lines)
    top = [b"/%d" % k for k in range(8)]
    values = torch.empty((8, R.docs), dtype=torch.int64, device="cuda")
    tags = torch.empty((8, R.docs), dtype=torch.uint8, device="cuda")

    def run_pointers():
        rc = R.p.at_pointers_device(R.tape.data_ptr(), R.tw, R.sbuf.data_ptr(), R.sb, R.table.data_ptr(), R.docs, top, values.data_ptr(), tags.data_ptr(), R.s)
        assert rc == 0, rc

    run_all, all_matches = R.paths([b"$[*]"])
    run_both, both_matches = R.paths([b"$[*]", b"$[2]"])
    assert all_matches == 9 * R.docs and both_matches == 10 * R.docs, (all_matches, both_matches, R.docs)
    thost, statuses = corpus.twitter_like(args.twitter_mib << 20, 7)
    W = Resident(torch, thost, 1)
    assert W.docs == 1
    run_ids, id_matches = W.paths([b"$.statuses[*].user.id"])
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
