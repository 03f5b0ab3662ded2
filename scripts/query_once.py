"""One measurement of the queries over device tapes (sjgpu_at_pointers_device, sjgpu_gather_strings_device) beside the tape build they follow.

Builds an amazon-like NDJSON stream of --mib MiB (simdjson_amd/csrc/corpus.c: every record an array of nine scalars), runs stage 1 once, and times in one
process, warmed, alternating, with events on the stream, median of --reps:
  (a) sjgpu_stage2_many_device on the stream          the tapes the queries read: what the extraction is to be small beside
  (b) sjgpu_at_pointers_device, 8 top-level pointers  /0 .. /7: eight typed columns
  (c) sjgpu_at_pointers_device, 8 three-token pointers /0/x/y .. /7/x/y -- on THIS corpus every one ends at the scalar its first token finds
      (NO_SUCH_FIELD): the price of the first level and of the compiled tokens, not of three levels
  (d) sjgpu_gather_strings_device on the column of /2 (the titles)
(b) and (c) only enqueue their walk: the second event is recorded behind it, so the figure is the walk's, the table check's and the call's.
Prints one JSON line.  For the kernel names run it once more under `rocprofv3 --kernel-trace --stats` with --reps 3 (tracing slows the host: the
timings of that run are not the ones to quote)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from simdjson_amd import build, capi, corpus  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this script measures, it does not fall back")
    build.build_sjgpu()
    host, lines = corpus.amazon_ndjson(args.mib << 20, 7)
    p = capi.DomParserImplementation(len(host) + 64)
    R = capi.ResidentStream(p, host, doc_cap=lines + 1)
    assert (R.code, R.docs) == (0, lines), (R.code, R.docs, lines)
    s, n, sbuf, docs, tw, sb = R.stream, R.n, R.sbuf, R.docs, R.tw, R.sb
    run_many = R.stage2
    top = [b"/%d" % k for k in range(8)]
    deep = [b"/%d/x/y" % k for k in range(8)]
    values = torch.empty((8, docs), dtype=torch.int64, device="cuda")
    tags = torch.empty((8, docs), dtype=torch.uint8, device="cuda")

    def run_pointers(pointers):
        rc = p.at_pointers_device(*R.args(), pointers, values.data_ptr(), tags.data_ptr(), s)
        assert rc == 0, rc

    run_pointers(deep)
    torch.cuda.synchronize()
    assert bool((tags == 20).all())  # every record's values are scalars
    run_pointers(top)
    torch.cuda.synchronize()
    col_tags = tags.cpu().numpy()
    assert (col_tags[:5] == ord('"')).all() and (col_tags[2] == ord('"')).all()  # asin, brand, title, url, image: strings in every record
    title_values, title_tags = values[2].clone(), tags[2].clone()
    offsets = torch.empty(docs + 1, dtype=torch.int32, device="cuda")
    chars = torch.empty(sb, dtype=torch.uint8, device="cuda")

    def run_gather():
        rc, total = p.gather_strings_device(sbuf.data_ptr(), sb, title_values.data_ptr(), title_tags.data_ptr(), docs, offsets.data_ptr(), chars.data_ptr(), sb, s)
        assert rc == 0, rc
        return total

    title_bytes = run_gather()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    runs = {"a_stage2_many_ms": run_many, "b_top_level_8_ms": lambda: run_pointers(top), "c_three_tokens_8_ms": lambda: run_pointers(deep), "d_gather_titles_ms": run_gather}
    for _ in range(args.warmup):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in runs}
    for _ in range(args.reps):  # alternating: what the clock and the neighbours do hits all four alike
        for name, fn in runs.items():
            times[name].append(timed(fn))
    out = {"mib": round(len(host) / 2 ** 20, 1), "records": int(docs), "tokens": int(n), "tape_words": int(tw), "string_bytes": int(sb), "title_bytes": int(title_bytes),
           "reps": args.reps}
    for name, t in times.items():
        out[name] = {"median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3)}
    base = statistics.median(times["a_stage2_many_ms"])
    for name in ("b_top_level_8_ms", "c_three_tokens_8_ms", "d_gather_titles_ms"):
        out[name.replace("_ms", "_over_a")] = round(statistics.median(times[name]) / base, 3)
    p.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
