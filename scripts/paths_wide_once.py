"""One measurement of the two roads of the paths over device tapes: sjgpu_at_paths_device (one lane per cell) beside sjgpu_at_paths_wide_device
(breadth first, one lane per word of a wildcard level), in the manner of scripts/paths_once.py.

Per case one process, warmed, alternating, events on the stream, median and min of --reps:
  the sjgpu_stage2_many_device that made the tapes, the narrow call, the wide call -- the two calls at the exact capacity a first call asked for.
Cases:
  one twitter-like document of --twitter-mib MiB (several sizes may be given):
    $.statuses[*].user.id
    $.statuses[*].entities.hashtags[*].text              the path as real tweets have it; the synthetic corpus keeps `entities` under `user` and its
                                                         hashtags hold only `indices`, so this one matches nothing: every branch ends at `.entities`
    $.statuses[*].user.entities.hashtags[*].indices[*]   the nearest path that matches in the corpus: three wildcard levels
  the amazon-like NDJSON of --mib MiB (scripts/query_once.py's: every record an array of nine scalars):
    $[*]
The outputs of the two calls are compared once, bit for bit, before anything is timed.  Writes --out (profiles/paths_wide.txt) and prints the same JSON
line.  For the split into kernels run it once more under `rocprofv3 --kernel-trace --stats` with --reps 3 (tracing slows the host: the timings of that
run are not the ones to quote)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from simdjson_amd import build, capi, corpus  # noqa: E402

TWITTER_PATHS = [b"$.statuses[*].user.id", b"$.statuses[*].entities.hashtags[*].text", b"$.statuses[*].user.entities.hashtags[*].indices[*]"]


def resident(host, doc_cap):
    """a host buffer's tapes (one per document) on the device, with a parser of its own"""
    R = capi.ResidentStream(capi.DomParserImplementation(len(host) + 64), host, doc_cap=doc_cap)
    assert R.code == 0, R.code
    return R


def roads(R, torch, paths):
    """-> (narrow, wide, matches): the two calls into outputs of the size a first call asked for, compared bit for bit once"""
    cells = len(paths) * R.docs
    args = (*R.args(), paths)
    rc, matches = R.p.at_paths_device(*args, torch.empty(cells + 1, dtype=torch.int32, device="cuda").data_ptr(), torch.empty(cells, dtype=torch.uint8, device="cuda").data_ptr(),
                                      0, 0, 0, R.stream)
    assert rc in (0, capi.SJGPU_E_OVERFLOW), rc
    outs, fns = [], []
    for call in (R.p.at_paths_device, R.p.at_paths_wide_device):
        out = (torch.zeros(cells + 1, dtype=torch.int32, device="cuda"), torch.zeros(cells, dtype=torch.uint8, device="cuda"),
               torch.zeros(max(matches, 1), dtype=torch.int64, device="cuda"), torch.zeros(max(matches, 1), dtype=torch.uint8, device="cuda"))

        def run(call=call, out=out):
            rc, m = call(*args, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), matches, R.stream)
            assert (rc, m) == (0, matches), (rc, m)
        run()
        outs.append(out)
        fns.append(run)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(*outs)), "the two roads disagree"
    return fns[0], fns[1], matches


def stage2_again(R):
    def run():
        assert R.stage2() == (0, R.docs, R.tw, R.sb)
    return run


def measure(torch, runs, reps, warmup):
    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)
    for _ in range(warmup):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in runs}
    for _ in range(reps):  # alternating: what the clock and the neighbours do hits all alike
        for name, fn in runs.items():
            times[name].append(timed(fn))
    return {name: {"median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3)} for name, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--twitter-mib", type=int, nargs="*", default=[64])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "paths_wide.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this script measures, it does not fall back")
    build.build_sjgpu()
    out = {"reps": args.reps, "unit": "ms", "cases": []}
    for mib in args.twitter_mib:
        host, statuses = corpus.twitter_like(mib << 20, 7)
        R = resident(host, 1)
        assert R.docs == 1
        for path in TWITTER_PATHS:
            narrow, wide, matches = roads(R, torch, [path])
            case = {"corpus": "twitter-like, one document", "mib": round(len(host) / 2 ** 20, 1), "tape_words": int(R.tw), "statuses": int(statuses), "path": path.decode(),
                    "matches": int(matches)}
            case.update(measure(torch, {"stage2_many": stage2_again(R), "narrow": narrow, "wide": wide}, args.reps, args.warmup))
            case["wide_min_over_narrow_min"] = round(case["wide"]["min"] / case["narrow"]["min"], 4)
            out["cases"].append(case)
            print(json.dumps(case), flush=True)
        R.p.close()
        del R
        torch.cuda.empty_cache()
    if args.mib:
        host, lines = corpus.amazon_ndjson(args.mib << 20, 7)
        R = resident(host, lines + 1)
        assert R.docs == lines
        narrow, wide, matches = roads(R, torch, [b"$[*]"])
        case = {"corpus": "amazon-like NDJSON", "mib": round(len(host) / 2 ** 20, 1), "tape_words": int(R.tw), "records": int(R.docs), "path": "$[*]", "matches": int(matches)}
        case.update(measure(torch, {"stage2_many": stage2_again(R), "narrow": narrow, "wide": wide}, args.reps, args.warmup))
        case["wide_min_over_narrow_min"] = round(case["wide"]["min"] / case["narrow"]["min"], 4)
        out["cases"].append(case)
        print(json.dumps(case), flush=True)
        R.p.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("scripts/paths_wide_once.py: sjgpu_at_paths_device (narrow) beside sjgpu_at_paths_wide_device (wide), milliseconds, median / min / max of %d, one process, warmed, "
                "alternating, events on the stream\n" % args.reps)
        for case in out["cases"]:
            f.write(json.dumps(case) + "\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
