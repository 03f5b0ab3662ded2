"""One measurement of the wide JSON text call (sjgpu_serialize_cells_wide_device) beside the narrow one (sjgpu_serialize_cells_device) and beside the mover both should
be compared with, by the protocol of scripts/json_text_once.py: one process, warmed, the calls alternating, events on the stream, median of --reps, every call at the
exact capacity, and the outputs compared first -- offsets, status and characters of the two calls must be equal before anything is timed.

Legs (a) to (d) of scripts/json_text_once.py over a twitter-like document of --mib MiB, an amazon-like NDJSON stream of --nd-mib MiB and --doubles doubles, wide beside
narrow; then the root of ONE twitter-like document as ONE cell at every size of --one-kib (64 KiB, 1, 16 and 256 MiB by default), wide beside sjgpu_minify_device over
the source and -- up to --narrow-up-to KiB, because it is one lane's work -- beside the narrow call.  The narrow call on one cell is first run ONCE under the clock:
when that run takes longer than --narrow-limit-s seconds it is the only one and is reported as such, otherwise as many repetitions as fit into that limit, --reps at
the most.
Writes --out (profiles/json_text_wide.txt) and prints the same JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from simdjson_amd import build, capi, corpus, json_text, json_text_wide  # noqa: E402

ENTRIES = {"narrow": json_text.serialize_cells_device, "wide": json_text_wide.serialize_cells_wide_device}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--nd-mib", type=int, default=256)
    ap.add_argument("--doubles", type=int, default=1 << 20)
    ap.add_argument("--one-kib", type=int, nargs="*", default=[64, 1 << 10, 16 << 10, 256 << 10])
    ap.add_argument("--narrow-up-to", type=int, default=16 << 10, help="KiB: the largest single cell the narrow call is run on")
    ap.add_argument("--narrow-limit-s", type=float, default=20.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "json_text_wide.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this script measures, it does not fall back")
    build.build_sjgpu()
    host, statuses = corpus.twitter_like(args.mib << 20, 7)
    nd_host, lines = corpus.amazon_ndjson(args.nd_mib << 20, 7)
    rng = np.random.default_rng(7)
    numbers = (rng.standard_normal(args.doubles) * 10.0 ** rng.integers(-8, 9, args.doubles)).tolist()
    d_host = np.frombuffer(("[" + ",".join(repr(x) for x in numbers) + "]").encode(), np.uint8)
    ones = {kib: corpus.twitter_like(kib << 10, 11)[0] for kib in args.one_kib}
    p = capi.DomParserImplementation(max([len(host), len(nd_host), len(d_host)] + [len(o) for o in ones.values()]) + 64)
    D = capi.ResidentStream(p, host, doc_cap=1)
    N = capi.ResidentStream(p, nd_host, doc_cap=lines)
    F = capi.ResidentStream(p, d_host, doc_cap=1)
    assert (D.code, D.docs, N.code, N.docs, F.code, F.docs) == (0, 1, 0, lines, 0, 1), (D.code, D.docs, N.code, N.docs, F.code, F.docs)
    s = D.stream

    def note(what):
        print(f"[json_text_wide_once] {what}", file=sys.stderr, flush=True)

    def rows_of(S, path, cap):
        offsets, status = torch.empty(2, dtype=torch.int32, device="cuda"), torch.empty(1, dtype=torch.uint8, device="cuda")
        values, tags = torch.empty(cap, dtype=torch.int64, device="cuda"), torch.empty(cap, dtype=torch.uint8, device="cuda")
        rc, rows = p.at_paths_wide_device(*S.args(), [path], offsets.data_ptr(), status.data_ptr(), values.data_ptr(), tags.data_ptr(), cap, s)
        assert rc == 0 and 0 < rows <= cap, (path, rc, rows)
        return values, tags, rows

    def roots_of(S):
        values, tags = torch.empty(S.docs, dtype=torch.int64, device="cuda"), torch.empty(S.docs, dtype=torch.uint8, device="cuda")
        assert p.at_pointers_device(*S.args(), [b""], values.data_ptr(), tags.data_ptr(), s) == 0
        return values, tags, S.docs

    class Serialize:
        """one row's texts at their exact capacity, by one of the two calls"""

        def __init__(self, which, S, row, bytes_known=None):
            self.entry, self.S, (self.values, self.tags, self.n) = ENTRIES[which], S, row
            self.offsets, self.status = torch.empty(self.n + 1, dtype=torch.int32, device="cuda"), torch.empty(self.n, dtype=torch.uint8, device="cuda")
            self.bytes = bytes_known
            if bytes_known is None:
                rc, self.bytes = self.entry(p, *S.args(), self.values.data_ptr(), self.tags.data_ptr(), self.n, self.offsets.data_ptr(), self.status.data_ptr(), 0, 0, s)
                assert rc == -5 and self.bytes > 0, (rc, self.bytes)
            self.chars = torch.empty(self.bytes, dtype=torch.uint8, device="cuda")

        def __call__(self):
            rc, total = self.entry(p, *self.S.args(), self.values.data_ptr(), self.tags.data_ptr(), self.n, self.offsets.data_ptr(), self.status.data_ptr(), self.chars.data_ptr(),
                                   self.bytes, s)
            assert (rc, total) == (0, self.bytes), (rc, total)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def stats(t):
        return {"median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3), "runs": len(t)}

    def equal(w, n, what):
        torch.cuda.synchronize()
        assert w.bytes == n.bytes and torch.equal(w.offsets, n.offsets) and torch.equal(w.status, n.status) and torch.equal(w.chars, n.chars), f"{what}: wide and narrow differ"
        assert not bool(w.status.any().item()), f"{what}: a cell was refused"

    out = {"mib": round(len(host) / 2 ** 20, 1), "nd_mib": round(len(nd_host) / 2 ** 20, 1), "reps": args.reps, "legs": {}, "one_cell": {}}
    # ---- legs (a) to (d): rows of many cells, wide beside narrow
    rows = {"a_entities": (D, rows_of(D, b"$.statuses[*].user.entities", statuses)), "b_statuses": (D, rows_of(D, b"$.statuses[*]", statuses)), "c_ndjson_roots": (N, roots_of(N)),
            "d_doubles": (F, rows_of(F, b"$[*]", args.doubles))}
    minified = torch.empty(len(nd_host) + 64, dtype=torch.uint8, device="cuda")

    def run_minify():
        assert p.minify_device(N.buf.data_ptr(), len(nd_host), minified.data_ptr(), s) == 0

    named = {}
    for leg, (S, row) in rows.items():
        n = Serialize("narrow", S, row)
        w = Serialize("wide", S, row, n.bytes)
        n()
        w()
        equal(w, n, leg)
        note(f"leg {leg}: {n.n} rows, {n.bytes} bytes, wide == narrow")
        named[leg + "/narrow"], named[leg + "/wide"] = n, w
        out["legs"][leg] = {"rows": int(n.n), "bytes": int(n.bytes)}
    named["c_minify_same_bytes"] = run_minify
    for _ in range(args.warmup):
        for fn in named.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in named}
    for _ in range(args.reps):  # alternating: what the clock and the neighbours do hits all alike
        for name, fn in named.items():
            times[name].append(timed(fn))
    for name, t in times.items():
        leg, _, which = name.partition("/")
        if which:
            out["legs"][leg][which + "_ms"] = stats(t)
            out["legs"][leg][which + "_gb_per_s_out"] = round(out["legs"][leg]["bytes"] / statistics.median(t) / 1e6, 2)
        else:
            out[name + "_ms"] = stats(t)
    for leg in rows:
        out["legs"][leg]["wide_over_narrow"] = round(out["legs"][leg]["wide_ms"]["median"] / out["legs"][leg]["narrow_ms"]["median"], 2)
    del named, rows, minified, D, N, F
    torch.cuda.empty_cache()
    # ---- ONE document as ONE cell, at every size
    for kib, one in ones.items():
        S = capi.ResidentStream(p, one, doc_cap=1)
        assert (S.code, S.docs) == (0, 1), (S.code, S.docs)
        row = roots_of(S)
        w = Serialize("wide", S, row)
        w()
        torch.cuda.synchronize()
        assert not bool(w.status.any().item())
        text = w.chars.cpu().numpy().tobytes()
        if kib <= 1 << 10:
            assert json.loads(text) == json.loads(one.tobytes()), "the text is not its document"
        small = torch.empty(len(one) + 64, dtype=torch.uint8, device="cuda")

        def run_small_minify():
            assert p.minify_device(S.buf.data_ptr(), len(one), small.data_ptr(), s) == 0
        entry = {"source_bytes": int(len(one)), "tape_words": int(S.tw), "bytes": int(w.bytes)}
        named = {"wide": w, "minify": run_small_minify}
        if kib <= args.narrow_up_to:
            n = Serialize("narrow", S, row, w.bytes)
            t0 = time.perf_counter()
            first = timed(n)
            wall = time.perf_counter() - t0
            equal(w, n, f"one cell of {kib} KiB")
            if wall > args.narrow_limit_s:
                entry["narrow_ms"] = {"median": round(first, 3), "min": round(first, 3), "max": round(first, 3), "runs": 1}
            else:
                named["narrow"] = n
                entry["narrow_reps"] = max(1, min(args.reps, int(args.narrow_limit_s / max(wall, 1e-4))))
        for _ in range(args.warmup):
            for name, fn in named.items():
                if name != "narrow":
                    fn()
        times = {name: [] for name in named}
        for i in range(args.reps):
            for name, fn in named.items():
                if name != "narrow" or i < entry["narrow_reps"]:
                    times[name].append(timed(fn))
        for name, t in times.items():
            entry[name + "_ms"] = stats(t)
        entry["wide_gb_per_s_out"] = round(w.bytes / entry["wide_ms"]["median"] / 1e6, 2)
        entry["wide_over_minify"] = round(entry["wide_ms"]["median"] / entry["minify_ms"]["median"], 1)
        if "narrow_ms" in entry:
            entry["narrow_over_wide"] = round(entry["narrow_ms"]["median"] / entry["wide_ms"]["median"], 1)
        out["one_cell"][f"{kib}_kib"] = entry
        note(f"one cell of {kib} KiB: {entry}")
        del S, w, small, named
        torch.cuda.empty_cache()
    p.close()
    line = json.dumps(out)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
