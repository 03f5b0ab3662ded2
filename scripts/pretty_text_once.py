"""One measurement of the two prettify calls (sjgpu_prettify_cells_device, sjgpu_prettify_cells_wide_device) beside their minify twins (sjgpu_serialize_cells_device,
sjgpu_serialize_cells_wide_device) on the same rows, by the protocol of scripts/json_text_once.py: one process, warmed, the calls alternating, events on the stream,
median of --reps, every call at the exact capacity, and the outputs compared before anything is timed -- offsets, status and characters of the wide call must be the
narrow call's, and a sample of the indented texts must parse with Python's json to what their minified twins parse to.

The legs of scripts/json_text_wide_once.py: (a) to (d) over a twitter-like document of --mib MiB, an amazon-like NDJSON stream of --nd-mib MiB and --doubles doubles,
the four calls side by side; then the root of ONE twitter-like document as ONE cell at every size of --one-kib (64 KiB, 1, 16 and 256 MiB by default), the two wide
calls side by side (the narrow ones up to --narrow-up-to KiB: one cell is one lane's work).  The yardstick of an indented text is its minify twin scaled by the bytes
written: per leg `pretty_over_minify` (time) stands beside `bytes_ratio`.

--minify-only times the two minify calls alone and imports nothing of the prettify calls: the same script then runs against a library built from an earlier commit
(SJGPU_LIB), which is how the minify calls are shown not to have slowed down -- --label names the column.
Writes --out (profiles/pretty_text.txt) and prints the same JSON line."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from simdjson_amd import build, capi, corpus, json_text, json_text_wide  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--nd-mib", type=int, default=256)
    ap.add_argument("--doubles", type=int, default=1 << 20)
    ap.add_argument("--one-kib", type=int, nargs="*", default=[64, 1 << 10, 16 << 10, 256 << 10])
    ap.add_argument("--narrow-up-to", type=int, default=1 << 10, help="KiB: the largest single cell the narrow calls are run on")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--minify-only", action="store_true")
    ap.add_argument("--label", default="this commit")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "pretty_text.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this script measures, it does not fall back")
    entries = {"minify_narrow": json_text.serialize_cells_device, "minify_wide": json_text_wide.serialize_cells_wide_device}
    if not args.minify_only:
        build.build_sjgpu()
        from simdjson_amd import pretty_text
        entries.update({"pretty_narrow": pretty_text.prettify_cells_device, "pretty_wide": pretty_text.prettify_cells_wide_device})
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
        print(f"[pretty_text_once] {what}", file=sys.stderr, flush=True)

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
        """one row's texts at their exact capacity, by one of the calls"""

        def __init__(self, which, S, row, bytes_known=None):
            self.entry, self.S, (self.values, self.tags, self.n) = entries[which], S, row
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

        def texts(self, which):
            at, chars = self.offsets.cpu().numpy().view(np.uint32), self.chars.cpu().numpy()
            return [chars[int(at[r]): int(at[r + 1])].tobytes() for r in which]

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

    def same_values(pretty, plain, n, what):
        sample = np.random.default_rng(1).integers(0, n, 200).tolist()
        for a, b in zip(pretty.texts(sample), plain.texts(sample)):
            assert a.endswith(b"\n") and json.loads(a) == json.loads(b), f"{what}: an indented text is not the value of its minified twin"

    def measure(named):
        for _ in range(args.warmup):
            for fn in named.values():
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name in named}
        for _ in range(args.reps):  # alternating: what the clock and the neighbours do hits all alike
            for name, fn in named.items():
                times[name].append(timed(fn))
        return times

    def ratios(entry):
        for road in ("narrow", "wide"):
            if f"pretty_{road}_ms" in entry and f"minify_{road}_ms" in entry:
                entry[f"{road}_pretty_over_minify"] = round(entry[f"pretty_{road}_ms"]["median"] / entry[f"minify_{road}_ms"]["median"], 2)
        if "pretty_bytes" in entry:
            entry["bytes_ratio"] = round(entry["pretty_bytes"] / entry["minify_bytes"], 2)

    out = {"label": args.label, "mib": round(len(host) / 2 ** 20, 1), "nd_mib": round(len(nd_host) / 2 ** 20, 1), "reps": args.reps, "legs": {}, "one_cell": {}}
    # ---- legs (a) to (d): rows of many cells, the calls side by side
    rows = {"a_entities": (D, rows_of(D, b"$.statuses[*].user.entities", statuses)), "b_statuses": (D, rows_of(D, b"$.statuses[*]", statuses)), "c_ndjson_roots": (N, roots_of(N)),
            "d_doubles": (F, rows_of(F, b"$[*]", args.doubles))}
    for leg, (S, row) in rows.items():
        named = {}
        for kind in ("minify",) if args.minify_only else ("minify", "pretty"):
            n = Serialize(kind + "_narrow", S, row)
            w = Serialize(kind + "_wide", S, row, n.bytes)
            n()
            w()
            equal(w, n, f"{leg} ({kind})")
            named[kind + "_narrow"], named[kind + "_wide"] = n, w
        entry = {"rows": int(row[2]), "minify_bytes": int(named["minify_narrow"].bytes)}
        if not args.minify_only:
            entry["pretty_bytes"] = int(named["pretty_narrow"].bytes)
            same_values(named["pretty_narrow"], named["minify_narrow"], row[2], leg)
        for name, t in measure(named).items():
            entry[name + "_ms"] = stats(t)
        ratios(entry)
        out["legs"][leg] = entry
        note(f"leg {leg}: {entry}")
        del named
        torch.cuda.empty_cache()
    del rows, D, N, F
    torch.cuda.empty_cache()
    # ---- ONE document as ONE cell, at every size
    for kib, one in ones.items():
        S = capi.ResidentStream(p, one, doc_cap=1)
        assert (S.code, S.docs) == (0, 1), (S.code, S.docs)
        row = roots_of(S)
        named = {}
        for kind in ("minify",) if args.minify_only else ("minify", "pretty"):
            w = Serialize(kind + "_wide", S, row)
            w()
            named[kind + "_wide"] = w
            if kib <= args.narrow_up_to:
                n = Serialize(kind + "_narrow", S, row, w.bytes)
                n()
                equal(w, n, f"one cell of {kib} KiB ({kind})")
                named[kind + "_narrow"] = n
        torch.cuda.synchronize()
        entry = {"source_bytes": int(len(one)), "tape_words": int(S.tw), "minify_bytes": int(named["minify_wide"].bytes)}
        if not args.minify_only:
            entry["pretty_bytes"] = int(named["pretty_wide"].bytes)
            if kib <= 1 << 10:
                assert json.loads(named["pretty_wide"].texts([0])[0]) == json.loads(one.tobytes()), "the text is not its document"
        for name, t in measure(named).items():
            entry[name + "_ms"] = stats(t)
        ratios(entry)
        out["one_cell"][f"{kib}_kib"] = entry
        note(f"one cell of {kib} KiB: {entry}")
        del S, named
        torch.cuda.empty_cache()
    p.close()
    line = json.dumps(out)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
