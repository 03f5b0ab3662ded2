"""One measurement of the typed getters over a column (sjgpu_cell_kinds_device, sjgpu_cast_cells_device) beside a copy of the same bytes, in the manner of
scripts/rows_once.py.

Builds one twitter-like document of --mib MiB (simdjson_amd/csrc/corpus.c: `{"statuses": [ ... ]}`), its tapes (sjgpu_stage2_many_device, one document), the rows of
`$.statuses[*]` (sjgpu_at_paths_wide_device, once) and the table of 8 pointers over them (sjgpu_at_pointers_from_cells_device): the workload of profiles/rows.txt.
Then times in one process, warmed, alternating, with events on the stream, median of --reps:
  (t) sjgpu_at_pointers_from_cells_device, the 8 columns                      what the cells cost to make (the call of profiles/rows.txt)
  (k) sjgpu_cell_kinds_device over the 8 x rows cells                         the census: reads 9 bytes per cell
  (c) sjgpu_cast_cells_device over them, the getters infer_getters picked     the cast: 18 bytes + 1 bit per cell
  (m) hipMemcpyAsync device to device of the cast's byte count                the yardstick of (c): a copy of B bytes reads B and writes B
and the same three -- (k), (c), (m) -- over ONE synthetic row of 2^--log2-cells cells (tags cycled over the nine tags and the four codes, words from a counter): the
table is a few million cells and its calls are launch-bound, the synthetic row is what the kernels do at size.
The cast's byte count: cells * 18 + the bitmap + the counts; the copy moves half of it from one buffer to another (that many bytes read and as many written).
Before anything is timed the table's cast is compared with a cast made on the host from the same cells (numpy).
Writes --out (profiles/casts.txt) and prints the same JSON line.  Kernel times: run it once more under `rocprofv3 --kernel-trace --stats` with --reps 3."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from simdjson_amd import build, capi, corpus  # noqa: E402
from rows_once import POINTERS  # noqa: E402


def host_cast_row(tags, values, getter):
    """the rules of include/sjgpu_cast.h for the four scalar getters the table meets, in numpy -> (values, codes)"""
    ok = {capi.GET_INT64: (tags == ord("l")) | ((tags == ord("u")) & (values < (1 << 63))), capi.GET_STRING: tags == ord('"'),
          capi.GET_DOUBLE: np.isin(tags, [ord(c) for c in "dlu"])}[getter]
    out = values.copy()
    if getter == capi.GET_DOUBLE:
        out = np.where(tags == ord("l"), values.view(np.int64).astype(np.float64).view(np.uint64), out)
        out = np.where(tags == ord("u"), values.astype(np.float64).view(np.uint64), out)
    codes = np.where(ok, 0, np.where((tags >= 1) & (tags <= 33), tags, np.where((getter == capi.GET_INT64) & (tags == ord("u")), 18, 17))).astype(np.uint8)
    return np.where(ok, out, 0).astype(np.uint64), codes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--log2-cells", type=int, default=26)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "casts.txt"))
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
    K = len(POINTERS)
    offsets = torch.empty(2, dtype=torch.int32, device="cuda")
    status = torch.empty(1, dtype=torch.uint8, device="cuda")
    root_values = torch.empty(statuses, dtype=torch.int64, device="cuda")
    root_tags = torch.empty(statuses, dtype=torch.uint8, device="cuda")
    rc, rows = p.at_paths_wide_device(*D.args(), [b"$.statuses[*]"], offsets.data_ptr(), status.data_ptr(), root_values.data_ptr(), root_tags.data_ptr(), statuses, s)
    assert (rc, rows) == (0, statuses), (rc, rows)
    values = torch.empty((K, rows), dtype=torch.int64, device="cuda")
    tags = torch.empty((K, rows), dtype=torch.uint8, device="cuda")

    def run_table():
        rc = p.at_pointers_from_cells_device(*D.args(), root_values.data_ptr(), root_tags.data_ptr(), rows, POINTERS, values.data_ptr(), tags.data_ptr(), s)
        assert rc == 0, rc

    class Column:
        """K rows of n cells on the device with the outputs of both calls and the two buffers of the copy"""

        def __init__(self, values, tags, getters=None):
            self.values, self.tags = values, tags
            self.K, self.n = tags.shape
            W = (self.n + 63) // 64
            self.kinds = torch.empty((self.K, 16), dtype=torch.int32, device="cuda")
            self.out_values = torch.empty((self.K, self.n), dtype=torch.int64, device="cuda")
            self.out_codes = torch.empty((self.K, self.n), dtype=torch.uint8, device="cuda")
            self.valid = torch.empty((self.K, W), dtype=torch.int64, device="cuda")
            self.counts = torch.empty((self.K, 4), dtype=torch.int32, device="cuda")
            self.cast_bytes = self.K * self.n * 18 + self.K * W * 8 + self.K * 16
            self.src = torch.empty(self.cast_bytes // 2, dtype=torch.uint8, device="cuda")
            self.dst = torch.empty(self.cast_bytes // 2, dtype=torch.uint8, device="cuda")
            self.getters = getters

        def run_kinds(self):
            rc = p.cell_kinds_device(self.values.data_ptr(), self.tags.data_ptr(), self.n, self.K, self.kinds.data_ptr(), s)
            assert rc == 0, rc

        def run_cast(self):
            rc = p.cast_cells_device(self.values.data_ptr(), self.tags.data_ptr(), self.n, self.getters, self.out_values.data_ptr(), self.out_codes.data_ptr(),
                                     self.valid.data_ptr(), self.counts.data_ptr(), s)
            assert rc == 0, rc

        def run_copy(self):
            self.dst.copy_(self.src, non_blocking=True)  # hipMemcpyAsync, device to device, on the current stream

    run_table()
    T = Column(values, tags)
    T.run_kinds()
    torch.cuda.synchronize()
    kinds = T.kinds.cpu().numpy().view(np.uint32)
    T.getters = capi.infer_getters(kinds)
    assert all(T.getters), (T.getters, kinds.tolist())
    T.run_cast()
    torch.cuda.synchronize()
    th, vh = tags.cpu().numpy(), values.cpu().numpy().view(np.uint64)
    oh, ch = T.out_values.cpu().numpy().view(np.uint64), T.out_codes.cpu().numpy()
    for k in range(K):
        want_values, want_codes = host_cast_row(th[k], vh[k], T.getters[k])
        assert np.array_equal(oh[k], want_values) and np.array_equal(ch[k], want_codes), POINTERS[k]
        assert np.array_equal(T.valid[k].cpu().numpy().view(np.uint8)[: (rows + 7) // 8], np.packbits(ch[k] == 0, bitorder="little")), POINTERS[k]
    n_big = 1 << args.log2_cells
    cycle = torch.from_numpy(np.frombuffer(b'{["ludtfn' + bytes([17, 19, 20, 22]), np.uint8).copy()).cuda()
    big_tags = cycle[torch.arange(n_big, device="cuda") % len(cycle)].reshape(1, n_big).contiguous()
    big_values = (torch.arange(n_big, dtype=torch.int64, device="cuda") * 0x1E3779B97F4A7C15).reshape(1, n_big)
    B = Column(big_values, big_tags, [capi.GET_DOUBLE])
    B.run_kinds()
    B.run_cast()
    torch.cuda.synchronize()
    assert B.kinds.cpu().numpy().view(np.uint32)[0, :9].sum() + B.kinds.cpu().numpy().view(np.uint32)[0, 10:14].sum() == n_big
    assert int(B.counts.cpu().numpy().view(np.uint32)[0, 0]) == sum((n_big - i + 12) // 13 for i in (3, 4, 5))  # the l, u and d cells of the cycle

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    runs = {"t_table_8_ms": run_table, "k_kinds_table_ms": T.run_kinds, "c_cast_table_ms": T.run_cast, "m_copy_table_ms": T.run_copy,
            "k_kinds_row_ms": B.run_kinds, "c_cast_row_ms": B.run_cast, "m_copy_row_ms": B.run_copy}
    for _ in range(args.warmup):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in runs}
    for _ in range(args.reps):  # alternating: what the clock and the neighbours do hits all alike
        for name, fn in runs.items():
            times[name].append(timed(fn))
    med = {name: statistics.median(t) for name, t in times.items()}
    out = {"mib": round(len(host) / 2 ** 20, 1), "rows": int(rows), "pointers": K, "getters": T.getters, "table_cells": K * int(rows), "table_cast_bytes": T.cast_bytes,
           "row_cells": n_big, "row_cast_bytes": B.cast_bytes, "reps": args.reps}
    for name, t in times.items():
        out[name] = {"median": round(med[name], 4), "min": round(min(t), 4), "max": round(max(t), 4)}
    out["cast_over_copy_table"] = round(med["c_cast_table_ms"] / med["m_copy_table_ms"], 3)
    out["cast_over_copy_row"] = round(med["c_cast_row_ms"] / med["m_copy_row_ms"], 3)
    out["kinds_over_copy_row"] = round(med["k_kinds_row_ms"] / med["m_copy_row_ms"], 3)
    out["cast_row_GBps"] = round(B.cast_bytes / med["c_cast_row_ms"] / 1e6, 1)
    out["kinds_row_GBps"] = round(n_big * 9 / med["k_kinds_row_ms"] / 1e6, 1)
    out["copy_row_GBps"] = round(B.cast_bytes / med["m_copy_row_ms"] / 1e6, 1)
    out["kinds_plus_cast_share_of_table_call"] = round((med["k_kinds_table_ms"] + med["c_cast_table_ms"]) / med["t_table_8_ms"], 3)
    p.close()
    line = json.dumps(out)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
