"""One measurement of stage 2 over a document stream (sjgpu_stage2_many_device) beside the single document's call on the same records.

Builds an amazon-like NDJSON stream of --mib MiB (simdjson_amd/csrc/corpus.c) and the SAME records wrapped as one array [r1,r2,...], runs stage 1 on
both, and times in one process, warmed, alternating, with events on the stream, median of --reps:
  (a) sjgpu_stage2_many_device on the stream     one tape per record
  (b) sjgpu_stage2_device on the array           the single document's road over the same tokens
  (c) the reference's stage 2 on the array, one core (oracle/_ref/libsjref.so, where it is present)
  (d) (a) on the stream with its LAST record broken: two runs by design
Prints one JSON line.  For the per-kernel split run it once more under `rocprofv3 --kernel-trace --stats` with --reps 3 (tracing slows the host: the
timings of that run are not the ones to quote)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from simdjson_amd import _paths, build, capi, corpus  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this script measures, it does not fall back")
    build.build_sjgpu()
    stream_host, lines = corpus.amazon_ndjson(args.mib << 20, 7)
    if stream_host[-1] != 0x0A:
        stream_host = np.concatenate([stream_host, np.frombuffer(b"\n", np.uint8)])
    array_host = np.concatenate([np.frombuffer(b"[", np.uint8), stream_host])
    nl = np.flatnonzero(array_host == 0x0A)  # (a JSON string holds no raw newline: every one of them ends a record)
    assert len(nl) == lines, (len(nl), lines)
    array_host[nl] = ord(",")
    array_host[nl[-1]] = ord("]")
    broken_host = stream_host.copy()
    assert broken_host[-2] == ord("]")  # (a record is an array; the stream ends "]\n")
    broken_host[-2] = ord("}")  # the last record's closing bracket is of the wrong kind: TAPE_ERROR at that token, every string still valid

    p = capi.DomParserImplementation(len(array_host) + 64)
    # three resident buffers, each with its tapes; the array's (one document to the stream call) are only what stage 1 leaves for the single document's call below
    S = capi.ResidentStream(p, stream_host, doc_cap=lines + 1)
    A = capi.ResidentStream(p, array_host, doc_cap=1)
    B = capi.ResidentStream(p, broken_host, doc_cap=lines + 1)
    assert (S.code, A.code) == (0, 0), (S.code, A.code)
    n_stream, n_array = S.n, A.n
    single_tape = torch.empty(len(array_host) + 8, dtype=torch.int64, device="cuda")
    run_many, run_broken = S.stage2, B.stage2

    def run_single():
        return p.stage2_device(A.buf.data_ptr(), len(array_host), A.idx.data_ptr(), n_array, single_tape.data_ptr(), len(array_host) + 8, A.sbuf.data_ptr(), A.sbuf.numel(),
                               stream=A.stream)

    # the two roads deliver the same words: an array adds its two brackets to the records' words, a stream two root words per record
    code, docs, tw_many, sb_many = run_many()
    assert (code, docs) == (0, lines), (code, docs, lines)
    code1, tw_single, sb_single = run_single()
    assert code1 == 0 and tw_many == (tw_single - 4) + 2 * lines and sb_many == sb_single, (code1, tw_many, tw_single, sb_many, sb_single)
    codeb, docsb, _, _ = run_broken()
    assert (codeb, docsb) == (3, lines - 1), (codeb, docsb)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    for _ in range(args.warmup):
        run_many(), run_single(), run_broken()
    t_many, t_single, t_broken = [], [], []
    for k in range(args.reps):  # alternating: what the clock and the neighbours do hits all three alike
        t_many.append(timed(run_many))
        t_single.append(timed(run_single))
        if k % 4 == 0:
            t_broken.append(timed(run_broken))
    out = {"mib": round(len(stream_host) / 2 ** 20, 1), "records": int(lines), "tokens_stream": int(n_stream), "tokens_array": int(n_array), "tape_words_stream": int(tw_many),
           "tape_words_array": int(tw_single), "string_bytes": int(sb_many), "reps": args.reps,
           "a_stream_ms": {"median": round(statistics.median(t_many), 3), "min": round(min(t_many), 3), "max": round(max(t_many), 3)},
           "b_array_ms": {"median": round(statistics.median(t_single), 3), "min": round(min(t_single), 3), "max": round(max(t_single), 3)},
           "ratio_a_over_b": round(statistics.median(t_many) / statistics.median(t_single), 3),
           "d_broken_last_record_ms": {"median": round(statistics.median(t_broken), 3), "reps": len(t_broken)}}
    if not args.no_cpu and os.path.exists(_paths.LIB_REF):
        R = ctypes.CDLL(_paths.LIB_REF)
        R.sjref_available.restype = ctypes.c_int
        R.sjref_available.argtypes = [ctypes.c_char_p]
        R.sjref_bench_stage2.restype = ctypes.c_double
        R.sjref_bench_stage2.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
        impl = next((i for i in (b"icelake", b"haswell", b"westmere") if R.sjref_available(i)), None)
        if impl:
            padded = np.concatenate([array_host, np.zeros(128, np.uint8)])
            err = ctypes.c_int(0)
            sec = R.sjref_bench_stage2(impl, padded.ctypes.data, len(array_host), 2, ctypes.byref(err))
            out["c_reference_stage2_ms"] = {"value": round(sec * 1e3, 1), "kernel": impl.decode(), "cores": 1, "error": err.value, "sample": "best of 2"}
    else:
        out["c_reference_stage2_ms"] = "not measured"
    p.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
