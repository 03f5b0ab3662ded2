"""CPU tier: the shape of bench.py's one JSON line, checked on what the final tree of the round produced on the GPU box
(profiles/r06_bench_final.json = the printed line, r06_bench_detail.json = the full record; the N = 2 dry run and the NDJSON line at N = 1 beside them) -- the fields the driver and the judge read (metric / value / unit / n_gpus / steps / warmup /
ms_per_step / higher_is_better / scaling / vs_baseline / dtype / data / config.workload / roofline / cpu_baseline), every leg with its
own roofline where one is defined, no leg failed, and the arithmetic the line claims (frac = achieved / peak, value = bytes / time)."""
import glob
import json
import os

from simdjson_amd import _paths


def _final_line():
    """The full record of the final tree's default run.  Round 6 on: `bench_detail.json` as bench.py wrote it, committed as profiles/rNN_bench_detail.json
    (the printed line is profiles/rNN_bench_final.json); rounds 1-5 printed the full record itself."""
    files = sorted(glob.glob(os.path.join(_paths.REPO_ROOT, "profiles", "r*_bench_detail.json"))) or \
        sorted(glob.glob(os.path.join(_paths.REPO_ROOT, "profiles", "r*_bench_final.json")))
    assert files, "no committed bench line"
    return json.load(open(files[-1])), files[-1]


def _strict(text):
    def refuse(x):
        raise ValueError("non-finite number in the line: " + x)
    return json.loads(text, parse_constant=refuse)


def test_the_printed_line_is_a_record_not_a_document():
    """round 5's one line had grown to 23 KB and the driver could not parse it (BENCH_r05.json: parsed = null).  The printed line is now
    compact_line(full record): <= 4096 characters, strict JSON (no NaN / Infinity), the contract's fields, every leg as a handful of numbers; the full record
    goes to the side-car.  Checked on every full record committed so far (N = 1, N = 2 dry run, NDJSON at N = 1) and on a record whose every string is long."""
    import sys
    sys.path.insert(0, _paths.REPO_ROOT)
    import bench
    assert bench.COMPACT_LINE_LIMIT == 4096
    prof = os.path.join(_paths.REPO_ROOT, "profiles")
    records = [f for f in sorted(glob.glob(os.path.join(prof, "r*_bench_*.json")))  # round 5 on: every record carries cpu_baseline and parity.ok at every N
               if os.path.basename(f) >= "r05" and (len(open(f).read()) > 4096 or "_detail" in f or "dry" in f or "ndjson" in f)]
    assert len(records) >= 3
    for f in records:
        d = json.load(open(f))
        if "legs" not in d and "config3_ndjson_sharded" not in d and "roofline" not in d:
            continue
        text = bench.compact_line(d)
        assert len(text) < 4096 and "\n" not in text, (f, len(text))
        c = _strict(text)
        for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
                    "roofline", "cpu_baseline", "parity"):
            assert key in c, (f, key)
        assert c["value"] == d["value"] and c["ms_per_step"] == d["ms_per_step"] and c["roofline"]["frac"] == d["roofline"]["frac"]
        for key in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
            assert key in c["roofline"], key
        for key in ("value", "unit", "cores", "kind", "sample"):
            assert key in c["cpu_baseline"], key
        assert "workload" in c["config"] and "model" not in c["config"]
        if "legs" in d:
            assert set(c["legs"]) == set(d["legs"]) and c["legs_failed"] == d["legs_failed"]
            for name, leg in c["legs"].items():
                assert len(json.dumps(leg)) < 400, name
            if "config3_amazon_ndjson" in d["legs"]:  # (the mid-round records of round 3 measured a subset of the legs)
                assert c["legs"]["config3_amazon_ndjson"]["frac"] == d["legs"]["config3_amazon_ndjson"]["roofline"]["frac"]
            if "ok" in d.get("legs", {}).get("config3_amazon_ndjson", {}).get("parity", {}):  # (round 3's records say "checked" only: a failure raised)
                assert c["legs"]["config3_amazon_ndjson"]["parity_ok"] is True
    # a record bloated with prose still yields a line under the limit (legs are dropped with a pointer to the side-car before the limit is crossed)
    d = json.load(open(records[-1]))
    fat = json.loads(json.dumps(d).replace("GB/s", "GB/s " + "x" * 300))
    fat.setdefault("legs", {})
    for i in range(40):
        fat["legs"][f"extra_{i}"] = {"ms_per_step": 1.0, "value": 1.0, "pipeline": "p" * 500, "roofline": {"frac": 0.5}}
    assert len(bench.compact_line(fat)) <= 4096


def test_the_committed_printed_line_is_the_compact_one():
    """From round 6 on profiles/rNN_bench_final.json is the line as PRINTED (what the driver parses), rNN_bench_detail.json the side-car of the same run."""
    prof = os.path.join(_paths.REPO_ROOT, "profiles")
    finals = [f for f in sorted(glob.glob(os.path.join(prof, "r*_bench_final.json"))) if os.path.basename(f) >= "r06"]
    for f in finals:
        text = open(f).read().strip()
        assert len(text) < 4096 and "\n" not in text, f
        c = _strict(text)
        det = f.replace("_final", "_detail")
        assert os.path.exists(det), det
        d = json.load(open(det))
        assert c["value"] == d["value"] and c["roofline"]["frac"] == d["roofline"]["frac"] and c["detail"] == "bench_detail.json"


def test_the_committed_bench_line_has_the_contract_s_fields():
    d, path = _final_line()
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
                "roofline", "cpu_baseline"):
        assert key in d, (path, key)
    assert d["n_gpus"] == 1 and d["higher_is_better"] is True and d["scaling"] == "weak" and d["dtype"] == "u8" and d["data"] == "synthetic"
    assert d["vs_baseline"] is None  # BASELINE.md holds no published number for this metric on this part
    assert "workload" in d["config"] and "large_random" in d["config"]["workload"] and "model" not in d["config"]
    base = json.load(open(os.path.join(_paths.REPO_ROOT, "BASELINE.json")))
    assert d["unit"] == "GB/s" and ("stage1" in d["metric"] or "stage 1" in d["metric"]), (d["metric"], base.get("metric"))
    r = d["roofline"]
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic", "traffic_static_from_profiles", "traffic_measured_in_this_run"):
        assert key in r, key
    assert r["traffic_measured_in_this_run"] is False and r["traffic"] == r["traffic_static_from_profiles"]  # a constant from profiles/traffic.json, and the line says so
    assert r["bound"] == "hbm" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 2e-3
    assert 0.3 < r["frac"] < 1.0 and r["traffic"] is not None and r["traffic"] >= 0.98 * r["algorithmic_bytes_per_launch"]
    # value = bytes per GPU / time per step; achieved = algorithmic bytes / GPU time of the step
    assert abs(d["value"] - d["config"]["bytes_per_gpu"] / d["ms_per_step"] / 1e6) / d["value"] < 0.01
    assert abs(r["achieved"] - r["algorithmic_bytes_per_launch"] / r["gpu_ms_per_step"] / 1e6) / r["achieved"] < 0.01
    assert r["gpu_ms_per_step"] <= d["ms_per_step"]
    c = d["cpu_baseline"]
    assert c["kind"] in ("reference", "port") and c["cores"] >= 1 and c["value"] > 0 and c["unit"] == d["unit"] and c["sample"]


def test_the_line_says_how_its_timed_regions_were_reached():
    """Round 4: 40 ms of untimed calls run in front of every timed region (bench.py: clock_warmup -- the first 30-40 calls after an idle phase run slow); the
    line says how many, and the per-call legs carry the figure of the first calls beside the sustained one."""
    d, _ = _final_line()
    assert isinstance(d.get("clock_warmup_calls"), int) and d["clock_warmup_calls"] >= 8
    # round 5: the headline is ALSO timed straight behind the --warmup steps (what a cold `--warmup W --steps K` run gives), beside the sustained figure
    assert d["first_reps_ms_per_step"] > 0 and d["value_first_reps"] > 0 and "clock_warmup" in d["timing"]
    assert abs(d["value_first_reps"] - d["config"]["bytes_per_gpu"] / d["first_reps_ms_per_step"] / 1e6) / d["value_first_reps"] < 0.01
    assert 0.8 < d["value_first_reps"] / d["value"] < 1.1
    assert "large_random" in d["same_workload_at_every_n"]
    for name in ("next_f3_depth_scan", "next_f3_parse_strings"):
        leg = d["legs"][name]
        assert leg["first_reps_ms_per_call"] > 0 and leg["gpu_ms_per_call"] > 0 and "clock_warmup" in leg["timing"], name
    for kind, leg in d["legs"]["next_f3_tape"].items():
        assert leg["first_reps_ms_per_call"] > 0 and leg["gpu_ms_per_call"] > 0, kind


def test_every_leg_is_there_and_none_failed():
    d, _ = _final_line()
    assert d.get("legs_failed") == []
    legs = d["legs"]
    for name in ("config0_twitter_json", "config2_minify", "config2_validate_utf8", "config3_amazon_ndjson", "config4_deep_nesting", "config4_escape_heavy",
                 "plugin_host_path", "next_f2_finish_device", "next_f3_depth_scan", "next_f3_parse_strings", "next_f3_tape"):
        assert name in legs and "error" not in legs[name], name
    for name in ("config2_minify", "config2_validate_utf8", "config3_amazon_ndjson", "config4_deep_nesting", "config4_escape_heavy", "next_f2_finish_device",
                 "next_f3_depth_scan", "next_f3_parse_strings"):
        r = legs[name]["roofline"]
        if r["bound"] == "latency":  # finish(): the boundary search stops at the first hit from the end -- four launches and a wait, no bandwidth to quote
            assert name == "next_f2_finish_device" and r["frac"] is None and legs[name]["ms_per_call"] < 0.2 and r["whole_list_bytes"] > 0
            continue
        assert r["peak"] == 8000.0 and 0 < r["frac"] < 1, name
    for kind, leg in legs["next_f3_tape"].items():
        assert 0 < leg["roofline"]["frac"] < 1 and "word for word" in leg["parity"] and leg["cpu_baseline"]["kind"] == "reference", kind
    assert legs["config3_amazon_ndjson"]["parity"]["checked"] and legs["config2_minify"]["parity"]["checked"]
    win = legs["plugin_host_path"]["parse_many_window_1MB"]
    assert win["mi355x_us_per_window"] < win["reference_us_per_window"] < win["mi355x_us_per_window_unregistered"]


def test_the_plug_in_leg_times_dom_parse_against_the_reference():
    """VERDICT r03 missing #4: dom::parser::parse end to end through both roads of the plug-in, beside the reference, at the sizes that decide
    SJGPU_STAGE2_FROM_KB -- the device road must win from the threshold on and lose below it (that is what a threshold is for)."""
    d, _ = _final_line()
    dp = d["legs"]["plugin_host_path"]["dom_parse"]
    kb = dp["threshold_SJGPU_STAGE2_FROM_KB"]
    sizes = dp["sizes"]
    assert len(sizes) >= 4 and all("error" not in v for v in sizes.values())
    for v in sizes.values():
        b_wins = v["road_b_sjgpu_parse_ms"] < v["road_a_gpu_stage1_plus_reference_stage2_ms"]
        if v["bytes"] >= kb * 1024:
            assert b_wins and v["road_b_sjgpu_parse_ms"] < v["reference_parse_ms"], v
        if v["bytes"] <= kb * 1024 // 3:
            assert not b_wins, v


def test_the_n2_dry_run_line_is_a_measurement():
    """for N > 1 the line carries cpu_baseline, parity (every rank's verdict reduced into it) and roofline like the N = 1
    line, takes the SAME workload as N = 1 (configs[1]: a curve assembled from `--gpus 1,2,4,8` must not jump workloads), carries the same-workload
    single-rank figure measured inside the same run and the efficiency computed from it -- for the top-level workload and for the sharded NDJSON
    (configs[3]) -- and says at top level which road the index concatenation took and how many ranks RCCL saw.  The committed line is bench.py --gpus 2
    launched WITHOUT a launcher (it became one) on a one-GPU box: both ranks on the one device over gloo, so RCCL cannot have seen two ranks -- the line
    must say that, too -- and two ranks sharing one device are worth one: the efficiency of the dry run is near 1/2, which is what makes it a check of
    the arithmetic."""
    path = sorted(glob.glob(os.path.join(_paths.REPO_ROOT, "profiles", "r*_bench_n2_dry_detail.json")))[-1]  # the full record (round 6 on; the printed line beside it)
    d = json.load(open(path))
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and "large_random" in d["config"]["workload"]
    for key in ("roofline", "cpu_baseline", "parity", "config3_ndjson_sharded", "one_document_shards", "index_concat", "n_ranks_seen_by_rccl", "n1_same_workload_GBps",
                "scaling_efficiency", "same_workload_at_every_n", "value_first_reps"):
        assert key in d, key
    assert d["parity"]["checked"] and d["parity"]["all_ranks_ok"] and d["parity"]["ranks_checked"] == 2 and d["parity"]["ranks_ok"] == 2
    assert d["cpu_baseline"]["cores"] == 1 and d["cpu_baseline"]["kind"] == "reference"
    assert 0 < d["roofline"]["frac"] < 1
    assert abs(d["scaling_efficiency"] - d["value"] / (2 * d["n1_same_workload_GBps"])) < 2e-3 and 0.3 < d["scaling_efficiency"] < 0.8
    nd = d["config3_ndjson_sharded"]
    assert "error" not in nd and nd.get("sorted_global_positions") is True and "amazon_ndjson" in nd["workload"]
    assert abs(nd["scaling_efficiency"] - nd["value_GBps"] / (2 * nd["n1_same_workload_GBps"])) < 2e-3
    assert nd["cpu_baseline"]["cores"] == 1 and nd["cpu_baseline_threads"]["cores"] > 1
    assert d["n_ranks_seen_by_rccl"] in (None, 2) and ("sjgpu_comm" in d["index_concat"] or "gather_to_root" in d["index_concat"])


def test_the_ndjson_line_at_one_gpu_is_first_class():
    """`--workload amazon_ndjson` at `--gpus 1` is a headline of its own -- roofline, the reference on one thread AND on all hardware
    threads of the box -- so that a sweep `--gpus 1,2,4,8 --workload amazon_ndjson` is one workload end to end."""
    d = json.load(open(sorted(glob.glob(os.path.join(_paths.REPO_ROOT, "profiles", "r*_bench_ndjson_n1_detail.json")))[-1]))
    assert d["n_gpus"] == 1 and "amazon_ndjson" in d["config"]["workload"] and "amazon_ndjson" in d["same_workload_at_every_n"]
    assert 0.3 < d["roofline"]["frac"] < 1 and d["parity"]["ok"]
    assert d["cpu_baseline"]["cores"] == 1 and d["cpu_baseline_threads"]["cores"] > 1 and d["cpu_baseline_threads"]["value"] > d["cpu_baseline"]["value"]


def test_the_token_stream_s_cost_and_gain_are_in_the_line():
    """Round 5: the token-byte stream out of stage 1 is opt-in because it costs stage 1; the line says how much, and what a list pass fed from it gains."""
    d, _ = _final_line()
    t = d["legs"]["next_f3_depth_scan"]["with_token_stream"]
    assert 0 < t["stage1_cost_of_the_stream"] < 1.0 and t["stage1_split_ms_with_tokens"] > t["stage1_split_ms_without_tokens"]
    assert t["depth_scan_ms_per_call"] < 0.5 * d["legs"]["next_f3_depth_scan"]["gpu_ms_per_call"]
    assert t["roofline"]["frac"] >= 0.30  # what VERDICT r04 asked of the depth scan
    for kind, leg in d["legs"]["next_f3_tape"].items():
        w = leg["with_token_stream"]
        # (round 5: faster with the stream.  Since round 6 the tape's token front stages the document's bytes for numbers and atoms anyway and takes the token
        # bytes from the same window: the stream is accepted and not read -- the same tape in the same time; two timed regions of one run differ by up
        # to 9 % with the clocks they meet: session r06f 1.508 / 1.640 ms, r06e 1.577 / 1.586)
        assert w["stage2_ms_per_call"] < 1.15 * leg["gpu_ms_per_call"] and "word for word" in w["parity"], kind


def _bench():
    import sys
    sys.path.insert(0, _paths.REPO_ROOT)
    import bench
    return bench


def test_the_plain_line_carries_the_headline_alone():
    """A plain run (no --full) measures the headline and nothing else: its line has the contract's headline fields and none of what --full adds."""
    bench = _bench()
    d, _ = _final_line()
    plain = {k: v for k, v in d.items() if k not in ("roofline", "cpu_baseline", "parity", "legs", "legs_failed", "first_reps_ms_per_step", "value_first_reps")}
    c = _strict(bench.compact_line(plain, full=False))
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype", "data", "config"):
        assert c[key] == (d[key] if key != "config" else c[key]), key
    for key in ("roofline", "cpu_baseline", "parity", "detail", "legs", "first_reps_ms_per_step"):
        assert key not in c, key
    assert _strict(bench.compact_line(d)) == _strict(bench.compact_line(d, full=True))


class _FakeParser:
    def __init__(self, n, flags, out_len):
        self.triple = (n, flags, out_len)

    def result(self, stream):
        return self.triple


def test_dumped_outputs_are_float_seeded_and_bounded(tmp_path):
    """--dump-outputs: what the last step returned, as float64 / float32 .npy files under 64 MB in all; a large output is kept as its two ends, a sample at
    seeded positions (the same positions in every run) and a digest of the whole; a small one whole."""
    import numpy as np
    import torch
    from simdjson_amd import capi
    bench = _bench()

    class Cx:
        pass
    cx = Cx()
    cx.torch, cx.capi = torch, capi
    rng = np.random.default_rng(7)
    for count in (1000, bench.DUMP_SAMPLE + 2 * bench.DUMP_EDGE + 12345):
        idx = np.sort(rng.integers(0, 1 << 30, size=count + 16)).astype(np.int32)
        out = torch.from_numpy(idx)
        got = [bench.step_outputs(cx, "stage1", _FakeParser(count - 3, 0, 0), out, 0) for _ in range(2)]
        assert got[0].keys() == got[1].keys() and all(np.array_equal(got[0][k], got[1][k]) for k in got[0])
        res = got[0]
        assert res["result_count"][0] == count - 3 and res["error_code"][0] == 0
        assert sum(a.nbytes for a in res.values()) <= bench.DUMP_LIMIT_BYTES
        limbs = res["structural_indexes_digest"].astype(np.uint64)
        assert int(sum(int(x) << (16 * i) for i, x in enumerate(limbs))) == bench.position_digest_host(idx[:count].astype(np.uint32))
        if "structural_indexes" in res:
            assert np.array_equal(res["structural_indexes"], idx[:count].astype(np.float64))
        else:
            at = res["structural_indexes_sample_at"].astype(np.int64)
            assert len(at) > bench.DUMP_SAMPLE // 2 and at.max() < count and np.all(np.diff(at) > 0)
            assert np.array_equal(res["structural_indexes_sample"], idx[at].astype(np.float64))
            assert np.array_equal(res["structural_indexes_head"], idx[:bench.DUMP_EDGE].astype(np.float64))
            assert np.array_equal(res["structural_indexes_tail"], idx[count - bench.DUMP_EDGE:count].astype(np.float64))
        bench.dump_outputs(str(tmp_path / str(count)), res)
        for name, a in res.items():
            back = np.load(tmp_path / str(count) / (name + ".npy"))
            assert back.dtype in (np.float32, np.float64) and np.array_equal(back, a)
