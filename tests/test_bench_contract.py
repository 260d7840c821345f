"""The bench line's contract (task statement), checked on the committed round-6 lines and on bench.py's
own byte model -- no GPU needed."""
import importlib.util
import json
import os

import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    spec = importlib.util.spec_from_file_location("gs_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_committed_bench_line_has_every_contract_field():
    with open(os.path.join(ROOT, "profiles", "r06_bench_default.json")) as f:
        b = json.load(f)
    with open(os.path.join(ROOT, "BASELINE.json")) as f:
        base = json.load(f)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline", "timed", "parity",
                "frames_per_s_exact", "frames_per_s_fast_blend", "frames_per_s_hw_exp", "completion_interval_ms", "other_configs",
                "sustained_frames_per_s"):
        assert key in b, key
    assert "frame_ms" not in b  # (completion intervals across streams are not a frame time: renamed)
    assert base["metric"].startswith(b["metric"])  # the headline clause of BASELINE.json's metric
    assert b["unit"] == "frames/s" and b["higher_is_better"] is True
    assert b["n_gpus"] == 1 and b["scaling"] == "weak" and b["vs_baseline"] is None and b["data"] == "synthetic"
    assert b["dtype"] == "f32" and "workload" in b["config"] and "model" not in b["config"]
    assert "configs[1]" in b["config"]["workload"]
    helpers.assert_value_is_frames_over_time(b)  # whole-job frames / wall time of the median batch, to 1e-5 (significant digits, not decimals)
    t = b["timed"]
    # every timed frame over every timed second, beside the median batch: the two may not drift apart (round 4: 7 %, a 40 ms stall of the
    # harness's garbage collector in one batch of every run -- profiles/r05_stall_hunt.txt)
    assert abs(b["sustained_frames_per_s"] - b["n_gpus"] * b["steps"] * t["batches"] / t["seconds"]) / b["value"] < 1e-3
    assert abs(b["sustained_frames_per_s"] - b["value"]) / b["value"] <= 0.02 and t["outliers"] == []
    assert t["batches"] >= 1 and t["batch_ms"]["min"] <= t["batch_ms"]["median"] <= t["batch_ms"]["max"]
    # what the warm-up did (verdict r5 item 7): the tuner had settled and the first timed batch is no slower than the rest
    assert t["tuner_settled_before_first_batch"] is True and t["warmup_batches"] >= 4 and t["first_batch_over_median"] <= 1.03
    assert isinstance(t["outliers"], list) and all(ms > 1.5 * t["batch_ms"]["median"] for _, ms in t["outliers"])
    # the headline frac is SURVEY 8d's flop view: it follows from the workload's walked-pair count and the frame time alone
    r = b["roofline"]
    for key in ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "ms_per_frame", "one_in_flight", "valu_issue", "hbm",
                "basis", "walked_pairs"):
        assert key in r, key
    assert r["bound"] == "valu" and r["unit"] == "TFLOP/s" and r["peak"] == 157.3 and r["kernel"].startswith("k_blend<1, false, true>")
    assert abs(r["ms_per_frame"] - b["ms_per_step"]) < 1e-3  # computed on the frame time, not on an overlapped span
    assert abs(r["frac"] - 22 * r["walked_pairs"] / (r["ms_per_frame"] * 1e-3) / 157.3e12) < 1e-3
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3 and 0 < r["frac"] < 1
    v = r["valu_issue"]  # the issue-slot occupancy beside it, labelled for what it is
    if v is not None:
        assert v["peak"] == 1228.8 and v["unit"] == "G wave64-inst/s" and v["wave_insts"] > 1e8 and "own" in v["note"]
        assert abs(v["frac"] - v["wave_insts"] / (r["ms_per_frame"] * 1e-3) / 1228.8e9) < 1e-3   # by division from profiles/
        assert r["traffic"] > 0
    assert r["hbm"]["peak"] == 8000.0 and r["hbm"]["unit"] == "GB/s" and abs(r["hbm"]["frac"] - r["hbm"]["achieved"] / 8000.0) < 1e-3
    # the default is the guarded blend: tolerance met (rounding noise, no pixel beyond 1e-5), then speed; the exact mode beside it
    assert "exp mode 3" in b["config"]["blend"] and b["config"]["blend_guard"]["quadrants"] == 240 * 135
    assert b["config"]["blend_lockstep"]["settled"] is True and b["config"]["blend_lockstep"]["on"] is False  # config B: bound by the pair loop
    p = b["parity"]
    assert "reference text" in p["against"]
    assert p["default"]["max_abs_vs_reference_text"] <= 1e-5 and p["default"]["pixels_above_1e-5"] == 0
    assert p["exact"]["bit_identical"] is True and p["exact"]["max_abs_vs_reference_text"] == 0.0
    assert p["fast"]["max_abs_vs_reference_text"] > 0
    assert b["frames_per_s_exact"] < b["value"]  # (the default's hand-written loop now beats the compiler's unguarded v_exp_f32 form as well)
    c = b["cpu_baseline"]
    for key in ("value", "unit", "cores", "kind", "sample", "one_core", "reference_text"):
        assert key in c, key
    assert c["kind"] in ("reference", "port") and c["cores"] >= 1 and c["unit"] == b["unit"]
    assert c["one_core"]["cores"] == 1 and c["reference_text"]["kind"] == "reference"
    # every reported number carries its measured N, V, D
    for key in ("gaussians", "visible", "instances", "tiles", "bins", "bin_tiles"):
        assert b["config"][key] > 0
    assert set(b["passes"]) == {"preprocess", "prefix_sum", "preprocess_sort", "sort", "tile_boundary", "render"}
    # the other BASELINE configs the one command shows: configs[4] and the trained-like stand-in for configs[2], driver-visible
    o = b["other_configs"]
    for name, marker in (("E", "configs[4]"), ("T", "configs[2]")):
        e = o[name]
        assert marker in e["workload"] and e["frames_per_s"] > 0 and e["gaussians"] == 6_000_000 and e["instances"] > 1e7
        assert set(e["passes_serial_ms"]) >= {"preprocess", "sort", "render", "total"}
        assert e["parity"]["exact_mode_bit_identical"] is True and e["parity"]["default_mode_max_abs"] <= 1e-5
        assert e["frames_per_s_one_in_flight"] > 0 and e["blend_lockstep"]["settled"] is True
    assert o["T"]["blend_lockstep"]["on"] is True  # the trained-like scene: bound by the blend's L1 misses


def test_the_drivers_command_line_holds_no_stall():
    """The line of `python bench.py --gpus 1 --steps 20 --warmup 5` (what the driver runs: ~110 batches of 20 frames) on the round-6 library."""
    with open(os.path.join(ROOT, "profiles", "r06_bench_driver_command.json")) as f:
        b = json.load(f)
    t = b["timed"]
    assert b["steps"] == 20 and b["warmup"] == 5 and t["batches"] >= 50
    assert t["outliers"] == [] and t["batch_ms"]["max"] <= 1.5 * t["batch_ms"]["median"]
    assert abs(b["sustained_frames_per_s"] - b["value"]) / b["value"] <= 0.02
    helpers.assert_value_is_frames_over_time(b)
    # the first timed batch within 3 % of the median (round 5's driver line: 19 % -- the ramp this round's warm-up waits out)
    assert t["first_batch_over_median"] <= 1.03 and t["tuner_settled_before_first_batch"] is True


def test_headline_identity_holds_at_any_rate():
    """`value` and `ms_per_step` are printed to significant digits, so `value == n_gpus * 1e3 / ms_per_step` holds to 1e-5 from
    1 frame/s to millions -- round 5's four fixed decimals broke it above 20 000 frames/s (GPUTEST_r05: red on the fourth of
    254 GPU tests).  The same helper is what the GPU tests of bench.py's CLI and of the two-rank run assert."""
    m = _bench_module()
    for world in (1, 2, 8):
        for steps in (1, 20, 200):
            for fps in (0.37, 3.5, 1000.0, 4450.0, 21120.22, 50_000.0, 200_000.0, 3_333_333.3):
                elapsed = world * steps / fps
                line = dict(m.headline_numbers(world, steps, elapsed), n_gpus=world)
                helpers.assert_value_is_frames_over_time(line)
                assert abs(line["value"] - fps) / fps < 1e-6
    assert m.sig(0.0473482, 7) == 0.0473482 and m.sig(0.04734829999, 4) == 0.04735 and m.sig(None) is None
    # ... and the round-5 form does NOT pass it at the driver's rate (the helper is not vacuous)
    import pytest
    with pytest.raises(AssertionError):
        helpers.assert_value_is_frames_over_time({"value": 21120.22, "ms_per_step": round(1e3 / 21120.22, 4), "n_gpus": 1}, rel=1e-3)


def test_algorithmic_bytes_model():
    m = _bench_module()
    n, v, d, e1, t, p = 1_000_000, 483_640, 4_893_565, 1_082_561, 8160, 1920 * 1080
    assert m.bin_count(1920, 1080, 8) == 15 * 9 and m.bin_count(1920, 1080, 4) == 30 * 17
    assert m.bin_count(3840, 2160, 8) == 30 * 17 and m.bin_count(256, 256, 8) == 4
    g = m.algorithmic_bytes(n, v, d, e1, t, p, 510, bin_local=False)
    b = m.algorithmic_bytes(n, v, d, e1, t, p, 510, bin_local=True)
    assert g["render"] == b["render"] == 40 * d + 16 * p
    assert g["preprocess"] == b["preprocess"] == n * 40 + v * 248
    assert g["sort"] - b["sort"] == 80 * v                      # four global passes over V on the global path only
    assert b["sort"] == 16 * e1 + 4 * d + 8 * t
    assert g["tile_boundary"] == b["tile_boundary"] == 0
    assert b["prefix_sum"] == 4 * n + 8 * v + 3 * 4 * 510 * 977
    assert all(x >= 0 for x in list(g.values()) + list(b.values()))


def test_workload_names_follow_the_arguments():
    m = _bench_module()
    assert "configs[1]" in m.workload_name(1_000_000, 1920, 1080, 1)
    assert "configs[3]" in m.workload_name(1_000_000, 1920, 1080, 8)
    assert "configs[4]" in m.workload_name(6_000_000, 3840, 2160, 1)
    assert "configs[2]" in m.workload_name(6_000_000, 1920, 1080, 1) and "stand-in" in m.workload_name(6_000_000, 1920, 1080, 1)
    assert "not a BASELINE config" in m.workload_name(123, 640, 480, 1)
    t = m.workload_name(6_000_000, 1920, 1080, 1, "T")
    assert "configs[2]" in t and "trained-scene statistics" in t and t.startswith("T(6000000)")


def test_roofline_block_without_counts_is_the_hbm_view(pkg):
    """A workload with neither a committed walked-pair count nor counters: the block falls back to the live HBM view,
    computed on the frame time (spans of frames in flight are not additive)."""
    m = _bench_module()
    r = m.roofline(pkg, "render", m.workload_key(12345, 640, 480, "S"), (3, False), 228_920_200, 0.25, 0.21, 0.30)
    assert r["bound"] == "hbm" and r["traffic"] is None and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert abs(r["achieved"] - 228_920_200 / 1e9 / 0.30e-3) < 1 and abs(r["frac"] - r["achieved"] / 8000.0) < 1e-3
    assert r["one_in_flight"]["ms"] == 0.21 and r["ms_per_frame"] == 0.30 and r["valu_issue"] is None


def test_headline_frac_is_work_not_instructions(pkg):
    """The blend's headline `frac` is SURVEY 8d's flop view -- 22 x the pairs the REFERENCE's loop walks over the frame time
    against 157.3 TFLOP/s -- so it is the same for every blend mode at the same frame time (a kernel that spends more
    instructions cannot raise it), and it falls when the frame gets slower."""
    m = _bench_module()
    wkey = m.workload_key(1_000_000, 1920, 1080, "S")
    work = m.committed_blend_work(wkey)
    assert work and work["walked_pairs"] > 5e8
    fr = {mode: m.roofline(pkg, "render", wkey, mode, 228_920_200, 0.40, 0.24, 0.30) for mode in ((3, False), (2, False), (0, True))}
    for r in fr.values():
        assert r["bound"] == "valu" and r["unit"] == "TFLOP/s" and r["peak"] == 157.3
        assert abs(r["frac"] - 22 * work["walked_pairs"] / 0.30e-3 / 157.3e12) < 1e-3
        assert abs(r["one_in_flight"]["frac"] - 22 * work["walked_pairs"] / 0.24e-3 / 157.3e12) < 1e-3
    slower = m.roofline(pkg, "render", wkey, (3, False), 228_920_200, 0.40, 0.24, 0.36)
    assert slower["frac"] < fr[(3, False)]["frac"]
    assert m.blend_kernel_name((3, False)) == "k_blend<1, false, true>" and m.blend_kernel_name((2, False)) == "k_blend<2, false, false>"
    assert m.blend_kernel_name((0, True)) == "k_blend<0, true, false>" and m.blend_kernel_name((3, True)) == "k_blend<1, true, false>"


def test_committed_counters_belong_to_the_library_as_built(pkg):
    """The newest committed counter run must have been collected from the kernel sources this library is built from
    (bench.py quotes nothing else): a kernel edited after the last profile shows here, on the CPU, before the driver's bench
    line would.  And the `valu_issue` figure must follow from profiles/ by division."""
    m = _bench_module()
    wkey = m.workload_key(1_000_000, 1920, 1080, "S")
    c, why = m.committed_counters(pkg, "render", wkey, (3, False))
    if c is None:  # a kernel was edited since the last counter run: bench.py prints the flop view without valu_issue until it is redone
        import pytest
        pytest.skip(f"stale counters -- re-run tools/profile_lite.sh: {why}")
    assert c["valu_wave_insts"] > 1e8 and c["traffic"] > 5e7 and c["file"].startswith("profiles/r") and c["kernel"] == "k_blend<1, false, true>"
    r = m.roofline(pkg, "render", wkey, (3, False), 228_920_200, 0.40, 0.24, 0.30)
    v = r["valu_issue"]
    assert r["counters"] == c["file"] and v["peak"] == 1228.8
    assert abs(v["frac"] - c["valu_wave_insts"] / 0.30e-3 / m.VALU_PEAK) < 1e-3          # per frame time
    assert abs(v["one_in_flight_frac"] - c["valu_wave_insts"] / 0.24e-3 / m.VALU_PEAK) < 1e-3


def test_rocprof_summary_agrees_with_the_bench_line():
    """The contract: `roofline.achieved` comes from the dominant kernel's launch duration measured live inside bench.py, and the committed
    `rocprofv3 --kernel-trace --stats` summary's average for that kernel must agree.  The live figure is the kernels' own stamps (blend start
    to frame end); the summary is profiles/r06_kernel_stats_B_serial.txt (one frame at a time, the same library)."""
    import re
    with open(os.path.join(ROOT, "profiles", "r06_bench_default.json")) as f:
        b = json.load(f)
    r = b["roofline"]
    live_ms = r["one_in_flight"]["ms"]
    avg_us = None
    with open(os.path.join(ROOT, "profiles", "r06_kernel_stats_B_serial.txt")) as f:
        for line in f:
            if line.startswith(r["kernel"]):
                avg_us = float(re.split(r"\s{2,}", line.strip())[3])
    assert avg_us is not None, r["kernel"]
    assert abs(live_ms * 1e3 - avg_us) / avg_us < 0.03, (live_ms, avg_us)
    # ... and the flop view follows from that duration and the committed pair count alone
    assert abs(r["one_in_flight"]["frac"] - 22 * r["walked_pairs"] / (live_ms * 1e-3) / 157.3e12) < 2e-3
    assert abs(b["passes_serial_ms"]["render"] - live_ms) < 1e-3


def test_dump_outputs_writes_float32_within_budget_and_samples_the_same_way(tmp_path):
    """--dump-outputs: every array as <name><suffix>.npy in float32; beyond the budget, a fixed, seeded sample of each array
    (its share of the budget by size) -- the same elements on every run, so that two builds can be compared output for output."""
    import numpy as np
    m = _bench_module()
    rng = np.random.default_rng(5)
    img = np.arange(90 * 160 * 4, dtype=np.float32).reshape(90, 160, 4)  # element k holds k: the sample shows which it took
    img8 = rng.integers(0, 256, (90, 160, 4), dtype=np.uint8)
    m.dump_outputs(str(tmp_path / "whole"), {"image": img, "image_bgra8": img8}, "", 10 ** 6)
    got = np.load(tmp_path / "whole" / "image.npy")
    assert got.dtype == np.float32 and np.array_equal(got, img)
    got8 = np.load(tmp_path / "whole" / "image_bgra8.npy")
    assert got8.dtype == np.float32 and np.array_equal(got8, img8.astype(np.float32))
    budget = 100_000
    for run in ("a", "b"):
        m.dump_outputs(str(tmp_path / run), {"image": img, "image_bgra8": img8}, "_rank1", budget)
    sizes = 0
    for name in ("image_rank1.npy", "image_bgra8_rank1.npy"):
        a, b = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert a.dtype == np.float32 and a.ndim == 1 and np.array_equal(a, b)
        sizes += a.nbytes
    assert 0.99 * budget <= sizes <= budget
    sample = np.load(tmp_path / "a" / "image_rank1.npy")
    assert sample[0] >= 0 and sample[-1] < img.size and (np.diff(sample) > 0).all()  # distinct elements, in their order
