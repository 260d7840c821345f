"""bench.py's command-line paths that the default run does not take, on small workloads (the default run is the driver's)."""
import json
import os
import subprocess
import sys

import pytest

import helpers

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, env=None, timeout=500):
    e = dict(os.environ)
    e.pop("GS_SORT_PATH", None)
    e.pop("GS_EXP_MODE", None)  # bench.py sets the blend's modes itself
    e.update(env or {})
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=timeout, env=e, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:] + out.stdout[-500:]
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])


def test_bench_takes_a_ply(pkg, gpu, tmp_path, _sort_path):
    """BASELINE configs[2] is a trained scene's PLY (none ships with the reference or this container): `--ply FILE` and
    GS_SCENE=FILE bench whatever file is given -- GSScene::load on rank 0, the same file through the checker's own reader for the
    CPU baseline and the parity block."""
    if _sort_path == "1":
        pytest.skip("independent of the depth-order path: runs once")
    n = 30_000
    ply = str(tmp_path / "scene.ply")
    pkg.synth.write_ply(ply, pkg.synth.synth_records(n, seed=7, kind="T"))
    common = ["--width", "640", "--height", "360", "--steps", "20", "--warmup", "5", "--full"]
    for args, env in ((["--ply", ply], None), ([], {"GS_SCENE": ply})):
        b = _bench(args + common, env={"GS_CPU_BASELINE_SECONDS": "1", **(env or {})})
        assert b["config"]["scene"] == "ply" and b["config"]["gaussians"] == n and "scene.ply" in b["config"]["workload"]
        assert "configs[2]" in b["config"]["workload"] and "other_configs" not in b
        helpers.assert_value_is_frames_over_time(b)
        p = b["parity"]
        assert p["default"]["max_abs_vs_reference_text"] <= 1e-5 and p["default"]["pixels_above_1e-5"] == 0
        assert p["exact"]["bit_identical"] is True
        assert b["cpu_baseline"]["value"] > 0 and f"N={n}" in b["cpu_baseline"]["sample"]
        assert b["roofline"]["bound"] in ("hbm", "valu")  # (no committed pair count for this workload: the HBM view)


def test_bench_modes_and_other_configs_switch(pkg, gpu, _sort_path):
    """--exact benches the bit-identical blend (its own frames/s becomes `value`, the default mode's appears beside it);
    `other_configs` belongs to the headline workload only."""
    if _sort_path == "1":
        pytest.skip("independent of the depth-order path: runs once")
    b = _bench(["--gaussians", "40000", "--width", "640", "--height", "360", "--steps", "20", "--warmup", "5", "--exact", "--no-cpu-baseline",
                "--full"])
    assert "exp mode 2" in b["config"]["blend"] and b["frames_per_s_exact"] is None and b["frames_per_s_default"] > 0
    assert "other_configs" not in b and "cpu_baseline" not in b and "parity" not in b
    assert b["roofline"]["kernel"] in ("k_blend<2, false, false>", "k_preprocess") and b["timed"]["outliers"] is not None


FULL_ONLY = ("roofline", "cpu_baseline", "parity", "other_configs", "rccl", "passes_serial_ms", "frames_per_s_one_in_flight",
             "frames_per_s_default", "frames_per_s_exact", "frames_per_s_fast_blend", "frames_per_s_hw_exp")


def test_plain_run_times_k_steps_and_dumps_the_last_frame(pkg, oracle, gpu, tmp_path, _sort_path):
    """A plain run (no --full) is the headline alone: it times exactly the K steps of --steps once, prints the contract fields and
    none of the diagnostics, and --dump-outputs writes the frame of the last timed step -- the checker's frame bit for bit in the
    exact mode, and the same bits on every run with the same arguments in the default mode."""
    import numpy as np
    if _sort_path == "1":
        pytest.skip("independent of the depth-order path: runs once")
    n, w, h = 40_000, 640, 360
    common = ["--gaussians", str(n), "--width", str(w), "--height", str(h), "--steps", "7", "--warmup", "3"]
    lines = {}
    for tag, extra in (("exact", ["--exact"]), ("default_1", []), ("default_2", [])):
        b = lines[tag] = _bench(common + extra + ["--dump-outputs", str(tmp_path / tag)])
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert key in b, key
        assert b["unit"] == "frames/s" and b["higher_is_better"] is True and b["dtype"] == "f32"
        assert b["steps"] == 7 and b["warmup"] == 3 and b["timed"]["batches"] == 1
        assert abs(b["timed"]["seconds"] - 7 * b["ms_per_step"] * 1e-3) <= 1e-6  # (seconds: 6 decimals)
        assert not [k for k in FULL_ONLY if k in b] and "blend_guard" not in b["config"]
        helpers.assert_value_is_frames_over_time(b)
        assert sorted(os.listdir(tmp_path / tag)) == ["image.npy"]
    assert "exp mode 2" in lines["exact"]["config"]["blend"] and "exp mode 3" in lines["default_1"]["config"]["blend"]
    exact = np.load(tmp_path / "exact" / "image.npy")
    assert exact.dtype == np.float32 and exact.shape == (h, w, 4)
    verts = oracle.activate_records(pkg.synth.synth_records(n, seed=0, kind="S"))
    ref = oracle.stages(verts, oracle.camera_uniforms(oracle.default_camera(rotation=pkg.dist.pose_quaternion(0)), w, h))
    helpers.assert_images_identical(exact, ref["image"], label="bench --dump-outputs, exact mode, vs the checker")
    d1, d2 = (np.load(tmp_path / t / "image.npy") for t in ("default_1", "default_2"))
    np.testing.assert_array_equal(d1.view(np.uint32), d2.view(np.uint32))
    assert float(np.abs(d1[..., :3].astype(np.float64) - ref["image"][..., :3]).max()) <= helpers.GUARD_TOL
