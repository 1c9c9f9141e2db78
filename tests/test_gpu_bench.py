"""bench.py on the GPU box, small: the line survives without rocprofv3 (event-timed roofline, `pmc: null` with the reason), and both N > 1 hosts run their whole
code path on one GPU — two torch.distributed ranks (gloo, IDKPT_BENCH_ONE_DEVICE=1: RCCL refuses two ranks on one device) and one two-member context — with the
sharded, exchanged frame equal to one device's bit for bit and the transport reported at the top level of the line (all of that with --full).  A plain run times
exactly --steps steps once, carries none of the --full measurements, and its --dump-outputs image is the frame a fresh context renders from the same samples."""
import json
import os
import subprocess
import sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
SMALL = ["--full", "--steps", "6", "--warmup", "3", "--repeats", "2", "--tris", "30000", "--width", "480", "--height", "270", "--batch", "3", "--no-extras", "--no-cpu-baseline"]
PLAIN = ["--steps", "8", "--warmup", "3", "--tris", "30000", "--width", "480", "--height", "270", "--batch", "3"]


def _line(cmd, env=None, timeout=600):
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=timeout, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-1500:]
    return json.loads(lines[0])


def test_line_survives_without_rocprofv3():
    d = _line([sys.executable, "bench.py"] + SMALL, env={"IDKPT_BENCH_ROCPROFV3": "/nonexistent/rocprofv3"})
    assert d["value"] > 0 and d["n_gpus"] == 1 and d["steps"] == 6
    rf = d["roofline"]
    assert rf["pmc"] is None and "rocprofv3" in rf["pmc_reason"] and rf["traffic"] is None
    assert rf["achieved"] > 0 and 0 < rf["frac"] < 1 and rf["avg_launch_us"] > 0          # from HIP events alone
    assert d["transport"].startswith("none") and d["rccl_ranks_seen"] is None


def test_two_ranks_on_one_gpu_run_the_whole_n_gpu_path():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29631", "bench.py", "--gpus", "2"] + SMALL + ["--no-pmc"]
    d = _line(cmd, env={"IDKPT_BENCH_ONE_DEVICE": "1"})
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["ranks"] == 2
    assert "gloo" in d["transport"] and d["rccl_ranks_seen"] is None                        # said, not hidden: this was a control-flow check on one GPU
    ng = d["config"]["n_gpu"]
    assert ng["members_share_gpus"] and ng["ranks"]["ranks_counted_by_all_reduce"] == 2
    assert ng["selftest"]["bits_equal"] is True


def test_one_context_on_two_members_reports_its_transport():
    d = _line([sys.executable, "bench.py", "--gpus", "2"] + SMALL + ["--no-pmc"])
    assert d["n_gpus"] == 2 and d["ranks"] == 2
    assert d["transport"].startswith("peer-copy") and "share GPU" in d["transport"] and d["rccl_ranks_seen"] is None
    assert d["config"]["n_gpu"]["selftest"]["bits_equal"] is True


def test_plain_run_is_lean_and_dumps_the_last_frame(tmp_path):
    import numpy as np
    sys.path.insert(0, ROOT)
    from idkengine_amd import scenes as S
    from idkengine_amd.bvh import NativeBuilder
    from idkengine_amd.pathtracer import PathTracer
    out = tmp_path / "outputs"
    d = _line([sys.executable, "bench.py"] + PLAIN + ["--dump-outputs", str(out)])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["value"] > 0 and d["steps"] == 8 and d["repeats"] == 1 and len(d["repeat_ms"]) == 1
    assert abs(d["ms_per_step"] * 8 - d["repeat_ms"][0]) <= 0.01 * d["repeat_ms"][0] + 1e-3   # one region of exactly --steps steps
    for k in ("roofline", "traversed_mray_s", "single_frame", "cpu_baseline", "eager_last_bounce"):
        assert k not in d, k                                                                 # --full only
    assert d["outputs"]["files"] == ["image.npy"]
    img = np.load(out / "image.npy")
    assert img.dtype == np.float32 and img.shape == (270, 480, 4) and np.isfinite(img).all()
    # 8 steps in displayed frames of 3 samples: the last frame holds samples 0 and 1 of a restarted accumulation
    pt = PathTracer(480, 270)
    pt.UploadScene(S.soup_scene(30000, NativeBuilder(), seed=1)); pt.SetCamera(S.Camera(480, 270))
    pt.RayDepth = 2; pt.SamplesPerPixel = 1; pt.DoRaySorting = 0; pt.set_max_batch(3)
    pt.ResetAccumulation(); pt.Compute(); pt.Compute()
    want = pt.Result
    pt.Dispose()
    assert img.tobytes() == want.tobytes()
