"""bench.py's launch path on a GPU-less machine: `--gpus N` starts its own N ranks (torch.distributed.run, 127.0.0.1),
they rendezvous (gloo in --dry-run), run the barrier-bracketed timing loop and rank 0 prints ONE JSON line.
The hot path itself never runs here (it has no CPU fallback); on hardware the same code path uses RCCL."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*extra, env=None):
    e = dict(os.environ)
    e.pop("WORLD_SIZE", None); e.pop("RANK", None); e.pop("LOCAL_RANK", None)
    e.update(env or {})
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--dry-run", "--steps", "4", "--warmup", "1", *extra],
                       capture_output=True, text=True, timeout=240, env=e)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    return r, lines


@pytest.mark.parametrize("mode", ["sample", "train", "guided"])
def test_bench_starts_its_own_ranks(mode):
    r, lines = _run("--gpus", "2", "--mode", mode)
    assert r.returncode == 0, r.stderr[-2000:]
    assert len(lines) == 1, r.stdout                      # rank 0 only
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["gloo_ranks"] == 2 and out["steps"] == 4 and out["warmup"] == 1 and out["dry_run"] is True and out["mode"] == mode
    if mode == "train":
        # what the real run builds before its first step: the product MDM under make_ddp, prepared for the captured step (the default at
        # every world size: unused parameters frozen, no unused-parameter search)
        assert out["parameters"] == 29_607_012 and out["graph_replayed"] is True
        assert out["ddp"]["find_unused_parameters"] is False and out["ddp"]["frozen"] == ["embed_style.bias", "embed_style.weight"]
        assert out["ddp"]["bucket_cap_mb"] == 32
    if mode == "guided":
        # BASELINE configs[3]: cond + uncond = 2 variants; configs[4]: the body-part wrapper's 9 evaluations de-duplicate to 4
        assert out["plans"]["cfg"]["variants"] == 2 and out["plans"]["bodypart_twocfg"]["variants"] == 4
        for plan in out["plans"].values():
            assert all(abs(sum(row) - 1.0) < 1e-6 for row in plan["weights"])          # a guidance formula's weights sum to 1 per block


@pytest.mark.parametrize("mode", ["sample", "train", "guided"])
def test_bench_dry_run_with_eight_ranks(mode):
    """What the driver launches on an 8-GPU node (`--gpus 8`, one rank per GPU) has never run on hardware: its launch path - eight ranks, rendezvous,
    barriers, the model and its DDP wrapper in train mode, ONE JSON line from rank 0 - must at least not fail for a trivial reason."""
    r, lines = _run("--gpus", "8", "--mode", mode)
    assert r.returncode == 0, r.stderr[-2000:]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 8 and out["gloo_ranks"] == 8 and out["dry_run"] is True and out["mode"] == mode
    if mode == "train":
        assert out["graph_replayed"] is True and out["ddp"]["find_unused_parameters"] is False and out["clips_per_gpu"] == 32


def test_capture_failure_on_any_rank_sends_every_rank_to_the_eager_step():
    """bench.capture_or_fallback: a capture that raises on one rank of a multi-rank job (or on none, while another rank's did) leaves EVERY rank
    without a captured step and with a reason for the JSON line's `graph_fallback`; with one rank the exception propagates."""
    import importlib.util
    import torch
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(REPO, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)

    class Dist:                                             # the MIN all-reduce of a 2-rank job whose other rank reports `other`
        class ReduceOp:
            MIN = "min"

        def __init__(self, other):
            self.other = other

        def all_reduce(self, t, op=None):
            t.fill_(min(int(t), self.other))

    class Step:
        closed = False

        def close(self):
            self.closed = True

    def boom():
        raise RuntimeError("hipErrorStreamCaptureInvalidated")
    g, why = bench.capture_or_fallback(boom, 2, Dist(1), lambda: None, "cpu")
    assert g is None and "hipErrorStreamCaptureInvalidated" in why
    mine = Step()
    g, why = bench.capture_or_fallback(lambda: mine, 2, Dist(0), lambda: None, "cpu")            # this rank captured, the other did not
    assert g is None and mine.closed and "another rank" in why
    g, why = bench.capture_or_fallback(lambda: mine, 2, Dist(1), lambda: None, "cpu")
    assert g is mine and why is None
    with pytest.raises(RuntimeError):
        bench.capture_or_fallback(boom, 1, None, lambda: None, "cpu")
    g, why = bench.capture_or_fallback(boom, 1, None, lambda: None, "cpu", force=True)
    assert g is None and why.startswith("RuntimeError")


def test_bench_train_dry_run_with_the_eager_step_wiring():
    """--no-train-graph with several ranks: the eager step, the wrapper searches for unused parameters (nothing frozen)."""
    r, lines = _run("--gpus", "2", "--mode", "train", "--no-train-graph")
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(lines[0])
    assert out["graph_replayed"] is False and out["ddp"]["find_unused_parameters"] is True and out["ddp"]["frozen"] == []


def test_bench_force_ddp_on_one_rank():
    """--force-ddp: one rank still builds the process group and the wrapper (what the driver's 1-GPU box times)."""
    r, lines = _run("--mode", "train", "--force-ddp")
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 1 and out["gloo_ranks"] == 1 and out["graph_replayed"] is True
    assert out["ddp"]["find_unused_parameters"] is False and out["ddp"]["frozen"] == ["embed_style.bias", "embed_style.weight"]


def test_bench_single_rank_and_launcher_mismatch():
    r, lines = _run()
    assert r.returncode == 0 and json.loads(lines[0])["n_gpus"] == 1
    # under an external launcher that started a different number of ranks the script refuses instead of mis-reporting
    r, lines = _run("--gpus", "4", env={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE=1" in r.stderr


def test_bench_refuses_to_run_the_hot_path_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    e = dict(os.environ); e.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--steps", "1"], capture_output=True, text=True, timeout=240, env=e)
    assert r.returncode != 0 and "no GPU visible" in r.stderr


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(REPO, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_dump_outputs_keeps_a_fixed_row_sample_under_64_mb(tmp_path):
    """--dump-outputs: float32 .npy files, at most 64 MB in all; an output larger than its share keeps the same seeded rows on every call,
    a small one is written whole."""
    import numpy as np
    import torch
    bench = _bench_module()
    x = torch.randn(1024, 1536, 1, 32)                                    # the headline's latent: 201 MB in float32
    a, b = tmp_path / "a", tmp_path / "b"
    ia, ib = bench.dump_outputs(str(a), {"x": x}, 0, 1), bench.dump_outputs(str(b), {"x": x.clone()}, 0, 1)
    assert ia == ib and ia["x"]["shape"][1:] == [1536, 1, 32] and 1 < ia["x"]["shape"][0] < 1024
    xa = np.load(a / "x.npy")
    assert xa.dtype == np.float32 and np.array_equal(xa, np.load(b / "x.npy")) and os.path.getsize(a / "x.npy") <= bench.DUMP_BYTES
    rows = [i for i in range(1024) if any(np.array_equal(x[i].numpy(), r) for r in xa[:3])]
    assert len(rows) == 3 and rows == sorted(rows)                           # rows of the input, in index order
    c = tmp_path / "c"
    info = bench.dump_outputs(str(c), {"loss": torch.tensor(0.25, dtype=torch.float64), "params": torch.randn(29_607_012)}, 0, 1)
    assert info["loss"]["rows"] == "all" and np.load(c / "loss.npy").tolist() == [0.25]
    assert sum(os.path.getsize(c / f) for f in os.listdir(c)) <= bench.DUMP_BYTES
    d = tmp_path / "d"
    bench.dump_outputs(str(d), {"x": torch.randn(8, 1536, 1, 32)}, 1, 2)   # rank 1 of 2: its own file, half the budget
    assert os.listdir(d) == ["x_rank1.npy"] and np.load(d / "x_rank1.npy").shape == (8, 1536, 1, 32)


@pytest.mark.gpu
def test_bench_dump_outputs_repeat_from_run_to_run(tmp_path):
    """Two runs with the same arguments: `steps` timed steps (12: ten-step replays and single-step ones), `ms_per_step` on the line, and the same
    latent after the last timed step, bit for bit."""
    import numpy as np
    got = []
    for k in range(2):
        d = tmp_path / f"run{k}"
        e = dict(os.environ); e.pop("WORLD_SIZE", None)
        r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "12", "--warmup", "2", "--batch", "64", "--no-extras",
                            "--no-cpu", "--no-small-batch", "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600, env=e)
        assert r.returncode == 0, r.stderr[-2000:]
        out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        assert out["steps"] == 12 and out["ms_per_step"] > 0 and len(out["roofline"]["timed_region_replays_ms_per_step"]) == 3
        assert out["dumped_outputs"]["files"]["x"] == {"shape": [64, 1536, 1, 32], "rows": "all"}
        got.append(np.load(d / "x.npy"))
    assert got[0].dtype == np.float32 and np.isfinite(got[0]).all() and np.array_equal(got[0], got[1])


@pytest.mark.gpu
def test_plain_run_carries_the_headline_and_full_run_the_rest():
    """A plain run times the headline workload and nothing else: no CPU baseline, other configuration, probe or second measurement on its line.
    `--full` adds them (here without the train / guided sub-objects and the practical peak: --no-extras)."""
    def line(*extra):
        e = dict(os.environ); e.pop("WORLD_SIZE", None)
        r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "12", "--warmup", "2", "--batch", "64", *extra],
                           capture_output=True, text=True, timeout=600, env=e)
        assert r.returncode == 0, r.stderr[-2000:]
        return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    plain = line()
    assert plain["metric"] == "denoising-steps/sec (128-frame clips)" and plain["unit"] == "clip-steps/s" and plain["higher_is_better"] is True
    assert plain["dtype"] == "bf16" and plain["steps"] == 12 and plain["ms_per_step"] > 0 and plain["value"] > 0
    assert not {"cpu_baseline", "small_batch", "steady_state", "train_step", "train_step_ddp_1rank", "guided"} & set(plain)
    assert "eager_stage_ms_per_step" not in plain["roofline"] and "practical_peak" not in plain["roofline"]
    assert plain["roofline"]["kernel"] and plain["roofline"]["frac"] > 0 and len(plain["roofline"]["timed_region_replays_ms_per_step"]) == 3
    full = line("--full", "--no-extras", "--cpu-seconds", "0.3")
    assert full["cpu_baseline"]["value"] > 0 and full["small_batch"]["us_per_step"] and full["steady_state"]["ms_per_step"] > 0
    assert full["roofline"]["eager_stage_ms_per_step"] and full["roofline"]["launches_per_step"] >= 1
    assert full["roofline"]["kernel"] == plain["roofline"]["kernel"]


def test_bench_dry_run_takes_full():
    r, lines = _run("--full")
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(lines[0])["dry_run"] is True
