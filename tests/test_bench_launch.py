"""CPU: `python bench.py --gpus N` with WORLD_SIZE unset starts its N ranks itself (BASELINE's metric is quoted at
1/2/4/8 GPUs; the plain command must not silently run one rank).  Driven in --plan-only mode: the ranks rendezvous over
gloo on 127.0.0.1, count themselves with an all-reduce of ones and rank 0 prints the line's skeleton."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None, timeout=180):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True,
                          timeout=timeout)


def _line(stdout):
    lines = [ln for ln in stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, stdout                      # ONE JSON line, from rank 0 only
    return json.loads(lines[0])


def test_plain_command_spawns_its_ranks():
    r = _run(["--gpus", "2", "--plan-only"])
    assert r.returncode == 0, r.stderr[-2000:]
    line = _line(r.stdout)
    assert line["n_gpus"] == 2 and line["ranks_seen"] == 2 and line["shards"] == [64, 64]


def test_three_ranks_and_equals_form():
    r = _run(["--gpus=3", "--plan-only"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert _line(r.stdout)["ranks_seen"] == 3


def test_mismatch_with_a_launcher_environment_fails_loudly():
    """under torchrun (WORLD_SIZE set) a --gpus that disagrees is an error, never a line with the wrong n_gpus."""
    r = _run(["--gpus", "2", "--plan-only"], {"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "{" not in r.stdout


def test_a_failing_rank_fails_the_launcher():
    r = _run(["--gpus", "2", "--plan-only", "--no-such-flag"])
    assert r.returncode != 0 and "{" not in r.stdout


def test_single_rank_needs_no_launcher():
    r = _run(["--gpus", "1", "--plan-only"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert _line(r.stdout)["n_gpus"] == 1


def test_zero_timed_steps_is_refused():
    r = _run(["--gpus", "1", "--steps", "0", "--plan-only"])
    assert r.returncode != 0 and "{" not in r.stdout


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_keeps_small_arrays_and_samples_large_ones_the_same_way(tmp_path):
    import numpy as np
    bench = _bench_module()
    a = np.arange(100_000, dtype=np.float32).reshape(4, -1)
    budget = 2 * (4096 + 40_000)                           # two arrays: 40 000 bytes of data each
    for d in ("one", "two"):
        bench.dump_outputs(str(tmp_path / d), {"small": a[:1, :10].astype(np.float64), "big": a}, budget)
    small = np.load(tmp_path / "one" / "small.npy")
    assert small.dtype == np.float64 and np.array_equal(small, a[:1, :10])
    big = np.load(tmp_path / "one" / "big.npy")
    assert big.dtype == np.float32 and big.nbytes == 40_000
    assert np.all(np.diff(big) > 0)                        # distinct elements of the flat array, in order
    assert np.array_equal(big, np.load(tmp_path / "two" / "big.npy"))
    assert sum(os.path.getsize(tmp_path / "one" / f) for f in os.listdir(tmp_path / "one")) <= budget


import pytest


@pytest.mark.gpu
def test_dumped_outputs_are_the_headline_decode_and_repeat(tmp_path):
    """--dump-outputs writes the samples the last timed step decoded: the CPU oracle's decode of the same seeded weights,
    features and noise, and bit-identical from one run to the next."""
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from oracle import cpu_ref
    from shallow_wavenet_amd import config as C
    from shallow_wavenet_amd.synth import synth_aux, synth_state_dict
    frames = 3                                             # the span the other BL6 decode tests hold to 1e-5 of the oracle
    dumps = []
    for d in ("a", "b"):
        r = _run(["--gpus", "1", "--steps", "2", "--warmup", "1", "--frames", str(frames), "--no-legs", "--no-cfg5",
                  "--no-cpu-baseline", "--detail", "", "--dump-outputs", str(tmp_path / d)], timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        assert _line(r.stdout)["steps"] == 2
        dumps.append(np.load(tmp_path / d / "samples.npy"))
    cfg = C.bl6_laplace(1, 0)
    n = frames * cfg.U
    assert dumps[0].dtype == np.float32 and dumps[0].shape == (1, n)
    assert np.array_equal(dumps[0], dumps[1])
    P = cpu_ref.as_params(synth_state_dict(cfg, seed=1, flavor="trained", identity_scale_in=True))
    noise = cpu_ref.laplace_noise(cfg, n, 1, generator=torch.Generator().manual_seed(1))
    ref = cpu_ref.laplace_generate(cfg, P, torch.from_numpy(synth_aux(cfg, 1, frames, seed=1)), [n], noise)[0]
    assert float(np.abs(dumps[0][0] - ref).max()) <= 1e-5


@pytest.mark.gpu
def test_two_rank_bench_rehearsal_on_one_gpu():
    """the whole N > 1 path of bench.py as the plain command runs it - self-launch, torchrun environment, packed-weight
    broadcast, per-rank decode, cfg5 leg on every rank, barrier + max over ranks, ONE line from rank 0 - with two ranks sharing
    the box's GPU (gloo instead of RCCL: the line says so; it is not a scaling measurement)."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "1", "--frames", "20", "--no-cpu-baseline"], timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = _line(r.stdout)
    assert line["n_gpus"] == 2 and line["ranks_seen"] == 2 and line["scaling"] == "weak"
    assert line["value"] > 0 and "cfg5" in line["legs"] and line["legs"]["cfg5"]["value"] > 0
    if torch.cuda.device_count() < 2:
        assert "rehearsal" in line
