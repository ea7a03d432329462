"""bench.py --dump-outputs: the last timed step's streams as .npy files (a fixed, seeded sample under 64 MB), and a
result line whose step count and ms_per_step describe the timed region.  The CPU test pins the file format; the
-m gpu tests run the bench at a small size, plain and with --full, and check the dump against the oracle's streams
of the same frames."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _streams(n, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, int(rng.integers(1, 3000)), dtype=np.uint8) for _ in range(n)]


def test_dump_outputs_format_and_determinism(tmp_path):
    outs = _streams(5, 3)
    outs.append(np.zeros(16, np.uint8))                                  # an empty stream in a larger buffer
    lens = [len(o) for o in outs[:-1]] + [0]
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), lens, outs)
    bench.dump_outputs(str(b), lens, [o.copy() for o in outs])
    got_len, got = np.load(a / "stream_lengths.npy"), np.load(a / "stream_bytes.npy")
    assert got_len.dtype == np.float64 and got_len.tolist() == lens
    assert got.dtype == np.float32 and got.shape == (6, 8192)
    for name in ("stream_lengths.npy", "stream_bytes.npy"):
        assert (a / name).read_bytes() == (b / name).read_bytes()
    for k in range(5):
        assert got[k, 0] == outs[k][0] and got[k, -1] == outs[k][lens[k] - 1]
        assert set(got[k].astype(np.uint8).tolist()) <= set(outs[k].tolist())
    assert not got[5].any()
    changed = [o.copy() for o in outs]
    changed[2][lens[2] // 2:] ^= 0xFF                                    # a stream that differs from its middle on
    bench.dump_outputs(str(b), lens, changed)
    assert not np.array_equal(np.load(b / "stream_bytes.npy")[2], got[2])


def test_dump_outputs_stays_under_budget(tmp_path):
    n = 4096
    bench.dump_outputs(str(tmp_path), [7] * n, [np.arange(7, dtype=np.uint8)] * n)
    total = sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path))
    assert total <= bench.DUMP_BUDGET and np.load(tmp_path / "stream_bytes.npy").shape[0] == n


@pytest.mark.gpu
def test_bench_steps_and_dumped_streams(pkg, oracle, tmp_path):
    """Three timed steps of four 512x512 frames: the line reports those steps and their time, and the dump is the
    oracle's streams of the same seeded frames, sampled the same way."""
    steps, batch, h, w = 3, 4, 512, 512
    dump = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                        "--batch", str(batch), "--height", str(h), "--width", str(w), "--full", "--no-extra-legs", "--no-cpu-baseline",
                        "--dump-outputs", str(dump)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == steps and line["bit_exact"] is True, line
    assert line["ms_per_step"] > 0 and line["bit_exact_checks"]["every_step_same_lengths"] is True
    streams = [np.frombuffer(oracle.encode(pkg.syn1(h, w, seed=k + 1), 0, 1)[0], np.uint8) for k in range(batch)]
    want = tmp_path / "want"
    bench.dump_outputs(str(want), [len(s) for s in streams], streams)
    for name in ("stream_lengths.npy", "stream_bytes.npy"):
        assert np.array_equal(np.load(dump / name), np.load(want / name)), name


@pytest.mark.gpu
def test_plain_bench_runs_only_the_headline(pkg, oracle, tmp_path):
    """Without --full the bench sets up, warms up, times its steps, dumps and prints the line, and nothing else: the
    line's value and ms_per_step describe the timed steps, it carries no checks, CPU baseline or extra legs, and the
    dump is still the oracle's streams of the same seeded frames."""
    steps, batch, h, w = 2, 3, 256, 384
    dump = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                        "--batch", str(batch), "--height", str(h), "--width", str(w), "--dump-outputs", str(dump)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == steps and line["warmup"] == 1 and line["ms_per_step"] > 0, line
    assert line["unit"] == "Mpixel/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    assert line["value"] == pytest.approx(batch * h * w / (line["ms_per_step"] * 1e-3) / 1e6, rel=1e-3)
    for moved in ("bit_exact", "bit_exact_checks", "gathered_ok", "cpu_baseline", "batch8_Mpixel_per_s", "single_frame_ms",
                  "value_h2d_inclusive"):
        assert moved not in line, moved
    streams = [np.frombuffer(oracle.encode(pkg.syn1(h, w, seed=k + 1), 0, 1)[0], np.uint8) for k in range(batch)]
    want = tmp_path / "want"
    bench.dump_outputs(str(want), [len(s) for s in streams], streams)
    for name in ("stream_lengths.npy", "stream_bytes.npy"):
        assert np.array_equal(np.load(dump / name), np.load(want / name)), name
