"""bench.py's plain run, --full and --dump-outputs: a plain run selects the headline alone,
the legs need --full, and the dumped arrays are the decoded chunks and statuses of the last
timed step (float32 / float64, at most 64 MB, the same from run to run)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402

LEGS = ("f2", "copy_ceiling", "e2e", "cfg3", "lz4", "bshuf", "cfg1", "zstd", "cfg5", "cfg5w", "cfg4", "cfg4_full")


def test_plain_run_selects_the_headline_alone():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert a.steps == 7 and a.warmup == 3 and not a.full and a.dump_outputs is None
    assert all(getattr(a, leg) == 0 for leg in LEGS) and a.cpu_seconds == 0


def test_full_keeps_every_leg_and_its_switches():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3", "--full"])
    assert a.full and all(getattr(a, leg) == 1 for leg in LEGS) and a.cpu_seconds > 0
    a = bench.parse_args(["--full", "--cfg3", "0", "--cpu-seconds", "0", "--dump-outputs", "d"])
    assert a.cfg3 == 0 and a.cfg1 == 1 and a.cpu_seconds == 0 and a.dump_outputs == "d"


def test_legs_only_run_needs_full():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--headline", "0"], cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and "--full" in p.stderr
    assert bench.parse_args(["--headline", "0", "--full"]).headline == 0


def _load(d, sfx=""):
    return {n: np.load(os.path.join(d, f"{n}{sfx}.npy"))
            for n in ("decoded_sample", "sample_chunks", "chunk_word_sums", "status")}


def test_dump_outputs_files(tmp_path):
    """dump_outputs over host tensors: names, dtypes, the sample's rows, the exact word sums,
    the size bound at the benchmark's own batch, and the same files for the same buffers"""
    import torch
    n = 50
    rng = np.random.default_rng(5)
    vals = rng.normal(size=(n, bench.CHUNK_BYTES // 4)).astype(np.float32)
    dst = torch.from_numpy(vals.view(np.uint8).reshape(-1).copy())
    st = torch.from_numpy(np.arange(n, dtype=np.int32) % 3 - 1)
    bench.dump_outputs(str(tmp_path / "a"), dst, st, n, 0, 1)
    bench.dump_outputs(str(tmp_path / "b"), dst, st, n, 0, 1)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(os.listdir(tmp_path / "a")) == sorted(f"{k}.npy" for k in a)
    assert a["decoded_sample"].dtype == np.float32 and all(a[k].dtype == np.float64 for k in a if k != "decoded_sample")
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    pick = a["sample_chunks"].astype(np.int64)
    assert len(pick) == bench.DUMP_SAMPLE_CHUNKS and len(set(pick)) == len(pick) and (np.diff(pick) > 0).all()
    assert np.array_equal(a["decoded_sample"], vals[pick])
    assert np.array_equal(a["chunk_word_sums"], vals.view(np.int32).astype(np.int64).sum(axis=1).astype(np.float64))
    assert np.array_equal(a["status"], st.numpy().astype(np.float64))
    # all files of the default 4096-chunk batch: the sample + three float64 vectors + headers
    assert bench.DUMP_SAMPLE_CHUNKS * bench.CHUNK_BYTES + 8 * (bench.DUMP_SAMPLE_CHUNKS + 2 * 4096) + 4 * 128 < 64e6
    bench.dump_outputs(str(tmp_path / "r"), dst, st, n, 1, 2)
    assert np.array_equal(_load(tmp_path / "r", "_rank1")["decoded_sample"], a["decoded_sample"])


@pytest.mark.gpu
def test_plain_run_dumps_what_it_decoded(tmp_path):
    """a small plain run end to end: the result line has the headline's keys and none of the
    legs, and the dumped chunks are the seeded corpus the run decoded"""
    chunks, unique, steps = 64, 16, 2
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--chunks", str(chunks), "--unique", str(unique),
                        "--dump-outputs", str(tmp_path / "out")], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [json.loads(x) for x in p.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, p.stdout
    d = lines[0]
    assert d["steps"] == steps and d["warmup"] == 1 and d["unit"] == "GB/s" and d["higher_is_better"] is True
    assert d["dtype"] == "u8" and d["ms_per_step"] > 0 and d["n_gpus"] == 1
    assert d["value"] == pytest.approx(chunks * bench.CHUNK_BYTES / (d["ms_per_step"] / 1e3) / 1e9, rel=1e-2)
    assert not set(d) & {"roofline", "f2", "lz4", "zstd", "bshuf", "e2e_pcie", "cfg1", "cfg3", "cfg4", "cfg4_full",
                         "cfg5", "cfg5_sharded_write", "cpu_baseline"}
    o = _load(tmp_path / "out")
    assert o["status"].shape == (chunks,) and not o["status"].any()
    raw = np.stack([bench.smooth_chunk(20261015 + k % unique) for k in range(chunks)])
    pick = o["sample_chunks"].astype(np.int64)
    assert o["decoded_sample"].dtype == np.float32 and np.array_equal(o["decoded_sample"], raw[pick])
    assert np.array_equal(o["chunk_word_sums"], raw.view(np.int32).astype(np.int64).sum(axis=1).astype(np.float64))
