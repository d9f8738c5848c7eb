"""The native drop-ins for the reference's binaries (build/kzgpot-preprocess-{kgz,fastkgz},
csrc/preprocess_main.cpp) run end to end on the GPU, and bench.py's plain / --full /
--dump-outputs runs at a small size.

This module sorts before every other GPU test on purpose: it starts the CLI and the bench as child processes
while the pytest process itself has not touched the GPU yet (no `gpu` fixture here), so no child
is ever started from a process that holds a HIP context."""
import hashlib
import json
import os
import shutil
import subprocess

import pytest

from conftest import GOLDEN, PKG


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["kgz", "fastkgz"])
def test_cli_preprocess_config1(mode, tmp_path):
    """Config 1 (N = 2^10 transcript) through the CLI: the kzg_setup file's BLAKE2b-512 equals the
    oracle pipeline's (tests/golden/transcript_n1024.json); with the default POWERSOFTAU_DIGEST
    check the synthetic transcript fails validation (exit 101, no output file)."""
    meta = json.load(open(os.path.join(GOLDEN, "transcript_n1024.json")))
    shutil.copy(os.path.join(GOLDEN, "transcript_n1024.bin"), tmp_path / "powersoftau")
    exe = os.path.join(PKG, "build", f"kzgpot-preprocess-{mode}")
    r = subprocess.run([exe, "--n-log2", "10", "--no-digest-check", "--output-digest"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = (tmp_path / "kzg_setup").read_bytes()
    assert len(out) == meta[f"{mode}_size"]
    assert hashlib.blake2b(out).hexdigest() == meta[f"{mode}_blake2b"]
    assert f"output BLAKE2b-512: {meta[f'{mode}_blake2b']}" in r.stdout
    assert f"transcript BLAKE2b-512: {meta['transcript_blake2b']}" in r.stdout
    (tmp_path / "kzg_setup").unlink()
    # the reference's own work: the transcript checked against a given digest, the output not hashed
    r = subprocess.run([exe, "--n-log2", "10", "--expect-digest", meta["transcript_blake2b"]], cwd=tmp_path,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "output BLAKE2b-512" not in r.stdout and "Checking passed" in r.stdout
    assert hashlib.blake2b((tmp_path / "kzg_setup").read_bytes()).hexdigest() == meta[f"{mode}_blake2b"]
    (tmp_path / "kzg_setup").unlink()
    r = subprocess.run([exe, "--n-log2", "10", "--expect-digest", "0" * 128], cwd=tmp_path, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 101 and "failed validation" in r.stderr and not (tmp_path / "kzg_setup").exists()
    r = subprocess.run([exe, "--n-log2", "10"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 101 and "failed validation" in r.stderr
    assert not (tmp_path / "kzg_setup").exists()


BENCH_SMALL = ["--gpus", "1", "--g1-log2", "10", "--g2-log2", "6", "--steps", "2", "--warmup", "1"]


def run_bench(extra, dump):
    import sys

    from conftest import ROOT

    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + BENCH_SMALL + extra +
                       ["--dump-outputs", str(dump)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    (line,) = r.stdout.strip().splitlines()  # the one JSON line
    return json.loads(line)


def load_dump(d):
    import numpy as np

    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.fixture(scope="module")
def bench_full(tmp_path_factory):
    """bench.py --full at 2^10 G1 + 2^6 G2 (no rows beyond the verification), outputs dumped."""
    d = tmp_path_factory.mktemp("dump_full")
    return run_bench(["--full", "--no-next-rows", "--no-cpu-baseline", "--oracle-sample-runs", "4"], d), load_dump(d)


@pytest.mark.gpu
def test_bench_dump_outputs_of_a_verified_run(bench_full):
    """--dump-outputs on a run whose output buffers the same process verified bit-exact (generator's
    expected bytes, C oracle sample): float arrays, every record when the stream is smaller than
    the sample, the whole-buffer byte sums equal to the records' bytes, no rejected point."""
    import numpy as np

    line, dump = bench_full
    assert line["verified_bit_exact"] is True and line["oracle_sample_check"]["equal"] is True
    assert line["steps"] == 2 and line["higher_is_better"] is True and line["unit"] == "points/s"
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 / (1024 + 64) - 1) < 1e-9
    assert sorted(dump) == ["first_bad", "g1_block_bytesum", "g1_record_index", "g1_records", "g2_block_bytesum",
                            "g2_record_index", "g2_records"]
    assert sum(a.nbytes for a in dump.values()) <= 64 << 20
    for kind, n, rout in (("g1", 1024, 96), ("g2", 64, 192)):
        rec = dump[f"{kind}_records"]
        assert rec.dtype == np.float32 and rec.shape == (n, rout)
        assert np.array_equal(rec, np.floor(rec)) and rec.min() >= 0 and rec.max() <= 255 and rec.any()
        assert dump[f"{kind}_record_index"].dtype == np.float64
        assert np.array_equal(dump[f"{kind}_record_index"], np.arange(n))
        sums = dump[f"{kind}_block_bytesum"]
        assert sums.dtype == np.float64 and sums.shape == (n,)  # gcd(n, 4096) slices: one per record here
        assert np.array_equal(sums, rec.astype(np.float64).sum(1))
    assert dump["first_bad"].dtype == np.float64 and dump["first_bad"].tolist() == [-1.0, -1.0]


@pytest.mark.gpu
def test_bench_plain_run_is_the_headline_only(bench_full, tmp_path):
    """A plain run (no --full) times the same steps on the same inputs, so its dumped outputs equal
    the verified run's array for array, and its line carries neither the verification nor the rows."""
    import numpy as np

    line = run_bench([], tmp_path)
    assert line["verified_bit_exact"] is None and line["oracle_sample_check"] is None
    assert "next_rows" not in line and "cpu_baseline" not in line
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert line[k] == bench_full[0][k] or k in ("value", "ms_per_step")
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["rejected_points"] == 0
    got, want = load_dump(tmp_path), bench_full[1]
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
