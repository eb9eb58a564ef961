"""GPU: the plain `python bench.py --gpus 1 --steps K --warmup W` line carries the headline figure and nothing that needs work of its
own (no oracle check, digest, CPU baseline: those are --full), and --dump-outputs writes a fixed sample of what the last timed
step computed -- the same bytes whatever the number of steps, equal to the CPU oracle where the sample falls into block 0."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + args, capture_output=True, text=True, timeout=1200, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def _words(directory):
    halves = np.load(os.path.join(directory, "dct_quant_out_sample.npy"))
    pos = np.load(os.path.join(directory, "dct_quant_out_sample_index.npy"))
    assert halves.dtype == np.float64 and pos.dtype == np.float64 and halves.shape == (pos.size, 2)
    assert sum(os.path.getsize(os.path.join(directory, f)) for f in os.listdir(directory)) <= 64 * 10 ** 6
    return (halves[:, 0].astype(np.uint64) << np.uint64(32)) | halves[:, 1].astype(np.uint64), pos.astype(np.int64)


def test_plain_line_and_dumped_outputs(oracle_mod, tmp_path):
    B = 128
    a = _plain(["--blocks", str(B), "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "a")])
    assert a["metric"] == "encrypted 8x8 blocks/sec (homomorphic DCT+quant)" and a["unit"] == "blocks/s" and a["higher_is_better"] is True
    assert a["steps"] == 3 and a["dtype"] in ("f64", "u64") and a["value"] > 0
    assert abs(a["value"] - B / (a["ms_per_step"] * 1e-3)) < 1e-6 * a["value"]
    assert a["verified_bit_exact_vs_oracle"] is None and a["output_digest"] is None and "cpu_baseline" not in a
    _plain(["--blocks", str(B), "--steps", "1", "--warmup", "0", "--dump-outputs", str(tmp_path / "b")])
    wa, pa = _words(str(tmp_path / "a"))
    wb, pb = _words(str(tmp_path / "b"))
    assert np.array_equal(pa, pb) and np.array_equal(wa, wb)
    orc = oracle_mod.Oracle.preset("P4096")
    block_words = 64 * 2 * orc.k * orc.n
    assert pa.size == 1 << 21 and pa[-1] < B * block_words and np.all(np.diff(pa) > 0)
    ref = orc.dct_quant(orc.random_ct(64, seed=oracle_mod.SEED).reshape(64, 2, orc.k, orc.n), oracle_mod.YQT).reshape(-1)
    first = pa < block_words
    assert first.sum() > 1000 and np.array_equal(wa[first], ref[pa[first]].astype(np.uint64))
