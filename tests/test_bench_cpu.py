"""bench.py contract on the CPU smoke path (tiny dummy model, same code
path): one JSON result line with ms_per_step, --steps sets the timed step
count, and --dump-outputs writes the last step's outputs reproducibly."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
NAMES = ["logits.npy", "logits_columns.npy", "tokens.npy"]


def _bench(steps, warmup, dump, *extra):
  cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--device", "cpu",
         "--dtype", "fp32", "--mb-batch", "3", "--prompt-len", "16",
         "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(dump), *extra]
  r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
  assert r.returncode == 0, r.stderr[-2000:]
  lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
  assert len(lines) == 1, r.stdout
  return json.loads(lines[0])


def _load(d):
  return {n: np.load(d / n) for n in NAMES}


@pytest.fixture(scope="module")
def run_w1_s3(tmp_path_factory):
  d = tmp_path_factory.mktemp("w1s3")
  return _bench(3, 1, d), d


def test_result_line_and_dump_format(run_w1_s3):
  res, d = run_w1_s3
  assert res["steps"] == 3 and res["warmup"] == 1
  assert res["ms_per_step"] > 0
  # value = global_batch * steps / elapsed, ms_per_step = elapsed / steps
  batch = res["config"]["global_batch"]
  assert batch == 3
  assert abs(res["value"] - batch * 1000.0 / res["ms_per_step"]) <= 0.01 * res["value"]
  for key in ("metric", "value", "unit", "higher_is_better", "dtype"):
    assert key in res
  assert sorted(f.name for f in d.iterdir()) == NAMES
  out = _load(d)
  assert all(x.dtype in (np.float32, np.float64) for x in out.values())
  assert sum(x.nbytes for x in out.values()) <= 64 << 20
  toks, logits, cols = out["tokens.npy"], out["logits.npy"], out["logits_columns.npy"]
  assert toks.shape == (1, 3) and logits.shape == (1, 3, cols.shape[0])
  assert np.isfinite(logits).all()
  # every column is dumped here, so the tokens are the logits' argmax
  assert np.array_equal(cols[logits.argmax(-1)], toks)


def test_same_arguments_same_dump(run_w1_s3, tmp_path):
  _, d = run_w1_s3
  _bench(3, 1, tmp_path, "--full")
  a, b = _load(d), _load(tmp_path)
  for n in NAMES:
    assert np.array_equal(a[n], b[n]), n


def test_steps_sets_the_number_of_decode_steps(run_w1_s3, tmp_path):
  """The dump is the state after warmup + steps decode steps: moving one step
  from --steps to --warmup leaves it unchanged, dropping one step changes it."""
  _, d = run_w1_s3
  same_total, one_less = tmp_path / "w2s2", tmp_path / "w1s2"
  _bench(2, 2, same_total)
  _bench(2, 1, one_less)
  a, b, c = _load(d), _load(same_total), _load(one_less)
  for n in NAMES:
    assert np.array_equal(a[n], b[n]), n
  assert not np.array_equal(a["logits.npy"], c["logits.npy"])
