"""LayerKV / ShardKVCache: row slices keep every field, for_config allocates
what the hand-built constructor does, and no decoder reads a cache by
position."""
import re
from pathlib import Path

import pytest
import torch

from xotorch_amd.engine.kvcache import LayerKV, ShardKVCache
from xotorch_amd.models.config import config_from_hf
from xotorch_amd.models.registry import BUILTIN_CONFIGS


def _fields(n):
  """n distinct [4, 3] tensors for the first n LayerKV fields."""
  return [torch.arange(12, dtype=torch.float32).reshape(4, 3) + 100 * i for i in range(n)]


@pytest.mark.parametrize("n", [2, 4, 5, 6])  # plain, packed, MLA fp8 (one scale), GQA fp8
def test_layerkv_rows_slices_every_field_as_a_view(n):
  kv = LayerKV(*_fields(n))
  rows = kv.rows(1, 3)
  assert isinstance(rows, LayerKV)
  for name, full, part in zip(LayerKV._fields, kv, rows):
    if full is None:
      assert part is None, name
      continue
    assert torch.equal(part, full[1:3]), name
    part[0, 0] = -7.0  # a view: the write lands in the parent's row 1
    assert full[1, 0] == -7.0, name
  assert [t is None for t in rows] == [False] * n + [True] * (6 - n)


def test_shardkvcache_rows_slices_every_layer():
  cache = ShardKVCache(3, 4, 2, 8, 16, torch.float32, "cpu")
  rows = cache.rows(2, 4)
  assert len(rows) == 3 and all(isinstance(r, LayerKV) for r in rows)
  for layer, r in zip(cache.caches, rows):
    assert r.k.shape == (2, 2, 8, 16) and r.k.data_ptr() == layer.k[2:4].data_ptr()
    assert r.v.data_ptr() == layer.v[2:4].data_ptr()
    assert r.kp is None and r.vsc is None


@pytest.mark.parametrize("model_id", ["llama-3.2-1b", "gemma2-27b", "deepseek-v2-lite"])
def test_for_config_matches_hand_built_constructor(model_id):
  cfg = config_from_hf(BUILTIN_CONFIGS[model_id], model_id)
  heads, k_dim, v_dim = cfg.kv_cache_dims()
  a = ShardKVCache.for_config(cfg, 2, 3, 40, torch.float32, "cpu")
  b = ShardKVCache(2, 3, heads, 40, k_dim, torch.float32, "cpu", v_dim=v_dim)
  assert (a.capacity, a.batch, len(a)) == (b.capacity, b.batch, len(b)) == (40, 3, 2)
  for la, lb in zip(a.caches, b.caches):
    for ta, tb in zip(la, lb):
      assert (ta is None and tb is None) or (ta.shape == tb.shape and ta.dtype == tb.dtype
                                             and torch.equal(ta, tb))
  assert a[0].k.shape == (3, heads, 40, k_dim) and a[0].v.shape == (3, heads, 40, v_dim)
  assert a.nbytes() == b.nbytes()


def test_no_positional_cache_reads_in_models():
  models = Path(__file__).resolve().parent.parent / "xotorch_amd" / "models"
  for path in sorted(models.glob("*.py")):
    src = path.read_text()
    assert "len(kv)" not in src, path.name
    assert not re.search(r"\bkv\[\d", src), path.name
