"""XOT_HIP_SAMPLE=1 on the serve ring: one ops.sample launch per tick from the
per-slot parameter tensors (dummy model at the GPU attention kernels' head dim,
world 1, eager decode)."""
import queue

import pytest
import torch

from xotorch_amd import serve_ring
from xotorch_amd.ops import torch_ref
from xotorch_amd.serve_ring import AdmitMsg, RingSlotWorker

pytestmark = pytest.mark.gpu
PROMPTS = {"a": [3, 99, 7, 250, 41], "b": [17, 5, 128], "c": [200, 1, 2, 3, 4, 5, 6]}
SAMPLED = dict(temp=0.8, top_p=0.5, top_k=4)


@pytest.fixture(scope="module")
def worker():
  mp = pytest.MonkeyPatch()
  cfg = dict(serve_ring.builtin_config("dummy"), head_dim=128)
  mp.setattr(serve_ring, "builtin_config", lambda model_id: cfg)
  torch.manual_seed(0)
  w = RingSlotWorker("dummy", 0, 1, device="cuda", dtype=torch.bfloat16, slots=4, max_seq=64,
                     use_graphs=False)
  mp.undo()
  return w


def _serve(w, max_new=6, ticks=None, **sampling):
  """Serve PROMPTS to the end on the caller's thread -> {rid: [tokens]}; `ticks`
  collects (logits_buf, tok_bcast, active) after every decode tick's sampling."""
  q, got, left = queue.Queue(), {}, set(PROMPTS)

  def emit(rid, tok, fin, meta):
    got.setdefault(rid, []).append(tok)
    if fin:
      left.discard(rid)
      if not left:
        q.put(AdmitMsg("stop", None, 0, 0.0))

  def recording():
    RingSlotWorker._sample_all(w)
    if ticks is not None:
      ticks.append((w.logits_buf.float().cpu(), w.tok_bcast.cpu(), list(w.active)))

  w._sample_all = recording
  w.samp_gen.manual_seed(1234)
  for rid, ids in PROMPTS.items():
    q.put(AdmitMsg(rid, torch.tensor([ids], dtype=torch.int64), max_new, sampling.get("temp", 0.0),
                   top_p=sampling.get("top_p", 0.0), top_k=sampling.get("top_k", 0)))
  w.serve_forever(q, emit, max_ticks=500)
  assert not left
  return got


def test_greedy_slots_match_the_torch_route(worker, monkeypatch):
  monkeypatch.setenv("XOT_HIP_SAMPLE", "0")
  ref = _serve(worker)
  monkeypatch.setenv("XOT_HIP_SAMPLE", "1")
  assert _serve(worker) == ref


def test_sampled_slots_stay_in_the_kept_set_and_repeat(worker, monkeypatch):
  monkeypatch.setenv("XOT_HIP_SAMPLE", "1")
  ticks = []
  got = _serve(worker, ticks=ticks, **SAMPLED)
  assert ticks and _serve(worker, **SAMPLED) == got  # the same seed, the same text
  for logits, toks, active in ticks:
    rows = torch.tensor([i for i, a in enumerate(active) if a])
    n = len(rows)
    keep, _, _ = torch_ref.sample_kept(logits[rows], torch.full((n,), 0.8), torch.full((n,), 4, dtype=torch.int32),
                                       torch.full((n,), 0.5))
    assert keep.gather(1, toks[rows][:, None]).all()
