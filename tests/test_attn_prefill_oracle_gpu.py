"""bf16 GQA prefill attention (attn_prefill_mfma_kernel<128, 2> / <256, 1>)
against the fp64 oracle of tests/attn_oracle.py: one launch per case over four
seeded families (limits, tiles, scores, plain) on a cache poisoned with +-1e30
from T = start_pos + S to its capacity, held to err <= 1 x the derived bf16-P
bound. tests/test_attn_prefill_oracle_cpu.py shows for the same cases that a
causal limit or window start off by one, a dropped half-tile, a q block's first
tile skipped, scale x sqrt 2, no softcap and the neighbouring kv head each move
every (row, head) they apply to by >= 4 x bound (weakest per case: 59.1, 6.5,
22.3, 8.2, 11.2, 33.0, 17.8, 5.3, 11.2), and that a torch fp32 emulation of
the kernel's loop stays inside it.

Worst err / bound, in case order, measured on the MI355X:
0.635, 0.722, 0.592, 0.604, 0.719, 0.618, 0.747, 0.635, 0.583
and of the CPU emulator, which ends on the same bf16 value at the worst element
of every case (the final rounding is the largest term):
0.635, 0.722, 0.592, 0.604, 0.719, 0.618, 0.747, 0.635, 0.583."""
import pytest
import torch

import attn_oracle as ao

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("sp", ao.PREFILL_SPECS, ids=lambda s: s.name)
def test_attn_prefill_vs_fp64(monkeypatch, sp):
  from xotorch_amd import ops
  assert ops.hip_available()
  c = ao.prefill_case(sp)
  Bl, S, H, hd = c.q.shape
  calls = []
  kernel = ops._hip.attn_prefill_mfma
  monkeypatch.setattr(ops._hip, "attn_prefill_mfma", lambda *a: calls.append(len(a)) or kernel(*a))
  monkeypatch.setattr(ops._hip, "attn_chunk_mfma", lambda *a: pytest.fail("the chunk kernel served the prefill"))
  monkeypatch.delenv("XOT_ATTN_CHUNK", raising=False)
  qkv = torch.zeros(Bl, S, H + 2 * sp.KVH, hd, dtype=torch.bfloat16)  # q as the strided view the models pass
  qkv[:, :, :H] = c.q
  kp, vp = ao.pack_k(c.kc, sp.cap).cuda(), ao.pack_v(c.vc, sp.cap).cuda()
  out = ops.attn_prefill(qkv.cuda()[:, :, :H], None, None, sp.start, S, kp, vp,
                         scale=sp.scale, softcap=sp.softcap, window=sp.window)
  assert calls == [7], "attn_prefill_mfma must serve the call once, without scales"
  assert out.shape == (Bl, S, H, hd) and out.dtype == torch.bfloat16
  r = (out.cpu().double() - c.ref).abs() / c.bound
  per_fam = {f: r[c.rows(f)].max().item() for f in ao.PF_FAMILIES}
  print(f"attn_prefill bf16 {sp.name} cap={sp.cap}: worst err / bound " + " ".join(f"{f} {x:.3f}" for f, x in per_fam.items()))
  worst = r.max().item()
  assert worst <= 1, (worst, per_fam)  # a NaN fails too
