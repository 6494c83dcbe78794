"""Device-event timings of the BERT variant (one JSON line).

    python tools/bench_bert.py [--steps K] [--warmup W]

  attention: fbl_mha_fwd / fbl_mha_bwd (rowdot + the two backward passes) at B=32, S=266, nh in {12, 16, 24}, ragged masks
             as bench.py draws them; at nh=24 beside fbl_disent_attn_fwd (the DeBERTa kernel, same shape) and ATen's unfused
             composition softmax(Q.K^T*scale + mask).V (forward, forward+backward) -- and F.scaled_dot_product_attention when
             this torch runs it.  The compared legs alternate inside one loop; per-leg means after warm-up.
  train:     BERT-base and BERT-large training step (forward + backward + clipped FusedAdam) at B=32, T=10, L=256.
  cfg1:      BERT-base forward with the loss, BASELINE config 1 (B=4, T=10, L=64), eval.
Kernel times without launch overhead: run under `rocprofv3 --kernel-trace --stats`.
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from frozenbilm_amd import lib as L

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--skip-train", action="store_true")
a = ap.parse_args()
dev = "cuda"
B, S, T = 32, 266, 10


def masks(seed=0):
    g = torch.Generator().manual_seed(seed)
    tl = torch.randint(32, S - T + 1, (B,), generator=g)
    tl[-1] = S - T
    vl = torch.randint(1, T + 1, (B,), generator=g)
    m = torch.zeros(B, S, dtype=torch.int32)
    for b in range(B):
        m[b, : vl[b]] = 1
        m[b, T: T + tl[b]] = 1
    return m.to(dev)


def alternate(legs, n, warm):
    """mean ms per leg; the legs run in turn inside each iteration"""
    ev = {k: [] for k in legs}
    for it in range(warm + n):
        for k, f in legs.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            f()
            e.record()
            if it >= warm:
                ev[k].append((s, e))
    torch.cuda.synchronize()
    return {k: round(sum(s.elapsed_time(e) for s, e in v) / len(v) * 1000.0, 1) for k, v in ev.items()}  # us


out = {"shape": dict(B=B, S=S), "attention_us": {}}
mask = masks()
klen = (mask * torch.arange(1, S + 1, device=dev, dtype=torch.int32)).amax(1).to(torch.int32).contiguous()
border = torch.argsort(klen, descending=True, stable=True).to(torch.int32).contiguous()
for nh in (12, 16, 24):
    H = nh * 64
    g = torch.Generator().manual_seed(nh)
    qkv = (torch.randn(B * S, 3 * H, generator=g) * 0.7).to(torch.bfloat16).to(dev)
    q, k, v = qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:]
    ctx = torch.empty(B * S, H, dtype=torch.bfloat16, device=dev)
    lse = torch.empty(B, nh, S, device=dev)
    dctx = torch.randn(B * S, H, device=dev).to(torch.bfloat16)
    Dv = torch.empty(B, nh, S, device=dev)
    dqkv = torch.empty(B * S, 3 * H, dtype=torch.bfloat16, device=dev)
    mf = mask.view(-1)

    def mha_fwd():
        L.mha_fwd(q, k, v, mf, 0.125, ctx, lse, B, S, nh, klen=klen, border=border)

    def mha_bwd():
        L.attn_rowdot(dctx, ctx, Dv, B, S, nh)
        L.mha_bwd(q, k, v, dctx, mf, lse, Dv, 0.125, dqkv[:, :H], dqkv[:, H:2 * H], dqkv[:, 2 * H:], B, S, nh, klen=klen,
                  border=border)

    legs = {"mha_fwd": mha_fwd, "mha_bwd": mha_bwd}
    if nh == 24:
        from frozenbilm_amd.model.relpos import rel_index_vector

        span2 = 512
        pqk = (torch.randn(span2, 2 * H, generator=g) * 0.7).to(torch.bfloat16).to(dev)
        relidx = torch.from_numpy(rel_index_vector(S, 256, 512, 256).copy()).to(dev)
        Sp = (S + 63) // 64 * 64
        ctx2 = torch.empty_like(ctx)

        def disent_fwd():
            L.disent_attn_fwd(q, k, v, pqk[:, H:], pqk[:, :H], relidx, mf, 1 / math.sqrt(192), ctx2, lse, B, S, Sp, nh, span2,
                              klen=klen, border=border, lin=128)

        qh, kh, vh = (t.view(B, S, nh, 64).transpose(1, 2) for t in (q, k, v))
        add = ((1.0 - mask.float()) * -10000.0)[:, None, None, :].to(torch.bfloat16)
        qg, kg, vg = (t.detach().clone().requires_grad_(True) for t in (qh, kh, vh))
        go = torch.randn(B, nh, S, 64, device=dev).to(torch.bfloat16)

        def aten_fwd():
            with torch.no_grad():
                torch.softmax(qh @ kh.transpose(-1, -2) * 0.125 + add, -1) @ vh

        def aten_fwd_bwd():
            o = torch.softmax(qg @ kg.transpose(-1, -2) * 0.125 + add, -1) @ vg
            o.backward(go)

        legs.update(disent_fwd=disent_fwd, aten_fwd=aten_fwd, aten_fwd_bwd=aten_fwd_bwd)
        try:
            F.scaled_dot_product_attention(qh, kh, vh, attn_mask=add)

            def sdpa_fwd():
                with torch.no_grad():
                    F.scaled_dot_product_attention(qh, kh, vh, attn_mask=add)

            legs["sdpa_fwd"] = sdpa_fwd
        except Exception as e:  # noqa: BLE001
            out["sdpa"] = f"unavailable: {type(e).__name__}"
    out["attention_us"][f"nh{nh}"] = alternate(legs, a.steps, a.warmup)

if not a.skip_train:
    from frozenbilm_amd.model import BertConfig, BertForMaskedLM
    from frozenbilm_amd.optim import FusedAdam

    out["train_ms"] = {}
    g = torch.Generator().manual_seed(1)
    Lt = S - T
    video = torch.randn(B, T, 768, generator=g).to(dev)
    ids = torch.randint(1000, 30522, (B, Lt), generator=g).to(dev)
    am = mask[:, T:].long().contiguous()
    vm = mask[:, :T].long().contiguous()
    labels = torch.where((torch.rand(B, Lt, generator=g).to(dev) < 0.15) & (am > 0), ids, torch.full_like(ids, -100))
    for name, cfg in (("bert_base", BertConfig.base()), ("bert_large", BertConfig.large())):
        torch.manual_seed(0)
        m = BertForMaskedLM(cfg, features_dim=768, max_feats=T).to(dev).train()
        opt = FusedAdam(m, lr=1e-4)

        def step():
            opt.zero_grad()
            o = m(video=video, video_mask=vm, input_ids=ids, attention_mask=am, labels=labels)
            o.loss.backward()
            opt.step(clip_max_norm=0.1)

        out["train_ms"][name] = round(alternate({name: step}, max(3, a.steps // 4), 2)[name] / 1000.0, 2)
        del m, opt
        torch.cuda.empty_cache()
    m = BertForMaskedLM(BertConfig.base(), features_dim=768, max_feats=10).to(dev).eval()
    g = torch.Generator().manual_seed(18)
    v1 = torch.randn(4, 10, 768, generator=g).to(dev)
    i1 = torch.randint(1000, 30522, (4, 64), generator=g).to(dev)
    l1 = torch.where(torch.rand(4, 64, generator=g).to(dev) < 0.15, i1, torch.full_like(i1, -100))

    def cfg1():
        with torch.no_grad():
            m(video=v1, input_ids=i1, labels=l1)

    out["cfg1_forward_ms"] = round(alternate({"cfg1": cfg1}, a.steps, a.warmup)["cfg1"] / 1000.0, 3)
print(json.dumps(out))
