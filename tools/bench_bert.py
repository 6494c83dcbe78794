"""Device-event timings of the BERT variant (one JSON line).

    python tools/bench_bert.py [--steps K] [--warmup W]

  attention: fbl_mha_fwd / fbl_mha_bwd (rowdot + the two backward passes) at B=32, S=266, nh in {12, 16, 24}, ragged masks
             as bench.py draws them; at nh=24 beside fbl_disent_attn_fwd (the DeBERTa kernel, same shape) and ATen's unfused
             composition softmax(Q.K^T*scale + mask).V (forward, forward+backward) -- and F.scaled_dot_product_attention when
             this torch runs it.  The compared legs alternate inside one loop; per-leg means after warm-up.
  train:     BERT-base and BERT-large training step (forward + backward + clipped FusedAdam) at B=32, T=10, L=256.
  cfg1:      BERT-base forward with the loss, BASELINE config 1 (B=4, T=10, L=64), eval.
  --packed-rows: instead of the above, the packed-row legs (model.packed_rows; fbl_mha_fwd_rows / fbl_mha_bwd_rows): the two
             attention entry-point pairs at nh in {12, 16} and the BERT-base / BERT-large training step (dropout live, clipped
             FusedAdam), padded and packed legs alternating inside one process; per leg the median and the 10th / 90th
             percentile after warm-up, and the share of rows that exist.
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
ap.add_argument("--packed-rows", action="store_true", help="time the packed-row legs against their padded siblings")
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


def alternate_stats(legs, n, warm, scale=1000.0, nd=1):
    """per leg {median, p10, p90} (us by default); the legs run in turn inside each iteration"""
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
    res = {}
    for k, v in ev.items():
        t = sorted(s.elapsed_time(e) * scale for s, e in v)
        pick = lambda q: round(t[min(len(t) - 1, int(q * len(t)))], nd)
        res[k] = {"median": pick(0.5), "p10": pick(0.1), "p90": pick(0.9), "n": len(t)}
    return res


def packed_rows_legs():
    from frozenbilm_amd.bert_engine import bert_packing
    from frozenbilm_amd.model import BertConfig, BertForMaskedLM
    from frozenbilm_amd.optim import FusedAdam

    mask = masks()
    Lt = S - T
    g = torch.Generator().manual_seed(1)
    video = torch.randn(B, T, 768, generator=g).to(dev)
    ids = torch.randint(1000, 30522, (B, Lt), generator=g).to(dev)
    am = mask[:, T:].long().contiguous()
    vm = mask[:, :T].long().contiguous()
    labels = torch.where((torch.rand(B, Lt, generator=g).to(dev) < 0.15) & (am > 0), ids, torch.full_like(ids, -100))
    full_labels = torch.cat([torch.full((B, T), -100, dtype=torch.long, device=dev), labels], 1).view(-1)
    pk = bert_packing(mask.view(-1), full_labels, None, B, S, T)
    res = {"shape": dict(B=B, S=S, T=T), "rows": {"padded": B * S, "packed": pk.n, "share": round(pk.n / (B * S), 3)},
           "attention_us": {}, "train_ms": {}}
    klen = (mask * torch.arange(1, S + 1, device=dev, dtype=torch.int32)).amax(1).to(torch.int32).contiguous()
    border = torch.argsort(klen, descending=True, stable=True).to(torch.int32).contiguous()
    mf = mask.view(-1)
    for nh in (12, 16):
        H = nh * 64
        gq = torch.Generator().manual_seed(nh)
        qkv = (torch.randn(B * S, 3 * H, generator=gq) * 0.7).to(torch.bfloat16).to(dev)
        dctx = torch.zeros(B * S, H, dtype=torch.bfloat16, device=dev)
        dctx[pk.sel] = torch.randn(pk.n, H, device=dev).to(torch.bfloat16)
        qp, dp = qkv[pk.sel].contiguous(), dctx[pk.sel].contiguous()
        ctx, ctxp = torch.empty(B * S, H, dtype=torch.bfloat16, device=dev), torch.empty(pk.n, H, dtype=torch.bfloat16, device=dev)
        lse, lsep, Dv = (torch.empty(B, nh, S, device=dev) for _ in range(3))
        dqkv, dqp = torch.empty_like(qkv), torch.empty_like(qp)

        def fwd():
            L.mha_fwd(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], mf, 0.125, ctx, lse, B, S, nh, klen=klen, border=border)

        def fwd_rows():
            L.mha_fwd_rows(qp[:, :H], qp[:, H:2 * H], qp[:, 2 * H:], mf, klen, pk.row0, 0.125, ctxp, lsep, B, S, nh, border=border)

        def bwd():
            L.attn_rowdot(dctx, ctx, Dv, B, S, nh)
            L.mha_bwd(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], dctx, mf, lse, Dv, 0.125, dqkv[:, :H], dqkv[:, H:2 * H],
                      dqkv[:, 2 * H:], B, S, nh, klen=klen, border=border)

        def bwd_rows():
            L.mha_bwd_rows(qp[:, :H], qp[:, H:2 * H], qp[:, 2 * H:], dp, ctxp, mf, klen, pk.row0, lsep, Dv, 0.125, dqp[:, :H],
                           dqp[:, H:2 * H], dqp[:, 2 * H:], B, S, nh, border=border)

        res["attention_us"][f"nh{nh}"] = alternate_stats({"mha_fwd": fwd, "mha_fwd_rows": fwd_rows, "mha_bwd": bwd,
                                                          "mha_bwd_rows": bwd_rows}, a.steps, a.warmup)
    if a.skip_train:
        return res
    for name, cfg in (("bert_base", BertConfig.base()), ("bert_large", BertConfig.large())):
        torch.manual_seed(0)
        m = BertForMaskedLM(cfg, features_dim=768, max_feats=T).to(dev).train()
        opt = FusedAdam(m, lr=1e-4)

        def step(packed):
            m.packed_rows = packed
            opt.zero_grad()
            o = m(video=video, video_mask=vm, input_ids=ids, attention_mask=am, labels=labels)
            o.loss.backward()
            opt.step(clip_max_norm=0.1)

        res["train_ms"][name] = alternate_stats({"padded": lambda: step(False), "packed": lambda: step(True)},
                                                max(5, a.steps // 2), 3, scale=1.0, nd=2)
        del m, opt
        torch.cuda.empty_cache()
    return res


if a.packed_rows:
    print(json.dumps(packed_rows_legs()))
    sys.exit(0)

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
