"""Device-event timings of a fine-tuning step at the xlarge dimensions (one JSON object).

    python tools/bench_finetune.py [--steps K] [--warmup W] [--layers N]

Two workloads, each a full training step -- forward, the caller's loss on the [MASK]-row logits, backward, clipped FusedAdam
-- in train mode with every dropout site live, through `videoqa.answer_logits` (the call both fine-tuning loops make):

  videoqa  B = 32 questions, 10 video slots, ragged short questions (8 .. 64 tokens, one [MASK] each), n_ans = 1000,
           cross-entropy on the answer logits (videoqa.py:66-83)
  mc       B = 8 questions x C = 4 candidates in ONE forward of 32 samples (mc.candidate_scores), ragged speech context up
           to S = 512, the 2-way answer head, balanced BCE on softmax[:, 0] (mc.py:64-92)

Legs of these two workloads:

  full         the default route: full [B, S, n_ans] logits, head forward and backward on every token row
  rows         args.train_logit_rows: head forward and backward on the [MASK] rows only (logit_rows under autograd)
  rows_packed  args.packed_rows: the same on packed rows (model.packed_rows)
  rows_decoder / rows_packed_decoder   the two above with args.decoder_rows: the enhanced mask decoder on the [MASK] rows only
  rows_graphs  args.finetune_graphs: the rows route replayed as two hipGraphs per length bucket (model.finetune_graphs); beside
               it, per leg, `host_ms`: the time the host needs to issue a step (wall clock inside the step call, the device
               idle in front of it; a pass of its own), and the number of graph captures the run made.  --pad-to-bucket pads the text of every leg to the graphs' length
               bucket, so that the eager legs run the grid the graphs leg runs

A further `videoqa` shape, `videoqa_short`: B = 32, T = 10, questions of 8 .. 24 tokens (S = 34): the subtitle-free datasets.

A third workload, `mlm`: B = 32, T = 10, ragged text U[32,256] with one sample of 256, labels on 15 % of the non-pad tokens,
forward with `labels`, backward, clipped FusedAdam; legs `default` and `decoder_rows` (model.decoder_rows).

The legs alternate inside one process (one model, one optimizer; every leg is a real update); per leg the median and the
10th / 90th percentile over the timed iterations, and the share of token rows that exist on the packed layout.
"""
import argparse
import json
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from frozenbilm_amd import mc as P_mc
from frozenbilm_amd import train_graph as TG
from frozenbilm_amd import videoqa as P_vqa
from frozenbilm_amd.model import DebertaV2Config, DebertaV2ForMaskedLM
from frozenbilm_amd.optim import FusedAdam

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20, help="timed iterations per leg (at least 20 for the record)")
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--layers", type=int, default=0, help="encoder layers (0: the xlarge model's 24)")
ap.add_argument("--only", choices=["videoqa_short", "videoqa", "mc", "mlm"], default=None)
ap.add_argument("--pad-to-bucket", action="store_true", help="pad the text to a multiple of model.GRAPH_L_BUCKET for every leg")
ap.add_argument("--legs", default="", help="comma-separated subset of the legs of the videoqa / mc workloads (default: all)")
a = ap.parse_args()
dev = torch.device("cuda")
T, FEAT, MASK = 10, 768, 128000


class Tok:
    mask_token_id, pad_token_id, sep_token_id = MASK, 0, 2


def texts(n, lo, hi, seed):
    """n ragged token rows padded to the longest (which is `hi` long), exactly one [MASK] inside each"""
    g = torch.Generator().manual_seed(seed)
    tlen = torch.randint(lo, hi + 1, (n,), generator=g)
    tlen[-1] = hi
    ids = torch.randint(5, 127000, (n, hi), generator=g) * (torch.arange(hi)[None] < tlen[:, None])
    ids[torch.arange(n), torch.stack([torch.randint(1, int(t), (1,), generator=g) for t in tlen]).view(-1)] = MASK
    return ids, tlen


def band(t):
    t = sorted(t)
    pick = lambda q: round(t[min(len(t) - 1, int(q * len(t)))], 2)
    return {"median": pick(0.5), "p10": pick(0.1), "p90": pick(0.9), "n": len(t)}


def alternate_stats(legs, n, warm):
    """per leg {median, p10, p90} in ms; the legs run in turn inside each iteration"""
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
    return {k: band([s.elapsed_time(e) for s, e in v]) for k, v in ev.items()}


def host_issue_stats(legs, n):
    """per leg the host's time to issue a step, in ms: wall clock inside the step call with an idle device in front of it
    (synchronised before every call, so that neither a full queue nor the step's one read of an input waits for older work);
    a pass of its own after the device-event pass, which must not be synchronised"""
    import time

    issue = {k: [] for k in legs}
    for _ in range(n):
        for k, f in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            issue[k].append((time.perf_counter() - t0) * 1e3)
    torch.cuda.synchronize()
    return {k: band(v) for k, v in issue.items()}


def peak_memory(legs):
    """per leg torch.cuda.max_memory_allocated of one step, in MB (a pass of its own, after the timed ones)"""
    out = {}
    for k, f in legs.items():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        f()
        torch.cuda.synchronize()
        out[k] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
    return out


def workload(name):
    cfg = DebertaV2Config()
    if a.layers:
        cfg.num_hidden_layers = a.layers
    n_ans = 2 if name == "mc" else 1000
    torch.manual_seed(0)
    m = DebertaV2ForMaskedLM(cfg, max_feats=T, features_dim=FEAT, ds_factor_attn=8, ds_factor_ff=8, dropout=0.1, n_ans=n_ans)
    m.to(dev).eval()
    g = torch.Generator().manual_seed(1)
    a2tok = torch.randint(5, cfg.vocab_size, (n_ans, 5), generator=g)
    m.set_answer_embeddings((a2tok * (torch.arange(5)[None] < torch.randint(1, 6, (n_ans, 1), generator=g))).to(dev))
    m.train()
    opt = FusedAdam(m, lr=1e-5)
    if name == "videoqa_short":
        B, C = 32, 1
        ids, tlen = texts(B, 8, 24, seed=5)
        target = torch.randint(0, n_ans, (B,), generator=g).to(dev)
    elif name == "videoqa":
        B, C = 32, 1
        ids, tlen = texts(B, 8, 64, seed=2)
        target = torch.randint(0, n_ans, (B,), generator=g).to(dev)
    else:
        B, C = 8, 4
        ids, tlen = texts(C * B, 64, 502, seed=3)
        target = torch.randint(0, C, (B,), generator=g).to(dev)
    if a.pad_to_bucket:
        Lb = min(-(-ids.shape[1] // m.GRAPH_L_BUCKET) * m.GRAPH_L_BUCKET, cfg.max_position_embeddings - T)
        ids = F.pad(ids, (0, Lb - ids.shape[1]))
    n = ids.shape[0]
    S = T + ids.shape[1]
    vlen = torch.randint(1, T + 1, (B,), generator=g)
    video = torch.randn(B, T, FEAT, generator=g).half().float().repeat(C, 1, 1).to(dev)
    vmask = (torch.arange(T)[None] < vlen[:, None]).long().repeat(C, 1).to(dev)
    feed = dict(video=video, video_mask=vmask, input_ids=ids.to(dev), attention_mask=(ids != 0).long().to(dev))
    rows_packed = int((tlen + T).sum())  # every sample keeps its video slots and its text up to the last token

    names = m.trainable_names()
    named = dict(m.named_parameters())
    nL = cfg.num_hidden_layers

    def set_live(kind):
        """partial fine-tuning legs: None = everything live; "topK" = adapters and LayerNorms of the top K layers (the head's
        LayerNorm with them), linear_video and everything below dead; "no_relln" = everything but deberta.encoder.LayerNorm"""
        for n in names:
            if kind is None:
                on = True
            elif kind == "no_relln":
                on = not n.startswith("deberta.encoder.LayerNorm.")
            else:
                k = int(kind[3:])
                on = n.startswith("lm_predictions.") or (n.startswith("deberta.encoder.layer.") and int(n.split(".")[3]) >= nL - k)
            named[n].requires_grad_(on)

    def step(live=None, **opt_in):
        set_live(live)
        args = types.SimpleNamespace(max_feats=T, use_video=True, **opt_in)
        m.packed_rows = bool(opt_in.get("packed_rows"))
        m.decoder_rows = bool(opt_in.get("decoder_rows"))
        m.finetune_graphs = bool(opt_in.get("finetune_graphs"))
        opt.zero_grad()
        logits = P_vqa.answer_logits(m, Tok, ids, args, **feed)
        if C == 1:
            loss = F.cross_entropy(logits, target)
        else:
            loss = P_mc.mc_loss(logits.softmax(-1)[:, 0].view(C, B).t(), target, C)
        loss.backward()
        opt.step(clip_max_norm=0.1)

    legs = {"full": lambda: step(), "rows": lambda: step(train_logit_rows=True), "rows_packed": lambda: step(packed_rows=True),
            "rows_decoder": lambda: step(train_logit_rows=True, decoder_rows=True),
            "rows_packed_decoder": lambda: step(packed_rows=True, decoder_rows=True),
            "rows_graphs": lambda: step(finetune_graphs=True),
            # partial fine-tuning (the default route, flags toggled): the backward stops below the lowest live layer
            "live_top24": lambda: step(live="top24"), "live_top12": lambda: step(live="top12"), "live_top4": lambda: step(live="top4"),
            "live_no_relln": lambda: step(live="no_relln")}
    if a.legs:
        legs = {k: legs[k] for k in a.legs.split(",")}
    res = {"shape": dict(samples=n, S=S, T=T, n_ans=n_ans, candidates=C, layers=cfg.num_hidden_layers, mask_rows=n),
           "rows": {"padded": n * S, "packed": rows_packed, "share": round(rows_packed / (n * S), 3)},
           "step_ms": alternate_stats(legs, a.steps, a.warmup), "host_ms": host_issue_stats(legs, a.steps),
           "peak_mb": peak_memory(legs),
           "graph_captures": TG.stats(m, TG.FINETUNE).captures,
           "graph_replays": TG.stats(m, TG.FINETUNE).replays}
    if "full" in legs:
        full = res["step_ms"]["full"]["median"]
        res["speedup_vs_full"] = {k: round(full / v["median"], 3) for k, v in res["step_ms"].items() if k != "full"}
    if "rows" in legs and "rows_graphs" in legs:
        res["graphs_vs_rows"] = round(res["step_ms"]["rows"]["median"] / res["step_ms"]["rows_graphs"]["median"], 3)
    del m, opt
    torch.cuda.empty_cache()
    return res


def workload_mlm():
    cfg = DebertaV2Config()
    if a.layers:
        cfg.num_hidden_layers = a.layers
    torch.manual_seed(0)
    m = DebertaV2ForMaskedLM(cfg, max_feats=T, features_dim=FEAT, ds_factor_attn=8, ds_factor_ff=8, dropout=0.1)
    m.to(dev).train()
    opt = FusedAdam(m, lr=1e-5)
    g = torch.Generator().manual_seed(4)
    B, Lt = 32, 256
    tlen = torch.randint(32, Lt + 1, (B,), generator=g)
    tlen[-1] = Lt
    valid = torch.arange(Lt)[None] < tlen[:, None]
    ids = torch.randint(5, 127000, (B, Lt), generator=g) * valid
    labels = torch.where(valid & (torch.rand(B, Lt, generator=g) < 0.15), ids, torch.full_like(ids, -100))
    ids = torch.where(labels != -100, torch.full_like(ids, MASK), ids)
    feed = dict(video=torch.randn(B, T, FEAT, generator=g).half().float().to(dev), video_mask=torch.ones(B, T, dtype=torch.long, device=dev),
                input_ids=ids.to(dev), attention_mask=valid.long().to(dev), labels=labels.to(dev))

    def step(on):
        m.decoder_rows = on
        opt.zero_grad()
        m(**feed).loss.backward()
        opt.step(clip_max_norm=0.1)

    legs = {"default": lambda: step(False), "decoder_rows": lambda: step(True)}
    res = {"shape": dict(samples=B, S=T + Lt, T=T, layers=cfg.num_hidden_layers, labelled_rows=int((labels != -100).sum()),
                         rows=B * (T + Lt)),
           "step_ms": alternate_stats(legs, a.steps, a.warmup)}
    res["speedup_vs_default"] = round(res["step_ms"]["default"]["median"] / res["step_ms"]["decoder_rows"]["median"], 3)
    del m, opt
    torch.cuda.empty_cache()
    return res


out = {"device": torch.cuda.get_device_name(0),
       "method": "device events around forward + loss + backward + clipped FusedAdam, train mode (dropout live); the legs of a workload "
                 f"alternate inside one process; median, 10th and 90th percentile of {a.steps} timed iterations after {a.warmup} "
                 "warm-up iterations; host_ms: wall clock the host spends inside the step call, the device idle in front of it, in a pass of its own"}
for w in ("videoqa_short", "videoqa", "mc"):
    if a.only in (None, w):
        out[w] = workload(w)
if a.only in (None, "mlm"):
    out["mlm"] = workload_mlm()
print(json.dumps(out))
