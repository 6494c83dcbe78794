"""Where the compact backward pays: the headline training step at the bench shape, the share of rows that exist swept
(one JSON object).

    python tools/bench_compact_bwd.py [--steps K] [--warmup W] [--layers N] [--shares 1.0,0.9,...]

The workload is the masked-LM step of bench.py -- B = 32, T = 10 video slots, text padded to 256 tokens (S = 266, 8512 grid rows),
labels on 15 % of the tokens, forward with `labels`, backward, clipped FusedAdam, train mode with every dropout site live.  Per
share Np/N the text lengths are set so that this share of the grid rows exists (one sample keeps 256 tokens, the others share
the rest evenly); 0.625 is the share of the bench batch.  Two legs alternate inside one process (one model, one optimizer, every
leg a real update): `padded` (model.compact_backward = False: the backward on the padded grid) and `compact`
(model.compact_backward = True: the route forced on whatever the share).  Per leg the median and the 10th / 90th percentile of
the device-event times; per share the gain and `spread_ms`, the p90 - p10 band of the padded leg.

`break_even`: the gain is not smooth in the share -- the big dX GEMMs lose time only where the row count drops below a whole
round of 256-row tiles over the chip -- so the sweep is read as a step: `largest_dropped_share_not_faster` is the
largest dropped share (1 - Np/N) at which compact does not beat padded by more than the run-to-run spread (the widest
p90 - p10 band of a padded leg in this sweep), `min_dropped` the smallest share of the sweep above it, from which on every
point of the sweep wins by more than that spread: the value of Engine.COMPACT_BWD_MIN_DROPPED.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from frozenbilm_amd.model import DebertaV2Config, DebertaV2ForMaskedLM
from frozenbilm_amd.optim import FusedAdam

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20, help="timed iterations per leg and share")
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--layers", type=int, default=0, help="encoder layers (0: the xlarge model's 24)")
ap.add_argument("--shares", default="1.0,0.9,0.8,0.7,0.66,0.65,0.64,0.63,0.625,0.55,0.45")
a = ap.parse_args()
dev = torch.device("cuda")
T, FEAT, MASK, B, Lt = 10, 768, 128000, 32, 256
S = T + Lt


def band(t):
    t = sorted(t)
    pick = lambda q: round(t[min(len(t) - 1, int(q * len(t)))], 3)
    return {"median": pick(0.5), "p10": pick(0.1), "p90": pick(0.9), "n": len(t)}


def batch_of(share, g):
    """text lengths with sum(T + tlen) ~= share * B * S: the last sample full, the others equal (the remainder spread one by one)"""
    rest = max(int(round(share * B * S)) - S - (B - 1) * T, B - 1)
    tlen = torch.full((B,), rest // (B - 1), dtype=torch.long)
    tlen[: rest % (B - 1)] += 1
    tlen = tlen.clamp(2, Lt)
    tlen[-1] = Lt
    valid = torch.arange(Lt)[None] < tlen[:, None]
    ids = torch.randint(5, 127000, (B, Lt), generator=g) * valid
    labels = torch.where(valid & (torch.rand(B, Lt, generator=g) < 0.15), ids, torch.full_like(ids, -100))
    labels[:, 1] = ids[:, 1]
    ids = torch.where(labels != -100, torch.full_like(ids, MASK), ids)
    feed = dict(video=torch.randn(B, T, FEAT, generator=g).half().float().to(dev), video_mask=torch.ones(B, T, dtype=torch.long, device=dev),
                input_ids=ids.to(dev), attention_mask=valid.long().to(dev), labels=labels.to(dev))
    return feed, int((tlen + T).sum())


cfg = DebertaV2Config()
if a.layers:
    cfg.num_hidden_layers = a.layers
torch.manual_seed(0)
m = DebertaV2ForMaskedLM(cfg, max_feats=T, features_dim=FEAT, ds_factor_attn=8, ds_factor_ff=8, dropout=0.1)
m.to(dev).train()
opt = FusedAdam(m, lr=1e-5)
g = torch.Generator().manual_seed(4)
used = {}


def step(feed, on):
    m.compact_backward = on
    opt.zero_grad()
    out = m(**feed)
    out.loss.backward()
    used[on] = out._run.bwd_compact
    opt.step(clip_max_norm=0.1)


sweep = []
for share in [float(x) for x in a.shares.split(",")]:
    feed, rows = batch_of(share, g)
    ev = {"padded": [], "compact": []}
    for it in range(a.warmup + a.steps):
        for name, on in (("padded", False), ("compact", True)):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            step(feed, on)
            e.record()
            if it >= a.warmup:
                ev[name].append((s, e))
    torch.cuda.synchronize()
    st = {k: band([s.elapsed_time(e) for s, e in v]) for k, v in ev.items()}
    sweep.append({"share_target": share, "rows": rows, "rows_padded": B * S, "dropped": round(1.0 - rows / (B * S), 4),
                  "compact_route_ran": bool(used[True]), "step_ms": st,
                  "gain_ms": round(st["padded"]["median"] - st["compact"]["median"], 3),
                  "spread_ms": round(st["padded"]["p90"] - st["padded"]["p10"], 3)})

spread = max(r["spread_ms"] for r in sweep)
ran = sorted((r for r in sweep if r["compact_route_ran"]), key=lambda r: r["dropped"])
losing = [r["dropped"] for r in ran if r["gain_ms"] <= spread]
winning = [r["dropped"] for r in ran if not losing or r["dropped"] > max(losing)]
out = {"device": torch.cuda.get_device_name(0),
       "method": "device events around forward + backward + clipped FusedAdam, train mode; the padded and the compact leg alternate "
                 f"inside one process; median / p10 / p90 of {a.steps} timed iterations after {a.warmup} warm-up iterations per share",
       "layers": cfg.num_hidden_layers, "sweep": sweep, "spread_ms": spread,
       "break_even": {"largest_dropped_share_not_faster": max(losing) if losing else None, "min_dropped": min(winning) if winning else None}}
print(json.dumps(out))
