"""Device-event timings of the moving average of the trainable weights (`FusedAdam(..., ema_decay=)`, include/fbl_ema.h); one
JSON object.

    python tools/bench_ema.py [--steps K] [--warmup W] [--layers N] [--out FILE]

The xlarge model (DeBERTa-v2-XLarge + adapters; its flat trainable buffer has 30 128 640 floats) is built once.

1. the clipped optimizer step on buffers of that size, the legs alternating in one process: the norm (fbl_sumsq) plus
   fbl_adam_flat (the default step), plus fbl_adam_flat_groups over one segment, plus fbl_adam_flat_groups_ema over one segment
   (the step with EMA on), and the same three over the segments of 54 groups (layer-wise rates, AdamW);
2. what entering `model.ema_weights()` costs: fbl_swap_f32 over the flat buffer, and the rebuild of the engine's operands that
   the bumped `params_version` causes (refresh_trainable_operands, joined with the side stream that composes the merged rows);
   next to them the eval forward inside `weights_frozen()` with the operands reused and right after an exchange.

Per leg: median, 10th and 90th percentile of `--steps` timed iterations after `--warmup`, device events around each iteration.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench as Bn
from frozenbilm_amd import lib as L
from frozenbilm_amd import live_set as LS
from frozenbilm_amd import param_groups as PG
from frozenbilm_amd.model import DebertaV2Config, DebertaV2ForMaskedLM

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20, help="timed iterations per leg (at least 20 for the record)")
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--layers", type=int, default=0, help="encoder layers (0: the xlarge model's 24)")
ap.add_argument("--out", default=None, help="also write the JSON object to this file")
a = ap.parse_args()
dev = torch.device("cuda")


def band(t):
    t = sorted(t)
    pick = lambda q: round(t[min(len(t) - 1, int(q * len(t)))], 4)  # noqa: E731
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


cfg = DebertaV2Config()
if a.layers:
    cfg.num_hidden_layers = a.layers
nL = cfg.num_hidden_layers
torch.manual_seed(0)
model = DebertaV2ForMaskedLM(cfg, max_feats=10, features_dim=1024, ds_factor_attn=8, ds_factor_ff=8, dropout=0.1)
model.to(dev).eval()
eng = model.engine()
N = eng.flat.numel()
numel = {n: eng.named[n].numel() for n in eng.order}

# ---- 1. the clipped step on buffers of the flat buffer's size
g_ = torch.Generator(device=dev).manual_seed(3)
p = torch.randn(N, generator=g_, device=dev) * 0.05
g = torch.randn(N, generator=g_, device=dev) * 0.01
m, v = torch.zeros(N, device=dev), torch.zeros(N, device=dev)
ema = p.clone()
ss = torch.zeros(1, device=dev)
ws = torch.empty(L.load().fbl_sumsq_ws_floats(), dtype=torch.float32, device=dev)
LR, B1, B2, EPS, WD, W = 3e-4, 0.9, 0.95, 1e-8, 0.01, 1.0 - 0.999
stages = LS.stage_names(nL, cfg.conv_kernel_size > 0)
group_of = {n: 2 * stages.index(LS.stage_of(n, nL)) + int("LayerNorm" in n or "bias" in n) for n in eng.order}
ng = 2 * len(stages)
seg1 = PG.segments(eng.order, eng.offsets, numel, eng.order, {n: 0 for n in eng.order})
segk = PG.segments(eng.order, eng.offsets, numel, eng.order, group_of)
tab1, tabk = L.group_table(seg1, N, dev, 1), L.group_table(segk, N, dev, ng)
hyper1 = L.adam_hyper([(LR, B1, B2, EPS, WD, False)])
hyperk = L.adam_hyper([(LR * 0.9 ** (len(stages) - 1 - k // 2), B1, B2, EPS, 0.0 if k % 2 else WD, True) for k in range(ng)])


def clipped(update):
    def step():
        ss.zero_()
        L.sumsq(g, ss, ws=ws)
        update()
    return step


kw = dict(sumsq_t=ss, max_norm=1.0)
legs = {
    "adam_flat": clipped(lambda: L.adam_flat(p, g, m, v, LR, B1, B2, EPS, WD, 3, **kw)),
    "groups_1": clipped(lambda: L.adam_flat_groups(p, g, m, v, tab1, hyper1, 3, **kw)),
    "groups_1_ema": clipped(lambda: L.adam_flat_groups_ema(p, g, m, v, ema, tab1, hyper1, 3, W, **kw)),
    f"groups_{ng}": clipped(lambda: L.adam_flat_groups(p, g, m, v, tabk, hyperk, 3, **kw)),
    f"groups_{ng}_ema": clipped(lambda: L.adam_flat_groups_ema(p, g, m, v, ema, tabk, hyperk, 3, W, **kw)),
}
out = {"device": torch.cuda.get_device_name(0),
       "method": f"device events around every iteration; the legs of a group alternate inside one process; median, 10th and 90th "
                 f"percentile of {a.steps} timed iterations after {a.warmup} warm-up iterations",
       "n": N, "layers": nL, "segments": {"groups_1": len(seg1), f"groups_{ng}": len(segk)}}
out["clipped_step_ms"] = alternate_stats(legs, a.steps, a.warmup)
st = out["clipped_step_ms"]
out["ema_overhead_us"] = {"one_group_vs_default": round(1e3 * (st["groups_1_ema"]["median"] - st["adam_flat"]["median"]), 1),
                          "one_group_vs_groups": round(1e3 * (st["groups_1_ema"]["median"] - st["groups_1"]["median"]), 1),
                          f"{ng}_groups_vs_groups": round(1e3 * (st[f"groups_{ng}_ema"]["median"] - st[f"groups_{ng}"]["median"]), 1),
                          "bytes_more_per_step": 8 * N, "us_at_4TBps": round(8 * N / 4e12 * 1e6, 1)}

# ---- 2. entering ema_weights(): the exchange and the rebuild it causes
B, T, Lt = 32, 10, 256
batch = Bn.synth_batch(B, T, 1024, Lt, cfg.vocab_size, seed=1, device=dev)
avg = eng.flat.clone()


def rebuild():
    eng.refresh_trainable_operands()
    if eng._compose_ev is not None:  # the merged rows are composed on the side stream: the timing includes them
        torch.cuda.current_stream().wait_event(eng._compose_ev[1])


def forward():
    with torch.no_grad():
        model(**batch).loss


def forward_after_exchange():
    L.swap_(eng.flat, avg)
    eng.invalidate_operands()
    forward()


out["enter_ms"] = alternate_stats({"fbl_swap_f32": lambda: L.swap_(p, ema), "rebuild_operands": rebuild}, a.steps, a.warmup)
with model.weights_frozen():
    out["eval_forward_ms"] = alternate_stats({"operands_reused": forward, "after_exchange": forward_after_exchange}, a.steps,
                                             a.warmup)
out["shape"] = dict(samples=B, S=T + Lt, rows=B * (T + Lt))
print(json.dumps(out))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
