"""Device-event timings of LoRA on the frozen Q/K/V projections (`lora_rank`, include/fbl_lora.h); one JSON object.

    python tools/bench_lora.py [--steps K] [--warmup W] [--layers N] [--rank R] [--out FILE] [--rank0-only]

BASELINE config 2 (DeBERTa-v2-XLarge + adapters, B = 32, 10 video slots, 256 text tokens), a rank-0 model and a model with
r = 16 on (query_proj, value_proj) side by side in one process, the legs alternating:

1. the MLM training step: forward with labels, backward, clipped FusedAdam, train mode;
2. the eval forward inside `model.weights_frozen()` (the merged route: nothing is composed, the launches are the rank-0 model's);
3. the compose launch alone (fbl_lora_compose over all sites) and the refresh of the position-chain copies.

Next to the measured overhead: a byte count of the compose (W fp32 read, two bf16 layouts written) and of the four narrow
products per site and execution (u = s.x.A^T, v = s.dy.B, dB += dy^T.u, dA += v^T.x: x and dy are read twice each).
--rank0-only: the rank-0 legs alone, through a constructor call without the LoRA arguments -- the same file runs on a tree
that predates them, for the comparison of the default path with the parent commit.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench as Bn
from frozenbilm_amd.model import DebertaV2Config, DebertaV2ForMaskedLM
from frozenbilm_amd.optim import FusedAdam

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20, help="timed iterations per leg (at least 20 for the record)")
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--layers", type=int, default=0, help="encoder layers (0: the xlarge model's 24)")
ap.add_argument("--rank", type=int, default=16)
ap.add_argument("--rank0-only", action="store_true")
ap.add_argument("--out", default=None, help="also write the JSON object to this file")
a = ap.parse_args()
dev = torch.device("cuda")
TARGETS = ("query_proj", "value_proj")


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
B, T, Lt = 32, 10, 256
batch = Bn.synth_batch(B, T, 1024, Lt, cfg.vocab_size, seed=1, device=dev)
eval_batch = {k: v for k, v in batch.items() if k != "labels"}


def make(rank):
    torch.manual_seed(0)
    kw = dict(lora_rank=rank, lora_targets=TARGETS) if rank else {}
    m = DebertaV2ForMaskedLM(cfg, max_feats=10, features_dim=1024, ds_factor_attn=8, ds_factor_ff=8, dropout=0.1, **kw)
    m.to(dev).train()
    if rank:  # a trained LoRA: B is not zero
        g = torch.Generator().manual_seed(2)
        for nm in m.lora_names():
            p = m.get_param(nm + ".lora_B.weight")
            p.data.copy_(torch.randn(p.shape, generator=g) * 0.02)
    return m, FusedAdam(m, lr=3e-5, betas=(0.9, 0.95))


models = {"rank0": make(0)}
if not a.rank0_only:
    models[f"r{a.rank}"] = make(a.rank)


def train_step(m, opt):
    m.train()
    opt.zero_grad()
    out = m(**batch)
    out.loss.backward()
    opt.step(clip_max_norm=0.1)


def eval_forward(m):
    with torch.no_grad():
        m(**batch).loss


out = {"device": torch.cuda.get_device_name(0),
       "method": f"device events; the legs of a group alternate inside one process; median, 10th and 90th percentile of {a.steps} "
                 f"timed iterations after {a.warmup} warm-up iterations",
       "shape": dict(samples=B, S=T + Lt, rows=B * (T + Lt), layers=cfg.num_hidden_layers, rank=a.rank, targets=list(TARGETS))}
out["train_step_ms"] = alternate_stats({k: (lambda mo=mo: train_step(*mo)) for k, mo in models.items()}, a.steps, a.warmup)
for m, _ in models.values():
    m.eval()
import contextlib

with contextlib.ExitStack() as st:
    for m, _ in models.values():
        st.enter_context(m.weights_frozen())
    out["eval_forward_frozen_ms"] = alternate_stats({k: (lambda mo=mo: eval_forward(mo[0])) for k, mo in models.items()}, a.steps,
                                                    a.warmup)
if not a.rank0_only:
    from frozenbilm_amd import lib as L

    key = f"r{a.rank}"
    eng = models[key][0].engine()
    H, nL, N, r = cfg.hidden_size, cfg.num_hidden_layers, B * (T + Lt), a.rank
    sites = len(eng.lora_sites)
    out["compose_ms"] = alternate_stats({"fbl_lora_compose": lambda: L.lora_compose(eng._lora_table),
                                         "compose_and_position_copies": eng._compose_lora}, a.steps, a.warmup)
    execs = nL + 1  # layers 0 .. nL-2 once, the last layer's two decoder passes
    compose_bytes = sites * H * H * (4 + 2 + 2)
    pos_copy_bytes = (nL + 2) * H * 2 * H * 2 * 2 if eng._lora_pos else 0
    products_bytes = execs * len(TARGETS) * (4 * N * H * 2 + 4 * N * 64 * 2)
    tr = out["train_step_ms"]
    out["estimate"] = dict(sites=sites, compose_bytes=compose_bytes, position_copy_bytes=pos_copy_bytes,
                           products_bytes=products_bytes, executions=execs,
                           compose_ms_at_4TBps=round(compose_bytes / 4e9, 3), products_ms_at_4TBps=round(products_bytes / 4e9, 3))
    out["train_overhead_ms"] = round(tr[key]["median"] - tr["rank0"]["median"], 3)
    ev = out["eval_forward_frozen_ms"]
    out["eval_overhead_ms"] = round(ev[key]["median"] - ev["rank0"]["median"], 3)
print(json.dumps(out))
if a.out:
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
