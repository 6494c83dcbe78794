"""Device-event timings of prompt tuning (`n_prompt`, include/fbl_prompt.h); one JSON object.

    python tools/bench_prompt.py [--steps K] [--warmup W] [--layers N] [--prompt P] [--prompt-depth D [D ...]] [--out FILE] [--p0-only]

BASELINE config 2 (DeBERTa-v2-XLarge + adapters, B = 32, 10 video slots, 256 text tokens), a model without a prompt and a model
with P = 20 prompt slots side by side in one process, the legs alternating (rows 32 x 266 against 32 x 286):

1. the MLM training step: forward with labels, backward, clipped FusedAdam, train mode;
2. the two kernels alone at that shape -- fbl_embed_assemble beside fbl_embed_gather (the P = 0 launch it stands in for) and
   beside the torch imitation (gather, expand, concatenate); fbl_prompt_grad beside the torch slice + sum.

--prompt-depth: one model with P prompt slots per depth given (1: the shallow prompt; D > 1: layers 1 .. D-1 read prompt rows of
their own, include/fbl_prompt_layers.h), all legs alternating; with a depth above 1 the row kernels of a deep layer are timed too:
the materialise of its input stream, fbl_prompt_rows_write and fbl_prompt_rows_grad.

--p0-only: the P = 0 leg alone, through a constructor call without the argument -- the same file runs on a tree that predates
it, for the comparison of the default path with the parent commit (run the two trees in turn, several times each).
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
ap.add_argument("--prompt", type=int, default=20)
ap.add_argument("--prompt-depth", type=int, nargs="+", default=[1], help="prompt_depth of the legs with a prompt (one model each)")
ap.add_argument("--p0-only", action="store_true")
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
B, T, Lt, P = 32, 10, 256, a.prompt
batch = Bn.synth_batch(B, T, 1024, Lt, cfg.vocab_size, seed=1, device=dev)


def make(n_prompt, depth=1):
    torch.manual_seed(0)
    kw = dict(n_prompt=n_prompt) if n_prompt else {}
    if depth != 1:
        kw["prompt_depth"] = depth
    m = DebertaV2ForMaskedLM(cfg, max_feats=10, features_dim=1024, ds_factor_attn=8, ds_factor_ff=8, dropout=0.1, **kw)
    m.to(dev).train()
    return m, FusedAdam(m, lr=3e-5, betas=(0.9, 0.95))


models = {"p0": make(0)}
leg = lambda d: f"p{P}" if d == 1 else f"p{P}d{d}"  # noqa: E731
first = leg(a.prompt_depth[0])
if not a.p0_only:
    for d in a.prompt_depth:
        models[leg(d)] = make(P, d)


def train_step(m, opt):
    opt.zero_grad()
    out = m(**batch)
    out.loss.backward()
    opt.step(clip_max_norm=0.1)


out = {"device": torch.cuda.get_device_name(0),
       "method": f"device events; the legs of a group alternate inside one process; median, 10th and 90th percentile of {a.steps} "
                 f"timed iterations after {a.warmup} warm-up iterations",
       "shape": dict(samples=B, video_slots=T, text=Lt, prompt=0 if a.p0_only else P, prompt_depth=[] if a.p0_only else a.prompt_depth, layers=cfg.num_hidden_layers,
                     rows={k: B * (T + Lt + (0 if k == "p0" else P)) for k in models})}
out["train_step_ms"] = alternate_stats({k: (lambda mo=mo: train_step(*mo)) for k, mo in models.items()}, a.steps, a.warmup)
if not a.p0_only:
    from frozenbilm_amd import lib as L

    tr = out["train_step_ms"]
    out["train_overhead_ms"] = {k: round(v["median"] - tr["p0"]["median"], 3) for k, v in tr.items() if k != "p0"}
    if len(out["train_overhead_ms"]) == 1:
        out["train_overhead_ms"] = out["train_overhead_ms"][first]
    out["train_ms_per_1000_rows"] = {k: round(v["median"] / out["shape"]["rows"][k] * 1000, 3) for k, v in tr.items()}
    H, S = cfg.hidden_size, T + P + Lt
    eng = models[first][0].engine()
    ids, E, prompt = batch["input_ids"].contiguous(), eng.E32, eng.P["deberta.embeddings.prompt_embeddings.weight"]
    vproj = torch.randn(B * T, H, device=dev)
    t_new, t_old = torch.empty(B, S, H, device=dev), torch.empty(B * (T + Lt), H, device=dev)
    dt0, g = torch.randn(B * S, H, device=dev), torch.zeros(P, H, device=dev)
    out["kernels_ms"] = alternate_stats({
        "fbl_embed_assemble": lambda: L.embed_assemble(ids, E, vproj, prompt, T, Lt, t_new),
        "fbl_embed_gather_p0": lambda: L.embed_gather(ids, E, vproj, T, t_old),
        "torch_gather_expand_cat": lambda: torch.cat([vproj.view(B, T, H), prompt.expand(B, -1, -1), E[ids]], 1),
        "fbl_prompt_grad": lambda: L.prompt_grad(dt0, None, B, S, T, g),
        "torch_slice_sum": lambda: g.add_(dt0.view(B, S, H)[:, T:T + P].sum(0)),
    }, max(a.steps, 50), a.warmup)
    out["kernel_bytes"] = dict(embed_assemble=2 * B * S * H * 4, prompt_grad=(B + 2) * P * H * 4)
    if max(a.prompt_depth) > 1:  # the row kernels one deep layer adds to a step, at this shape
        n = eng.P["deberta.encoder.layer.0.output.LayerNorm.weight"]
        t_, stats = torch.randn(B * S, H, device=dev), torch.stack([torch.zeros(B * S, device=dev), torch.ones(B * S, device=dev)], 1)
        f32, b16 = torch.empty(B * S, H, device=dev), torch.empty(B * S, H, dtype=torch.bfloat16, device=dev)
        dx = torch.randn(B * S, H, device=dev)
        out["deep_layer_kernels_ms"] = alternate_stats({
            "fbl_ln_materialize": lambda: L.ln_materialize(t_, stats.contiguous(), n, n, out_f32=f32, out_bf16=b16),
            "fbl_prompt_rows_write": lambda: L.prompt_rows_write(prompt, None, B, S, T, out_f32=f32, out_bf16=b16),
            "fbl_prompt_rows_grad": lambda: L.prompt_rows_grad(dx, None, B, S, T, P, g),
        }, max(a.steps, 50), a.warmup)
        out["deep_layer_kernel_bytes"] = dict(ln_materialize=B * S * H * (4 + 4 + 2), prompt_rows_write=B * P * H * (4 + 2) + P * H * 4,
                                              prompt_rows_grad=(2 * B + 2) * P * H * 4)
print(json.dumps(out))
if a.out:
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
