"""Device-event timings of the row predictions (`model.predict_topk`, include/fbl_predict.h); one JSON object.

    python tools/bench_predict.py [--steps K] [--warmup W] [--layers N] [--out FILE]

1. The kernel, fbl_row_predict, at (R, V) = (1277, 128100), (32, 128100), (32, 1000) with k = 5, labels and a given row_lse
   (what a labelled call runs), against the torch route on the SAME fp32 [R, ldv] buffer:
   `torch.topk(x[:, :V], 5)` + `torch.logsumexp(x[:, :V], 1)` + the rank comparison `(x[:, :V] > x_label).sum(1)`.
2. The MLM training step at the benchmark shape (B = 32, 10 video slots, 256 text tokens, ~1300 labelled rows): forward with
   labels, backward, clipped FusedAdam, train mode -- with predict_topk = 0, with predict_topk = 5, and with predict_topk = 0
   plus `out.logits.view(-1, V)[rows].topk(5)`, which fills the [B*S, V] logits: the only route to the predictions without
   this feature.

The legs of a group alternate inside one process; per leg the median and the 10th / 90th percentile of the timed iterations.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench as Bn
from frozenbilm_amd import lib as L
from frozenbilm_amd.model import DebertaV2Config, DebertaV2ForMaskedLM
from frozenbilm_amd.optim import FusedAdam

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20, help="timed iterations per leg (at least 20 for the record)")
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--layers", type=int, default=0, help="encoder layers of the step (0: the xlarge model's 24)")
ap.add_argument("--no-step", action="store_true", help="kernel timings only")
ap.add_argument("--out", default=None, help="also write the JSON object to this file")
a = ap.parse_args()
dev = torch.device("cuda")
K = 5


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


def kernel_legs(R, V):
    g = torch.Generator(device=dev).manual_seed(R + V)
    ld = (V + 63) // 64 * 64
    x = torch.randn(R, ld, generator=g, device=dev) * 3.0
    labels = torch.randint(0, V, (R,), generator=g, device=dev)
    lse = torch.logsumexp(x[:, :V], 1)

    def kernel():
        L.row_predict(x, V, K, labels=labels, row_lse=lse)

    def kernel_own_lse():
        L.row_predict(x, V, K, labels=labels)

    def torch_route():
        xv = x[:, :V]
        top = torch.topk(xv, K, dim=1)
        ls = torch.logsumexp(xv, 1)
        xl = xv.gather(1, labels[:, None])
        rank = (xv > xl).sum(1)
        return top.indices, top.values - ls[:, None], rank, ls - xl[:, 0]

    ids, _, rank, _ = L.row_predict(x, V, K, labels=labels, row_lse=lse)
    t_ids, _, t_rank, _ = torch_route()
    assert torch.equal(ids.long(), t_ids) and torch.equal(rank.long(), t_rank)  # (continuous random logits: no ties)
    res = alternate_stats({"kernel": kernel, "kernel_computing_lse": kernel_own_lse, "torch": torch_route}, a.steps, a.warmup)
    res["bytes_read"] = R * V * 4
    res["kernel_GBps"] = round(R * V * 4 / res["kernel"]["median"] / 1e6, 1)
    res["torch_over_kernel"] = round(res["torch"]["median"] / res["kernel"]["median"], 2)
    return res


def step_legs():
    cfg = DebertaV2Config()
    if a.layers:
        cfg.num_hidden_layers = a.layers
    torch.manual_seed(0)
    m = DebertaV2ForMaskedLM(cfg, max_feats=10, features_dim=1024, ds_factor_attn=8, ds_factor_ff=8, dropout=0.1)
    m.to(dev).train()
    opt = FusedAdam(m, lr=3e-5, betas=(0.9, 0.95))
    B, T, Lt = 32, 10, 256
    batch = Bn.synth_batch(B, T, 1024, Lt, cfg.vocab_size, seed=1, device=dev)
    keep = []

    def step(k, full_logits=False):
        m.predict_topk = k
        opt.zero_grad()
        out = m(**batch)
        if full_logits:
            rows = out._run.rows
            keep[:] = [out.logits.view(-1, out.logits.shape[-1])[rows].topk(K, dim=1)]
        elif k:
            keep[:] = [out.predictions.accuracy(1), out.predictions.accuracy(K)]
        out.loss.backward()
        opt.step(clip_max_norm=0.1)

    legs = {"predict_topk_0": lambda: step(0), "predict_topk_5": lambda: step(K),
            "logits_topk_5": lambda: step(0, full_logits=True)}
    res = {"shape": dict(samples=B, S=T + Lt, layers=cfg.num_hidden_layers, labelled_rows=int((batch["labels"] != -100).sum()),
                         rows=B * (T + Lt)),
           "step_ms": alternate_stats(legs, a.steps, a.warmup)}
    ms = res["step_ms"]
    res["predict_topk_5_minus_0_ms"] = round(ms["predict_topk_5"]["median"] - ms["predict_topk_0"]["median"], 3)
    res["logits_topk_5_minus_0_ms"] = round(ms["logits_topk_5"]["median"] - ms["predict_topk_0"]["median"], 3)
    return res


out = {"device": torch.cuda.get_device_name(0),
       "method": f"device events; the legs of a group alternate inside one process; median, 10th and 90th percentile of {a.steps} "
                 f"timed iterations after {a.warmup} warm-up iterations; k = {K}",
       "kernel_ms": {f"R{R}_V{V}": kernel_legs(R, V) for R, V in ((1277, 128100), (32, 128100), (32, 1000))}}
if not a.no_step:
    out["mlm_step"] = step_legs()
text = json.dumps(out)
print(text)
if a.out:
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
