"""Device-event timings of fbl_adam_flat_groups (include/fbl_groups.h) against fbl_adam_flat_live on the same ranges; one JSON
object.

    python tools/bench_adam_groups.py [--timings 5] [--launches 20] [--warmup 3] [--out FILE]

The buffers have the xlarge model's trainable size (30 128 640 floats: linear_video, 48 adapters, the LayerNorms; the layout
comes from the model's own shape table, no model is built).  Two live patterns: everything live, and the partial-fine-tuning
pattern "top two layers live".  Legs per pattern: fbl_adam_flat_live (the yardstick), fbl_adam_flat_groups with 1 group, and
with 54 groups (the 27 backward stages x {decayed, undecayed}, every one with its own rate and decay, AdamW).  All with the clip
on (a device norm is read).  A timing is the device time of `--launches` back-to-back launches divided by their number; the legs
alternate inside each timing; per leg all timings, their median and their spread (max - min).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from frozenbilm_amd import lib as L
from frozenbilm_amd import live_set as LS
from frozenbilm_amd import param_groups as PG
from frozenbilm_amd.model import DebertaV2Config
from frozenbilm_amd.model.deberta import flat_order, param_shapes

ap = argparse.ArgumentParser()
ap.add_argument("--timings", type=int, default=5)
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=None, help="also write the JSON object to this file")
a = ap.parse_args()
dev = torch.device("cuda")

cfg = DebertaV2Config()
nL = cfg.num_hidden_layers
shapes = param_shapes(cfg, 1024, 8, 8, 0)
names = [n for n in shapes if "linear_video" in n or "adapter" in n or "LayerNorm" in n]
order = flat_order(cfg, names)
numel = {n: 1 for n in order}
for n in order:
    for d in shapes[n]:
        numel[n] *= d
offsets, N = LS.flat_layout(order, numel)
assert N == 30128640, N
stages = LS.stage_names(nL, cfg.conv_kernel_size > 0)
assert len(stages) == 27
group54 = {n: 2 * stages.index(LS.stage_of(n, nL)) + int("LayerNorm" in n or "bias" in n) for n in order}
top_two = [n for n in order if n.startswith(f"deberta.encoder.layer.{nL - 1}.") or n.startswith(f"deberta.encoder.layer.{nL - 2}.")]

g_ = torch.Generator(device=dev).manual_seed(3)
p = torch.randn(N, generator=g_, device=dev) * 0.05
g = torch.randn(N, generator=g_, device=dev) * 0.01
m = torch.zeros(N, device=dev)
v = torch.zeros(N, device=dev)
ss = torch.ones(1, device=dev)
LR, B1, B2, EPS, WD = 3e-4, 0.9, 0.95, 1e-8, 0.01
hyper1 = L.adam_hyper([(LR, B1, B2, EPS, WD, False)])
hyper54 = L.adam_hyper([(LR * 0.9 ** (26 - k // 2), B1, B2, EPS, 0.0 if k % 2 else WD, True) for k in range(54)])


def band(t):
    t = sorted(t)
    return {"timings_us": [round(x, 2) for x in t], "median_us": round(t[len(t) // 2], 2), "spread_us": round(t[-1] - t[0], 2)}


res = {"n": N, "launches_per_timing": a.launches}
for pat, live in (("all_live", order), ("top_two_layers_live", top_two)):
    ranges = LS.live_ranges(order, offsets, numel, live)
    live_tab = L.live_table(ranges, N, dev)
    seg1 = PG.segments(order, offsets, numel, live, {n: 0 for n in order})
    seg54 = PG.segments(order, offsets, numel, live, group54)
    tab1, tab54 = L.group_table(seg1, N, dev, 1), L.group_table(seg54, N, dev, 54)
    legs = {
        "adam_flat_live": lambda: L.adam_flat_live(p, g, m, v, live_tab, LR, B1, B2, EPS, WD, 3, sumsq_t=ss, max_norm=1.0),
        "groups_1": lambda: L.adam_flat_groups(p, g, m, v, tab1, hyper1, 3, sumsq_t=ss, max_norm=1.0),
        "groups_54": lambda: L.adam_flat_groups(p, g, m, v, tab54, hyper54, 3, sumsq_t=ss, max_norm=1.0),
    }
    times = {k: [] for k in legs}
    for it in range(a.warmup + a.timings):
        for k, f in legs.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(a.launches):
                f()
            e.record()
            e.synchronize()
            if it >= a.warmup:
                times[k].append(1e3 * s.elapsed_time(e) / a.launches)
    n_live = sum(e - b for b, e in ranges)
    res[pat] = {"live_elements": n_live, "ranges": len(ranges), "segments_1": len(seg1), "segments_54": len(seg54),
                "groups_met_54": len({k for _, _, k in seg54}), **{k: band(t) for k, t in times.items()}}
    for k in legs:
        res[pat][k]["GB_per_s"] = round(28.0 * n_live / (res[pat][k]["median_us"] * 1e-6) / 1e9, 1)
print(json.dumps(res))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
