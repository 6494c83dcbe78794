"""HIP-event timings of the selected-query-row attention (include/fbl_qrows.h) beside the full-grid launches it would replace
in the two enhanced-mask-decoder executions, at the two shapes where few rows reach the head:

    mlm   B = 32, T = 10, ragged text U[32,256] with one sample of 256 (S = 266), labels on 15 % of the text tokens
    mc    B = 32, S = 512, ragged U[256,512], one [MASK] row per sample

    python tools/bench_attn_qrows.py [iters]        # prints one JSON line

Legs alternate inside one process; the median and the p10 / p90 of `iters` (default 30) timed calls per leg, in microseconds:
  full_fwd    fbl_disent_attn_fwd, saving its probabilities (the training forward)
  full_bwd    the shipped backward from the saved probabilities, position-table gradients included (attn_bwd.disent_attn_bwd)
  qrows_fwd   fbl_disent_attn_fwd_qrows
  qrows_bwd   fbl_disent_attn_bwd_qrows (three launches, position-table gradients included)

The full_bwd leg drives attn_bwd.disent_attn_bwd with bare stand-ins for the engine, the run and the saved state, as the kernel
tests do (that function names the attributes it reads for this purpose), and forms the position-table gradients of ONE execution
on its own, whereas a training step batches them over all executions (pos_table_grads_batched): the full-grid backward figure
is an upper bound of what one decoder execution costs inside a step.  Step-level numbers: tools/bench_finetune.py.
"""
import json
import math
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from frozenbilm_amd import lib as L
from frozenbilm_amd.attn_bwd import disent_attn_bwd
from frozenbilm_amd.model.relpos import rel_index_vector
from frozenbilm_amd.row_plan import plan_query_rows

ITERS = int(sys.argv[1]) if len(sys.argv) > 1 else 30
NH, SPAN2, DEV, BF16 = 24, 512, "cuda", torch.bfloat16
H = NH * 64
SCALE = 1 / math.sqrt(192)


def shape(name, g):
    B = 32
    if name == "mlm":
        T, S = 10, 266
        tl = torch.randint(32, 257, (B,), generator=g)
        tl[-1] = 256
        mask = torch.zeros(B, S, dtype=torch.int32)
        rows = []
        for b in range(B):
            mask[b, : T + tl[b]] = 1
            n = max(1, int(round(0.15 * int(tl[b]))))
            rows += (b * S + T + torch.randperm(int(tl[b]), generator=g)[:n]).tolist()
    else:
        S = 512
        ln = torch.randint(256, 513, (B,), generator=g)
        mask = torch.zeros(B, S, dtype=torch.int32)
        rows = []
        for b in range(B):
            mask[b, : ln[b]] = 1
            rows.append(b * S + int(ln[b]) - 2)
    return B, S, mask.to(DEV), torch.tensor(rows, device=DEV)


def main():
    g = torch.Generator().manual_seed(0)
    out = {}
    for name in ("mlm", "mc"):
        B, S, mask, rows = shape(name, g)
        Sp = (S + 63) // 64 * 64
        qkv = (torch.randn(B * S, 3 * H, generator=g) * 0.7).to(BF16).to(DEV)
        pqk = (torch.randn(SPAN2, 2 * H, generator=g) * 0.7).to(BF16).to(DEV)
        relidx = torch.from_numpy(rel_index_vector(S, 256, 512, 256).copy()).to(DEV)
        klen = (mask * torch.arange(1, S + 1, device=DEV, dtype=torch.int32)).amax(1).to(torch.int32).contiguous()
        border = torch.argsort(klen, descending=True, stable=True).to(torch.int32).contiguous()
        pl = plan_query_rows(rows, B, S)
        R = pl.R
        q, k, v, pq, pk = qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], pqk[:, :H], pqk[:, H:]
        # full grid
        ctx = torch.empty(B * S, H, dtype=BF16, device=DEV)
        lse = torch.empty(B, NH, S, device=DEV)
        psave = torch.empty(B, NH, Sp, Sp, dtype=BF16, device=DEV)
        msave = torch.empty(B, NH, Sp // 64, S, device=DEV)
        dctx = torch.zeros(B * S, H, dtype=BF16, device=DEV)
        dctx[pl.grid] = torch.randn(R, H, device=DEV).to(BF16)
        dqkv = torch.zeros(B * S, 3 * H, dtype=BF16, device=DEV)
        dpqk = torch.zeros(SPAN2, 2 * H, dtype=BF16, device=DEV)
        eng, run, sv = types.SimpleNamespace(), types.SimpleNamespace(), types.SimpleNamespace()
        eng.H, eng.nh, eng.span2, eng.dev = H, NH, SPAN2, torch.device(DEV)
        eng.relidx = lambda S_: relidx
        eng.cfg = types.SimpleNamespace(position_buckets=256, max_rel=512, att_span=256)
        run.B, run.S, run.mask_i32, run.p_att, run.klen, run.border = B, S, mask.view(-1), 0.1, klen, border
        sv.qkv, sv.pqk, sv.ctx, sv.lse, sv.seed_att, sv.psave, sv.msave = qkv, pqk, ctx, lse, 3, psave, msave
        # selected rows
        qc = q[pl.grid].contiguous()
        ctx_c = torch.empty(R, H, dtype=BF16, device=DEV)
        lse_c = torch.empty(NH, R, device=DEV)
        dO = dctx[pl.grid].contiguous()
        dQ = torch.empty(R, H, dtype=BF16, device=DEV)
        dKV = torch.empty(B * S, 2 * H, dtype=BF16, device=DEV)
        dPK, dPQ = torch.empty(NH, SPAN2, 64, device=DEV), torch.empty(NH, SPAN2, 64, device=DEV)
        ws = torch.empty(L.disent_attn_bwd_qrows_ws_bytes(R, Sp, NH), dtype=torch.uint8, device=DEV)
        legs = {
            "full_fwd": lambda: L.disent_attn_fwd(q, k, v, pk, pq, relidx, mask.view(-1), SCALE, ctx, lse, B, S, Sp, NH, SPAN2, p_drop=0.1,
                                                  seed=3, klen=klen, border=border, lin=128, psave=psave, msave=msave),
            "full_bwd": lambda: disent_attn_bwd(eng, run, sv, dctx, dqkv, dpqk),
            "qrows_fwd": lambda: L.disent_attn_fwd_qrows(qc, pl.rseg, pl.rpos, k, v, pk, pq, relidx, mask.view(-1), klen, SCALE, ctx_c,
                                                         lse_c, B, S, Sp, NH, SPAN2, p_drop=0.1, seed=3),
            "qrows_bwd": lambda: L.disent_attn_bwd_qrows(qc, pl.rseg, pl.rpos, k, v, pk, pq, relidx, mask.view(-1), klen, dO, ctx_c, lse_c,
                                                         SCALE, dQ, dKV[:, :H], dKV[:, H:], dPK, dPQ, 0, SPAN2, ws, B, S, Sp, NH, SPAN2,
                                                         p_drop=0.1, seed=3),
        }
        times = {n: [] for n in legs}
        for it in range(ITERS + 3):  # three warm-up rounds
            for n, fn in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if it >= 3:
                    times[n].append(e0.elapsed_time(e1) * 1e3)
        res = {"B": B, "S": S, "rows": R, "iters": ITERS}
        for n, t in times.items():
            t = sorted(t)
            res[n] = {"median_us": round(t[len(t) // 2], 1), "p10_us": round(t[len(t) // 10], 1), "p90_us": round(t[(len(t) * 9) // 10], 1)}
        out[name] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
