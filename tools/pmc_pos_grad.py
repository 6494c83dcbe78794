"""The end-of-backward fbl_attn_pos_grad launches alone (25 executions, bench geometry, ragged lengths) for rocprofv3 --pmc."""
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from frozenbilm_amd import lib as L
from frozenbilm_amd.attn_bwd import _delta_ranges

B, S, nh, E = 32, 266, 24, 25
H, Sp, dev = nh * 64, 320, "cuda"
g = torch.Generator().manual_seed(0)
tl = torch.randint(32, 257, (B,), generator=g)
tl[-1] = 256
klen = (tl + 10).to(torch.int32).to(dev)
cfg = types.SimpleNamespace(position_buckets=256, max_rel=512, att_span=256)
dlo, dcnt, dmax = _delta_ranges(S, cfg, torch.device(dev), limit=None)
rcnt = dlo.numel()
x0 = (torch.randn(B, nh, Sp, Sp, generator=g) * 0.1).to(torch.bfloat16).to(dev)
y0 = torch.randn(B * S, 3 * H, generator=g).to(torch.bfloat16).to(dev)
xs = [x0.clone() for _ in range(E)]
ys = [y0.clone() for _ in range(E)]
out = torch.empty(E, nh, rcnt, 64, device=dev)
for it in range(int(sys.argv[1]) if len(sys.argv) > 1 else 3):
    L.attn_pos_grad(0, xs, [y[:, :H] for y in ys], dlo, dcnt, dmax, out, B, S, Sp, nh, rcnt, klen=klen)
    L.attn_pos_grad(1, xs, [y[:, H:2 * H] for y in ys], dlo, dcnt, dmax, out, B, S, Sp, nh, rcnt, klen=klen)
torch.cuda.synchronize()
print("done", float(out.abs().max()))
