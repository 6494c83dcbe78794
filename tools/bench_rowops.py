"""HIP-event timings of the LayerNorm kernels at the bench shape (N = 8512, H = 1536, dropout 0.1), and of clip norm + Adam over the
flat trainable buffer with their live-set twins."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from frozenbilm_amd import lib as L
L.load()
dev = "cuda"
N, H = 8512, 1536
print("# " + (os.environ.get("FBL_LIB") or "libfbl.so"), flush=True)
y, r = torch.randn(N, H, device=dev), torch.randn(N, H, device=dev)
g, b = torch.ones(H, device=dev), torch.zeros(H, device=dev)
t = torch.empty(N, H, device=dev); st = torch.empty(N, 2, device=dev); ob = torch.empty(N, H, dtype=torch.bfloat16, device=dev)
dout = torch.randn(N, H, device=dev); dt = torch.empty(N, H, device=dev); dyb = torch.empty(N, H, dtype=torch.bfloat16, device=dev)
dg, db, dys = torch.zeros(H, device=dev), torch.zeros(H, device=dev), torch.zeros(H, device=dev)
ws = L.ln_bwd_ws(H, dev)
def timeit(fn, n=40):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n): fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / n
L.ln_fwd(y=y, p_drop=0.1, seed=5, r_plain=r, gamma=g, beta=b, eps=1e-7, out_t=t, out_stats=st, out_bf16=ob, N=N, H=H)
for rep in range(2):
    print(f"ln_fwd full   {timeit(lambda: L.ln_fwd(y=y, p_drop=0.1, seed=5, r_plain=r, gamma=g, beta=b, eps=1e-7, out_t=t, out_stats=st, out_bf16=ob, N=N, H=H)):7.1f} us")
    print(f"ln_fwd stats  {timeit(lambda: L.ln_fwd(y=t, gamma=g, beta=b, eps=1e-7, out_stats=st, out_bf16=ob, N=N, H=H)):7.1f} us")
    print(f"ln_bwd (+fold){timeit(lambda: L.ln_bwd(dout, t, st, g, p_drop=0.1, seed=5, out_dt=dt, out_dy_bf16=dyb, dgamma=dg, dbeta=db, dysum=dys, ws=ws)):7.1f} us")
    print(f"ln_bwd p=0    {timeit(lambda: L.ln_bwd(dout, t, st, g, p_drop=0.0, seed=0, out_dt=dt, out_dy_bf16=dyb, dgamma=dg, dbeta=db, dysum=dys, ws=ws)):7.1f} us   (no mask regeneration: what the hash costs)")

# ---- clip norm + Adam over the flat trainable buffer (30.1 M floats at the xlarge model) and their live-set twins
# (include/fbl_live.h) with one range over the whole buffer and with 150 alternating ranges.  Adam streams 7 words per live
# element (p, g, m, v read; p, m, v written), the norm one; the share of the 8 TB/s HBM roof is printed beside the time.
n = 30_100_000 // 8 * 8
p, gr, m, v = (torch.randn(n, device=dev) * 0.01 for _ in range(4))
v.abs_()
ss, wss = torch.zeros(1, device=dev), torch.empty(L.load().fbl_sumsq_ws_floats(), device=dev)
seg = n // 300 // 8 * 8
tables = {"1 range": [(0, n)], "150 ranges": [(2 * i * seg, (2 * i + 1) * seg) for i in range(150)]}
ROOF = 8.0e12
def line(name, us, words):
    print(f"{name:34s}{us:8.1f} us   {words * 4 / (us * 1e-6) / ROOF:5.2f} of the HBM roof")
for rep in range(2):
    line("fbl_sumsq", timeit(lambda: L.sumsq(gr, ss, ws=wss)), n)
    line("fbl_adam_flat", timeit(lambda: L.adam_flat(p, gr, m, v, 1e-5, 0.9, 0.95, 1e-8, 0.0, 3, sumsq_t=ss, max_norm=1.0)), 7 * n)
    for name, rg in tables.items():
        tab = L.live_table(rg, n, dev)
        live = sum(e - b for b, e in rg)
        line(f"fbl_sumsq_live, {name}", timeit(lambda: L.sumsq_live(gr, tab, ss, wss)), live)
        line(f"fbl_adam_flat_live, {name}", timeit(lambda: L.adam_flat_live(p, gr, m, v, tab, 1e-5, 0.9, 0.95, 1e-8, 0.0, 3, sumsq_t=ss,
                                                                           max_norm=1.0)), 7 * live)
