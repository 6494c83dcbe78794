"""Case table and exact reference of fbl_row_predict (include/fbl_predict.h); importable without a GPU.

The reference works on float64 copies of the same fp32 values: the columns of a row are sorted by the rule of the header
(descending by value, equal values ascending by column, -inf an ordinary smallest value, NaN below -inf), the rank is
counted by its definition, lse and NLL are float64.
"""
from collections import namedtuple

import torch

MAX_K = 16
CHUNK = 8192  # FBL_PREDICT_CHUNK: columns per workgroup of the first launch

# Where the kernel's ownership of a column changes (predict.hip): column c of a chunk belongs to 16-byte load j = c / 1024 of
# thread (c / 4) % 256; threads 0..63 are wave 0.  A duplicated maximum straddles each of these:
BOUNDARIES = {
    "element inside a lane's 16 bytes": (1, 2),
    "lane": (3, 4),
    "wave": (255, 256),
    "per-thread load": (1023, 1024),
    "workgroup (chunk)": (CHUNK - 1, CHUNK),
    "second chunk": (2 * CHUNK - 1, 2 * CHUNK),
}

Case = namedtuple("Case", "name R V k")


def sweep_cases():
    """V x R x k; the vocabulary width with R = 3 only"""
    out = []
    for V in (1, 2, 5, 63, 64, 65, 257, 1000):
        for R in (0, 1, 3, 67):
            for k in (1, 5, 16):
                out.append(Case(f"V{V}-R{R}-k{k}", R, V, k))
    for k in (1, 5, 16):
        out.append(Case(f"V128100-R3-k{k}", 3, 128100, k))
    return out


def ids(cases):
    return [c.name for c in cases]


def ru(x, m):
    return (x + m - 1) // m * m


# ------------------------------------------------------------------------------------------------ reference
def ref_order(x64):
    """int64 [R, V]: the columns of every row in the total order"""
    nan = torch.isnan(x64)
    vals = torch.where(nan, torch.full_like(x64, -float("inf")), x64)
    first = torch.argsort(vals, dim=1, descending=True, stable=True)       # ties keep ascending columns
    nan_sorted = torch.gather(nan, 1, first).to(torch.int8)
    second = torch.argsort(nan_sorted, dim=1, stable=True)                 # NaNs behind every number, order kept
    return torch.gather(first, 1, second)


def ref_predict(x, V, k, labels=None, lse=None):
    """x: fp32 [R, >= V] (any device).  Returns a dict: ids int64 [R, k] (-1 beyond V), logprob float64 [R, k] (-inf beyond V),
    lse float64 [R], and with labels rank int64 [R], nll float64 [R].  lse: use these values (float64 of the fp32 the kernel is
    given) instead of the float64 log-sum-exp."""
    x64 = x[:, :V].double()
    R = x64.shape[0]
    order = ref_order(x64)
    kk = min(k, V)
    ids_ = torch.full((R, k), -1, dtype=torch.int64, device=x.device)
    lp = torch.full((R, k), -float("inf"), dtype=torch.float64, device=x.device)
    lse64 = torch.logsumexp(x64, 1) if lse is None else lse.double()
    ids_[:, :kk] = order[:, :kk]
    lp[:, :kk] = torch.gather(x64, 1, order[:, :kk]) - lse64[:, None]
    out = {"ids": ids_, "logprob": lp, "lse": lse64}
    if labels is not None:
        xl = torch.gather(x64, 1, labels[:, None])
        col = torch.arange(V, device=x.device)[None, :]
        out["rank"] = ((x64 > xl).sum(1) + ((x64 == xl) & (col < labels[:, None])).sum(1)).to(torch.int64)
        out["nll"] = lse64 - xl[:, 0]
    return out


# ------------------------------------------------------------------------------------------------ inputs
def random_rows(R, V, seed, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(R, V, generator=g) * 3.0).to(device)
    labels = torch.randint(0, V, (R,), generator=g).to(device)
    return x, labels


def adversarial_rows(V, k, device="cpu"):
    """(names, x fp32 [n, V], labels int64 [n]): the rows the header's order and the kernel's boundaries can get wrong"""
    g = torch.Generator().manual_seed(1234 + V)
    names, rows, labels = [], [], []

    def add(name, row, label):
        names.append(name); rows.append(row.float()); labels.append(int(label))

    base = lambda: torch.randn(V, generator=g) * 3.0  # noqa: E731
    add("all equal", torch.full((V,), 2.5), V // 2)
    for what, (a, b) in BOUNDARIES.items():
        if b < V:
            r = base(); r[a] = r[b] = 40.0
            add(f"maximum duplicated across the {what} boundary, label on the later one", r, b)
            r = base(); r[a] = r[b] = 40.0
            add(f"maximum duplicated across the {what} boundary, label on the earlier one", r, a)
    r = base()
    dup = sorted({c for ab in BOUNDARIES.values() for c in ab if c < V})
    r[dup] = 41.0
    add("maximum duplicated on every boundary column", r, dup[-1])
    own = [(j * 256 + 5) * 4 + e for j in range(8) for e in range(4)]   # the 32 columns of thread 5 of chunk 0
    own = [c for c in own if c < V]
    r = base()
    r[own] = 50.0 + torch.arange(len(own), dtype=torch.float32) * 0.25
    add("the top values all inside one thread's columns", r, own[0])
    add("strictly ascending", torch.arange(V, dtype=torch.float32) * 1e-3, V - 1)
    add("strictly descending", -torch.arange(V, dtype=torch.float32) * 1e-3, 0)
    r = torch.full((V,), -float("inf"))
    keep = sorted({0, V // 3, V - 1})[: max(1, min(3, k - 1))]
    r[keep] = torch.tensor([1.0, -2.0, 0.5])[: len(keep)]
    add("-inf in more than V - k columns, label on a -inf", r, min(V - 1, 1))
    add("-inf everywhere", torch.full((V,), -float("inf")), V - 1)
    r = base(); r[min(7, V - 1)] = float("nan"); r[V - 1] = float("nan")
    add("NaN columns", r, V // 2 if V > 2 else 0)
    if V >= 8:
        lab = V // 2
        r = base(); r[lab - 3: lab + 1] = 39.0
        add("label tied with three lower-numbered columns", r, lab)
        r = base(); r[lab: lab + 4] = 39.0
        add("label tied with three higher-numbered columns", r, lab)
    add("label in column 0", base(), 0)
    add("label in column V-1", base(), V - 1)
    r = base(); r[0] = 0.0; r[V - 1] = -0.0; r[1:V - 1] = -torch.rand(V - 2, generator=g) - 0.5
    add("+0 and -0 tie", r, V - 1)
    return names, torch.stack(rows).to(device), torch.tensor(labels, dtype=torch.int64, device=device)


def padded(x, ld, fill):
    """fp32 [R, ld] whose columns V.. hold `fill`"""
    R, V = x.shape
    out = torch.full((R, ld), fill, dtype=torch.float32, device=x.device)
    out[:, :V] = x
    return out


# ------------------------------------------------------------------------------------------------ bounds
U = 2.0 ** -24


def value_bound(c_lse, lse64, value64):
    """|got - ref| allowed for a value = logit - lse (or lse - logit) the kernel forms from an fp32 lse: the bound of the lse --
    c_lse * U * max(|lse|, 1), the form and constant tests/test_gpu_rowops.py applies to fbl_ce_fwd's row_lse -- plus the one
    rounding of the subtraction, U * |value|"""
    return c_lse * U * lse64.abs().clamp(min=1.0) + U * value64.abs()
