"""What the LoRA tests share: seeded LoRA tensors under the model's parameter names, and the oracle's view of a LoRA model --
its parameters with P[<proj>.weight] = W + s . B @ A (fp32), which oracle._rb then rounds like any other weight."""
import torch

TARGETS = ("query_proj", "key_proj", "value_proj")


def lora_names(n_layers, targets):
    return [f"deberta.encoder.layer.{i}.attention.self.{t}" for i in range(n_layers) for t in TARGETS if t in targets]


def lora_tensors(hidden, n_layers, rank, targets, seed=0, sigma=0.02, zero_B=False):
    """{<proj>.lora_A.weight: [r, H], <proj>.lora_B.weight: [H, r]}: N(0, sigma) entries (B zero on request)"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for nm in lora_names(n_layers, targets):
        out[nm + ".lora_A.weight"] = torch.randn(rank, hidden, generator=g) * sigma
        b = torch.randn(hidden, rank, generator=g) * sigma
        out[nm + ".lora_B.weight"] = torch.zeros_like(b) if zero_B else b
    return out


def merged_params(P, lora, scale, requires_grad=False):
    """(P', leaves): the oracle's parameters with every LoRA'd weight replaced by W + s . B @ A.  requires_grad: the LoRA
    tensors become autograd leaves (detached copies, returned under their names) and P' carries the graph to them."""
    leaves = {n: t.detach().clone().requires_grad_(requires_grad) for n, t in lora.items()}
    Pm = dict(P)
    for n in leaves:
        if n.endswith(".lora_A.weight"):
            mod = n[: -len(".lora_A.weight")]
            Pm[mod + ".weight"] = P[mod + ".weight"] + scale * (leaves[mod + ".lora_B.weight"] @ leaves[n])
    return Pm, leaves
