"""Host plan of the selected query rows of fbl_disent_attn_fwd_qrows / _bwd_qrows (include/fbl_qrows.h).

Pure torch, importable without a GPU; on a device tensor it makes no host synchronisation (no nonzero, no bincount, no
.item()): the number of rows is the length of the input.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch


@dataclass
class QueryRowPlan:
    """rows[order] is the COMPACT order: grouped by sample, the caller's order kept inside a sample (stable)."""
    order: torch.Tensor   # int64 [R]: caller index of each compact row
    back: torch.Tensor    # int64 [R]: compact index of each caller row (compact[back] is in the caller's order)
    rseg: torch.Tensor    # int32 [B+1]: sample b owns the compact rows [rseg[b], rseg[b+1])
    rpos: torch.Tensor    # int32 [R]: position of each compact row inside its sample
    grid: torch.Tensor    # int64 [R]: padded-grid row b*S + s of each compact row
    krows: torch.Tensor   # int64 [R]: the same row in the key layout (the grid, or packed rows through `inv`)
    R: int


def plan_query_rows(rows: torch.Tensor, B: int, S: int, inv: Optional[torch.Tensor] = None) -> QueryRowPlan:
    """rows: integer tensor [R] of padded-grid rows b*S + s in the caller's order (unsorted, duplicates allowed, may be empty);
    inv: int64 [B*S] packed row of each grid row (engine.Packing.inv) when keys and values live on packed rows."""
    rows = rows.reshape(-1).long()
    R = rows.numel()
    dev = rows.device
    b = torch.div(rows, S, rounding_mode="floor")
    order = torch.argsort(b, stable=True)
    back = torch.empty_like(order)
    back[order] = torch.arange(R, device=dev)
    grid = rows[order]
    counts = torch.zeros(B, dtype=torch.int64, device=dev).index_add_(0, b, torch.ones_like(b))
    rseg = torch.zeros(B + 1, dtype=torch.int32, device=dev)
    rseg[1:] = torch.cumsum(counts, 0).to(torch.int32)
    rpos = (grid - torch.div(grid, S, rounding_mode="floor") * S).to(torch.int32)
    krows = grid if inv is None else inv[grid]
    return QueryRowPlan(order=order, back=back, rseg=rseg, rpos=rpos, grid=grid, krows=krows, R=R)
