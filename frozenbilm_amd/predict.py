"""What the model predicts on the rows a call already has logits for (opt-in ``model.predict_topk``): top-k ids and
log-probabilities, and on a labelled call the label's rank and the row's NLL -- one pass of fbl_row_predict
(include/fbl_predict.h) over the [R, ldv] fp32 logits the route formed anyway.  Never the full [B*S, V] logits.

Host logic only at import: the kernel is reached through ``lib.row_predict`` when a call asks for predictions.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

MAX_TOPK = 16  # FBL_PREDICT_MAX_K


def check_topk(value) -> int:
    """``model.predict_topk`` as read at a call: an int in 0..16 (0 = off).  A bool is refused -- ``True`` would silently mean
    "top 1" -- and so is anything that is not an int."""
    if isinstance(value, bool) or not isinstance(value, int):
        raise ValueError(f"predict_topk must be an int in 0..{MAX_TOPK} (0 = off), got {value!r}")
    if not 0 <= value <= MAX_TOPK:
        raise ValueError(f"predict_topk must be in 0..{MAX_TOPK} (0 = off), got {value}")
    return value


@dataclass
class Predictions:
    """Predictions of R rows.  ``rows``: int64 [R], indices b*S + s into the flat [B*S] token grid, in the order the route
    holds them -- ascending grid index on a labelled call, the caller's order on a ``logit_rows`` call, 0 .. B*S-1 otherwise.
    ``topk_ids`` int64 [R, k] and ``topk_logprobs`` fp32 [R, k]: descending by logit, equal logits ascending by id; slots
    beyond the head's width hold id -1 and -inf.  ``label_rank`` int64 [R] (0 = the label is the top prediction) and
    ``row_nll`` fp32 [R] on a labelled call, else None.  All detached."""
    rows: torch.Tensor
    topk_ids: torch.Tensor
    topk_logprobs: torch.Tensor
    label_rank: Optional[torch.Tensor] = None
    row_nll: Optional[torch.Tensor] = None

    def _ranked(self) -> torch.Tensor:
        if self.label_rank is None:
            raise ValueError("label_rank is only known on a labelled call")
        return self.label_rank

    def correct(self, n: int = 1) -> torch.Tensor:
        """bool [R]: the label is among the row's first n predictions"""
        return self._ranked() < n

    def count(self) -> torch.Tensor:
        """number of rows, a scalar on the predictions' device (no host read)"""
        return torch.full((), float(self.rows.numel()), dtype=torch.float32, device=self.rows.device)

    def accuracy(self, n: int = 1) -> torch.Tensor:
        """fraction of rows whose label is among the first n predictions, a device scalar; 0 (never NaN) for no rows"""
        hit = self.correct(n).sum().to(torch.float32)
        return hit / max(self.rows.numel(), 1)


def empty(k: int, device, labelled: bool) -> Predictions:
    z = lambda dt, *s: torch.empty(*s, dtype=dt, device=device)  # noqa: E731
    return Predictions(rows=z(torch.int64, 0), topk_ids=z(torch.int64, 0, k), topk_logprobs=z(torch.float32, 0, k),
                       label_rank=z(torch.int64, 0) if labelled else None, row_nll=z(torch.float32, 0) if labelled else None)


def of_call(run, logits, k: int, rows_labelled, logit_rows) -> Predictions:
    """Predictions of the call behind `run` (Engine.run / BertEngine.run, after the forward) from what it already holds:
    a labelled call: `run.logits_c` [R, ldv] with the `run.row_lse` / `run.labels_c` of its cross entropy, one row per labelled
      grid row `rows_labelled` (ascending; padded grid, packed rows and decoder rows keep that order);
    a logit_rows call: `logits` [R, ldv], one row per requested grid row, in the caller's order;
    neither: `logits` [B*S, ldv], every grid row.
    Reads the filled columns only; never triggers fill_logits."""
    from . import lib as L

    V = run.Vout
    with torch.no_grad():
        if run.labels is not None:
            if run.logits_c is None:
                return empty(k, rows_labelled.device, True)
            ids, lp, rank, nll = L.row_predict(run.logits_c, V, k, labels=run.labels_c, row_lse=run.row_lse)
            return Predictions(rows=rows_labelled, topk_ids=ids.long(), topk_logprobs=lp, label_rank=rank.long(), row_nll=nll)
        src = logits.detach()
        if logit_rows is not None:
            rows = logit_rows.to(src.device).long().reshape(-1)
        else:
            rows = torch.arange(src.shape[0], device=src.device)
        if rows.numel() == 0:
            return empty(k, src.device, False)
        ids, lp, _, _ = L.row_predict(src, V, k)
        return Predictions(rows=rows, topk_ids=ids.long(), topk_logprobs=lp)
