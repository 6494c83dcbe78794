"""Partial fine-tuning, host side: which stages of the backward a step runs and which ranges of the flat buffer train.

Two sets of parameters (DESIGN.md "Partial fine-tuning"):

* trainable by construction -- what the constructor flags make trainable (`model.trainable_names()`).  The flat layout, its
  offsets, the data-parallel buckets and the optimizer-state schema follow this set and never move during a run.
* live -- the members of that set whose `requires_grad` is true right now, read at the start of every grad-mode forward.

Everything here is a pure function of names and numbers (no tensor, no GPU): tests/test_live_set_host.py.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

REL_LN = "deberta.encoder.LayerNorm."


def stage_names(n_layers: int, conv: bool) -> List[str]:
    """The backward stages of the DeBERTa engine, bottom first: the embedding stage, layer 0, the conv stage, layers
    1 .. nL-2, the decoder passes (both enhanced-mask-decoder executions of the last layer, and its own third execution when
    hidden_states[nL] carries a gradient), the head."""
    s = ["emb"]
    for i in range(n_layers - 1):
        s.append(f"layer{i}")
        if i == 0 and conv:
            s.append("conv")
    if n_layers == 1 and conv:
        s.append("conv")
    return s + ["decoder", "head"]


def stage_of(name: str, n_layers: int) -> str:
    """the LOWEST stage whose backward forms the gradient of parameter `name`"""
    if name.startswith("lm_predictions."):
        return "head"
    if name.startswith("deberta.encoder.layer."):
        i = int(name.split(".")[3])
        return "decoder" if i == n_layers - 1 else f"layer{i}"
    if name.startswith("deberta.encoder.conv."):
        return "conv"
    if name.startswith(REL_LN):
        # the LayerNorm over the relative-position table collects from every attention execution: it lies in every encoder
        # layer and every decoder pass (not in the embedding stage)
        return "layer0" if n_layers > 1 else "decoder"
    return "emb"  # deberta.embeddings.*: linear_video, the embedding LayerNorm


@dataclass(frozen=True)
class StagePlan:
    """Stages whose backward runs in a step: those at or above the lowest one that holds a live leaf or an input that takes a
    gradient.  `lowest` is None when nothing does (the call then keeps no gradient bookkeeping at all)."""
    stages: Tuple[str, ...]          # all stages, bottom first
    lowest: Optional[int]            # index into `stages`

    def runs(self, stage: str) -> bool:
        return self.lowest is not None and stage in self.stages and self.stages.index(stage) >= self.lowest

    @property
    def running(self) -> Tuple[str, ...]:
        return () if self.lowest is None else self.stages[self.lowest:]


def stage_plan(n_layers: int, conv: bool, live_names: Iterable[str], grad_inputs: Sequence[str] = ()) -> StagePlan:
    """grad_inputs: the inputs that take a gradient of their own ("video", "embeds"); they enter at the embedding stage.  (A
    gradient arriving on a hidden_states[i] is a source, not a leaf: it flows down only as far as something below asks.)"""
    stages = tuple(stage_names(n_layers, conv))
    idx = [stages.index(stage_of(n, n_layers)) for n in live_names]
    if grad_inputs:
        idx.append(0)
    return StagePlan(stages, min(idx) if idx else None)


def flat_layout(order: Sequence[str], numel: Dict[str, int]) -> Tuple[Dict[str, int], int]:
    """offsets of the parameters `order` in the flat buffer (every one padded to 8 floats) and its size"""
    offs, total = {}, 0
    for n in order:
        offs[n] = total
        total += (numel[n] + 7) // 8 * 8
    return offs, total


def live_ranges(order: Sequence[str], offsets: Dict[str, int], numel: Dict[str, int], live: Iterable[str]) -> List[Tuple[int, int]]:
    """The live set as sorted, disjoint, 8-aligned [begin, end) ranges of the flat buffer; neighbours are merged (a parameter's
    range takes its padding along: the padding of a live parameter holds zeros, p = g = m = v = 0 stays 0 under Adam)."""
    live = set(live)
    out: List[Tuple[int, int]] = []
    for n in sorted((n for n in order if n in live), key=lambda n: offsets[n]):
        b, e = offsets[n], offsets[n] + (numel[n] + 7) // 8 * 8
        if out and out[-1][1] == b:
            out[-1] = (out[-1][0], e)
        else:
            out.append((b, e))
    return out


def unsupported_leaf_message(name: str) -> str:
    return (f"parameter '{name}' has requires_grad=True, but it is not trainable by construction: the MI355X path trains "
            "linear_video, the adapters and (ft_ln) the LayerNorms only -- frozen LM weights, the prediction head and the answer "
            "module stay frozen (freeze_lm / freeze_mlm / freeze_last); set requires_grad_(False) on it")


def refuse_unsupported_leaves(named, trainable_by_construction) -> None:
    """`requires_grad_(True)` on a frozen LM weight, a prediction-head weight or the answer module stays unsupported: the
    next grad-mode forward raises and names the parameter"""
    for n, p in named.items():
        if p.requires_grad and n not in trainable_by_construction:
            raise NotImplementedError(unsupported_leaf_message(n))


class LiveSetMixin:
    """What both engines keep of the live set.  The engine provides `named`, `order` (the trainable-by-construction set in flat
    order), `offsets`, `G` (the views of the flat gradient buffer) and `flat_grad`; this adds
        live_order    the live names, in flat order             Gl         their gradient views (what a backward may write)
        live_any / all_live                                     live_version   a number per DISTINCT set seen on this engine
        live_ranges() / live_table()                            the ranges of the flat buffer fbl_*_live walk
    """

    def _init_live(self):
        self._cons = set(self.order)
        self._numel = {n: self.named[n].numel() for n in self.order}
        self._live_flags = None
        self._live_versions: Dict[tuple, int] = {}
        self._live_tables: Dict[int, object] = {}
        self._live_ranges: Dict[int, list] = {}
        self._set_live(tuple(bool(self.named[n].requires_grad) for n in self.order))

    def update_live(self) -> bool:
        """Read `requires_grad` of every parameter (start of a grad-mode forward).  A parameter outside the
        trainable-by-construction set that asks for a gradient is refused by name.  Returns whether anything is live."""
        refuse_unsupported_leaves(self.named, self._cons)
        flags = tuple(bool(self.named[n].requires_grad) for n in self.order)
        if flags != self._live_flags:
            self._set_live(flags)
        return self.live_any

    def _set_live(self, flags: tuple):
        first = self._live_flags is None
        self._live_flags = flags
        self.live_order = [n for n, f in zip(self.order, flags) if f]
        self.Gl = {n: self.G[n] for n in self.live_order}
        self.live_any, self.all_live = any(flags), all(flags)
        self.live_version = self._live_versions.setdefault(flags, len(self._live_versions))
        # a parameter that left the live set keeps no gradient: its slice of the flat buffer reads exactly zero from now on
        # (nothing writes it while it is dead), and travels as zeros through a data-parallel exchange
        if not (first and self.all_live):
            for n, f in zip(self.order, flags):
                if not f:
                    self.G[n].zero_()

    def live_ranges(self) -> List[Tuple[int, int]]:
        r = self._live_ranges.get(self.live_version)
        if r is None:
            r = self._live_ranges[self.live_version] = live_ranges(self.order, self.offsets, self._numel, self.live_order)
        return r

    def live_table(self):
        """the device table of include/fbl_live.h for the current live set (built once per distinct set)"""
        from . import lib as L

        t = self._live_tables.get(self.live_version)
        if t is None:
            t = self._live_tables[self.live_version] = L.live_table(self.live_ranges(), self.flat.numel(), self.flat.device)
        return t
