"""Parameter groups of FusedAdam, host side: which group every trainable parameter belongs to, which segments of the flat
buffer a step walks, what learning rate a group has, and the groups that layer-wise rate decay needs.

A group is what torch calls one: a dict with `params` and hyper-parameters (`lr`, `betas`, `eps`, `weight_decay`,
`decoupled_weight_decay`).  `params` may hold parameter names, `fnmatch` patterns over the names, or the parameter tensors
themselves.  Every member of the trainable-by-construction set (`model.trainable_names()`, live_set.py) lands in exactly one
group; what no group names joins group 0.  One more key, `lr_scale`: the group's rate is `param_groups[0]["lr"] * lr_scale`, read
at every step, so a schedule that writes group 0 alone (the reference's util/misc.py adjust_learning_rate) moves every group.

Everything here is a pure function of names and numbers (no tensor, no GPU): tests/test_param_groups_host.py.
"""
from __future__ import annotations

import fnmatch
import re
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

from .live_set import REL_LN, stage_of

MAX_GROUPS = 64     # include/fbl_groups.h FBL_ADAM_MAX_GROUPS
_WILD = re.compile(r"[*?\[]")
_BERT_LAYER = "bert.encoder.layer."


def resolve(groups: Sequence[dict], trainable: Sequence[str], name_of_id: Optional[Dict[int, str]] = None) -> List[List[str]]:
    """The names of every group's members, each list in the order of `trainable`.  An entry of `params` is a name, an fnmatch
    pattern, or any other object -- a parameter tensor -- that `name_of_id` maps from its id() to its name.  ValueError: a
    parameter named twice (by two entries of any groups), a name, pattern or tensor that meets nothing in `trainable`.
    What nothing names joins group 0 (which exists even when `groups` is empty)."""
    order = {n: i for i, n in enumerate(trainable)}
    if len(order) != len(trainable):
        raise ValueError("the trainable set names a parameter twice")
    owner: Dict[str, int] = {}
    out: List[List[str]] = [[] for _ in range(max(len(groups), 1))]

    def take(name: str, k: int, what: str):
        if name in owner:
            raise ValueError(f"parameter '{name}' is named twice: in group {owner[name]} and, by {what}, in group {k}")
        owner[name] = k
        out[k].append(name)

    for k, grp in enumerate(groups):
        params = grp["params"]
        if isinstance(params, str) or not isinstance(params, (list, tuple)):
            params = [params]
        for e in params:
            if isinstance(e, str):
                if e in order:
                    take(e, k, f"'{e}'")
                elif _WILD.search(e):
                    hits = [n for n in trainable if fnmatch.fnmatchcase(n, e)]
                    if not hits:
                        raise ValueError(f"group {k}: pattern '{e}' meets no trainable parameter")
                    for n in hits:
                        take(n, k, f"pattern '{e}'")
                else:
                    raise ValueError(f"group {k}: '{e}' is not trainable by construction (model.trainable_names())")
            else:
                name = (name_of_id or {}).get(id(e))
                if name is None or name not in order:
                    raise ValueError(f"group {k}: a tensor that is no trainable-by-construction parameter of the model"
                                     + (f" ('{name}')" if name else ""))
                take(name, k, "its tensor")
    for n in trainable:
        if n not in owner:
            owner[n] = 0
            out[0].append(n)
    return [sorted(g, key=order.__getitem__) for g in out]


def group_of(group_names: Sequence[Sequence[str]]) -> Dict[str, int]:
    return {n: k for k, names in enumerate(group_names) for n in names}


def index_lists(group_names: Sequence[Sequence[str]]) -> List[List[int]]:
    """`param_groups[k]["params"]` of torch's state-dict schema: the parameter indices run through the groups in order"""
    out, i = [], 0
    for names in group_names:
        out.append(list(range(i, i + len(names))))
        i += len(names)
    return out


def segments(order: Sequence[str], offsets: Dict[str, int], numel: Dict[str, int], live: Iterable[str],
             group_of: Dict[str, int]) -> List[Tuple[int, int, int]]:
    """The live set cut by groups: sorted, disjoint, 8-aligned (begin, end, group) runs of the flat buffer, each a maximal run
    that is live and belongs to one group (a parameter's run takes its padding along, as live_set.live_ranges)."""
    live = set(live)
    out: List[Tuple[int, int, int]] = []
    for n in sorted((n for n in order if n in live), key=lambda n: offsets[n]):
        b, e, k = offsets[n], offsets[n] + (numel[n] + 7) // 8 * 8, group_of[n]
        if out and out[-1][1] == b and out[-1][2] == k:
            out[-1] = (out[-1][0], e, k)
        else:
            out.append((b, e, k))
    return out


def check_groups(groups: Sequence[dict]) -> None:
    """the rules of `lr_scale` and the group limit, on the dicts as the user wrote them"""
    if len(groups) > MAX_GROUPS:
        raise ValueError(f"{len(groups)} parameter groups: the fused update takes {MAX_GROUPS}")
    for k, g in enumerate(groups):
        if "lr_scale" in g:
            if k == 0:
                raise ValueError("group 0 cannot carry lr_scale: it is the rate the others are relative to")
            if "lr" in g:
                raise ValueError(f"group {k} has both lr and lr_scale")


def learning_rates(groups: Sequence[dict]) -> List[float]:
    """every group's rate right now: its own `lr`, or `groups[0]["lr"] * lr_scale`"""
    base = groups[0]["lr"]
    return [base * g["lr_scale"] if "lr_scale" in g else g["lr"] for g in groups]


def depth_below_top(name: str, n_layers: int) -> int:
    """How many stages below the top a parameter sits.  0: the head, the decoder passes (the last layer), and the LayerNorm over
    the relative-position table, which collects from every layer; layer i: n_layers - 1 - i; the convolution counts with layer
    0; the embedding stage sits one below layer 0.  The BERT model: the same rule on its own layer names."""
    if name.startswith(_BERT_LAYER):
        return n_layers - 1 - int(name.split(".")[3])
    if name.startswith("bert.embeddings."):
        return n_layers
    if name.startswith("bert.") or name.startswith("cls."):
        return 0
    if name.startswith(REL_LN):
        return 0
    st = stage_of(name, n_layers)
    if st in ("head", "decoder"):
        return 0
    if st == "conv":
        return n_layers - 1
    if st == "emb":
        return n_layers
    return n_layers - 1 - int(st[len("layer"):])


def layerwise_groups(names: Sequence[str], n_layers: int, decay: float, no_decay: Sequence[str] = ("LayerNorm", "bias")) -> List[dict]:
    """Groups for layer-wise learning-rate decay: a stage i steps below the top trains at `decay**i` of group 0's rate, and
    each depth splits into a decayed group and an undecayed one (`weight_decay = 0`) holding the names that contain one of
    the `no_decay` substrings.  Group 0 is the decayed group of the top (it carries no lr_scale and may be empty); the other
    groups follow top-down, decayed before undecayed, empty ones left out."""
    if not 0.0 < decay <= 1.0:
        raise ValueError(f"decay {decay} outside (0, 1]")
    by: Dict[Tuple[int, bool], List[str]] = {}
    for n in names:
        by.setdefault((depth_below_top(n, n_layers), any(s in n for s in no_decay)), []).append(n)
    out = [dict(params=by.pop((0, False), []))]
    for d, nd in sorted(by):
        g = dict(params=by[(d, nd)], lr_scale=float(decay) ** d)
        if nd:
            g["weight_decay"] = 0.0
        out.append(g)
    check_groups(out)
    return out
