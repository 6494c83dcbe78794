"""MI355X-native DebertaV2ForMaskedLM with video prefix + adapters: drop-in for the reference's
model/deberta.py:1289-1501 on the masked-LM path.

Same constructor and ``forward`` signature, same ``state_dict`` key names, same freeze policy
(model/deberta.py:1152-1158, 1334-1339).  Underneath there is no ATen math: ``forward`` runs the explicit HIP pipeline
of ``frozenbilm_amd.engine`` (C-ABI kernels of libfbl.so on the current HIP stream) and, when gradients are enabled,
returns a loss whose ``backward()`` runs the explicit backward pipeline (one autograd node for the whole model).

Host-side layout (288 GB HBM: replicate freely):
  * fp32 masters under the reference parameter names; every TRAINABLE parameter (linear_video, adapters, LayerNorms)
    is a view into ONE flat fp32 buffer, its gradient a view into one flat grad buffer ordered by backward completion
    (head LN, layer 23 ... layer 0, conv LN, encoder LN, embeddings) -> fused clip+Adam and bucketed RCCL all-reduce
    work on contiguous slices.
  * frozen matrices are packed once to bf16 MFMA operands, both W ([out,in], forward) and W^T (dX = dY.W).
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, List, Optional, Tuple

import torch
from torch import nn

from .. import lib as L
from .adapter import Adapter  # noqa: F401  (re-export, mirrors `from model.adapter import Adapter`)
from .config import DebertaV2Config


class MaskedLMOutput(dict):
    """Attribute + item access (`out.loss`, `out["loss"]`), like transformers' MaskedLMOutput (main.py:67).

    When a loss was asked for (``labels`` given) the forward computes only the labelled rows of the prediction head;
    the full ``logits`` tensor is allocated -- and wired into the autograd graph like the reference's -- but its
    contents are produced on first access, by any accessor of this mapping (``out.logits``, ``out["logits"]``,
    ``out[1]``, ``get``, ``values``, ``items``, iteration / ``dict(out)`` / ``**out``).

    ``predictions`` (``out.predictions`` / ``out["predictions"]``): None unless ``model.predict_topk`` > 0, then a
    ``predict.Predictions``; an extension, not part of the ``return_dict=False`` tuple.  Reading it does not fill the logits."""

    _fill = None  # callable that materialises the logits, or None

    def _sync_logits(self):
        fill = self.__dict__.get("_fill")
        if fill is not None:
            self.__dict__["_fill"] = None
            fill()

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e

    def __getitem__(self, k):
        if isinstance(k, int):
            self._sync_logits()
            return [v for v in super().values() if v is not None][k]
        if k == "logits":
            self._sync_logits()
        return super().__getitem__(k)

    def get(self, k, default=None):
        if k == "logits":
            self._sync_logits()
        return super().get(k, default)

    def __iter__(self):  # (also takes dict(out) / {**out} off CPython's fast path, which would bypass __getitem__)
        self._sync_logits()
        return super().__iter__()

    def keys(self):
        self._sync_logits()
        return super().keys()

    def values(self):
        self._sync_logits()
        return super().values()

    def items(self):
        self._sync_logits()
        return super().items()

    def copy(self):
        self._sync_logits()
        return dict(super().items())

    def pop(self, k, *default):
        if k == "logits":
            self._sync_logits()
        return super().pop(k, *default)


class _Node(nn.Module):
    """Bare container used to reproduce the reference's module tree (hence its state_dict key names)."""


def _round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def param_shapes(cfg: DebertaV2Config, features_dim: int, ds_attn: int, ds_ff: int, n_ans: int) -> "OrderedDict[str, tuple]":
    H, I, V = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size
    sh: "OrderedDict[str, tuple]" = OrderedDict()
    e = "deberta.embeddings"
    sh[e + ".word_embeddings.weight"] = (V, H)
    sh[e + ".position_embeddings.weight"] = (cfg.max_position_embeddings, H)
    sh[e + ".LayerNorm.weight"] = (H,)
    sh[e + ".LayerNorm.bias"] = (H,)
    if features_dim:
        sh[e + ".linear_video.weight"] = (H, features_dim)
        sh[e + ".linear_video.bias"] = (H,)
    for i in range(cfg.num_hidden_layers):
        p = f"deberta.encoder.layer.{i}"
        for n in ("query_proj", "key_proj", "value_proj"):
            sh[f"{p}.attention.self.{n}.weight"] = (H, H)
            sh[f"{p}.attention.self.{n}.bias"] = (H,)
        sh[p + ".attention.output.dense.weight"] = (H, H)
        sh[p + ".attention.output.dense.bias"] = (H,)
        sh[p + ".attention.output.LayerNorm.weight"] = (H,)
        sh[p + ".attention.output.LayerNorm.bias"] = (H,)
        if ds_attn:
            A = H // ds_attn
            sh[p + ".attention.output.adapter.down.weight"] = (A, H)
            sh[p + ".attention.output.adapter.down.bias"] = (A,)
            sh[p + ".attention.output.adapter.up.weight"] = (H, A)
            sh[p + ".attention.output.adapter.up.bias"] = (H,)
        sh[p + ".intermediate.dense.weight"] = (I, H)
        sh[p + ".intermediate.dense.bias"] = (I,)
        sh[p + ".output.dense.weight"] = (H, I)
        sh[p + ".output.dense.bias"] = (H,)
        sh[p + ".output.LayerNorm.weight"] = (H,)
        sh[p + ".output.LayerNorm.bias"] = (H,)
        if ds_ff:
            A = H // ds_ff
            sh[p + ".output.adapter.down.weight"] = (A, H)
            sh[p + ".output.adapter.down.bias"] = (A,)
            sh[p + ".output.adapter.up.weight"] = (H, A)
            sh[p + ".output.adapter.up.bias"] = (H,)
    c = "deberta.encoder"
    sh[c + ".rel_embeddings.weight"] = (2 * cfg.att_span, H)
    sh[c + ".LayerNorm.weight"] = (H,)
    sh[c + ".LayerNorm.bias"] = (H,)
    if cfg.conv_kernel_size > 0:
        sh[c + ".conv.conv.weight"] = (H, H, cfg.conv_kernel_size)
        sh[c + ".conv.conv.bias"] = (H,)
        sh[c + ".conv.LayerNorm.weight"] = (H,)
        sh[c + ".conv.LayerNorm.bias"] = (H,)
    h = "lm_predictions.lm_head"
    sh[h + ".bias"] = (V,)
    sh[h + ".dense.weight"] = (H, H)
    sh[h + ".dense.bias"] = (H,)
    sh[h + ".LayerNorm.weight"] = (H,)
    sh[h + ".LayerNorm.bias"] = (H,)
    if n_ans:
        sh["answer_embeddings.weight"] = (n_ans, H)
        sh["answer_bias"] = (n_ans,)
    return sh


LORA_TARGETS = ("query_proj", "key_proj", "value_proj")  # the frozen projections a low-rank update may sit on
LORA_DEFAULT_TARGETS = ("query_proj", "value_proj")
LORA_MAX_RANK = 64  # FBL_LORA_MAX_RANK of include/fbl_lora.h


def check_lora(rank, alpha, targets):
    """(rank, scale s = alpha / rank, targets in the order of LORA_TARGETS) of the constructor arguments, or ValueError"""
    if isinstance(rank, bool) or not isinstance(rank, int) or not 0 <= rank <= LORA_MAX_RANK:
        raise ValueError(f"lora_rank must be an integer in 0..{LORA_MAX_RANK} (got {rank!r})")
    if isinstance(targets, str):
        targets = (targets,)
    targets = tuple(targets)
    unknown = [t for t in targets if t not in LORA_TARGETS]
    if unknown:
        raise ValueError(f"lora_targets must be a subset of {LORA_TARGETS} (got {unknown})")
    if rank > 0 and not targets:
        raise ValueError("lora_rank > 0 needs at least one of lora_targets " + str(LORA_TARGETS))
    if rank == 0:
        return 0, 0.0, ()
    alpha = rank if alpha is None else alpha
    return rank, float(alpha) / rank, tuple(t for t in LORA_TARGETS if t in targets)


def lora_shapes(cfg: DebertaV2Config, rank: int, targets) -> "OrderedDict[str, tuple]":
    """the LoRA parameters: per layer and target, lora_A.weight [r, H] and lora_B.weight [H, r]"""
    sh: "OrderedDict[str, tuple]" = OrderedDict()
    for i in range(cfg.num_hidden_layers if rank else 0):
        for t in targets:
            p = f"deberta.encoder.layer.{i}.attention.self.{t}"
            sh[p + ".lora_A.weight"] = (rank, cfg.hidden_size)
            sh[p + ".lora_B.weight"] = (cfg.hidden_size, rank)
    return sh


PROMPT_MAX = 128  # FBL_PROMPT_MAX of include/fbl_prompt.h
PROMPT_NAME = "deberta.embeddings.prompt_embeddings.weight"


def check_n_prompt(n_prompt) -> int:
    """the number of soft-prompt slots of the constructor argument, or ValueError"""
    if isinstance(n_prompt, bool) or not isinstance(n_prompt, int) or not 0 <= n_prompt <= PROMPT_MAX:
        raise ValueError(f"n_prompt must be an integer in 0..{PROMPT_MAX} (got {n_prompt!r})")
    return n_prompt


def layer_prompt_name(i: int) -> str:
    """deep prompt tuning: the prompt rows that encoder layer i >= 1 reads in the prompt slots of its input"""
    return f"deberta.encoder.layer.{i}.prompt.weight"


def check_prompt_depth(prompt_depth, n_prompt: int, n_layers: int) -> int:
    """the number of stages with prompt rows of their own (the embeddings, then layers 1 .. depth-1), or ValueError"""
    if isinstance(prompt_depth, bool) or not isinstance(prompt_depth, int) or not 1 <= prompt_depth <= n_layers:
        raise ValueError(f"prompt_depth must be an integer in 1..num_hidden_layers={n_layers} (got {prompt_depth!r})")
    if prompt_depth > 1 and not n_prompt:
        raise ValueError(f"prompt_depth={prompt_depth} needs prompt slots: n_prompt > 0")
    return prompt_depth


def flat_order(cfg: DebertaV2Config, names: List[str]) -> List[str]:
    """Trainable names in backward-completion order (bucket order of the gradient all-reduce)."""
    def take(prefix):
        return [n for n in names if n.startswith(prefix)]

    out: List[str] = []
    out += take("lm_predictions.")
    for i in reversed(range(cfg.num_hidden_layers)):
        if i == 0:
            out += take("deberta.encoder.conv.")
        out += take(f"deberta.encoder.layer.{i}.")
    out += take("deberta.encoder.LayerNorm.")
    out += take("deberta.embeddings.")
    rest = [n for n in names if n not in set(out)]
    return out + rest


class DebertaV2ForMaskedLM(nn.Module):
    def __init__(
        self,
        config,
        max_feats=10,
        features_dim=768,
        freeze_lm=True,
        freeze_mlm=True,
        ds_factor_attn=8,
        ds_factor_ff=8,
        ft_ln=True,
        dropout=0.1,
        n_ans=0,
        freeze_last=True,
        lora_rank=0,
        lora_alpha=None,
        lora_targets=LORA_DEFAULT_TARGETS,
        n_prompt=0,
        prompt_depth=1,
    ):
        super().__init__()
        # prompt tuning (an extension): n_prompt trainable embedding rows between the video slots and the text of every sample
        # (engine.Engine._forward assembles them with fbl_embed_assemble); 0 is the reference's sequence
        self.n_prompt = check_n_prompt(n_prompt)
        # LoRA on the frozen Q/K/V projections (an extension): W' = W + (alpha / rank) . B . A is the module's weight wherever
        # it is used; merged into the packed bf16 operands once per step (engine.Engine._compose_lora), no dropout
        self.lora_rank, self.lora_scale, self.lora_targets = check_lora(lora_rank, lora_alpha, lora_targets)
        self.config = DebertaV2Config.from_any(config)
        self.config.validate_supported()
        cfg = self.config
        # deep prompt tuning (an extension): layers 1 .. prompt_depth-1 read rows of their own in the prompt slots of their input
        # (engine.Engine._prompt_overwrite); 1 is the shallow prompt, whose rows enter at the embeddings only
        self.prompt_depth = check_prompt_depth(prompt_depth, self.n_prompt, cfg.num_hidden_layers)
        for ds in (ds_factor_attn, ds_factor_ff):
            if ds:
                assert not cfg.hidden_size % ds  # model/adapter.py:10
        self.max_feats = max_feats
        self.features_dim = features_dim
        self.ds_factor_attn = ds_factor_attn
        self.ds_factor_ff = ds_factor_ff
        self.adapter_dropout = float(dropout) if dropout else 0.0
        self.n_ans = n_ans
        self.freeze_lm, self.freeze_mlm, self.ft_ln, self.freeze_last = freeze_lm, freeze_mlm, ft_ln, freeze_last
        if not (freeze_lm and freeze_mlm):
            raise NotImplementedError(
                "the MI355X path implements FrozenBiLM's frozen-LM regime (freeze_lm=freeze_mlm=True): "
                "only linear_video, adapters and LayerNorms receive gradients")
        if n_ans and not freeze_last:
            raise NotImplementedError("--ft_last (trainable answer-embedding module) is not implemented: the answer "
                                      "head is used frozen, the reference's default (args.py:358-363)")

        shapes = param_shapes(cfg, features_dim, ds_factor_attn, ds_factor_ff, n_ans)
        g = torch.Generator().manual_seed(0)
        for name, shape in shapes.items():
            if "LayerNorm" in name:
                t = torch.ones(shape) if name.endswith("weight") else torch.zeros(shape)
            elif name.endswith(".bias") or name == "answer_bias":
                t = torch.zeros(shape)  # model/deberta.py:1085-1086
            else:
                t = torch.randn(shape, generator=g) * cfg.initializer_range  # :1084,1088
            if name.endswith("word_embeddings.weight"):
                t[cfg.pad_token_id].zero_()  # :1089-1090
            self._register(name, nn.Parameter(t, requires_grad=self._trainable(name)))
        # the LoRA parameters come from a generator of their own: every other parameter keeps its initial bits whatever the rank
        g2 = torch.Generator().manual_seed(1)
        for name, shape in lora_shapes(cfg, self.lora_rank, self.lora_targets).items():
            if ".lora_A." in name:  # nn.Linear's reset_parameters: kaiming_uniform_(a=sqrt(5)) = U(-1/sqrt(fan_in), 1/sqrt(fan_in))
                bound = 1.0 / shape[1] ** 0.5
                t = (torch.rand(shape, generator=g2) * 2 - 1) * bound
            else:
                t = torch.zeros(shape)
            self._register(name, nn.Parameter(t, requires_grad=True))
        if self.n_prompt:  # a generator of its own again: N(0, initializer_range), like the word embeddings it stands beside
            g3 = torch.Generator().manual_seed(2)
            t = torch.randn((self.n_prompt, cfg.hidden_size), generator=g3) * cfg.initializer_range
            self._register(PROMPT_NAME, nn.Parameter(t, requires_grad=True))
        if self.prompt_depth > 1:  # the layers' prompts, layer 1 first, from one more generator: prompt_depth = 1 draws nothing
            g4 = torch.Generator().manual_seed(3)
            for i in range(1, self.prompt_depth):
                t = torch.randn((self.n_prompt, cfg.hidden_size), generator=g4) * cfg.initializer_range
                self._register(layer_prompt_name(i), nn.Parameter(t, requires_grad=True))
        emb = self._module("deberta.embeddings")
        emb.register_buffer("position_ids", torch.arange(cfg.max_position_embeddings).expand((1, -1)))
        self._engine = None
        self.engine_options = {}  # read once when the engine is built (engine.Engine.__init__ lists the keys; defaults = shipped)
        # the launch graphs (train_graph.py), each opt-in: the `logit_rows` inference forward replayed as one hipGraph, the MLM
        # training step as two, the fine-tuning step (`logit_rows` under autograd, no labels) as two; `_graph_routes` is what
        # the routes remember besides their caches (train_graph.stats)
        self.inference_graphs = self.training_graphs = self.finetune_graphs = False
        from ..train_graph import new_states

        self._graph_routes = new_states()
        # opt-in: ragged batches run without the padding rows behind each sample's last used position (engine.Packing) whenever
        # the call's outputs live on selected rows (labels / logit_rows given).  Rows that exist get the same values as on the
        # padded grid; `logits` / `hidden_states` read as zero at the dropped positions (the reference computes values there
        # that nothing on this path reads), training-mode dropout draws a different -- equally distributed -- mask stream, and
        # the launch graphs (shape-static) are not used while it is on.
        self.packed_rows = False
        # opt-in: the two enhanced-mask-decoder passes, the head and their backward on the selected rows only (engine.py)
        self.decoder_rows = False
        # the compact backward (Engine._backward_rows): the padded step's backward on the rows that exist, same gradient bits.
        # None: the engine's rule decides per batch; False: always the padded backward (A/B runs); True: the rule without its
        # share threshold (tests)
        self.compact_backward = None
        # opt-in, read per call: an int k in 1..16 makes every call return `predictions` (predict.Predictions) -- top-k ids and
        # log-probabilities of the rows the call forms logits for anyway (the labelled rows, the `logit_rows`, else every row),
        # with the label's rank and the row's NLL on a labelled call.  One extra pass over those [R, V] logits; never fills the
        # full [B*S, V] logits.  Loss, logits and gradients are those of the same call with 0 (off); such a call runs eagerly.
        self.predict_topk = 0
        self._weights_frozen = 0  # nesting depth of weights_frozen(): inference forwards may reuse the packed operands
        self._reducer = None  # parallel.GradReducer attached to this model (survives engine rebuilds)
        self.step_seed = 0  # advanced every training forward; keys the counter-based dropout
        self._seed_salt = None  # torch seed (args.seed + rank in the reference's main()) and rank, fixed at first use

    # ---------------------------------------------------------------- module tree helpers
    def _module(self, dotted: str) -> nn.Module:
        m: nn.Module = self
        for part in dotted.split("."):
            if part not in m._modules:
                m.add_module(part, _Node())
            m = m._modules[part]
        return m

    def _register(self, name: str, p: nn.Parameter):
        if "." in name:
            mod, leaf = name.rsplit(".", 1)
            self._module(mod).register_parameter(leaf, p)
        else:
            self.register_parameter(name, p)

    def _trainable(self, name: str) -> bool:
        if name.startswith("answer_"):
            return not self.freeze_last
        if "linear_video" in name or "adapter" in name or ".lora_" in name or name == PROMPT_NAME:
            return True
        if name.startswith("deberta.encoder.layer.") and name.endswith(".prompt.weight"):
            return True
        return bool(self.ft_ln and "LayerNorm" in name)

    def trainable_names(self) -> List[str]:
        """The trainable-BY-CONSTRUCTION set, in `named_parameters()` order: what the constructor flags make trainable, whatever
        `requires_grad` says right now.  The engine lays its flat buffer out by it and the optimizer numbers its states by it,
        so neither moves when the caller freezes or unfreezes a parameter during a run; which of these train in a step is the
        live set (frozenbilm_amd/live_set.py).  A parameter outside this set that asks for a gradient is refused by the next
        grad-mode forward (live_set.unsupported_leaf_message)."""
        return [n for n, _ in self.named_parameters() if self._trainable(n)]

    # ---------------------------------------------------------------- reference API
    @property
    def device(self):
        return next(self.parameters()).device

    def get_param(self, name: str) -> torch.Tensor:
        m: nn.Module = self
        parts = name.split(".")
        for part in parts[:-1]:
            m = m._modules[part]
        return m._parameters[parts[-1]]

    def set_answer_embeddings(self, a2tok, freeze_last=True):
        """model/deberta.py:1358-1380: answer table = masked mean of the word embeddings of each answer's tokens.
        (The reference assigns ``answer_bias.weight``, an attribute, so the effective bias keeps its value.)"""
        if not freeze_last:
            raise NotImplementedError("--ft_last (trainable answer-embedding module) is not implemented")
        E = self.get_param("deberta.embeddings.word_embeddings.weight")
        pad = self.config.pad_token_id
        a2tok = a2tok.to(E.device)
        keep = (a2tok != pad)
        table = (E.data[a2tok] * keep.float()[:, :, None]).sum(1) / keep.sum(1, keepdim=True).clamp(min=1)
        if len(table) != self.n_ans or "answer_embeddings" not in self._modules:
            assert not self.training
            self.n_ans = len(table)
            self._register("answer_embeddings.weight", nn.Parameter(table.clone(), requires_grad=False))
            old = self._parameters.get("answer_bias")
            self.register_parameter("answer_bias", nn.Parameter(torch.zeros(self.n_ans, device=E.device), requires_grad=False))
            del old
        else:
            self.get_param("answer_embeddings.weight").data = table
        self.freeze_last = freeze_last
        self.get_param("answer_embeddings.weight").requires_grad_(False)
        self.get_param("answer_bias").requires_grad_(False)
        self.invalidate()

    def weights_frozen(self):
        """Context manager: inside it the caller promises not to modify the trainable parameters behind the engine's back
        (through `.data`, `vector_to_parameters`, raw writes into `engine().flat`), so inference forwards skip the rebuild
        of the bf16 operands / composed adapter rows unless FusedAdam.step or an in-place update through a parameter object
        happened in between.  Outside it every forward rebuilds them.  The evaluate loops run inside it."""
        import contextlib

        @contextlib.contextmanager
        def scope():
            self._weights_frozen += 1
            try:
                yield self
            finally:
                self._weights_frozen -= 1
                if self._weights_frozen == 0 and self._engine is not None:
                    self._engine._ops_version = None

        return scope()

    def ema_weights(self):
        """Context manager: inside it the trainable parameters are the moving average kept by the attached
        `FusedAdam(..., ema_decay=)` (frozenbilm_amd/ema.py; optim.FusedAdam.ema_weights) -- evaluate, export or save the
        averaged model there; leaving restores every bit.  RuntimeError when no optimizer with an average is attached.  While it
        is open `merge_lora()` and `load_state_dict()` are refused: what they write could not be swapped back."""
        from ..ema import weights

        return weights(self)

    def lora_names(self) -> List[str]:
        """the module names that carry a LoRA pair (`<name>.lora_A.weight`, `<name>.lora_B.weight`), layer by layer"""
        return [f"deberta.encoder.layer.{i}.attention.self.{t}" for i in range(self.config.num_hidden_layers if self.lora_rank else 0)
                for t in self.lora_targets]

    @torch.no_grad()
    def merge_lora(self):
        """W <- W + s.B.A in the fp32 masters of every LoRA'd projection -- the compose kernel's own fp32 result, so the bf16
        operands (hence the eval logits) keep their bits -- then B <- 0 and the engine is rebuilt on next use.  The state_dict
        without its `lora_*` keys is then a plain reference checkpoint."""
        from ..ema import refuse_if_open

        refuse_if_open(self, "merge_lora()")
        if not self.lora_rank:
            return self
        self.engine().merge_lora()
        self.invalidate()
        return self

    @torch.no_grad()
    def init_prompt_from_ids(self, ids):
        """Text initialisation of prompt tuning: prompt row p <- the word embedding of token ids[p] (LongTensor [n_prompt])."""
        if not self.n_prompt:
            raise RuntimeError("init_prompt_from_ids needs a model built with n_prompt > 0")
        E = self.get_param("deberta.embeddings.word_embeddings.weight")
        ids = torch.as_tensor(ids)
        if ids.dtype != torch.long or tuple(ids.shape) != (self.n_prompt,):
            raise ValueError(f"ids must be a LongTensor of shape [{self.n_prompt}] (got {ids.dtype} {tuple(ids.shape)})")
        if int(ids.min()) < 0 or int(ids.max()) >= E.shape[0]:
            raise ValueError(f"ids outside the vocabulary 0..{E.shape[0] - 1}")
        self.get_param(PROMPT_NAME).data.copy_(E.data[ids.to(E.device)])
        self.invalidate()
        return self

    def layer_prompt_names(self) -> List[str]:
        """the parameters of deep prompt tuning, layer 1 first (empty for prompt_depth = 1)"""
        return [layer_prompt_name(i) for i in range(1, self.prompt_depth)]

    @torch.no_grad()
    def init_prompt_layers_from_hidden(self, hidden_states, T):
        """Start deep prompt tuning near the shallow model: layer i's prompt rows <- the batch mean of
        hidden_states[i][:, T:T+n_prompt] for i = 1 .. prompt_depth-1.  hidden_states: the tuple of an
        output_hidden_states=True call ([B, S, H] each, S = T + n_prompt + text); T: its number of video slots."""
        if self.prompt_depth < 2:
            raise RuntimeError("init_prompt_layers_from_hidden needs a model built with prompt_depth > 1")
        P, H = self.n_prompt, self.config.hidden_size
        if isinstance(T, bool) or not isinstance(T, int) or T < 0:
            raise ValueError(f"T must be a non-negative integer (got {T!r})")
        if len(hidden_states) < self.prompt_depth:
            raise ValueError(f"hidden_states holds {len(hidden_states)} tensors, prompt_depth={self.prompt_depth} needs the first "
                             f"{self.prompt_depth}")
        for i in range(1, self.prompt_depth):
            h = hidden_states[i]
            if h.dim() != 3 or h.shape[0] < 1 or h.shape[1] < T + P or h.shape[2] != H:
                raise ValueError(f"hidden_states[{i}] must be [batch, at least T + n_prompt = {T + P}, {H}] (got {tuple(h.shape)})")
            w = self.get_param(layer_prompt_name(i))
            w.data.copy_(h[:, T:T + P].detach().to(torch.float32).mean(0))
        self.invalidate()
        return self

    def invalidate(self):
        """Drop the packed bf16 operands / flat buffers (after load_state_dict, .to(), set_answer_embeddings)."""
        self._engine = None
        from ..train_graph import ROUTES

        for route in ROUTES:  # captured graphs hold the old engine's buffers
            self.__dict__.pop(route.cache, None)

    def _load_from_state_dict(self, *a, **k):
        self.invalidate()
        return super()._load_from_state_dict(*a, **k)

    def load_state_dict(self, state_dict, strict=True, **kw):
        from ..ema import refuse_if_open

        refuse_if_open(self, "load_state_dict()")
        self.invalidate()
        # tolerate the reference-only keys (untied decoder copy, buffers)
        sd = {k: v for k, v in state_dict.items() if "lm_head.decoder" not in k}
        return super().load_state_dict(sd, strict=strict, **kw)

    def _apply(self, fn, *a, **k):
        self.invalidate()
        return super()._apply(fn, *a, **k)

    def engine(self):
        if self._engine is None:
            from ..engine import Engine

            self._engine = Engine(self)
            if self._reducer is not None:
                self._reducer.rebind(self._engine)
        return self._engine

    def dropout_seed_base(self) -> int:
        """Seed of this training step's dropout sites.  The reference draws its masks from the per-process torch RNG,
        seeded with args.seed + rank (main.py:161-165): mixing torch.initial_seed() and the rank gives every data-parallel
        rank and every differently seeded run its own mask stream; ``step_seed`` (saved in checkpoints) advances it."""
        if self._seed_salt is None:
            rank = 0
            try:
                import torch.distributed as dist

                if dist.is_available() and dist.is_initialized():
                    rank = dist.get_rank()
            except Exception:
                rank = 0
            self._seed_salt = ((torch.initial_seed() & 0xFFFFFFFF) * 2654435761 + rank * 40503 + 12345) & 0xFFFFFFFFFFFF
        return (self.step_seed * 1000003 + self._seed_salt) & 0xFFFFFFFFFFFF

    GRAPH_L_BUCKET = 32  # the launch graphs pad text lengths up to a multiple of this (train_graph.build_feed)

    def forward(
        self,
        input_ids=None,
        attention_mask=None,
        token_type_ids=None,
        position_ids=None,
        inputs_embeds=None,
        labels=None,
        output_attentions=None,
        return_dict=None,
        video=None,
        video_mask=None,
        mlm=False,
        output_hidden_states=False,
        logit_rows=None,
    ):
        """Reference signature (model/deberta.py:1414-1427) plus two keyword extensions: ``output_hidden_states`` and
        ``logit_rows`` -- int tensor of flat row indices b*S + s into the [B, S] token grid (S = video slots + prompt slots +
        text; ``n_prompt`` trainable rows sit between the video and the text, with mask 1 and no label): the
        prediction head then runs on those rows only and ``logits`` is [len(logit_rows), V] (the downstream loops read one
        [MASK] row per sample: videoqa.py:66-69,164-168, mc.py:166-170).  Under autograd these logits are differentiable and
        the head's backward runs on the same rows; the indices must then be distinct and inside the grid (ValueError), and
        ``labels`` cannot be given next to them.  ``inputs_embeds`` (float [B, L, hidden_size]) stands in for ``E[input_ids]``
        (:1204-1225).  In grad mode a ``video`` or ``inputs_embeds`` that requires grad receives its gradient, and the
        ``hidden_states`` of an ``output_hidden_states=True`` call are differentiable outputs."""
        if input_ids is not None and inputs_embeds is not None:
            raise ValueError("You cannot specify both input_ids and inputs_embeds at the same time")
        if input_ids is None and inputs_embeds is None:
            raise ValueError("You have to specify either input_ids or inputs_embeds")
        if inputs_embeds is not None:  # (checked on the host, before the engine is touched)
            if not torch.is_tensor(inputs_embeds) or inputs_embeds.dim() != 3 or inputs_embeds.shape[-1] != self.config.hidden_size:
                raise ValueError(f"inputs_embeds must be [batch, text length, hidden_size={self.config.hidden_size}] "
                                 f"(got {tuple(getattr(inputs_embeds, 'shape', ()))})")
            if not inputs_embeds.is_floating_point():
                raise ValueError(f"inputs_embeds must have a floating dtype (got {inputs_embeds.dtype})")
        from ..predict import check_topk

        check_topk(self.predict_topk)  # (ValueError at the call, whichever route would serve it)
        eng = self.engine()
        from .. import train_graph as TG  # (the launch graphs, opt-in: which calls they serve is TG.route_for's to say)

        TG.restore_reducer_overlap_if_routes_off(self, eng)
        route = TG.route_for(self, TG.Call(
            ids=input_ids is not None, embeds=inputs_embeds is not None, labels=labels is not None,
            rows=None if logit_rows is None else logit_rows.numel(), video_grad=video is not None and video.requires_grad,
            mlm=bool(mlm), hidden_states=bool(output_hidden_states), attentions=bool(output_attentions),
            grad=torch.is_grad_enabled()))
        res = route and TG.serve(self, eng, route, input_ids, attention_mask, video, video_mask, labels, mlm, logit_rows)
        # output_attentions=True (model/deberta.py:1414-1427, :544-560): the fused attention kernel never materialises its
        # probabilities; on request a plain kernel rebuilds them per encoder layer from the stored log-sum-exp (eval mode)
        if res is None:
            res = eng.run(input_ids, attention_mask, video, video_mask, labels, mlm, output_hidden_states,
                          logit_rows=logit_rows, want_attn=bool(output_attentions), inputs_embeds=inputs_embeds)
        out = MaskedLMOutput(loss=res["loss"], logits=res["logits"], hidden_states=res.get("hidden_states"),
                             attentions=res.get("attentions"), predictions=res.get("predictions"))
        run = res.get("run")
        out.__dict__["_run"] = run  # (tests read the saved bottleneck activations through this)
        if run is not None and run.logits_pending:
            out.__dict__["_fill"] = lambda: eng.fill_logits(run)
        if return_dict is False:
            return tuple(v for v in (out["loss"], out["logits"], out["hidden_states"], out["attentions"]) if v is not None)
        return out
