"""MI355X-native BertForMaskedLM with the video prefix: drop-in for the reference's model/bert.py:705-872 (BERT-Base /
BERT-Large as the language model of every task, ``--model_name=bert-*``).

Same constructor and ``forward`` keywords, same ``state_dict`` key names, same freeze rule (model/bert.py:547-553, :748-750):
with ``freeze_lm`` the trainable tensors are ``linear_video`` and -- with ``ft_ln`` -- the LayerNorms under ``bert.``; with
``freeze_mlm`` the whole ``cls`` head is frozen, its LayerNorm included (unlike the DeBERTa head).  ``forward`` runs the
explicit HIP pipeline of ``frozenbilm_amd.bert_engine``; no adapters exist on this model (model/__init__.py:49-51).
"""
from __future__ import annotations

import dataclasses
from typing import Optional

import torch
from torch import nn

from .deberta import DebertaV2ForMaskedLM, MaskedLMOutput


@dataclasses.dataclass
class BertConfig:
    """``transformers.BertConfig`` fields this path reads; the defaults are bert-base-uncased's."""
    vocab_size: int = 30522
    hidden_size: int = 768
    num_hidden_layers: int = 12
    num_attention_heads: int = 12
    intermediate_size: int = 3072
    hidden_act: str = "gelu"
    hidden_dropout_prob: float = 0.1
    attention_probs_dropout_prob: float = 0.1
    max_position_embeddings: int = 512
    type_vocab_size: int = 2
    initializer_range: float = 0.02
    layer_norm_eps: float = 1e-12
    pad_token_id: int = 0
    use_return_dict: bool = True

    @classmethod
    def from_any(cls, cfg) -> "BertConfig":
        if isinstance(cfg, cls):
            return dataclasses.replace(cfg)
        src = cfg if isinstance(cfg, dict) else vars(cfg) if not hasattr(cfg, "to_dict") else cfg.to_dict()
        names = {f.name for f in dataclasses.fields(cls)}
        return cls(**{k: v for k, v in src.items() if k in names})

    @classmethod
    def base(cls) -> "BertConfig":
        return cls()

    @classmethod
    def large(cls) -> "BertConfig":
        return cls(hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096)


def param_shapes(cfg: BertConfig, features_dim: int, n_ans: int):
    H, I, V = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size
    s = {}
    e = "bert.embeddings."
    s[e + "word_embeddings.weight"] = (V, H)
    s[e + "position_embeddings.weight"] = (cfg.max_position_embeddings, H)
    s[e + "token_type_embeddings.weight"] = (cfg.type_vocab_size, H)
    s[e + "LayerNorm.weight"] = (H,)
    s[e + "LayerNorm.bias"] = (H,)
    if features_dim:
        s[e + "linear_video.weight"] = (H, features_dim)
        s[e + "linear_video.bias"] = (H,)
    for i in range(cfg.num_hidden_layers):
        p = f"bert.encoder.layer.{i}."
        for n in ("query", "key", "value"):
            s[p + f"attention.self.{n}.weight"] = (H, H)
            s[p + f"attention.self.{n}.bias"] = (H,)
        s[p + "attention.output.dense.weight"] = (H, H)
        s[p + "attention.output.dense.bias"] = (H,)
        s[p + "attention.output.LayerNorm.weight"] = (H,)
        s[p + "attention.output.LayerNorm.bias"] = (H,)
        s[p + "intermediate.dense.weight"] = (I, H)
        s[p + "intermediate.dense.bias"] = (I,)
        s[p + "output.dense.weight"] = (H, I)
        s[p + "output.dense.bias"] = (H,)
        s[p + "output.LayerNorm.weight"] = (H,)
        s[p + "output.LayerNorm.bias"] = (H,)
    c = "cls.predictions."
    s[c + "bias"] = (V,)
    s[c + "transform.dense.weight"] = (H, H)
    s[c + "transform.dense.bias"] = (H,)
    s[c + "transform.LayerNorm.weight"] = (H,)
    s[c + "transform.LayerNorm.bias"] = (H,)
    if n_ans:
        s["answer_embeddings.weight"] = (n_ans, H)
        s["answer_bias"] = (n_ans,)
    return s


class BertForMaskedLM(nn.Module):
    def __init__(self, config, features_dim=768, max_feats=10, freeze_lm=True, ft_ln=True, freeze_mlm=True, n_ans=0,
                 freeze_last=True, lora_rank=0, lora_alpha=None, lora_targets=("query_proj", "value_proj"), n_prompt=0,
                 prompt_depth=1):
        super().__init__()
        if prompt_depth != 1:
            raise NotImplementedError("deep prompt tuning (prompt_depth > 1) is implemented for the DeBERTa model only")
        if n_prompt:
            raise NotImplementedError("prompt tuning (n_prompt > 0) is implemented for the DeBERTa model only: the prompt slots "
                                      "would shift the absolute position rows of the text")
        if lora_rank:
            raise NotImplementedError("LoRA on the frozen attention projections (lora_rank > 0) is implemented for the DeBERTa "
                                      "model only")
        self.config = BertConfig.from_any(config)
        cfg = self.config
        self.features_dim, self.max_feats = features_dim, max_feats
        self.freeze_lm, self.ft_ln, self.freeze_mlm, self.freeze_last = freeze_lm, ft_ln, freeze_mlm, freeze_last
        self.n_ans = n_ans
        if not freeze_lm:
            raise NotImplementedError("the MI355X BERT path implements the frozen-LM regime (freeze_lm=True): only "
                                      "linear_video and the LayerNorms receive gradients")
        if not freeze_mlm:
            raise NotImplementedError("the MI355X BERT path keeps the MLM head frozen (freeze_mlm=True)")
        if n_ans and not freeze_last:
            raise NotImplementedError("--ft_last (trainable answer-embedding module) is not implemented for BERT")
        g = torch.Generator().manual_seed(0)
        for name, shape in param_shapes(cfg, features_dim, n_ans).items():
            if "LayerNorm" in name:
                t = torch.ones(shape) if name.endswith("weight") else torch.zeros(shape)
            elif name.endswith("bias"):
                t = torch.zeros(shape)
            else:
                t = torch.randn(shape, generator=g) * cfg.initializer_range
            if name.endswith("word_embeddings.weight"):
                t[cfg.pad_token_id].zero_()
            self._register(name, nn.Parameter(t, requires_grad=self._trainable(name)))
        self._module("bert.embeddings").register_buffer("position_ids",
                                                        torch.arange(cfg.max_position_embeddings).expand((1, -1)))
        self._engine = None
        # opt-in attributes the loops set on the DeBERTa model: the launch graphs are accepted and this path runs eagerly;
        # packed_rows is honoured (bert_engine.bert_packing)
        self.inference_graphs = False
        self.training_graphs = False
        self.finetune_graphs = False
        self.packed_rows = False
        self.decoder_rows = False  # accepted, does nothing: this model has no enhanced mask decoder
        self.predict_topk = 0  # opt-in, as on the DeBERTa model: k in 1..16 makes every call return `predictions`
        self._weights_frozen = 0
        self._reducer = None
        self.step_seed = 0
        self._seed_salt = None

    def _trainable(self, name: str) -> bool:
        if name.startswith("answer_"):
            return not self.freeze_last
        if "linear_video" in name:
            return True
        return bool(self.ft_ln and name.startswith("bert.") and "LayerNorm" in name)

    # module tree, engine life cycle and dropout seeds work as on the DeBERTa model
    trainable_names = DebertaV2ForMaskedLM.trainable_names
    _module = DebertaV2ForMaskedLM._module
    _register = DebertaV2ForMaskedLM._register
    get_param = DebertaV2ForMaskedLM.get_param
    device = DebertaV2ForMaskedLM.device
    weights_frozen = DebertaV2ForMaskedLM.weights_frozen
    ema_weights = DebertaV2ForMaskedLM.ema_weights
    invalidate = DebertaV2ForMaskedLM.invalidate
    dropout_seed_base = DebertaV2ForMaskedLM.dropout_seed_base

    def _load_from_state_dict(self, *a, **k):
        self.invalidate()
        return super()._load_from_state_dict(*a, **k)

    def _apply(self, fn, *a, **k):
        self.invalidate()
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, state_dict, strict=True, **kw):
        from ..ema import refuse_if_open

        refuse_if_open(self, "load_state_dict()")
        self.invalidate()
        # the reference's state dict also holds the tied decoder (cls.predictions.decoder.{weight,bias})
        sd = {k: v for k, v in state_dict.items() if not k.startswith("cls.predictions.decoder.")}
        return super().load_state_dict(sd, strict=strict, **kw)

    def engine(self):
        if self._engine is None:
            from ..bert_engine import BertEngine

            self._engine = BertEngine(self)
            if self._reducer is not None:
                self._reducer.rebind(self._engine)
        return self._engine

    def set_answer_embeddings(self, a2tok, freeze_last=True):
        """model/bert.py:761-788: answer table = masked mean of the word embeddings of each answer's tokens.  (The reference
        assigns ``answer_bias.weight``, an attribute, so the effective bias keeps its value.)"""
        if not freeze_last:
            raise NotImplementedError("--ft_last (trainable answer-embedding module) is not implemented for BERT")
        E = self.get_param("bert.embeddings.word_embeddings.weight")
        a2tok = a2tok.to(E.device)
        keep = a2tok != self.config.pad_token_id
        table = (E.data[a2tok] * keep.float()[:, :, None]).sum(1) / keep.sum(1, keepdim=True).clamp(min=1)
        if len(table) != self.n_ans or "answer_embeddings" not in self._modules:
            assert not self.training
            self.n_ans = len(table)
            self._register("answer_embeddings.weight", nn.Parameter(table.clone(), requires_grad=False))
            self.register_parameter("answer_bias", nn.Parameter(torch.zeros(self.n_ans, device=E.device), requires_grad=False))
        else:
            self.get_param("answer_embeddings.weight").data = table
        self.freeze_last = freeze_last
        self.invalidate()

    def forward(self, video=None, video_mask=None, input_ids=None, attention_mask=None, token_type_ids=None,
                position_ids=None, head_mask=None, inputs_embeds=None, encoder_hidden_states=None, encoder_attention_mask=None,
                labels=None, output_attentions=None, output_hidden_states=None, return_dict=None, mlm=False, logit_rows=None):
        """Reference keywords (model/bert.py:790-810) plus ``logit_rows`` -- flat row indices b*S + s of the [B, S] token grid
        (S = video slots + text): the head then runs on those rows only and ``logits`` is [len(logit_rows), V]; under autograd
        they are differentiable (distinct rows inside the grid, no ``labels`` next to them)."""
        if input_ids is not None and inputs_embeds is not None:
            raise ValueError("You cannot specify both input_ids and inputs_embeds at the same time")
        if inputs_embeds is not None:
            raise NotImplementedError("inputs_embeds is not on the FrozenBiLM hot path")
        if input_ids is None:
            raise ValueError("You have to specify either input_ids or inputs_embeds")
        if output_attentions:
            raise NotImplementedError("output_attentions is not served by the BERT path (the fused attention never "
                                      "materialises its probabilities)")
        if head_mask is not None or encoder_hidden_states is not None or encoder_attention_mask is not None:
            raise NotImplementedError("head_mask / cross-attention inputs are not on the FrozenBiLM hot path")
        if token_type_ids is not None and bool((token_type_ids != 0).any()):
            raise NotImplementedError("only token type 0 is on the FrozenBiLM hot path")
        if position_ids is not None:
            S = input_ids.shape[1] + (video.shape[1] if (video is not None and self.features_dim) else 0)
            default = torch.arange(S, device=position_ids.device).expand_as(position_ids)
            if position_ids.shape[-1] != S or bool((position_ids != default).any()):
                raise NotImplementedError("only the default positions 0..S-1 are on the FrozenBiLM hot path")
        eng = self.engine()
        res = eng.run(input_ids, attention_mask, video, video_mask, labels, mlm, bool(output_hidden_states), logit_rows=logit_rows)
        out = MaskedLMOutput(loss=res["loss"], logits=res["logits"], hidden_states=res.get("hidden_states"), attentions=None,
                             predictions=res.get("predictions"))
        run = res["run"]
        out.__dict__["_run"] = run
        if run.logits_pending:
            out.__dict__["_fill"] = lambda: eng.fill_logits(run)
        if return_dict is False:
            return tuple(v for v in (out["loss"], out["logits"], out["hidden_states"]) if v is not None)
        return out
