"""Explicit forward / backward pipelines of the FrozenBiLM masked-LM hot path on MI355X.

No tracing compiler and no ATen math: the step is a fixed sequence of C-ABI kernel launches (lib.py -> libfbl.so)
on the current HIP stream; torch only owns HBM allocations.  Semantics follow SURVEY.md App. C / the reference lines
quoted per stage.  Precision: bf16 MFMA operands, fp32 accumulation, fp32 residual stream / LayerNorm statistics /
softmax / logits / gradients of the trainable parameters.

Residual stream representation: a LayerNorm output is kept as (t, stats, gamma, beta[, rowmask]) -- the pre-norm
fp32 tensor plus per-row (mean, rstd) -- together with its bf16 copy (the next GEMM operand).  Consumers re-normalise
on the fly, so the fp32 normalised tensor is never written to HBM, and ``t`` doubles as the tensor saved for backward.
"""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np
import torch

from . import lib as L
from .predict import check_topk, of_call as predictions_of_call
from .live_set import REL_LN, LiveSetMixin, flat_layout, stage_plan
from .attn_bwd import ATTN_SCALE, _relidx_range, disent_attn_bwd, pos_chain_buffers, pos_table_grads_batched
from .model.deberta import PROMPT_NAME, layer_prompt_name
from .model.relpos import rel_index_vector

BF16, F32 = torch.bfloat16, torch.float32


def _ru(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def check_logit_rows(logit_rows: torch.Tensor, n_grid: int) -> None:
    """`logit_rows` of a call that keeps gradient bookkeeping: the backward adds the head's input gradient into the rows with
    a plain += (fbl_scatter_rows_f32), so an index given twice would race and one outside the [B, S] grid would write out
    of bounds.  Both are refused here, on the host, before anything is queued (one read of an input, like the label count)."""
    r = logit_rows.reshape(-1)
    if r.numel() == 0:
        return
    s = torch.sort(r.long()).values
    dup = (s[1:] == s[:-1]).any() if s.numel() > 1 else torch.zeros((), dtype=torch.bool, device=s.device)
    lo, hi, dup = torch.stack([s[0], s[-1], dup.long()]).tolist()
    if lo < 0 or hi >= n_grid:
        raise ValueError(f"logit_rows must index the [B, S] token grid: 0 <= row < {n_grid} (got {lo} .. {hi})")
    if dup:
        raise ValueError("logit_rows holds an index more than once: with gradients every requested row must be distinct")


@dataclass
class NormRef:
    """A tensor given in LayerNorm-normalised form (see module docstring)."""
    t: torch.Tensor
    stats: torch.Tensor
    gamma: torch.Tensor
    beta: torch.Tensor
    rowmask: Optional[torch.Tensor] = None

    def as_args(self):
        return (self.t, self.stats, self.gamma, self.beta, self.rowmask)


@dataclass
class Stream:
    """One activation stream: bf16 GEMM operand + its fp32 value as NormRef or plain tensor."""
    bf16: torch.Tensor
    norm: Optional[NormRef] = None
    plain: Optional[torch.Tensor] = None
    full: Optional[torch.Tensor] = None  # [N + 2*span, H] buffer whose first N rows are `bf16`: the tail receives the
    #                                      relative-position table R so that one GEMM yields Q|K|V and PQ|PK


@dataclass
class Packing:
    """Row layout of a ragged batch without its trailing padding (opt-in `model.packed_rows`): sample b owns the activation
    rows [row0[b], row0[b+1]) = its positions 0 .. plen[b]-1, where plen[b] - 1 is the last position that anything reads
    (valid token, label, requested logit row; at least the video slots).  Every kernel between the embedding and the
    head is row-wise except the attention kernels (which take row0, include/fbl.h) and three once-per-step stages that
    go through the padded grid (embedding gather, the k=3 convolution's im2col, the position embeddings of the decoder)."""
    row0: torch.Tensor   # int32 [B+1]
    sel: torch.Tensor    # int64 [Np]: padded row b*S+s of each packed row
    inv: torch.Tensor    # int64 [B*S]: packed row of each padded row, -1 where it has none
    pos: torch.Tensor    # int64 [Np]: position s of each packed row
    n: int               # Np
    sel32: Optional[torch.Tensor] = None  # sel / inv as int32, as the row kernels of include/fbl_rows.h take them (the
    inv32: Optional[torch.Tensor] = None  # backward's own layout only: Engine._backward_rows)


@dataclass
class MergedPack:
    """What the merged adapters of one site type (attention output / FFN output) share over the layers, all in reverse layer
    order (j = nL-1-layer): a dense layer followed by an adapter runs as ONE GEMM against [W ; Wd.W]
    (fbl_dense_adapter_down_fwd); the composed rows Wd.W change with every optimizer step (_compose_adapter_down)."""
    A: int
    WT: torch.Tensor                # bf16 [nL, K, H]: W^T of the frozen dense layer
    WM: torch.Tensor                # bf16 [nL, H + A, K]: [W ; Wd.W]
    bM: torch.Tensor                # fp32 [nL, H + A]: [b ; Wd.b + bd]
    b16: torch.Tensor               # bf16 [nL, 1, H]: b as a GEMM operand
    WF: Optional[torch.Tensor]      # bf16 [nL, H, Kf]: [W^T | (Wd.W)^T | 0] of the folded backward (attention output only)
    groups: list                    # (j0, layers, offset of down.weight, of down.bias, stride) per strided batch, layer 0 first


@dataclass
class AdapterSite:
    """One adapter of one layer.  Built once: every tensor is a view of the flat parameter buffers or of a pack that never
    moves (captured graphs keep reading them); only upT / downT are per step.  The routes follow from the shapes:
      merged   dense + down-projection as one GEMM, fused tail, and (attention output) dx folded into the dense dX GEMM: needs
               the bottleneck unpadded, A % 64 == 0, and the segment boundary H on a wave's column range, H % 64 == 0
               (include/fbl.h); otherwise neither the composed weights nor their per-step rebuild exist
      grouped  weight-gradient products parked for a grouped launch (fbl_adapter_bwd_dw takes Ap <= 256 and H % 8 == 0);
               otherwise launched per adapter on the side stream (_adapter_bwd)"""
    name: str
    A: int
    Ap: int                                   # A rounded up to 64
    down: torch.Tensor                        # bf16 [A, H]
    up: torch.Tensor                          # bf16 [H, Ap]: the parameter's bf16 copy, or a zero-padded copy of it when Ap != A
    bd: torch.Tensor                          # fp32 [A]
    bu: torch.Tensor                          # fp32 [H]
    merged: bool
    grouped: bool
    WM: Optional[torch.Tensor] = None         # merged: this layer's rows of MergedPack.WM / .bM / .WF
    bM: Optional[torch.Tensor] = None
    WF: Optional[torch.Tensor] = None
    upT: Optional[torch.Tensor] = None        # bf16 [A, H] / [H, Ap]: operands of the adapter backward, rebuilt on first use
    downT: Optional[torch.Tensor] = None      # after every refresh (_adapter_bwd_operands)


@dataclass
class LoraSite:
    """LoRA on one frozen projection of one layer: W' = W + s.B.A lives in the rows [t*H, (t+1)*H) of that layer's packed Wqkv
    (and the matching columns of WqkvT); lora_A.weight is the `down` and lora_B.weight the `up` of its gradient products."""
    name: str   # the module: deberta.encoder.layer.<li>.attention.self.<query|key|value>_proj
    li: int
    t: int      # 0 query, 1 key, 2 value
    idx: int    # its place in the compose table and in the backward operand packs


class Engine(LiveSetMixin):
    def __init__(self, model):
        self.m = model
        cfg = model.config
        self.cfg = cfg
        self.H, self.I, self.V = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size
        self.nh = cfg.num_attention_heads
        self.nL = cfg.num_hidden_layers
        self.span2 = 2 * cfg.att_span
        # |i - j| < lin_span: identity buckets of the relative-position map (model/deberta.py:578-589: mid = bucket_size // 2)
        self.lin_span = min(cfg.position_buckets // 2, cfg.att_span) if cfg.position_buckets > 0 else 0
        self.F = model.features_dim
        self.Fp = _ru(self.F, 64) if self.F else 0
        self.A1 = self.H // model.ds_factor_attn if model.ds_factor_attn else 0
        self.A2 = self.H // model.ds_factor_ff if model.ds_factor_ff else 0
        self.Vp = _ru(self.V, 64)
        dev = model.device
        if dev.type != "cuda":
            raise RuntimeError("frozenbilm_amd runs on MI355X only: move the model to a cuda (HIP) device; "
                               "there is no CPU fallback")
        L.load()
        self.dev = dev
        # Engine options: `model.engine_options` (a dict read ONCE, when the engine is built; the product reads no environment
        # variable).  Defaults are the shipped configuration.  None of them picks an adapter route: those follow from the
        # shapes alone (AdapterSite.merged / .grouped).
        o = dict(getattr(model, "engine_options", None) or {})
        unknown = set(o) - {"eager_logits", "dw_group", "attn_save_p"}
        if unknown:
            raise ValueError(f"unknown engine_options: {sorted(unknown)}")
        #   eager_logits   fill the full [N, V] logits in every forward even when only the loss is consumed (reference-eager)
        self.eager_logits = bool(o.get("eager_logits", False))
        #   attn_save_p    False = the attention backward recomputes the probabilities and forms dK by the key-major shear pass
        #                  instead of reading the ones the training forward saved (157 MB per layer execution at the bench shape,
        #                  held until the backward)
        self.attn_save_p = bool(o.get("attn_save_p", True))
        #   dw_group       adapter gradient products per launch (<= 16)
        self.dw_group = max(1, min(L.ADW_MAX_ADAPTERS, int(o.get("dw_group", 16))))
        self.n_prompt = int(getattr(model, "n_prompt", 0))  # prompt tuning: trainable embedding rows in front of the text
        # deep prompt tuning: layers 1 .. prompt_depth-1 read their own rows in the prompt slots of their input (_prompt_overwrite)
        self.prompt_depth = int(getattr(model, "prompt_depth", 1))
        self._build_flat()
        self._pack_frozen()
        self._build_trainable_operands()
        self._build_lora()
        self._compose_ev = None  # (event after layer 0, event after everything) of the last compose (refresh_trainable_operands)
        self._relidx: Dict[int, torch.Tensor] = {}
        self._pos_cache: Dict[int, torch.Tensor] = {}  # per-layer position projections of inference forwards (_pos_proj_cached)
        self._no_pos_cache = False  # set while an inference graph is captured: a replay must not depend on state kept outside it
        self.reducer = None  # set by parallel.GradReducer for data-parallel training
        self._dyz_pool: Dict[tuple, list] = {}  # [N, K_fold] operands of the folded adapter backward with their padding zeroed once
        self._dyz_shape = None                   # ... of the current batch shape only
        self._dyz_compact = None                 # ... of the compact backward: one buffer of the current row count (_layer_bwd_compact)
        self.params_version = 0  # bumped by FusedAdam.step (which updates the flat buffer through raw pointers)
        self._ops_version = None
        self.skip_dead_layer = True
        self._ln_ws = L.ln_bwd_ws(self.H, dev)
        self._cs_ws = L.colsum_ws(max(self.H, self.I), dev)
        # split-K partials (main stream): 192 MiB, enough for the prediction-head backward of ~2000 labelled rows (15 slices x
        # rows x H floats) -- with a smaller workspace that GEMM falls back to atomic adds and the step stops being
        # reproducible bit for bit
        self.sk_ws = torch.empty(48 << 20, dtype=F32, device=dev)
        # trainable-weight gradients are off the critical path (nothing downstream in backward reads them): they run on a
        # side HIP stream and fill the tails of the big dX GEMMs; own workspaces so they never race with the main stream
        self.side = torch.cuda.Stream(device=dev)  # (stream priorities were measured: no effect on the interference)
        self.side_ws = torch.empty(8 << 20, dtype=F32, device=dev)
        self.side_cs_ws = L.colsum_ws(max(self.H, self.I), dev)
        # the caller-provided aux stream of the GEMM entry points (remainder rows of multi-round problems run there,
        # concurrently with the big tiles; include/fbl.h): one per device, owned by the host side
        if L._AUX.get(dev.index if dev.index is not None else torch.cuda.current_device()) is None:
            L.set_aux_stream(torch.cuda.Stream(device=dev), dev)
        L.exclude_from_aux(self.side)  # side-stream GEMMs never fork into the aux stream of the main stream's GEMMs

    # ------------------------------------------------------------------ parameter plumbing
    def _build_flat(self):
        """Re-home every parameter that is trainable BY CONSTRUCTION (model.trainable_names(): the constructor flags) into one
        flat fp32 buffer, and its grad into a flat grad buffer.  The layout does not look at `requires_grad`: a parameter the
        caller froze by hand keeps its place -- offsets, data-parallel buckets and the optimizer-state schema never move during
        a run; which of them train in a step is the live set (live_set.LiveSetMixin)."""
        from .model.deberta import flat_order

        m = self.m
        named = dict(m.named_parameters())
        train_names = m.trainable_names()
        order = flat_order(self.cfg, train_names)
        offs, total = flat_layout(order, {n: named[n].numel() for n in order})  # every view 32-byte aligned (padded to 8 floats)
        self.flat = torch.zeros(total, dtype=F32, device=self.dev)
        # the gradient buffer is preceded by a few floats that travel with the first data-parallel bucket (the step's logged
        # loss: parallel.GradReducer.stage_scalars); clip + Adam and p.grad only ever see `flat_grad`
        from .parallel import SCALAR_SLOT

        self.flat_grad_full = torch.zeros(SCALAR_SLOT + total, dtype=F32, device=self.dev)
        self.flat_grad = self.flat_grad_full[SCALAR_SLOT:]
        self.flat_bf16 = torch.zeros(total, dtype=BF16, device=self.dev)
        self.offsets, self.order = offs, order
        self._adT_offs = {}
        self.G: Dict[str, torch.Tensor] = {}
        self.Pb: Dict[str, torch.Tensor] = {}
        for n in order:
            p = named[n]
            o, k = offs[n], p.numel()
            view = self.flat[o:o + k].view(p.shape)
            view.copy_(p.data)
            p.data = view
            self.G[n] = self.flat_grad[o:o + k].view(p.shape)
            self.Pb[n] = self.flat_bf16[o:o + k].view(p.shape)
        self.P = {n: p.data for n, p in named.items()}
        self.named = named
        # bucket boundaries (one bucket per backward stage) for the gradient all-reduce
        self.bucket_ends: Dict[str, int] = {}
        for n in order:
            key = self._bucket_key(n)
            self.bucket_ends[key] = offs[n] + _ru(named[n].numel(), 8)
        self._plans: Dict[tuple, object] = {}
        self._init_live()

    def plan(self, grad_in=()):
        """the backward stages of a step with the current live set (live_set.stage_plan), per (live set, inputs with a gradient)"""
        key = (self.live_version, bool(grad_in))
        pl = self._plans.get(key)
        if pl is None:
            pl = self._plans[key] = stage_plan(self.nL, bool(self.cfg.conv_kernel_size), self.live_order, grad_in)
        return pl

    def _bucket_key(self, name: str) -> str:
        if name.startswith("lm_predictions."):
            return "head"
        if name.startswith("deberta.encoder.layer."):
            return "layer" + name.split(".")[3]
        if name.startswith("deberta.encoder.conv."):
            return "conv"
        if name.startswith("deberta.encoder.LayerNorm"):
            return "relln"
        return "emb"

    def attach_grads(self):
        """Make p.grad of the LIVE parameters the views of the flat grad buffer; zero it when the user dropped the grads
        (set_to_none).  A dead parameter gets no .grad (its slice of the buffer is zero: LiveSetMixin._set_live)."""
        fresh = all(self.named[n].grad is None for n in self.live_order)
        if fresh:
            L.zero_(self.flat_grad)
        for n in self.live_order:
            p = self.named[n]
            if p.grad is None:
                if not fresh:
                    self.G[n].zero_()
                p.grad = self.G[n]
            elif p.grad.data_ptr() != self.G[n].data_ptr():
                self.G[n].copy_(p.grad)
                p.grad = self.G[n]

    def _pack_frozen(self):
        P, H, I = self.P, self.H, self.I
        nL, dev = self.nL, self.dev
        bf = lambda t: t.to(BF16).contiguous()
        # The transposed frozen weights in front of the two adapter sites live in one tensor per site type, in REVERSE layer
        # order (index j = nL-1-layer) -- the order of the adapters in the flat trainable buffer: the per-step compose of
        # the merged weights runs over them as strided batches (_build_trainable_operands, _compose_adapter_down)
        self.WoT_rev = torch.empty(nL, H, H, dtype=BF16, device=dev)
        self.WdT_rev = torch.empty(nL, I, H, dtype=BF16, device=dev)
        self.Lw = []
        for i in range(self.nL):
            p = f"deberta.encoder.layer.{i}"
            s = p + ".attention.self."
            j = nL - 1 - i
            Wqkv = torch.cat([P[s + "query_proj.weight"], P[s + "key_proj.weight"], P[s + "value_proj.weight"]], 0)
            self.WoT_rev[j].copy_(P[p + ".attention.output.dense.weight"].t())
            self.WdT_rev[j].copy_(P[p + ".output.dense.weight"].t())
            d = dict(
                Wqkv=bf(Wqkv), WqkvT=bf(Wqkv.t()),
                bqkv=torch.cat([P[s + "query_proj.bias"], P[s + "key_proj.bias"], P[s + "value_proj.bias"]]).float().contiguous(),
                Wo=bf(P[p + ".attention.output.dense.weight"]), WoT=self.WoT_rev[j],
                bo=P[p + ".attention.output.dense.bias"].float().contiguous(),
                Wi=bf(P[p + ".intermediate.dense.weight"]), WiT=bf(P[p + ".intermediate.dense.weight"].t()),
                bi=P[p + ".intermediate.dense.bias"].float().contiguous(),
                Wd=bf(P[p + ".output.dense.weight"]), WdT=self.WdT_rev[j],
                bd=P[p + ".output.dense.bias"].float().contiguous(),
            )
            self.Lw.append(d)
        # [Wq ; Wk]^T of every layer EXECUTION that has a backward, in backward order (the last layer's two enhanced-mask-decoder
        # passes, then layers nL-2 .. 0): the position-table gradients of all of them are projected by one strided-batch GEMM
        # (behind them the last layer once more: its own encoder execution, which has a backward only when a gradient arrives on
        # hidden_states[nL]; it joins the chain last, so every other step takes the first nL + 1 entries as before)
        order = [nL - 1, nL - 1] + list(range(nL - 2, -1, -1)) + [nL - 1]
        self.WposT_exec = torch.empty(len(order), H, 2 * H, dtype=BF16, device=dev)
        for e, li in enumerate(order):
            self.WposT_exec[e].copy_(self.Lw[li]["WqkvT"][:, : 2 * H])
        if self.cfg.conv_kernel_size:
            w = P["deberta.encoder.conv.conv.weight"]  # [H_out, H_in, 3] -> [H_out, k*H_in + c]
            W2 = w.permute(0, 2, 1).reshape(H, 3 * H)
            self.Wc, self.WcT = bf(W2), bf(W2.t())
            self.bc = P["deberta.encoder.conv.conv.bias"].float().contiguous()
        hd = "lm_predictions.lm_head."
        self.Wh, self.WhT = bf(P[hd + "dense.weight"]), bf(P[hd + "dense.weight"].t())
        self.bh = P[hd + "dense.bias"].float().contiguous()
        E = P["deberta.embeddings.word_embeddings.weight"]
        self.E32 = E.float().contiguous()
        self.Eb = bf(E)
        self.ETb = torch.zeros(H, self.Vp, dtype=BF16, device=self.dev)
        self.ETb[:, : self.V] = E.t().to(BF16)
        self.head_bias = P[hd + "bias"].float().contiguous()
        self.rel_emb = P["deberta.encoder.rel_embeddings.weight"].float().contiguous()
        self.pos_emb = P["deberta.embeddings.position_embeddings.weight"].float().contiguous()
        if self.m.n_ans:
            T = P["answer_embeddings.weight"]
            self.n_ans = T.shape[0]
            self.Ansb = bf(T)
            self.ans_bias = P["answer_bias"].float().contiguous()

    def _build_trainable_operands(self):
        """The adapter sites and the video projection: stable views / persistent buffers of every bf16 operand that follows
        the trainable parameters (refresh_trainable_operands fills them)."""
        H, nL, dev = self.H, self.nL, self.dev
        self.sites = [[None, None] for _ in range(nL)]  # per layer: [attention-output adapter, FFN-output adapter] or None
        self.packs: List[MergedPack] = []
        for k, (blk, A, K, WT, wkey, bkey) in enumerate(((".attention.output.adapter", self.A1, H, self.WoT_rev, "Wo", "bo"),
                                                         (".output.adapter", self.A2, self.I, self.WdT_rev, "Wd", "bd"))):
            if not A:
                continue
            Ap = _ru(A, 64)
            merged = A % 64 == 0 and H % 64 == 0
            names = [f"deberta.encoder.layer.{i}{blk}" for i in range(nL)]
            pack = None
            if merged:
                # backward twin of the merged weights: dctx = [dy | dz] . [Wo^T | (Wd.Wo)^T]^T folds the adapter's dx = dy + dz.Wd
                # into the dense layer's dX GEMM (K = H + A1, padded to an even number of 64-wide K tiles with zero columns)
                WF = torch.zeros(nL, H, _ru(H + A, 128), dtype=BF16, device=dev) if k == 0 else None
                # Layers nL-1 .. 1 sit at a constant stride in the flat trainable buffer: one strided batch; layer 0 (the conv
                # LayerNorm sits between it and layer 1) gets its own and goes first
                ow = [self.offsets[n + ".down.weight"] for n in names]
                ob = [self.offsets[n + ".down.bias"] for n in names]
                if nL >= 3 and len({ow[i - 1] - ow[i] for i in range(2, nL)}) == 1 and \
                        len({ob[i - 1] - ob[i] for i in range(2, nL)}) == 1 and ow[nL - 2] - ow[nL - 1] == ob[nL - 2] - ob[nL - 1] > 0:
                    groups = [(nL - 1, 1, ow[0], ob[0], A * H), (0, nL - 1, ow[nL - 1], ob[nL - 1], ow[nL - 2] - ow[nL - 1])]
                else:
                    groups = [(nL - 1 - i, 1, ow[i], ob[i], A * H) for i in range(nL)]
                pack = MergedPack(A=A, WT=WT, WM=torch.zeros(nL, H + A, K, dtype=BF16, device=dev),
                                  bM=torch.zeros(nL, H + A, dtype=F32, device=dev),
                                  b16=torch.zeros(nL, 1, H, dtype=BF16, device=dev), WF=WF, groups=groups)
                self.packs.append(pack)
            for i, n in enumerate(names):
                j = nL - 1 - i
                # (Ap != A: the zero-padded copy of up.weight [H, A] lives in a persistent buffer)
                up = self.Pb[n + ".up.weight"] if Ap == A else torch.zeros(H, Ap, dtype=BF16, device=dev)
                site = AdapterSite(name=n, A=A, Ap=Ap, down=self.Pb[n + ".down.weight"], up=up, bd=self.P[n + ".down.bias"],
                                   bu=self.P[n + ".up.bias"], merged=merged, grouped=Ap <= 256 and H % 8 == 0)
                if merged:
                    pack.WM[j, :H].copy_(self.Lw[i][wkey])
                    pack.bM[j, :H].copy_(self.Lw[i][bkey])
                    pack.b16[j, 0].copy_(self.Lw[i][bkey])
                    site.WM, site.bM = pack.WM[j], pack.bM[j]
                    if pack.WF is not None:
                        pack.WF[j, :, :H].copy_(WT[j])
                        site.WF = pack.WF[j]
                self.sites[i][k] = site
        self.all_sites = [a for pair in self.sites for a in pair if a is not None]
        if self.F:
            wv = self.Pb["deberta.embeddings.linear_video.weight"]
            self.Wv = wv if self.Fp == self.F else torch.zeros(H, self.Fp, dtype=BF16, device=dev)

    def _build_lora(self):
        """The LoRA sites (model.lora_rank > 0): the table of the compose launch (include/fbl_lora.h) over the fp32 masters, the
        LoRA parameters in the flat buffer and the packed operands, all of which never move."""
        from .model.deberta import LORA_TARGETS

        m, H = self.m, self.H
        self.lora_r = int(getattr(m, "lora_rank", 0) or 0)
        self.lora_sites: Dict[tuple, LoraSite] = {}
        self.lora_composes = 0   # compose launches so far (tests: inside weights_frozen() two forwards compose once)
        self._lora_ops = None    # backward operands (_lora_bwd_operands), dropped by every refresh
        self._lora_idx = None
        self._lora_names = set()
        self._lora_pos = False
        if not self.lora_r:
            return
        self.lora_s = float(m.lora_scale)
        recs = []
        for i in range(self.nL):
            for tname in m.lora_targets:
                t = LORA_TARGETS.index(tname)
                nm = f"deberta.encoder.layer.{i}.attention.self.{tname}"
                self.lora_sites[(i, t)] = LoraSite(name=nm, li=i, t=t, idx=len(recs))
                recs.append(dict(W=self.P[nm + ".weight"], A=self.P[nm + ".lora_A.weight"], B=self.P[nm + ".lora_B.weight"],
                                 scale=self.lora_s, dst=self.Lw[i]["Wqkv"][t * H:(t + 1) * H],
                                 dstT=self.Lw[i]["WqkvT"][:, t * H:(t + 1) * H]))
        self._lora_recs = recs
        self._lora_table = L.LoraTable(recs, self.dev)
        self._lora_names = {s.name for s in self.lora_sites.values()}
        self._lora_pos = any(t < 2 for (_, t) in self.lora_sites)  # query / key: their weights also project the position table
        self._lora_Aop = torch.zeros(len(recs), 64, H, dtype=BF16, device=self.dev)   # [A ; 0]: K-contiguous, r padded to 64
        self._lora_BTop = torch.zeros(len(recs), 64, H, dtype=BF16, device=self.dev)  # [B^T ; 0]

    def _compose_lora(self):
        """W' = W + s.B.A of every LoRA site into the packed bf16 operands, one launch on the current stream; then the
        [Wq ; Wk]^T copies of the position-gradient chain follow the composed WqkvT."""
        L.lora_compose(self._lora_table)
        self.lora_composes += 1
        if self._lora_pos:
            H, nL = self.H, self.nL
            for e, li in enumerate([nL - 1, nL - 1] + list(range(nL - 2, -1, -1)) + [nL - 1]):
                self.WposT_exec[e].copy_(self.Lw[li]["WqkvT"][:, : 2 * H])

    def merge_lora(self):
        """W <- W + s.B.A in the fp32 masters (the compose kernel's fp32 result: the same arithmetic as the packed operands),
        then B <- 0.  The caller drops this engine (model.merge_lora)."""
        L.lora_compose(L.LoraTable([dict(r, dst32=r["W"]) for r in self._lora_recs], self.dev))
        for r in self._lora_recs:
            r["B"].zero_()
        self.invalidate_operands()

    def _lora_bwd_operands(self):
        """[A ; 0] and [B^T ; 0] (bf16 [sites, 64, H]) of every LoRA site, gathered out of the flat bf16 parameter copy on first
        use after a refresh: the K-contiguous operands of the two narrow GEMMs in front of the weight-gradient products."""
        if self._lora_ops is None:
            r, H, dev = self.lora_r, self.H, self.dev
            if self._lora_idx is None:
                i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)
                sites = sorted(self.lora_sites.values(), key=lambda s: s.idx)
                oA = i64([self.offsets[s.name + ".lora_A.weight"] for s in sites])
                oB = i64([self.offsets[s.name + ".lora_B.weight"] for s in sites])
                rowmajor = torch.arange(r * H, device=dev)
                transposed = (torch.arange(H, device=dev)[None, :] * r + torch.arange(r, device=dev)[:, None]).reshape(-1)
                self._lora_idx = ((oA[:, None] + rowmajor[None]).reshape(-1), (oB[:, None] + transposed[None]).reshape(-1))
            ns = len(self.lora_sites)
            self._lora_Aop[:, :r].copy_(self.flat_bf16.index_select(0, self._lora_idx[0]).view(ns, r, H))
            self._lora_BTop[:, :r].copy_(self.flat_bf16.index_select(0, self._lora_idx[1]).view(ns, r, H))
            self._lora_ops = (self._lora_Aop, self._lora_BTop)
        return self._lora_ops

    def _lora_products(self, site: LoraSite, dy, x):
        """The operands of one execution's two weight-gradient products of a LoRA site, in the shape of an adapter's
        (fbl_adapter_bwd_dw): dB += dy^T.u with u = s.x.A^T, dA += v^T.x with v = s.dy.B; u, v bf16 [rows, 64], zero beyond r."""
        Aop, BTop = self._lora_bwd_operands()
        n = dy.shape[0]
        u = torch.empty(n, 64, dtype=BF16, device=self.dev)
        v = torch.empty(n, 64, dtype=BF16, device=self.dev)
        L.gemm(x, Aop[site.idx], alpha=self.lora_s, out_bf16=u)
        L.gemm(dy, BTop[site.idx], alpha=self.lora_s, out_bf16=v)
        return (dy, u, v, x)

    def _lora_live(self, site: Optional[LoraSite]) -> bool:
        return site is not None and any((site.name + k) in self.Gl for k in (".lora_A.weight", ".lora_B.weight"))

    def _lora_bwd(self, run, li: int, t: int, dy, x):
        """Park the weight-gradient products of LoRA site (li, t) for one layer execution: dy bf16 [N, H] the gradient of the
        projection's output, x bf16 [N, H] its input.  A site without a live member launches nothing."""
        site = self.lora_sites.get((li, t))
        if not self._lora_live(site):
            return
        run.dw_pending.append((self.lora_r, site.name, self._lora_products(site, dy, x), run.dw_count, None))
        run.dw_count += 1

    def _dw_outputs(self, nm: str, Gl):
        """(dWu, dWd, dbd) views of the flat gradient buffer behind the parked products of `nm` (None: dead, no output): an
        adapter's up / down weights and down bias, or a LoRA site's lora_B (the `up`) and lora_A (the `down`)"""
        if nm in getattr(self, "_lora_names", ()):
            return Gl.get(nm + ".lora_B.weight"), Gl.get(nm + ".lora_A.weight"), None
        return Gl.get(nm + ".up.weight"), Gl.get(nm + ".down.weight"), Gl.get(nm + ".down.bias")

    def _lora_pos_bwd(self, run, pc, dpb):
        """The position path of the LoRA'd query / key projections: PQ = query_proj(R_e), PK = key_proj(R_e) of every execution
        e, R_e the normalised table behind that execution's position dropout.  dpb bf16 [E, rcnt, 2H] = [dPQ | dPK] of the
        table rows rmin .. rmin + rcnt (the others have zero gradient).  Same two products as the token path, rows = rcnt."""
        H, nL = self.H, self.nL
        order = [nL - 1, nL - 1] + list(range(nL - 2, -1, -1)) + [nL - 1]  # the executions of the chain (WposT_exec)
        segs: Dict[str, list] = {}
        for e in range(dpb.shape[0]):
            sites = [self.lora_sites.get((order[e], t)) for t in (0, 1)]
            if not any(self._lora_live(s) for s in sites):
                continue
            if run.p_hid > 0:
                xe = torch.empty(self.span2, H, dtype=BF16, device=self.dev)
                L.dropout_f32(run.R32, run.p_hid, pc.seeds[e], out_bf16=xe)
            else:
                xe = run.Rb
            x = xe[pc.rmin:pc.rmin + pc.rcnt]
            for t, site in enumerate(sites):
                if self._lora_live(site):
                    segs.setdefault(site.name, []).append(self._lora_products(site, dpb[e][:, t * H:(t + 1) * H], x))
        groups, nseg = [], 0
        for nm, sg in list(segs.items()) + [(None, None)]:
            if groups and (nm is None or len(groups) == L.ADW_MAX_ADAPTERS or nseg + len(sg) > L.ADW_MAX_SEGMENTS):
                L.adapter_bwd_dw(groups, A=self.lora_r)
                groups, nseg = [], 0
            if nm is not None:
                groups.append((sg, *self._dw_outputs(nm, self.Gl)))
                nseg += len(sg)

    def relidx(self, S: int) -> torch.Tensor:
        if S not in self._relidx:
            v = rel_index_vector(S, self.cfg.position_buckets, self.cfg.max_rel, self.cfg.att_span)
            self._relidx[S] = torch.from_numpy(np.ascontiguousarray(v)).to(self.dev)
        return self._relidx[S]

    def _refresh_if_stale(self, need_grad: bool):
        """bf16 operands / composed adapter rows follow the trainable parameters: rebuilt before EVERY forward by default
        (0.2 ms of GPU time).  Only inside `model.weights_frozen()` -- the evaluate loops, the inference-graph path -- is the
        rebuild skipped while nothing the engine can see has written to them: FusedAdam.step (params_version) and in-place
        updates through the parameter objects (autograd version counters).  Writes through `.data`, into `engine.flat` or by
        a broadcast into the flat buffer bump neither counter, which is why skipping is opt-in."""
        frozen = getattr(self.m, "_weights_frozen", 0) > 0
        ver = (self.params_version, tuple(self.named[n]._version for n in self.order)) if (frozen and not need_grad) else None
        if ver is None or ver != self._ops_version:
            self.refresh_trainable_operands()
            self._ops_version = ver

    def seed_word_value(self) -> int:
        """the 64-bit word a training pass adds to its per-site dropout seeds: the model's position in its mask stream"""
        return (self.m.dropout_seed_base() * 0x9E3779B1) & 0x7FFFFFFFFFFFFFFF

    def prepare_inference(self):
        """Everything an inference forward needs from OUTSIDE its launch sequence, done now: the bf16 operand copies /
        composed adapter rows are current (rebuilt in place: a captured graph keeps reading the same buffers) and the
        current stream has waited for the side stream that composes them (a captured forward may not wait on events
        recorded outside its capture, so `_compose_ev` is consumed here)."""
        self._refresh_if_stale(False)
        if self._compose_ev is not None:
            torch.cuda.current_stream().wait_event(self._compose_ev[1])
            self._compose_ev = None

    def invalidate_operands(self):
        """the trainable parameters were modified in a way the engine cannot see (through `.data`): rebuild on next use"""
        self._ops_version = None
        self.params_version += 1

    def refresh_trainable_operands(self):
        """bf16 MFMA operands of the trainable matrices (they change every optimizer step)."""
        self._pos_cache.clear()
        L.cast_bf16(self.flat, self.flat_bf16)
        for a in self.all_sites:
            if a.Ap != a.A:
                a.up[:, :a.A] = self.Pb[a.name + ".up.weight"]
            a.upT = a.downT = None
        # composed rows of the merged dense + down-projection weights: off the critical path, on the side stream (layer 0
        # first -- the forward reaches its merged GEMM after ~0.3 ms -- then all other layers in one strided batch)
        if self.packs:
            self.side.wait_stream(torch.cuda.current_stream())  # the bf16 cast of the flat buffer above
            with torch.cuda.stream(self.side):
                self._compose_ev = self._compose_adapter_down()
        if self.F and self.Fp != self.F:
            self.Wv[:, : self.F] = self.Pb["deberta.embeddings.linear_video.weight"]
        if self.lora_r:  # W' = W + s.B.A into the packed Q/K/V operands (fp32 masters: does not wait for the cast above)
            self._lora_ops = None
            self._compose_lora()

    def _compose_adapter_down(self):
        """Rows [H, H+A) of the merged weights / biases: Wd.W and Wd.b + bd for every layer (see MergedPack), from the
        current adapter weights: one strided-batch GEMM each for the matrix and the bias per group of layers, layer 0 of
        every site type first.  Returns (event after layer 0, event after everything) recorded on the current stream."""
        H = self.H

        def run_group(pk: MergedPack, grp):
            A, (j0, nb, o_w, o_b, st) = pk.A, grp
            wd3 = torch.as_strided(self.flat_bf16, (nb, A, H), (st, H, 1), o_w)
            L.gemm(wd3, pk.WT[j0:j0 + nb], out_bf16=pk.WM[j0:j0 + nb, H:H + A, :])                # Wd . W
            if pk.WF is not None:  # (Wd . W)^T next to W^T: the K-extension of the folded backward GEMM
                L.gemm(pk.WT[j0:j0 + nb], wd3, out_bf16=pk.WF[j0:j0 + nb, :, H:H + A])
            bd3 = torch.as_strided(self.flat, (nb, A, 1), (st, 1, 1), o_b)
            bo3 = torch.as_strided(pk.bM, (nb, A, 1), (pk.bM.stride(0), 1, 1), pk.bM[j0, H:].storage_offset())
            L.gemm(wd3, pk.b16[j0:j0 + nb], aux=bd3, aux_kind=L.AUX_ADD_F32, out_f32=bo3)        # Wd . b + bd

        for pk in self.packs:
            run_group(pk, pk.groups[0])
        ev0 = torch.cuda.Event()
        ev0.record()
        for pk in self.packs:
            for grp in pk.groups[1:]:
                run_group(pk, grp)
        ev1 = torch.cuda.Event()
        ev1.record()
        return ev0, ev1

    def _adapter_bwd_operands(self, site: AdapterSite):
        """W^T operands for the adapter backward (trainable, so rebuilt after every optimizer step): all adapters of a
        shape are transposed by ONE batched launch straight out of the flat bf16 parameter copy, on first use in a
        step.  Bottlenecks that are not a multiple of 64 take the zero-padded per-adapter path."""
        if site.upT is None:
            H = self.H
            groups = {}
            for a in self.all_sites:
                groups.setdefault((a.A, a.Ap), []).append(a)
            for (A, Ap), sites in groups.items():
                upT_all = torch.empty(len(sites), A, H, dtype=BF16, device=self.dev)
                for i, a in enumerate(sites):
                    a.upT = upT_all[i]  # [A,H] = up.weight[H,A]^T
                cache = self._adT_offs.get((A, Ap))
                if cache is None:
                    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=self.dev)
                    cache = dict(up_src=i64([self.offsets[a.name + ".up.weight"] for a in sites]),
                                 dn_src=i64([self.offsets[a.name + ".down.weight"] for a in sites]),
                                 dst=i64([i * A * H for i in range(len(sites))]))
                    self._adT_offs[(A, Ap)] = cache
                L.transpose_batched_bf16(self.flat_bf16, cache["up_src"], upT_all, cache["dst"], H, A)
                if Ap == A:
                    dnT_all = torch.empty(len(sites), H, A, dtype=BF16, device=self.dev)
                    L.transpose_batched_bf16(self.flat_bf16, cache["dn_src"], dnT_all, cache["dst"], A, H)
                    for i, a in enumerate(sites):
                        a.downT = dnT_all[i]  # [H,A] = down.weight[A,H]^T
                else:  # K of the consuming GEMM must be a multiple of 64: zero-padded columns
                    for a in sites:
                        a.downT = torch.zeros(H, Ap, dtype=BF16, device=self.dev)
                        a.downT[:, :A].copy_(a.down.t())
        return site.upT, site.downT

    # ------------------------------------------------------------------ public entry
    def run(self, input_ids, attention_mask, video, video_mask, labels, mlm, want_hidden, logit_rows=None, want_attn=False,
            inputs_embeds=None):
        """inputs_embeds: float [B, L, H] in place of E[input_ids] (input_ids is then None; model/deberta.py:1204-1225)."""
        m = self.m
        train = m.training
        k_pred = check_topk(getattr(m, "predict_topk", 0))  # opt-in `model.predict_topk`, read per call (ValueError here)
        text = input_ids if inputs_embeds is None else inputs_embeds
        if text.device != self.dev:
            raise RuntimeError(f"inputs must be on {self.dev}")
        B, Lt = text.shape[:2]
        if attention_mask is None:
            attention_mask = (torch.ones_like(input_ids) if inputs_embeds is None
                              else torch.ones(B, Lt, dtype=torch.long, device=self.dev))
        use_video = bool(self.F) and video is not None
        # inputs that take a gradient of their own: they become tensor inputs of the step's autograd node (_StepFn)
        grad_on = torch.is_grad_enabled()
        grad_in = []
        if grad_on and use_video and video.requires_grad:
            grad_in.append(("video", video))
        if grad_on and inputs_embeds is not None and inputs_embeds.requires_grad:
            grad_in.append(("embeds", inputs_embeds))
        # the live set: the trainable-by-construction parameters whose requires_grad is true NOW (a host loop over the flags);
        # nothing live and no input with a gradient: the call keeps no bookkeeping, as under no_grad (dropout stays live)
        need_grad = grad_on and (self.update_live() or bool(grad_in))
        T = video.shape[1] if use_video else 0
        Pn = self.n_prompt  # prompt tuning: the sequence is [video T | prompt Pn | text Lt]; the text starts at T + Pn
        S = T + Pn + Lt
        if S > self.cfg.max_position_embeddings:
            raise RuntimeError(
                f"sequence of {S} positions (video {T} + " + (f"prompt {Pn} + " if Pn else "") + f"text {Lt}) exceeds "
                f"max_position_embeddings={self.cfg.max_position_embeddings} (the reference fails the same way, "
                "model/deberta.py:1020-1021,1392)")
        front = []
        if use_video:
            if video_mask is None:
                video_mask = torch.ones(video.shape[:2], device=self.dev, dtype=attention_mask.dtype)
            front.append(video_mask.to(attention_mask.dtype))
        if Pn:  # prompt slots: mask 1, label -100
            front.append(torch.ones(B, Pn, device=self.dev, dtype=attention_mask.dtype))
        mask = torch.cat([*front, attention_mask], 1) if front else attention_mask
        mask = mask.to(torch.int32).contiguous()
        full_labels = None
        if labels is not None:
            if T + Pn:
                full_labels = torch.cat([torch.full((B, T + Pn), -100, dtype=torch.long, device=self.dev), labels], 1)
            else:
                full_labels = labels
            full_labels = full_labels.contiguous().view(-1)
            # The labelled rows are a function of the INPUT only: find them before anything is queued, so the host
            # synchronisation inside nonzero() waits for the previous step at most, never for this forward.
            rows_labelled = torch.nonzero(full_labels != -100).view(-1)
        # The backward's own row layout (_backward_rows): decided here, from the INPUT, and read back at the point where the
        # host already waits for the label rows -- the forward below does not use it.
        bwd_rows = self._backward_rows(m, need_grad, tuple(k for k, _ in grad_in), mask, full_labels, logit_rows, want_hidden, want_attn,
                                        B, S, T)
        if logit_rows is not None:
            if full_labels is not None:
                raise RuntimeError("logit_rows cannot be combined with labels (the loss of a labelled call lives on its own rows)")
            if need_grad:  # (the no-grad path only gathers: it stays as permissive as it was)
                check_logit_rows(logit_rows, B * S)
        # Packed rows (opt-in, frozenbilm_amd extension): drop the trailing padding rows of every sample.  Only for calls
        # whose outputs live on selected rows (a loss, logit_rows); like the label rows, the layout is a function of the
        # INPUT, read back before anything is queued.
        pk = None
        if (getattr(m, "packed_rows", False) and not want_attn and (full_labels is not None or logit_rows is not None)
                and not torch.cuda.is_current_stream_capturing()):
            pk = self._make_packing(mask, full_labels, logit_rows, B, S, T)
        if train:
            m.step_seed += 1
        # Dropout seeds = a per-site constant (a function of the site index only) + the position of this step in the model's
        # mask stream.  Eager launches add the two on the host (Run.next_seed); a captured launch sequence keeps the per-site
        # constants as kernel arguments and reads the position from a device word (train_graph.py; include/fbl.h "Dropout
        # seeds") -- the same sum, so eager and replayed steps draw identical masks.
        run = Run(B=B, S=S, T=T, P=Pn, Lt=Lt, train=train, save=need_grad, seed_base=self.seed_word_value() if train else 0,
                  p_hid=self.cfg.hidden_dropout_prob if train else 0.0,
                  p_att=self.cfg.attention_probs_dropout_prob if train else 0.0,
                  p_ad=m.adapter_dropout if train else 0.0, mask=mask.view(-1), pk=pk, N=pk.n if pk is not None else B * S,
                  want_attn=bool(want_attn), labels=full_labels, rows=rows_labelled if full_labels is not None else None,
                  bwd_rows=bwd_rows)
        if want_attn and train and run.p_att > 0:
            raise NotImplementedError("output_attentions=True is served in eval mode (the probabilities of a training forward "
                                      "carry the attention dropout mask, which the fused kernel regenerates instead of storing)")
        # Decoder on the selected rows (opt-in `model.decoder_rows`): both enhanced-mask-decoder passes, the head and their
        # backward run on the labelled rows / the logit_rows only; calls that need every row keep the full decoder.
        # (a model with LoRA on its attention projections takes the full decoder: the selected-rows route is not checked with it)
        if (getattr(m, "decoder_rows", False) and not self.lora_r and not want_attn and not want_hidden and not self.eager_logits
                and (full_labels is not None or logit_rows is not None) and not torch.cuda.is_current_stream_capturing()):
            run.dec_grid = (rows_labelled if full_labels is not None else logit_rows.to(self.dev).long().view(-1))
        if pk is not None and full_labels is not None:  # the head works on packed rows; the labels are looked up on the grid
            run.label_rows = rows_labelled
            run.rows = pk.inv[rows_labelled]
        self._refresh_if_stale(need_grad)  # bf16 operands / composed adapter rows of the trainable parameters
        use_ans = bool(m.n_ans) and not mlm
        if logit_rows is not None:  # the head runs on these rows only; with gradients its backward does too (_backward)
            run.logit_rows = logit_rows.to(self.dev).to(torch.int32).contiguous().view(-1)
            if pk is not None:
                run.logit_rows = pk.inv[run.logit_rows.long()].to(torch.int32)
        run.embeds = inputs_embeds
        run.video_dtype = video.dtype if use_video else None
        run.grad_in = tuple(k for k, _ in grad_in)
        if need_grad:  # the stages whose backward this step runs: the forward saves nothing below the lowest of them
            run.plan, run.live_version = self.plan(run.grad_in), self.live_version
        run.hid_grad = bool(want_hidden) and need_grad  # the hidden states handed out are outputs of the step's node
        with L.seed_word(run.seed_word):
            logits, loss_t = self._forward(run, input_ids.contiguous() if inputs_embeds is None else None, video, use_ans,
                                           want_hidden or want_attn)
        Vout = self.n_ans if use_ans else self.V
        if logit_rows is not None:  # [R, Vout]; under autograd the node below carries them (fine-tuning on the [MASK] rows)
            res = {"logits": logits[:, :Vout], "loss": None, "run": run}
        else:  # (packed rows: `logits` is the [B*S, V] grid tensor here too -- allocated in _forward, filled on access)
            res = {"logits": logits.view(B, S, -1)[:, :, :Vout] if logits is not None else None, "loss": None, "run": run}
        if k_pred:  # top-k / label rank / NLL of the rows this call already holds logits for (predict.py); detached
            res["predictions"] = predictions_of_call(run, logits, k_pred, rows_labelled if full_labels is not None else None,
                                                     logit_rows)
        if want_hidden:
            res["hidden_states"] = run.hidden_out
        if want_attn:
            res["attentions"] = tuple(run.attn_out)
        if need_grad and res["logits"] is not None:
            # one autograd node for the whole model; both outputs are differentiable: the loss (MLM training,
            # main.py:67-84) and the logits (downstream fine-tuning computes its own loss on them, videoqa.py:66-83,
            # mc.py:64-92)
            lt = loss_t if loss_t is not None else torch.zeros((), dtype=F32, device=self.dev)
            hid = res["hidden_states"] if run.hid_grad else ()
            outs = _StepFn.apply(self, run, lt, res["logits"], len(hid), *hid, *[t for _, t in grad_in],
                                 *[self.named[n] for n in self.order])
            loss_o, res["logits"] = outs[:2]
            res["loss"] = loss_o if full_labels is not None else None
            if hid:
                res["hidden_states"] = tuple(outs[2:])
        elif full_labels is not None:
            res["loss"] = loss_t
        return res

    # Share of dropped rows from which the compact backward is faster than the padded one: the smallest share of the sweep of
    # tools/bench_compact_bwd.py from which on every point beats the padded leg by more than the sweep's run-to-run spread
    # (profiles/compact_backward.json; the gain is a step where the big dX GEMMs lose a round of tiles).  Measured
    # at the bench grid (B = 32, S = 266).
    COMPACT_BWD_MIN_DROPPED = 0.37

    def _backward_rows(self, m, need_grad, grad_in, mask, full_labels, logit_rows, want_hidden, want_attn, B, S, T) -> Optional[Packing]:
        """THE rule of the compact backward: the row layout the backward of this step runs its row-wise work on,
        or None = the padded grid, exactly the backward there always was.  The forward is the padded one either way; the
        gradients are the same bits either way (tests/test_gpu_compact_backward.py), so the choice is by shape and state only.
        Compact needs ALL of:
          * a step that keeps gradient bookkeeping, with a labelled loss (the configuration that is tested: calls with
            logit_rows, output_hidden_states -- a gradient handed in on a hidden state reaches the padding rows -- or
            output_attentions stay padded; so does a backward that is handed a gradient on the logits, decided in _backward);
          * no stream capture (a captured step cannot follow a row count that changes with the batch);
          * none of the other row layouts: model.packed_rows, model.decoder_rows;
          * no LoRA, no prompt slots, no gradient reducer, probabilities saved by the forward (engine option attn_save_p):
            not covered by a test on this route, they stay padded;
          * every stage of the backward runs (partial fine-tuning with a dead bottom stays padded: not tested here);
          * a batch with rows to drop, and -- unless model.compact_backward is True -- a dropped share of at least
            COMPACT_BWD_MIN_DROPPED.
        model.compact_backward: None (default) = this rule, False = always padded (A/B runs), True = the rule without the
        share threshold (tests)."""
        force = getattr(m, "compact_backward", None)
        if (force is False or not need_grad or full_labels is None or logit_rows is not None or want_hidden or want_attn
                or torch.cuda.is_current_stream_capturing() or getattr(m, "packed_rows", False) or getattr(m, "decoder_rows", False)
                or self.lora_r or self.n_prompt or self.reducer is not None or not self.attn_save_p):
            return None
        plan = self.plan(grad_in)
        if plan is not None and plan.lowest != 0:
            return None
        pk = self._make_packing(mask, full_labels, None, B, S, T)
        if pk is None or (force is not True and 1.0 - pk.n / (B * S) < self.COMPACT_BWD_MIN_DROPPED):
            return None
        pk.sel32, pk.inv32 = pk.sel.to(torch.int32), pk.inv.to(torch.int32)
        return pk

    def _make_packing(self, mask, full_labels, logit_rows, B, S, T) -> Optional[Packing]:
        """Packing of this batch, or None when no row can be dropped (one host read of B lengths)."""
        dev = self.dev
        keep = mask.view(B, S) != 0
        if full_labels is not None:
            keep = keep | (full_labels.view(B, S) != -100)
        if logit_rows is not None:
            want = torch.zeros(B * S, dtype=torch.bool, device=dev)
            want[logit_rows.to(dev).long().view(-1)] = True
            keep = keep | want.view(B, S)
        pos1 = torch.arange(1, S + 1, device=dev, dtype=torch.int32)
        plen_h = [max(int(v), T, 1) for v in (keep.to(torch.int32) * pos1).amax(1).tolist()]
        n = sum(plen_h)
        if n >= B * S:
            return None
        offs = [0]
        for v in plen_h:
            offs.append(offs[-1] + v)
        row0 = torch.tensor(offs, dtype=torch.int32, device=dev)
        b_of = torch.repeat_interleave(torch.arange(B, device=dev), torch.tensor(plen_h, device=dev), output_size=n)
        pos = torch.arange(n, device=dev) - row0[:-1].long()[b_of]
        sel = b_of * S + pos
        inv = torch.full((B * S,), -1, dtype=torch.int64, device=dev)
        inv[sel] = torch.arange(n, device=dev)
        return Packing(row0=row0, sel=sel, inv=inv, pos=pos, n=n)

    # ------------------------------------------------------------------ forward
    def _ln(self, run, name, *, y, resid: Optional[Stream], N, p_drop=0.0, rowmask=None, want_f32=False, tail=0):
        H = self.H
        g, b = self.P[name + ".weight"], self.P[name + ".bias"]
        t = torch.empty(N, H, dtype=F32, device=self.dev)
        stats = torch.empty(N, 2, dtype=F32, device=self.dev)
        full = torch.empty(N + tail, H, dtype=BF16, device=self.dev)
        ob = full[:N]
        of = torch.empty(N, H, dtype=F32, device=self.dev) if want_f32 else None
        seed = run.next_seed() if p_drop > 0 else 0
        r_norm = resid.norm.as_args() if resid is not None and resid.norm is not None else None
        r_plain = resid.plain if resid is not None and r_norm is None else None
        L.ln_fwd(y=y, p_drop=p_drop, seed=seed, r_plain=r_plain, r_norm=r_norm,
                 gamma=g, beta=b, eps=self.cfg.layer_norm_eps, rowmask=rowmask, out_t=t, out_stats=stats, out_bf16=ob,
                 out_f32=of, N=N, H=H)
        return Stream(bf16=ob, norm=NormRef(t, stats, g, b, rowmask), plain=of, full=full if tail else None), seed

    def _adapter_fwd(self, run, site: AdapterSite, x_f32, x_bf16, N):
        """y = x + up(drop(relu(down(x))))  (model/adapter.py:33-45): fbl_adapter_down_fwd, then the up-projection as a GEMM
        with bias + residual epilogue.  Returns (y, bottleneck z, dropout seed)."""
        A, Ap = site.A, site.Ap
        z = torch.zeros(N, Ap, dtype=BF16, device=self.dev) if Ap != A else torch.empty(N, Ap, dtype=BF16, device=self.dev)
        seed = run.next_seed() if run.p_ad > 0 else 0
        L.adapter_down_fwd(x_bf16, site.down, site.bd, z, A=A, p_drop=run.p_ad, seed=seed)  # ReLU + dropout in the epilogue
        y = torch.empty(N, self.H, dtype=F32, device=self.dev)
        L.gemm(z, site.up, bias=site.bu, aux=x_f32, aux_kind=L.AUX_ADD_F32, out_f32=y)
        return y, z, seed

    def _dense_adapter_ln(self, run, li, x_bf16, W, bias, site: Optional[AdapterSite], N, ln_name, resid: Stream, tail=0):
        """dense -> adapter -> dropout -> LayerNorm(. + resid)  (model/deberta.py:254-260 / 328-334).  Returns (output
        Stream, dense output bf16, z, adapter seed, LayerNorm-dropout seed).  With a merged adapter site the block is three
        launches -- merged dense + down-projection GEMM (bf16 y, z), up-projection GEMM whose epilogue adds the adapter
        input, applies the block's dropout and adds the residual (writes the pre-norm tensor t once), LayerNorm statistics
        + bf16 operand -- and neither the fp32 dense output nor the fp32 adapter output exist in HBM.  Any other site: the
        plain dense GEMM (W, bias), the adapter if there is one, the full LayerNorm kernel."""
        H, dev = self.H, self.dev
        ob = torch.empty(N, H, dtype=BF16, device=dev)  # bf16 dense output: the adapter's GEMM operand / saved for its backward
        if site is None or not site.merged:
            y = torch.empty(N, H, dtype=F32, device=dev)
            L.gemm(x_bf16, W, bias=bias, out_f32=y, out_bf16=ob)
            z, seed_ad = None, 0
            if site is not None:
                y, z, seed_ad = self._adapter_fwd(run, site, y, ob, N)
            out, seed_ln = self._ln(run, ln_name, y=y, resid=resid, N=N, p_drop=run.p_hid, tail=tail)
            return out, ob, z, seed_ad, seed_ln
        if self._compose_ev is not None:  # the composed rows of this layer must be there (layer 0: first event, others: second)
            torch.cuda.current_stream().wait_event(self._compose_ev[0 if li == 0 else 1])
        A = site.A
        z = torch.empty(N, A, dtype=BF16, device=dev)
        seed_ad = run.next_seed() if run.p_ad > 0 else 0
        L.dense_adapter_down_fwd(x_bf16, site.WM, site.bM, H, z, y_bf16=ob, p_drop=run.p_ad, seed=seed_ad)
        g, b = self.P[ln_name + ".weight"], self.P[ln_name + ".bias"]
        t = torch.empty(N, H, dtype=F32, device=dev)
        stats = torch.empty(N, 2, dtype=F32, device=dev)
        full = torch.empty(N + tail, H, dtype=BF16, device=dev)
        seed_ln = run.next_seed() if run.p_hid > 0 else 0
        r_norm = resid.norm.as_args() if resid.norm is not None else None
        L.adapter_up_resid_fwd(z, site.up, site.bu, ob, t, A=A, p_drop=run.p_hid, seed=seed_ln,
                               r_plain=resid.plain if r_norm is None else None, r_norm=r_norm)
        L.ln_fwd(y=t, gamma=g, beta=b, eps=self.cfg.layer_norm_eps, out_stats=stats, out_bf16=full[:N], N=N, H=H)
        return (Stream(bf16=full[:N], norm=NormRef(t, stats, g, b, None), full=full if tail else None), ob, z, seed_ad,
                seed_ln)

    def _pos_proj_cached(self, li: int, W, Rb: torch.Tensor) -> torch.Tensor:
        """[PQ|PK] = R.[Wq;Wk]^T + b of layer `li` ([2*span, 2H] bf16, model/deberta.py:847-853) for inference forwards inside
        model.weights_frozen(): R = LayerNorm_enc(rel_embeddings) only changes with the trainable parameters, and every
        rebuild of their operands (refresh_trainable_operands) drops this cache."""
        c = self._pos_cache.get(li)
        if c is None:
            c = torch.empty(self.span2, 2 * self.H, dtype=BF16, device=self.dev)
            L.gemm(Rb, W["Wqkv"][: 2 * self.H], bias=W["bqkv"][: 2 * self.H], out_bf16=c)
            self._pos_cache[li] = c
        return c

    def _pos_cache_allowed(self, run) -> bool:
        """an inference forward (no gradient bookkeeping, no position dropout) inside model.weights_frozen(), and not the capture
        of an inference graph: the position projections of a layer may come from _pos_proj_cached"""
        return not run.save and run.p_hid == 0 and getattr(self.m, "_weights_frozen", 0) > 0 and not self._no_pos_cache

    def _layer_fwd(self, run, li: int, kv: Stream, q: Optional[Stream], Rb: torch.Tensor):
        """One execution of encoder layer ``li`` (model/deberta.py:351-375); q != None is the EMD form where the
        query stream (and the attention residual, :290-292) differs from the key/value stream."""
        W = self.Lw[li]
        B, S, H, nh = run.B, run.S, self.H, self.nh
        N = run.N
        Sp = _ru(S, 64)
        dev = self.dev
        sv = LayerSave(li=li, emd=q is not None)
        # One GEMM gives Q|K|V for the N tokens AND the shared-key position projections [PQ|PK] = R.[Wq|Wk]^T (:847-853):
        # the relative-position table R (pos_dropout applied, :779) is written into the P tail rows of the activations.
        P_ = self.span2
        if run.p_hid > 0:
            sv.seed_pos = run.next_seed()

        def put_r(full):
            if run.p_hid > 0:
                L.dropout_f32(run.R32, run.p_hid, sv.seed_pos, out_bf16=full[N:])
            else:
                full[N:].copy_(Rb)

        # Inference shortcuts (no gradient bookkeeping, no position dropout -- results are bit-identical to the general path):
        #  * inside model.weights_frozen() the position projections [PQ|PK] of a layer are the same in every forward: computed
        #    once per layer and kept (dropped whenever the trainable operands are rebuilt), the QKV GEMM then has N rows;
        #  * the second pass of the enhanced mask decoder projects the SAME key/value stream with the same weights as the
        #    first (model/deberta.py:1395-1408): only its query projection is new, written over the first pass's Q columns.
        infer = not run.save and run.p_hid == 0
        pqk_c = self._pos_proj_cached(li, W, Rb) if self._pos_cache_allowed(run) else None
        reuse = infer and q is not None and run.emd_qkv is not None
        if reuse:
            qkv = run.emd_qkv
            if pqk_c is None:
                put_r(q.full)
            L.gemm(q.full if pqk_c is None else q.bf16, W["Wqkv"][:H], bias=W["bqkv"][:H], out_bf16=qkv[:, :H])
        else:
            rows_in = N if pqk_c is not None else N + P_
            qkv = torch.empty(rows_in, 3 * H, dtype=BF16, device=dev)
            kin = kv.full[:rows_in]
            if pqk_c is None:
                put_r(kv.full)
            if q is None:
                L.gemm(kin, W["Wqkv"], bias=W["bqkv"], out_bf16=qkv)
            else:
                if pqk_c is None:
                    put_r(q.full)
                L.gemm(q.full[:rows_in], W["Wqkv"][:H], bias=W["bqkv"][:H], out_bf16=qkv[:, :H])
                L.gemm(kin, W["Wqkv"][H:], bias=W["bqkv"][H:], out_bf16=qkv[:, H:])
                if infer:
                    run.emd_qkv = qkv
        if pqk_c is not None:
            pq, pk = pqk_c[:, :H], pqk_c[:, H:]
        else:
            pq, pk = qkv[N:, :H], qkv[N:, H:2 * H]
        ctx = torch.empty(N, H, dtype=BF16, device=dev)
        lse = torch.empty(B, nh, S, dtype=F32, device=dev)
        sv.seed_att = run.next_seed() if run.p_att > 0 else 0
        # training: the forward leaves its un-normalised probabilities (bf16, 157 MB per execution at the bench shape; only the
        # tile pairs it visits are written) so that the backward does not recompute the scores (attn_bwd.hip, kernel A / dsp)
        psave = msave = None
        if run.save and self.attn_save_p:
            psave = torch.empty(B, nh, Sp, Sp, dtype=BF16, device=dev)
            msave = torch.empty(B, nh, Sp // 64, S, dtype=F32, device=dev)
        L.disent_attn_fwd(qkv[:N, :H], qkv[:N, H:2 * H], qkv[:N, 2 * H:], pk, pq, self.relidx(S), run.mask_i32,
                          ATTN_SCALE, ctx, lse, B, S, Sp, nh, self.span2, p_drop=run.p_att, seed=sv.seed_att, klen=run.klen,
                          border=run.border, lin=self.lin_span, row0=run.row0, psave=psave, msave=msave)
        sv.psave, sv.msave = psave, msave
        if run.want_attn and q is None:
            # output_attentions=True: the encoder layers' probabilities (model/deberta.py:544-560; the enhanced-mask-decoder
            # passes are called with return_att=False, :1395-1408), materialised by a plain kernel from the stored lse
            probs = torch.empty(B, nh, S, S, dtype=F32, device=dev)
            L.disent_attn_probs(qkv[:N, :H], qkv[:N, H:2 * H], pk, pq, self.relidx(S), run.mask_i32, lse,
                                ATTN_SCALE, probs, B, S, nh)
            run.attn_out.append(probs)
        if run.save:
            sv.qkv, sv.pqk, sv.ctx, sv.lse = qkv[:N], qkv[N:, : 2 * H], ctx, lse  # (run.save: never the inference shortcuts)
            if self.lora_r:  # the projections' bf16 inputs, kept for the LoRA weight-gradient products (N x H x 2 bytes each)
                sv.xkv, sv.xq = kv.bf16, (q.bf16 if q is not None else None)
        return self._layer_tail(run, li, sv, ctx, q if q is not None else kv, N, tail=self.span2)

    def _layer_tail(self, run, li: int, sv: "LayerSave", ctx, resid: Stream, N: int, tail=0) -> Stream:
        """Everything behind the attention of one layer execution, on N rows (the token rows, or the selected rows of the
        decoder): attention output and FFN.  Fills what `sv` keeps of them with their four dropout seeds and, under run.save,
        puts `sv` on run.layers (the caller has set what its attention keeps).  tail: see Stream.full."""
        W, (a1, a2) = self.Lw[li], self.sites[li]
        p = f"deberta.encoder.layer.{li}"
        # attention output: dense -> adapter -> dropout -> LN(. + residual)   (:254-260)
        a, ob, z1, sv.seed_ad1, sv.seed_ln1 = self._dense_adapter_ln(
            run, li, ctx, W["Wo"], W["bo"], a1, N, p + ".attention.output.LayerNorm", resid=resid)
        # FFN: gelu(dense) -> dense -> adapter -> dropout -> LN(. + a)          (:310-313, :328-334)
        h = torch.empty(N, self.I, dtype=BF16, device=self.dev)
        hpre = torch.empty(N, self.I, dtype=BF16, device=self.dev) if run.save else None
        # training: the epilogue stores gelu'(pre) (bf16) next to gelu(pre) so the backward epilogue is a plain multiply
        L.gemm(a.bf16, W["Wi"], bias=W["bi"], act=L.ACT_GELU_GRAD if run.save else L.ACT_GELU, out_bf16=h, out_pre=hpre)
        out, fb, z2, sv.seed_ad2, sv.seed_ln2 = self._dense_adapter_ln(
            run, li, h, W["Wd"], W["bd"], a2, N, p + ".output.LayerNorm", resid=Stream(bf16=a.bf16, norm=a.norm), tail=tail)
        if run.save:
            sv.ob, sv.z1, sv.ln1 = ob, z1, a.norm
            sv.hpre, sv.fb, sv.z2, sv.ln2 = hpre, fb, z2, out.norm
            run.layers.append(sv)
        return out

    @staticmethod
    def _stage_runs(run, stage: str) -> bool:
        """whether the backward of this step runs `stage` (a Run without a plan -- built by hand -- runs every stage)"""
        return run.plan is None or run.plan.runs(stage)

    def _skip_tail_seeds(self, run, li: int):
        """The seeds of a _layer_tail that is not executed (the decoder with no row selected), drawn in its order -- adapter and
        LayerNorm dropout of the attention output, then of the FFN output: the sites behind it keep their place in the mask stream."""
        a1, a2 = self.sites[li]
        for on in (a1 is not None and run.p_ad > 0, run.p_hid > 0, a2 is not None and run.p_ad > 0, run.p_hid > 0):
            if on:
                run.next_seed()

    def _forward(self, run, input_ids, video, use_ans, want_hidden):
        cfg, H, dev = self.cfg, self.H, self.dev
        B, S, T, Lt, Pn = run.B, run.S, run.T, run.Lt, run.P
        pk = run.pk
        N = run.N
        run.mask_i32 = run.mask  # [B*S]: the attention kernels index the mask on the padded grid
        run.rowmask = run.mask if pk is None else run.mask[pk.sel].contiguous()  # per activation row
        pos1 = torch.arange(1, S + 1, device=dev, dtype=torch.int32)
        run.klen = (run.mask.view(B, S) * pos1).amax(1).to(torch.int32).contiguous()  # last valid position + 1
        # attention work per sample grows with klen^2: the attention kernels dispatch the samples longest first
        run.border = torch.argsort(run.klen, descending=True, stable=True).to(torch.int32).contiguous()
        mask_f = run.rowmask.to(F32)
        run.mask_f = mask_f
        # ---- embeddings (model/deberta.py:997-1058): cat(linear_video(video), E[ids]) -> LN -> *mask -> dropout
        vproj = None
        if T:
            vb = torch.zeros(B * T, self.Fp, dtype=BF16, device=dev)
            vb[:, : self.F] = video.detach().reshape(B * T, self.F)  # (detached: its gradient comes from the step's own backward)
            vproj = torch.empty(B * T, H, dtype=F32, device=dev)
            L.gemm(vb, self.Wv, bias=self.P["deberta.embeddings.linear_video.bias"], out_f32=vproj)
            run.video_bf16 = vb
        t0 = torch.empty(B * S, H, dtype=F32, device=dev)
        if Pn:  # [video | prompt | text]: the prompt rows straight from the fp32 master (no packed copy, nothing to refresh)
            L.embed_assemble(input_ids if run.embeds is None else None, self.E32, vproj, self.P[PROMPT_NAME], T, Lt,
                             t0.view(B, S, H))
            if run.embeds is not None:
                t0.view(B, S, H)[:, T + Pn:].copy_(run.embeds.detach())
        elif run.embeds is None:
            L.embed_gather(input_ids, self.E32, vproj, T, t0)
        else:  # inputs_embeds in place of the gathered table rows (fp32, like them); the video slots in front as the gather puts them
            g0 = t0.view(B, S, H)
            if T:
                g0[:, :T].copy_(vproj.view(B, T, H))
            g0[:, T:].copy_(run.embeds.detach())
        if pk is not None:
            t0 = t0.index_select(0, pk.sel)
        want_plain = run.p_hid > 0
        emb, _ = self._ln(run, "deberta.embeddings.LayerNorm", y=t0, resid=None, N=N, rowmask=run.rowmask,
                          want_f32=want_plain, tail=self.span2)
        run.emb_norm = emb.norm
        if want_plain:  # post-LN dropout: materialise x0
            run.seed_emb = run.next_seed()
            L.dropout_f32(emb.plain, run.p_hid, run.seed_emb, out_f32=emb.plain, out_bf16=emb.bf16)
            emb = Stream(bf16=emb.bf16, plain=emb.plain, full=emb.full)
        # ---- relative-position table: R = LayerNorm_enc(rel_embeddings.weight)   (:474-478)
        r, _ = self._ln(run, "deberta.encoder.LayerNorm", y=self.rel_emb, resid=None, N=self.span2, want_f32=run.p_hid > 0)
        run.rel_norm, run.R32, Rb = r.norm, r.plain, r.bf16
        if self._lora_pos and run.save:  # (only a model with LoRA on query / key keeps it beyond the forward: a rank-0 model's
            run.Rb = Rb                  #  tensors live exactly as long as they always did)
        # ---- encoder (:507-575)
        hs: List[Stream] = [emb]
        x = emb
        nL = self.nL
        for i in range(nL):
            if i == nL - 1 and self.skip_dead_layer and not want_hidden:
                break  # its output feeds nothing; executed only when hidden_states are requested
            # An execution is saved for the backward only when its stage runs there (run.plan): below the lowest stage with a
            # live leaf nothing is kept -- no LayerSave, no attention probabilities (the forward variant of attn_save_p=False).
            # The forward itself -- numerics, dropout sites, seeds -- is the same either way.
            keep = run.save
            if i == nL - 1:
                # differentiable hidden states: hs[nL] may receive a gradient, so this execution is saved like any other -- a
                # third execution of the last layer's weights in the backward (LayerSave.extra); it draws the seeds it always
                # drew.  Otherwise its output feeds nothing that has a backward.
                run.save = keep and run.hid_grad and self._stage_runs(run, "decoder")
                x = self._layer_fwd(run, i, x, None, Rb)
                if run.save:
                    run.layers[-1].extra = True
            else:
                run.save = keep and self._stage_runs(run, f"layer{i}")
                x = self._layer_fwd(run, i, x, None, Rb)
            run.save = keep
            if i == 0 and cfg.conv_kernel_size:
                x = self._conv_fwd(run, emb, x)
                if not (run.save and self._stage_runs(run, "conv")):
                    run.conv_c = run.conv_norm = None
            if 1 <= i + 1 < self.prompt_depth:  # deep prompt tuning: layer i+1 has prompt rows of its own
                x = self._prompt_overwrite(run, i + 1, x)
            hs.append(x)
        if not (run.save and self._stage_runs(run, "emb")):
            run.emb_norm = run.video_bf16 = None
        # ---- enhanced mask decoder (:1382-1412): q0 = pos_emb + hs[-2]; two passes of the last layer
        kv = hs[nL - 1]
        if run.dec_grid is not None:  # model.decoder_rows: q0 and everything behind it on the selected rows only
            return self._decoder_rows_fwd(run, kv, Rb, use_ans)
        q32 = torch.empty(N, H, dtype=F32, device=dev)
        qfull = torch.empty(N + self.span2, H, dtype=BF16, device=dev)
        if pk is None:
            self._materialize(kv, add=self.pos_emb, S=S, out_f32=q32, out_bf16=qfull[:N])
        else:  # packed rows: the position of a row is not row % S (once per step: plain tensor ops, same fp32 arithmetic)
            n_ = kv.norm
            if n_ is not None:
                L.ln_materialize(n_.t, n_.stats, n_.gamma, n_.beta, rowmask=n_.rowmask, out_f32=q32)
            else:
                q32.copy_(kv.plain)
            q32.add_(self.pos_emb.index_select(0, pk.pos))
            qfull[:N].copy_(q32)
        q = Stream(bf16=qfull[:N], plain=q32, full=qfull)
        keep = run.save
        run.save = keep and self._stage_runs(run, "decoder")
        for _ in range(2):
            q = self._layer_fwd(run, nL - 1, kv, q, Rb)
        run.save = keep
        if want_hidden:
            if pk is None:
                run.hidden_out = tuple(self._materialize(s).view(B, S, H) for s in hs)
            else:  # (positions without a row read as zero)
                run.hidden_out = tuple(torch.zeros(B * S, H, dtype=F32, device=dev).index_copy_(0, pk.sel, self._materialize(s))
                                       .view(B, S, H) for s in hs)
        # ---- MLM head (:1544-1558): LN(gelu(dense(x))) . table^T + bias
        hin = q.bf16
        rows_only = run.logit_rows
        # an inference forward that is only asked for the loss (evaluate, main.py:139) runs the head's dense + GELU +
        # LayerNorm on the labelled rows only, like the vocabulary GEMM below; fill_logits redoes it on every row if the
        # logits are read after all
        loss_rows = (rows_only is None and run.labels is not None and not run.save and not self.eager_logits
                     and 0 < run.rows.numel() < N)
        if loss_rows:
            run.head_in_all = q.bf16
            rows_only = run.rows.to(torch.int32)
        if rows_only is not None:  # selected token rows only (the [MASK] rows of videoqa.py:66-69,164-168 / mc.py:166-170);
            N = rows_only.numel()    # what the head saves for its backward (head_pre, head_norm) is then row-compact too
            hin = torch.empty(N, H, dtype=BF16, device=dev)
            if N:
                L.gather_rows_bf16(q.bf16, rows_only, hin)
        hp, hl = self._head_stage(run, hin, N)
        run.head_pre, run.head_norm, run.head_ln_bf16 = hp, hl.norm, hl.bf16
        Vout, table, bias, ldv = self._head_tables(run, use_ans)
        if run.labels is not None:
            # A loss is asked for: it only needs the labelled rows.  Their logits come from a small GEMM so CE (and the
            # backward) can follow at once; the full [N, V] logits tensor -- an OUTPUT of the reference API that neither
            # main.py's train_one_epoch nor evaluate reads (main.py:67,139) -- is allocated but only FILLED on first
            # access (MaskedLMOutput -> fill_logits): 4.4 GB of writes and 3.4 TFLOP per step at the xlarge vocabulary.
            rows = run.rows
            run.rows_i32 = rows.to(torch.int32)
            R = rows.numel()
            lc = labels_c = None
            if R > 0:
                if loss_rows:
                    hrows = hl.bf16  # the head already ran on exactly these rows
                else:
                    hrows = torch.empty(R, H, dtype=BF16, device=dev)
                    L.gather_rows_bf16(hl.bf16, run.rows_i32, hrows)
                lc = torch.empty(R, ldv, dtype=F32, device=dev)
                L.gemm(hrows, table, bias=bias, out_f32=lc, N=Vout)
                lab_rows = run.label_rows  # (packed rows: `rows` are activation rows, the labels live on the grid)
                labels_c = run.labels[rows if lab_rows is None else lab_rows]
            loss_t = self._labelled_loss(run, lc, labels_c)
            if self.eager_logits:
                self.fill_logits(run)
            return run.logits, loss_t
        logits = torch.empty(N, ldv, dtype=F32, device=dev)
        L.gemm(hl.bf16, table, bias=bias, out_f32=logits, N=Vout)
        run.logits = logits
        return logits, None

    def _head_tables(self, run, use_ans):
        """The table behind the head of this pass -- the vocabulary, or the answer embeddings -- noted on `run` for fill_logits and
        the backward.  Returns (Vout, table, bias, ldv)."""
        if use_ans:
            Vout, table, bias = self.n_ans, self.Ansb, self.ans_bias
        else:
            Vout, table, bias = self.V, self.Eb, self.head_bias
        ldv = _ru(Vout, 64)
        run.Vout, run.head_table, run.head_bias, run.ldv = Vout, table, bias, ldv
        return Vout, table, bias, ldv

    def _labelled_loss(self, run, lc, labels):
        """The loss of a labelled call, the mean over its labelled rows (CrossEntropyLoss, :1483-1488), from their fp32 logits
        `lc` [R, ldv] and labels [R] (both None: no row is labelled); keeps what the backward reads of it.  Allocates the
        [B*S, ldv] logits that the call hands out, filled on first access (fill_logits)."""
        run.loss_acc = L.zeros(2, dtype=F32, device=self.dev)
        if lc is not None:
            run.labels_c = labels.contiguous()
            run.row_lse = torch.empty(lc.shape[0], dtype=F32, device=self.dev)
            L.ce_fwd(lc, run.labels_c, run.Vout, run.row_lse, run.loss_acc)
            run.logits_c = lc
        run.logits = torch.empty(run.B * run.S, run.ldv, dtype=F32, device=self.dev)
        run.logits_pending = True
        return run.loss_acc[0] / run.loss_acc[1]

    def _decoder_rows_fwd(self, run, kv: Stream, Rb, use_ans):
        """The enhanced mask decoder, the head and the loss on the selected rows only (model.decoder_rows).  A decoder row
        depends on its own query row and on all of hs[-2] (both passes take keys and values from it; everything behind the
        attention is row-wise), so this is exact.  K|V of hs[-2] are projected once for both passes; per pass the query
        projection runs on the R compact rows and [PQ|PK] on the position table (its own position-dropout seed), the attention
        is fbl_disent_attn_fwd_qrows, and dense / adapter / LayerNorm / FFN run at N = R.  Row-keyed dropout sites key by the
        compact row.  run.next_seed() is called in the order of _layer_fwd: position table, attention, then the sites of
        _layer_tail (or _skip_tail_seeds)."""
        from .row_plan import plan_query_rows

        H, nh, dev = self.H, self.nh, self.dev
        B, S, N = run.B, run.S, run.N
        li = self.nL - 1
        W = self.Lw[li]
        pk = run.pk
        pl = plan_query_rows(run.dec_grid, B, S, inv=pk.inv if pk is not None else None)
        run.dec_plan = pl
        R = pl.R
        Sp = _ru(S, 64)
        q = None
        if R:
            # q0 = pos_emb[pos] + hs[-2][rows], materialised for the R selected rows only
            n_ = kv.norm
            if n_ is not None:
                qc32 = torch.empty(R, H, dtype=F32, device=dev)
                rm = n_.rowmask.index_select(0, pl.krows) if n_.rowmask is not None else None
                L.ln_materialize(n_.t.index_select(0, pl.krows), n_.stats.index_select(0, pl.krows), n_.gamma, n_.beta, rowmask=rm,
                                 out_f32=qc32)
            else:
                qc32 = kv.plain.index_select(0, pl.krows)
            qc32.add_(self.pos_emb.index_select(0, pl.rpos.long()))
            q = Stream(bf16=qc32.to(BF16), plain=qc32)
            kvp = torch.empty(N, 2 * H, dtype=BF16, device=dev)
            L.gemm(kv.bf16, W["Wqkv"][H:], bias=W["bqkv"][H:], out_bf16=kvp)
        keep = run.save
        run.save = keep and self._stage_runs(run, "decoder")  # (below the lowest live stage: nothing of the passes is kept)
        for _ in range(2):
            sv = LayerSave(li=li, emd=True)
            if run.p_hid > 0:
                sv.seed_pos = run.next_seed()
            sv.seed_att = run.next_seed() if run.p_att > 0 else 0
            if not R:  # nothing selected: no decoder work; the seeds of the remaining sites are drawn as the full route draws them
                self._skip_tail_seeds(run, li)
                continue
            if run.p_hid > 0:
                Rd = torch.empty(self.span2, H, dtype=BF16, device=dev)
                L.dropout_f32(run.R32, run.p_hid, sv.seed_pos, out_bf16=Rd)
            else:
                Rd = Rb
            if self._pos_cache_allowed(run):
                pqk = self._pos_proj_cached(li, W, Rb)
            else:
                pqk = torch.empty(self.span2, 2 * H, dtype=BF16, device=dev)
                L.gemm(Rd, W["Wqkv"][: 2 * H], bias=W["bqkv"][: 2 * H], out_bf16=pqk)
            qp = torch.empty(R, H, dtype=BF16, device=dev)
            L.gemm(q.bf16, W["Wqkv"][:H], bias=W["bqkv"][:H], out_bf16=qp)
            ctx = torch.empty(R, H, dtype=BF16, device=dev)
            lse = torch.empty(nh, R, dtype=F32, device=dev)
            L.disent_attn_fwd_qrows(qp, pl.rseg, pl.rpos, kvp[:, :H], kvp[:, H:], pqk[:, H:], pqk[:, :H], self.relidx(S), run.mask_i32,
                                    run.klen, ATTN_SCALE, ctx, lse, B, S, Sp, nh, self.span2, p_drop=run.p_att, seed=sv.seed_att,
                                    row0=run.row0)
            if run.save:
                sv.qc, sv.kvp, sv.pqk, sv.ctx, sv.lse = qp, kvp, pqk, ctx, lse
            q = self._layer_tail(run, li, sv, ctx, q, R)
        run.save = keep
        # ---- head on the compact rows directly (no gather)
        Vout, table, bias, ldv = self._head_tables(run, use_ans)
        hin = q.bf16 if R else torch.empty(0, H, dtype=BF16, device=dev)
        hp, hl = self._head_stage(run, hin, R)
        run.head_pre, run.head_norm, run.head_ln_bf16 = hp, hl.norm, hl.bf16
        lc = torch.empty(R, ldv, dtype=F32, device=dev)
        if R:
            L.gemm(hl.bf16, table, bias=bias, out_f32=lc, N=Vout)
        if run.labels is None:  # logit_rows: [R, Vout] in the caller's order
            run.logits = lc.index_select(0, pl.back)
            return run.logits, None
        # labelled call: nonzero() lists the rows in ascending order, which is the compact order
        run.rows_i32 = run.rows.to(torch.int32)
        loss_t = self._labelled_loss(run, lc, run.labels[pl.grid]) if R else self._labelled_loss(run, None, None)
        return run.logits, loss_t  # (the logits: the selected rows, zero elsewhere)

    def fill_logits(self, run):
        """Full [N, V] logits of a forward that only computed the labelled rows (see _forward); idempotent.  Writes into
        the storage of the tensor already handed out (and already wired into the autograd node), on the current stream."""
        if run.logits_pending:
            run.logits_pending = False
            if run.dec_plan is not None:  # decoder on selected rows: only those rows have logits, the others read zero
                run.logits.zero_()
                if run.dec_plan.R:
                    run.logits.index_copy_(0, run.dec_plan.grid, run.logits_c)
                return
            hin_all = run.head_in_all
            if hin_all is not None:  # the forward ran the head on the labelled rows only: now on every row
                _, hl = self._head_stage(run, hin_all, hin_all.shape[0])
                run.head_ln_bf16, run.head_in_all = hl.bf16, None
            pk = run.pk
            if pk is None:
                L.gemm(run.head_ln_bf16, run.head_table, bias=run.head_bias, out_f32=run.logits, N=run.Vout)
            else:  # packed rows: grid positions without a row read as zero; the others arrive in slabs of 1024 rows
                run.logits.zero_()
                for r0 in range(0, pk.n, 1024):
                    r1 = min(pk.n, r0 + 1024)
                    slab = torch.empty(r1 - r0, run.logits.shape[1], dtype=F32, device=self.dev)
                    L.gemm(run.head_ln_bf16[r0:r1], run.head_table, bias=run.head_bias, out_f32=slab, N=run.Vout)
                    run.logits.index_copy_(0, pk.sel[r0:r1], slab)

    def _head_stage(self, run, hin, N):
        """prediction head in front of the vocabulary GEMM (model/deberta.py:1544-1552): LayerNorm(gelu(dense(x)))"""
        hp = torch.empty(N, self.H, dtype=F32, device=self.dev)
        L.gemm(hin, self.Wh, bias=self.bh, out_f32=hp)
        hg = torch.empty(N, self.H, dtype=F32, device=self.dev)
        L.dropout_gelu_fwd(hp, 0.0, 0, hg)
        hl, _ = self._ln(run, "lm_predictions.lm_head.LayerNorm", y=hg, resid=None, N=N)
        return hp, hl

    def _materialize(self, s: Stream, add=None, S=1, out_f32=None, out_bf16=None):
        N, H = s.bf16.shape
        if s.plain is not None and add is None and out_bf16 is None:
            return s.plain
        if out_f32 is None:
            out_f32 = torch.empty(N, H, dtype=F32, device=self.dev)
        if s.norm is not None:
            n = s.norm
            L.ln_materialize(n.t, n.stats, n.gamma, n.beta, rowmask=n.rowmask, add_bcast=add, S=S, out_f32=out_f32,
                             out_bf16=out_bf16)
        else:
            v = s.plain if add is None else (s.plain.view(-1, S, H) + add[:S]).view(N, H)
            out_f32.copy_(v)
            if out_bf16 is not None:
                out_bf16.copy_(v)
        return out_f32

    def _prompt_overwrite(self, run, i: int, x: Stream) -> Stream:
        """Deep prompt tuning: hs[i], the input of layer i (1 <= i < prompt_depth), with that layer's prompt rows in the prompt
        slots of every sample.  A normalised stream cannot express an overwritten row, so hs[i] becomes a materialised fp32
        stream with a bf16 operand copy of its own (norm=None, the form the embedding stream has behind its dropout): the rows
        are the parameter's fp32 bits -- no LayerNorm, mask or dropout -- and their one rounding to bf16.  What layer i-1 saved
        for its backward (its LayerNorm's pre-norm tensor and statistics) is not touched: that LayerNorm ran on the real values
        and receives zero gradient rows at the slots (_backward)."""
        N, H = run.N, self.H
        f32 = torch.empty(N, H, dtype=F32, device=self.dev)
        full = torch.empty(N + self.span2, H, dtype=BF16, device=self.dev)
        self._materialize(x, out_f32=f32, out_bf16=full[:N])
        L.prompt_rows_write(self.P[layer_prompt_name(i)], run.row0, run.B, run.S, run.T, out_f32=f32, out_bf16=full[:N])
        return Stream(bf16=full[:N], plain=f32, full=full)

    def _conv_fwd(self, run, emb: Stream, l0: Stream) -> Stream:
        """ConvLayer (:395-419): LN(l0 + gelu(drop(mask * conv1d_k3(emb)))) * mask, conv as a K=3H GEMM on an im2col."""
        B, S, H, dev = run.B, run.S, self.H, self.dev
        N = run.N
        pk = run.pk
        if pk is None:
            col = torch.empty(N, 3 * H, dtype=BF16, device=dev)
            L.im2col3(emb.bf16, col, B, S, H)
        else:  # packed rows: the neighbours of a position are found on the padded grid (masked embedding rows are zero there too)
            grid = torch.zeros(B * S, H, dtype=BF16, device=dev).index_copy_(0, pk.sel, emb.bf16)
            colg = torch.empty(B * S, 3 * H, dtype=BF16, device=dev)
            L.im2col3(grid, colg, B, S, H)
            col = colg.index_select(0, pk.sel)
        c = torch.empty(N, H, dtype=F32, device=dev)
        L.gemm(col, self.Wc, bias=self.bc, rowscale=run.mask_f, out_f32=c)
        y = torch.empty(N, H, dtype=F32, device=dev)
        run.seed_conv = run.next_seed() if run.p_hid > 0 else 0
        L.dropout_gelu_fwd(c, run.p_hid, run.seed_conv, y)
        out, _ = self._ln(run, "deberta.encoder.conv.LayerNorm", y=y, resid=l0, N=N, rowmask=run.rowmask, tail=self.span2)
        run.conv_c, run.conv_norm = c, out.norm
        return out

    # ------------------------------------------------------------------ backward
    def _ln_bwd(self, name, dout, norm: NormRef, p_drop, seed, want_dy_bf16=True, dysum=None, tail=0, dy_out=None, cb=None):
        """dysum: optional [H] accumulator for colsum(dy) = the bias gradient of whatever produced y (adapter up.bias).
        tail > 0: dt is the first N rows of a [N+tail, H] buffer whose tail is zeroed (aux operand of the dX GEMM that
        also produces the position-table gradient rows); the full buffer is returned as third value.
        cb: the compact backward (Run.cb) -- dout, dt and dy live on its rows, `norm` on the padded ones; the padded bf16 dy
        (zero where a row has no compact row: what the adapter weight gradients read) is returned as third value."""
        N, H = dout.shape
        if cb is not None:
            dt = torch.empty(N, H, dtype=F32, device=self.dev)
            dyb = dy_out if dy_out is not None else torch.empty(N, H, dtype=BF16, device=self.dev)
            dy_pad = torch.empty(norm.t.shape[0], H, dtype=BF16, device=self.dev)
            L.ln_bwd_rows(dout, cb.inv32, norm.t, norm.stats, norm.gamma, rowmask=norm.rowmask, p_drop=p_drop, seed=seed, out_dt=dt,
                          out_dy_bf16=dyb, out_dy_pad=dy_pad, dgamma=self.Gl.get(name + ".weight"), dbeta=self.Gl.get(name + ".bias"),
                          dysum=dysum, ws=self._ln_ws)
            return dt, dyb, dy_pad
        dt_full = torch.empty(N + tail, H, dtype=F32, device=self.dev)
        dt = dt_full[:N]
        if tail:
            dt_full[N:].zero_()
        dyb = dy_out if dy_out is not None else (torch.empty(N, H, dtype=BF16, device=self.dev) if want_dy_bf16 else None)
        L.ln_bwd(dout, norm.t, norm.stats, norm.gamma, rowmask=norm.rowmask, p_drop=p_drop, seed=seed, out_dt=dt,
                 out_dy_bf16=dyb, dgamma=self.Gl.get(name + ".weight"), dbeta=self.Gl.get(name + ".bias"), dysum=dysum,
                 ws=self._ln_ws)
        if tail:
            return dt, dyb, dt_full
        return dt, dyb

    def _adapter_bwd(self, run, site: AdapterSite, dyb, z, xin_b, seed, dz_out=None, pooled=None, pad=None):
        """Backward of _adapter_fwd.  dyb: grad of the adapter output (bf16 [N,H]); returns grad of its input (bf16).
        dz_out: the caller folds dx = dy + dz.Wd into the next GEMM ([dy | dz] operand, _layer_bwd): dz is written there
        (a column slice of that operand), no dx is formed and None is returned.
        pad = (dy, z) on the padded rows, compact backward only (dyb and z are then on its rows, xin_b padded as ever): the
        weight-gradient products keep the padded operands -- their reduction order over the rows is part of the result -- with
        dz put back on the padded rows, zeros where a row has no compact row."""
        N, H = dyb.shape
        A, Ap = site.A, site.Ap
        dev = self.dev
        upT, downT = self._adapter_bwd_operands(site)
        if dz_out is not None:
            dz = dz_out
        else:
            dz = torch.zeros(N, Ap, dtype=BF16, device=dev) if Ap != A else torch.empty(N, Ap, dtype=BF16, device=dev)
        inv_keep = 1.0 / (1.0 - run.p_ad) if run.p_ad > 0 else 1.0
        L.gemm(dyb, upT, alpha=inv_keep, aux=z, aux_kind=L.AUX_MUL_POS_BF16, out_bf16=dz, N=A)
        dx = None
        if dz_out is None:
            dx = torch.empty(N, H, dtype=BF16, device=dev)
            L.gemm(dz, downT, aux=dyb, aux_kind=L.AUX_ADD_BF16, out_bf16=dx)
        nm = site.name
        # the weight-gradient products of this adapter that feed a LIVE leaf (a dead one gets none: nothing is launched for it)
        gwu, gwd, gbd = (self.Gl.get(nm + k) for k in (".up.weight", ".down.weight", ".down.bias"))
        if gwu is None and gwd is None and gbd is None:
            return dx
        if pad is not None:
            dz_c, (dyb, z) = dz, pad
            dz = torch.empty(dyb.shape[0], dz_c.shape[1], dtype=BF16, device=dev)
            L.scatter_rows_zero_bf16(dz_c, run.cb.inv32, dz)
        sk = max(2, min(16, dyb.shape[0] // 512))

        if site.grouped:
            # dWu += dy^T z, dWd += dz^T x, dbd += colsum(dz) are NOT launched here: one adapter alone has 48 output tiles.
            # The operands are parked until `dw_group` adapters are pending and go through ONE launch
            # (fbl_adapter_bwd_dw: every tile walks all rows, no split-K round trip) on the MAIN stream -- its workgroups live
            # for the whole pass, and a resident side-stream workgroup keeps the one-per-CU tiles of the big GEMMs off its CU.
            # (up.bias's gradient colsum(dy) comes out of ln_bwd.)
            run.dw_pending.append((A, nm, (dyb, z, dz, xin_b), run.dw_count, pooled))
            run.dw_count += 1
            return dx

        # Bottlenecks wider than 256: the generic route, launched right away on the side stream (nothing downstream in
        # backward reads the weight gradients) with its own workspaces
        self.side.wait_stream(torch.cuda.current_stream())  # inputs (dyb, z, dz, xin_b) are ready once main reaches this point
        with torch.cuda.stream(self.side):
            if gwu is not None:
                L.gemm_tn_acc(dyb, z, gwu, self.side_ws, N=A, splitk=sk)      # dWu[H,A] += dy^T z
            if gwd is not None:
                L.gemm_tn_acc(dz, xin_b, gwd, self.side_ws, M=A, splitk=sk)  # dWd[A,H] += dz^T x
            if gbd is not None:
                L.colsum(dz, gbd, self.side_cs_ws, cols=A)
        if not torch.cuda.is_current_stream_capturing():
            for t in (dyb, z, dz, xin_b):
                t.record_stream(self.side)  # keep the allocator from recycling them before the side stream is done
        else:  # (inside a capture: referenced for the life of the captured step instead)
            run._pos_keep.extend((dyb, z, dz, xin_b))
        run.side_used = True
        if self.reducer is not None:  # what a data-parallel bucket has to wait for: the dW work queued so far
            run.dw_event = torch.cuda.Event()
            run.dw_event.record(self.side)
        return dx

    def _dw_flush(self, run, red=None, force=False):
        """Launch the parked adapter-gradient products (see _adapter_bwd) once `dw_group` distinct adapters are pending -- one
        launch of 2 x H/64 workgroups per adapter; 16 adapters = 768 workgroups = three per CU, all resident -- or all of
        them (force), and only then tell the gradient reducer about the stages whose buckets they complete.  An adapter
        appears once per launch: the second execution of the last layer (enhanced mask decoder) waits for the next one,
        so that no launch has a double-length tile."""
        pend = run.dw_pending
        while pend and (force or len({rec[1] for rec in pend}) >= self.dw_group):
            take, names, rest = {}, set(), []
            for rec in pend:
                A, nm, seg = rec[:3]
                if nm in names or len(names) >= min(self.dw_group, L.ADW_MAX_ADAPTERS):
                    rest.append(rec)
                else:
                    names.add(nm)
                    take.setdefault((A, getattr(seg[0], "shape", (None,))[0]), []).append((nm, seg))  # one launch takes one row count
            for (A, _rows), recs in take.items():
                Gl = getattr(self, "Gl", None)  # the gradient views of the live leaves (before a live set exists: all of them)
                Gl = self.G if Gl is None else Gl
                L.adapter_bwd_dw([([seg], *Engine._dw_outputs(self, nm, Gl)) for nm, seg in recs], A=A)  # (a dead member: no output)
            kept = {id(r) for r in rest}
            for rec in pend:  # [dy | dz | 0] operands whose last reader has now been enqueued go back to the pool (same stream)
                if id(rec) not in kept and rec[4] is not None and tuple(rec[4].shape) == self._dyz_shape:
                    self._dyz_pool.setdefault(self._dyz_shape, []).append(rec[4])  # (buffers of an earlier batch shape are dropped)
            pend[:] = rest
        if red is not None:  # a finished stage is final once none of ITS adapters has a parked product left (any order: the
            # repeated last layer waits one launch longer than the layers behind it, and must not hold their buckets back)
            parked = {self._bucket_key(rec[1] + ".up.weight") for rec in pend}
            still = []
            for key in run.dw_ready_keys:
                if key in parked:
                    still.append(key)
                elif not (getattr(run, "lora_pos_wait", False) and key.startswith("layer")):
                    red.ready(key)  # (LoRA on query / key: the position chain at the end of backward still adds to the layers'
                    #                  buckets; they leave with finish())
            run.dw_ready_keys[:] = still

    def _layer_bwd(self, run, sv: "LayerSave", dout: torch.Tensor):
        """Backward of one layer execution.  dout: fp32 grad of its output.  Returns (dx, None) for ordinary encoder layers (one
        input stream) and (dq_in fp32, [dK | dV] bf16 operand of the key/value-stream gradient) for the decoder form."""
        li = sv.li
        W, (a1, a2) = self.Lw[li], self.sites[li]
        H, I, dev = self.H, self.I, self.dev
        N = dout.shape[0]
        p = f"deberta.encoder.layer.{li}"
        cb = run.cb
        if cb is not None:
            return self._layer_bwd_compact(run, sv, dout, cb)
        dt2, dy2 = self._ln_bwd(p + ".output.LayerNorm", dout, sv.ln2, run.p_hid, sv.seed_ln2,
                                dysum=self.Gl.get(a2.name + ".up.bias") if a2 is not None else None)
        df = dy2
        if a2 is not None:
            df = self._adapter_bwd(run, a2, dy2, sv.z2, sv.fb, sv.seed_ad2)
        dh = torch.empty(N, I, dtype=BF16, device=dev)
        L.gemm(df, W["WdT"], aux=sv.hpre, aux_kind=L.AUX_MUL_BF16, out_bf16=dh)  # sv.hpre holds gelu'(pre)
        da = torch.empty(N, H, dtype=F32, device=dev)
        L.gemm(dh, W["WiT"], aux=dt2, aux_kind=L.AUX_ADD_F32, out_f32=da)
        del dh
        dctx = torch.empty(N, H, dtype=BF16, device=dev)
        if a1 is not None and a1.merged:
            # dctx = dx . Wo with dx = dy + dz . Wd  ==  [dy | dz] . [Wo^T | (Wd.Wo)^T]^T: LayerNorm backward and the dz GEMM
            # write the two column blocks of ONE operand and the dense dX GEMM runs with K = H + A (+ zero padding) -- the
            # K = A GEMM that formed dx, its 26 MB output and its re-read are gone (25 us per layer execution)
            A1, Kf = a1.A, a1.WF.shape[1]
            # The K padding columns only have to hold finite values (their weight columns are zero): buffers come from a small
            # pool whose padding was zeroed ONCE -- nobody writes those columns -- instead of a strided fill per layer execution
            # (25 launches a step).  A buffer returns to the pool when the parked gradient products that read its [dy | dz]
            # blocks have been enqueued (_dw_flush).  Captured steps and the immediate-launch route allocate as before.
            pooled = None
            can_pool = not torch.cuda.is_current_stream_capturing() and a1.grouped and sv.kvp is None  # (one pooled shape: N rows)
            if can_pool and self._dyz_shape != (N, Kf):  # a new batch shape (text padded to the longest sample): one pool, of
                self._dyz_pool.clear()                           # the current shape only -- never one per shape seen
                self._dyz_shape = (N, Kf)
            free = self._dyz_pool.get((N, Kf)) if can_pool else None
            if free:
                dyz = pooled = free.pop()
            elif can_pool:
                dyz = pooled = torch.zeros(N, Kf, dtype=BF16, device=dev)
            else:
                dyz = torch.empty(N, Kf, dtype=BF16, device=dev)
                if Kf > H + A1:
                    dyz[:, H + A1:].zero_()  # finite values under the zero weight columns
            dt1, dy1 = self._ln_bwd(p + ".attention.output.LayerNorm", da, sv.ln1, run.p_hid, sv.seed_ln1,
                                    dysum=self.Gl.get(a1.name + ".up.bias"), dy_out=dyz[:, :H])
            self._adapter_bwd(run, a1, dy1, sv.z1, sv.ob, sv.seed_ad1, dz_out=dyz[:, H:H + A1], pooled=pooled)
            L.gemm(dyz, a1.WF, out_bf16=dctx)
            if pooled is not None and not any((a1.name + k) in self.Gl for k in (".up.weight", ".down.weight", ".down.bias")):
                # nothing was parked for a dead adapter: this GEMM was the last reader, the buffer returns to the pool at once
                self._dyz_pool.setdefault(self._dyz_shape, []).append(pooled)
        else:
            dt1, dy1 = self._ln_bwd(p + ".attention.output.LayerNorm", da, sv.ln1, run.p_hid, sv.seed_ln1,
                                    dysum=self.Gl.get(a1.name + ".up.bias") if a1 is not None else None)
            do = dy1
            if a1 is not None:
                do = self._adapter_bwd(run, a1, dy1, sv.z1, sv.ob, sv.seed_ad1)
            L.gemm(do, W["WoT"], out_bf16=dctx)
        if self.reducer is not None:  # ~0.15 ms (0.35 until round 6) without one-workgroup-per-CU GEMM tiles: where gradient collectives may start
            self.reducer.window()
        if not sv.emd:
            dqkv = self._attn_bwd(run, sv, dctx)
            for t in range(3 if self.lora_r else 0):
                self._lora_bwd(run, li, t, dqkv[:, t * H:(t + 1) * H], sv.xkv)
            dx = torch.empty(N, H, dtype=F32, device=dev)
            L.gemm(dqkv, W["WqkvT"], aux=dt1, aux_kind=L.AUX_ADD_F32, out_f32=dx)
            return dx, None
        # Enhanced mask decoder (model/deberta.py:1382-1412): the query stream and the key/value stream differ.  Returns the
        # gradient of the query stream and, in place of the key/value-stream gradient, the bf16 [dK | dV] operand it is the
        # product of -- the caller chains both passes' products into ONE accumulator through the GEMM epilogues
        # (dx = dq_first + dkv_second + dkv_first: no stand-alone additions of [N, H] fp32 tensors).
        if sv.kvp is not None:  # decoder on selected rows: dQ is compact, [dK | dV] covers every key row
            dq_op, dkv_op = self._attn_bwd_qrows(run, sv, dctx)
        else:
            dqkv = self._attn_bwd(run, sv, dctx)
            dq_op, dkv_op = dqkv[:, :H], dqkv[:, H:]
            for t in range(3 if self.lora_r else 0):  # the query projection reads the query stream, key / value read hs[-2]
                self._lora_bwd(run, li, t, dqkv[:, t * H:(t + 1) * H], sv.xq if t == 0 else sv.xkv)
        dq = torch.empty(N, H, dtype=F32, device=dev)
        L.gemm(dq_op, W["WqkvT"][:, :H], aux=dt1, aux_kind=L.AUX_ADD_F32, out_f32=dq)
        return dq, dkv_op

    def _layer_bwd_compact(self, run, sv: "LayerSave", dout: torch.Tensor, cb: Packing):
        """_layer_bwd on the compact rows of `cb` (dout [Np, H]; same return values, on compact rows).  Every GEMM and the attention
        backward are row-independent: they run the same code on fewer rows and give each row the bits the padded pass gives it.
        What reduces over rows keeps the padded order: the column sums of the LayerNorm backward (fbl_ln_bwd_rows walks the
        padded rows and skips the ones without a compact row) and the adapter weight gradients (padded operands, _adapter_bwd).
        One fused gather brings what the compact kernels read from the padded forward onto their rows."""
        li = sv.li
        W, (a1, a2) = self.Lw[li], self.sites[li]
        H, I, dev = self.H, self.I, self.dev
        Np = dout.shape[0]
        p = f"deberta.encoder.layer.{li}"
        pairs = [(t, torch.empty(Np, t.shape[1], dtype=t.dtype, device=dev))
                 for t in (sv.qkv, sv.ctx, sv.hpre, sv.z1 if a1 is not None else None, sv.z2 if a2 is not None else None) if t is not None]
        L.gather_rows_multi(pairs, cb.sel32)
        got = {id(src): dst for src, dst in pairs}
        qkv, ctx, hpre = got[id(sv.qkv)], got[id(sv.ctx)], got[id(sv.hpre)]
        dt2, dy2, dy2p = self._ln_bwd(p + ".output.LayerNorm", dout, sv.ln2, run.p_hid, sv.seed_ln2,
                                      dysum=self.Gl.get(a2.name + ".up.bias") if a2 is not None else None, cb=cb)
        df = dy2
        if a2 is not None:
            df = self._adapter_bwd(run, a2, dy2, got[id(sv.z2)], sv.fb, sv.seed_ad2, pad=(dy2p, sv.z2))
        del dy2p
        dh = torch.empty(Np, I, dtype=BF16, device=dev)
        L.gemm(df, W["WdT"], aux=hpre, aux_kind=L.AUX_MUL_BF16, out_bf16=dh)
        da = torch.empty(Np, H, dtype=F32, device=dev)
        L.gemm(dh, W["WiT"], aux=dt2, aux_kind=L.AUX_ADD_F32, out_f32=da)
        del dh, hpre
        dctx = torch.empty(Np, H, dtype=BF16, device=dev)
        if a1 is not None and a1.merged:  # the folded [dy | dz] operand (_layer_bwd), on compact rows
            A1, Kf = a1.A, a1.WF.shape[1]
            # its zeroed padding columns: ONE buffer per row count (the dense GEMM below is its last reader: the weight
            # gradients read the padded copies), not a strided fill per layer execution
            dyz = self._dyz_compact
            if dyz is None or tuple(dyz.shape) != (Np, Kf):
                dyz = self._dyz_compact = torch.zeros(Np, Kf, dtype=BF16, device=dev)
            dt1, dy1, dy1p = self._ln_bwd(p + ".attention.output.LayerNorm", da, sv.ln1, run.p_hid, sv.seed_ln1,
                                          dysum=self.Gl.get(a1.name + ".up.bias"), dy_out=dyz[:, :H], cb=cb)
            self._adapter_bwd(run, a1, dy1, got[id(sv.z1)], sv.ob, sv.seed_ad1, dz_out=dyz[:, H:H + A1], pad=(dy1p, sv.z1))
            L.gemm(dyz, a1.WF, out_bf16=dctx)
        else:
            dt1, dy1, dy1p = self._ln_bwd(p + ".attention.output.LayerNorm", da, sv.ln1, run.p_hid, sv.seed_ln1,
                                          dysum=self.Gl.get(a1.name + ".up.bias") if a1 is not None else None, cb=cb)
            do = dy1
            if a1 is not None:
                do = self._adapter_bwd(run, a1, dy1, got[id(sv.z1)], sv.ob, sv.seed_ad1, pad=(dy1p, sv.z1))
            L.gemm(do, W["WoT"], out_bf16=dctx)
        del dy1p
        svc = dataclasses.replace(sv, qkv=qkv, ctx=ctx)  # the attention backward reads q / k / v / O on compact rows (row0)
        dqkv = self._attn_bwd(run, svc, dctx)
        sv.psave = sv.msave = None
        if not sv.emd:
            dx = torch.empty(Np, H, dtype=F32, device=dev)
            L.gemm(dqkv, W["WqkvT"], aux=dt1, aux_kind=L.AUX_ADD_F32, out_f32=dx)
            return dx, None
        dq = torch.empty(Np, H, dtype=F32, device=dev)
        L.gemm(dqkv[:, :H], W["WqkvT"][:, :H], aux=dt1, aux_kind=L.AUX_ADD_F32, out_f32=dq)
        return dq, dqkv[:, H:]

    def _attn_bwd(self, run, sv, dctx):
        """Backward of the attention of one layer execution on the token rows: the bf16 [dQ | dK | dV] operand [N, 3H]."""
        dqkv = torch.empty(dctx.shape[0], 3 * self.H, dtype=BF16, device=self.dev)
        # The position-table gradients of this execution (dPK = G1^T.Q, dPQ = G2^T.K) are NOT formed here: its dS / dS^T and
        # q / k go on the per-step lists, and one chain at the END of backward handles all executions
        # (attn_bwd.pos_table_grads_batched).  ft_ln=False: nothing trainable sits behind the position tables, nothing is kept.
        st = disent_attn_bwd(self, run, sv, dctx, dqkv, None, defer_pos=True)
        if run.pos_chain is not None and sv.extra:
            run.pos_extra = (st, sv.seed_pos)  # joins the chain as its LAST execution, where WposT_exec has its weights
        elif run.pos_chain is not None:
            run.pos_chain.add(st, sv.seed_pos)
        return dqkv

    def _attn_bwd_qrows(self, run, sv, dctx):
        """Backward of the attention of one decoder execution on selected rows (fbl_disent_attn_bwd_qrows): returns dQ bf16
        [R, H] and [dK | dV] bf16 [N, 2H]; its position-table gradients go straight onto the step's chain."""
        B, S, H, nh, dev = run.B, run.S, self.H, self.nh, self.dev
        pl = run.dec_plan
        R, Sp = pl.R, _ru(S, 64)
        rmin, rcnt = _relidx_range(S, self.cfg)
        dqc = torch.empty(R, H, dtype=BF16, device=dev)
        dkv = torch.empty(run.N, 2 * H, dtype=BF16, device=dev)
        # the table gradients are written straight into the chain's buffer of all executions; without a chain (nothing trainable
        # behind the position table) the table pass is not launched
        dpk, dpq = run.pos_chain.formed_slot() if run.pos_chain is not None else (None, None)
        ws = torch.empty(L.disent_attn_bwd_qrows_ws_bytes(R, Sp, nh), dtype=torch.uint8, device=dev)
        kvp, pqk = sv.kvp, sv.pqk
        L.disent_attn_bwd_qrows(sv.qc, pl.rseg, pl.rpos, kvp[:, :H], kvp[:, H:], pqk[:, H:], pqk[:, :H], self.relidx(S), run.mask_i32,
                                run.klen, dctx, sv.ctx, sv.lse, ATTN_SCALE, dqc, dkv[:, :H], dkv[:, H:], dpk, dpq,
                                rmin, rcnt, ws, B, S, Sp, nh, self.span2, p_drop=run.p_att, seed=sv.seed_att, row0=run.row0)
        if run.pos_chain is not None:
            run.pos_chain.add_formed(sv.seed_pos)
        return dqc, dkv

    def _dlog_operand(self, g):
        """A gradient handed in on logits, g [rows, Vout], as the bf16 [rows, Vp] operand of _head_bwd (padding columns zero)."""
        rows, Vout = g.shape
        Vp = _ru(Vout, 64)
        dlog = torch.zeros(rows, Vp, dtype=BF16, device=self.dev) if Vp != Vout else torch.empty(rows, Vp, dtype=BF16, device=self.dev)
        dlog[:, :Vout].copy_(g)
        return dlog

    def _head_bwd(self, run, rows, dlog, dq, all_rows=False, compact=False, to_rows=None):
        """Backward of the prediction head for the rows `rows` (int32 indices into the N token rows) given their bf16
        logit gradients dlog [R, Vp]: dq[rows] += d/d(head input).  Head LayerNorm gradients are accumulated.
        compact: the forward ran the head on exactly these rows (logit_rows), so what it saved is already [R, .].
        to_rows: the rows of dq that receive the result when dq has another row layout than the forward (compact backward)."""
        H, dev = self.H, self.dev
        R, Vp = dlog.shape
        Vout = run.Vout
        if Vout == self.V:
            tableT = self.ETb
        else:
            tableT = torch.zeros(H, Vp, dtype=BF16, device=dev)
            tableT[:, :Vout] = self.Ansb.t()
        dhl = L.zeros(R, H, dtype=F32, device=dev)
        if R >= 2048:  # enough rows to fill the chip without splitting K
            L.gemm(dlog, tableT, out_f32=dhl)
        else:  # few rows, long K -> split-K so the grid covers the chip (accumulates into zeros)
            L.gemm(dlog, tableT, out_f32=dhl, splitk=max(2, min(16, Vp // 8192)), ws=self.sk_ws)
        hn = run.head_norm
        if compact:
            sub, pre = hn, run.head_pre
        else:
            rl = rows.long()
            sub, pre = NormRef(hn.t[rl].contiguous(), hn.stats[rl].contiguous(), hn.gamma, hn.beta), run.head_pre[rl].contiguous()
        dt, _ = self._ln_bwd("lm_predictions.lm_head.LayerNorm", dhl, sub, 0.0, 0, want_dy_bf16=False)
        dpre = torch.empty(R, H, dtype=BF16, device=dev)
        L.dropout_gelu_bwd(dt, pre, 0.0, 0, out_bf16=dpre)
        dqr = torch.empty(R, H, dtype=F32, device=dev)
        L.gemm(dpre, self.WhT, out_f32=dqr)
        if all_rows:
            dq.add_(dqr)
        else:
            L.scatter_rows_f32(dqr, rows if to_rows is None else to_rows, dq)  # first contribution: dq is still zero at these rows

    def backward(self, run, gloss: Optional[torch.Tensor], glogits: Optional[torch.Tensor] = None, attach: bool = True,
                 ghid=None):
        """Explicit backward of _forward; accumulates into the flat gradient buffer (p.grad views).  gloss: gradient
        of the internal MLM loss (or None); glogits: gradient w.r.t. the returned logits [B,S,Vout] (or None); ghid: gradients
        w.r.t. the returned hidden states, [B,S,H] or None each (run.hid_grad).  Returns the gradients of the inputs named in
        run.grad_in as a dict ("video": [B,T,F], "embeds": [B,L,H], in the inputs' dtypes).
        attach=False: the caller has already made p.grad the views of the flat buffer (a captured backward must not contain
        the conditional zero fill of attach_grads)."""
        if not run.save:
            raise RuntimeError("forward was run without gradient bookkeeping")
        with L.seed_word(run.seed_word):
            return self._backward(run, gloss, glogits, attach, ghid)

    def _hid_grad(self, run, ghid, i):
        """the gradient handed in on hidden_states[i] as fp32 activation rows [N, H], or None"""
        g = ghid[i] if ghid is not None and i < len(ghid) else None
        if g is None:
            return None
        g = g.reshape(run.B * run.S, self.H).to(F32)
        return g.index_select(0, run.pk.sel) if run.pk is not None else g.contiguous()

    def _backward(self, run, gloss, glogits, attach, ghid=None):
        cfg, H, dev = self.cfg, self.H, self.dev
        B, S, T = run.B, run.S, run.T
        N = run.N
        pk = run.pk
        if run.plan is not None and run.live_version != self.live_version:
            raise RuntimeError("requires_grad of a trainable parameter changed between this step's forward and its backward: "
                               "the forward saved what the live set of ITS time needs; change the flags between steps")
        if attach:
            self.attach_grads()
        reducer = self.reducer
        runs = lambda stage: self._stage_runs(run, stage)  # (run.plan: stages below the lowest live leaf have no backward)
        if ghid is not None and all(g is None for g in ghid):
            ghid = None
        if run.logit_rows is not None and run.logit_rows.numel() == 0 and reducer is None and ghid is None:
            return  # no row was asked for: every gradient is exactly zero, nothing is launched (a reducer still needs its buckets)

        red = _Ready(self, run, reducer) if reducer is not None else None
        run.dw_pending, run.dw_ready_keys, run.dw_count = [], [], 0
        dec = run.dec_plan  # decoder on selected rows: the head and the decoder work on the R compact rows
        # The compact backward (_backward_rows made its layout with the forward): from here down to layer 0 on the rows that exist.
        # Only the loss's own gradient keeps the padding rows at exactly zero: one handed in on the logits or on a hidden state
        # reaches them, and such a backward stays on the padded grid.
        cb = run.cb = run.bwd_rows if (glogits is None and ghid is None and gloss is not None and dec is None and pk is None) else None
        run.bwd_compact = cb is not None
        dq = L.zeros(dec.R if dec is not None else (cb.n if cb is not None else N), H, dtype=F32, device=dev)
        Vout = run.Vout
        Vp = _ru(Vout, 64)
        # ---- CE + head, on the labelled rows only (all other rows have exactly zero gradient)
        if gloss is not None and run.labels is not None:
            rows = run.rows_i32
            R = rows.numel()
            if R > 0:
                dlog = torch.empty(R, Vp, dtype=BF16, device=dev)
                # the incoming loss gradient stays on the device (read by the kernel): no host sync at backward start
                gs = gloss.detach().to(F32) if (isinstance(gloss, torch.Tensor) and gloss.is_cuda) else float(gloss)
                ar = torch.arange(R, dtype=torch.int32, device=dev)  # logits_c holds the labelled rows only
                L.ce_bwd_rows(run.logits_c, run.labels_c, ar, Vout, Vp, run.row_lse, run.loss_acc, gs, dlog)
                if dec is not None:
                    self._head_bwd(run, None, dlog, dq, all_rows=True, compact=True)
                else:
                    self._head_bwd(run, rows, dlog, dq, to_rows=cb.inv32[rows.long()] if cb is not None else None)
                del dlog
        # ---- gradient handed in on the logits of the requested rows (logit_rows): the head backward on those R rows only,
        # scatter-added into the zeroed dq at their activation rows (distinct: check_logit_rows)
        if glogits is not None and run.logit_rows is not None:
            rows = run.logit_rows
            R = rows.numel()
            if R > 0:
                gl = glogits.reshape(R, Vout)
                if dec is not None:  # the caller's order -> the compact order
                    self._head_bwd(run, None, self._dlog_operand(gl.index_select(0, dec.order)), dq, all_rows=True, compact=True)
                else:
                    self._head_bwd(run, rows, self._dlog_operand(gl), dq, compact=True)
        # ---- gradient handed in on the logits themselves (downstream losses): every token row
        elif glogits is not None and dec is not None:
            # decoder on selected rows: out.logits holds the selected rows and constants (zero) elsewhere, so only the gradient
            # handed in at those rows has anything to flow into -- taken at the grid rows in compact order
            if dec.R:
                gl = glogits.reshape(B * S, Vout).index_select(0, dec.grid)
                self._head_bwd(run, None, self._dlog_operand(gl), dq, all_rows=True, compact=True)
        elif glogits is not None:
            gl = glogits.reshape(B * S, Vout)
            if pk is not None:  # (gradients handed in at positions without a row have nothing to flow into)
                gl = gl.index_select(0, pk.sel)
            self._head_bwd(run, torch.arange(N, dtype=torch.int32, device=dev), self._dlog_operand(gl), dq, all_rows=True)

        def stage_done(key):  # a stage's gradients are final once the adapter products parked in it have been launched
            run.dw_ready_keys.append(key)
            self._dw_flush(run, red)

        D = self.prompt_depth

        def prompt_rows(i, dx):
            """deep prompt tuning: dx becomes the complete gradient of hs[i] (1 <= i < D) -- what the caller handed in on
            hidden_states[i] joins here, not one stage further down -- its prompt slots' rows, summed over the batch in ascending
            b, are the gradient of layer i's prompt (nothing is summed for a frozen one), and are then cleared: everything
            upstream of the overwrite receives exactly zero from them (fbl_prompt_rows_grad)"""
            g = self._hid_grad(run, ghid, i)
            if g is not None:
                dx.add_(g)
            L.prompt_rows_grad(dx, run.row0, B, S, T, run.P, self.Gl.get(layer_prompt_name(i)))

        def to_grid(x):
            """compact backward: fp32 rows back onto the padded grid (zeros where a row has no compact row) -- what follows runs
            there: the convolution's taps cross row boundaries, the embedding stage ends on the grid"""
            run.cb = None
            return L.zeros(N, H, dtype=F32, device=dev).index_copy_(0, cb.sel, x)

        def end(dx_emb=None):
            """the tail every backward ends with, wherever its lowest stage is: the parked products, the side stream, the
            position-table chain (all of its executions have run whenever its LayerNorm is live), the embedding stage when it
            runs, and the gradient exchange -- finish() releases the buckets of the stages that did not run"""
            run.cb = None
            self._dw_flush(run, red, force=True)
            if run.side_used:
                torch.cuda.current_stream().wait_stream(self.side)  # all adapter dW/db are in the flat grad buffer
            return self._backward_bottom(run, red, ghid, dx_emb)

        stage_done("head")
        run.pos_chain = None
        if not runs("decoder"):
            return end()
        # the position-table gradients feed only encoder.LayerNorm: dead, the whole chain (fbl_attn_pos_grad, the strided-batch
        # projection behind it) is not launched and the attention backward keeps nothing for it
        run.lora_pos_wait = self._lora_pos and any(t < 2 and self._lora_live(s) for (_, t), s in self.lora_sites.items())
        if any(REL_LN + k in self.Gl for k in ("weight", "bias")) or run.lora_pos_wait:
            run.pos_chain = pos_chain_buffers(self, run)
            if dec is not None:  # the two decoder executions are the first of the chain also when nothing was selected (R = 0:
                # they were not saved; zero tables keep the chain's order equal to the order of WposT_exec)
                run.pos_chain.n_exec = len(run.layers) + (0 if dec.R else 2)
                if not dec.R:
                    for _ in range(2):
                        dpk, dpq = run.pos_chain.formed_slot()
                        dpk.zero_(); dpq.zero_()
                        run.pos_chain.add_formed(0)
        # ---- EMD: two executions of the last layer, newest first
        layers = run.layers
        dkv_ops = []
        for _ in range(2 if dec is None or dec.R else 0):
            sv = layers.pop()
            dq, dkv_op = self._layer_bwd(run, sv, dq)
            dkv_ops.append(dkv_op)
        if dec is not None:  # the query-stream gradient of the first pass lands on its rows of hs[-2] (distinct under gradients)
            dqc, dq = dq, L.zeros(N, H, dtype=F32, device=dev)
            if dec.R:
                L.scatter_rows_f32(dqc, dec.krows.to(torch.int32), dq)
        # q0 = pos_emb + hs[-2]: the query-stream gradient flows into hs[-2] too, next to both passes' key/value-stream
        # gradients [dK | dV] . [Wk ; Wv] -- accumulated by the epilogues of those two GEMMs
        # (the decoder is the lowest stage that runs: nothing below asks for the gradient of hs[-2], it is not formed)
        below = run.plan is None or run.plan.lowest < run.plan.stages.index("decoder")
        # (deep prompt tuning down to the last layer: its prompt's gradient is the slots' rows of the gradient of hs[-2])
        top_prompt = D == self.nL and D > 1
        dx = None
        if below or (top_prompt and layer_prompt_name(self.nL - 1) in self.Gl):
            WkvT = self.Lw[self.nL - 1]["WqkvT"][:, H:]
            dx = dq
            for op in dkv_ops:
                acc = torch.empty(dx.shape[0], H, dtype=F32, device=dev)
                L.gemm(op, WkvT, aux=dx, aux_kind=L.AUX_ADD_F32, out_f32=acc)
                dx = acc
        del dkv_ops
        # ---- the last layer's own encoder execution (differentiable hidden states only): hs[nL] = layer(hs[nL-1]); a gradient
        # handed in on hs[nL] flows through it into hs[nL-1] and, as a third execution, into the last layer's parameters
        if layers and layers[-1].extra:
            sv = layers.pop()
            g = self._hid_grad(run, ghid, self.nL)
            if g is not None:
                dxe, _ = self._layer_bwd(run, sv, g)
                if dx is not None:
                    dx.add_(dxe)
                del dxe
            del sv
        if top_prompt and dx is not None:
            prompt_rows(self.nL - 1, dx)
        stage_done(f"layer{self.nL - 1}")
        if not below:
            return end()
        # ---- encoder layers nL-2 .. 0
        while layers:
            sv = layers.pop()
            # handed in on this layer's output (behind the convolution for layer 0); a boundary with prompt rows took it already
            g = self._hid_grad(run, ghid, sv.li + 1) if not 1 <= sv.li + 1 < D else None
            if g is not None:
                dx.add_(g)
            if sv.li == 0 and cfg.conv_kernel_size and cb is not None:
                # compact backward: the convolution stage on the padded grid (its dropout is keyed by the padded element, its taps
                # reach the neighbouring rows), layer 0 on the compact rows in between
                dx, dcol = self._conv_bwd(run, to_grid(dx))
                run.cb = cb
                dx, _ = self._layer_bwd(run, sv, dx.index_select(0, cb.sel))
                dx = to_grid(dx)
                L.col2im3(dcol, dx, B, S, H, 1)
                stage_done("conv")
            elif sv.li == 0 and cfg.conv_kernel_size:
                dx, dcol = self._conv_bwd(run, dx)
                dx, _ = self._layer_bwd(run, sv, dx)
                if pk is None:
                    L.col2im3(dcol, dx, B, S, H, 1)
                else:  # packed rows: fold the three taps on the padded grid, add the rows that exist
                    dcg = torch.zeros(B * S, 3 * H, dtype=F32, device=dev).index_copy_(0, pk.sel, dcol)
                    dxg = torch.zeros(B * S, H, dtype=F32, device=dev)
                    L.col2im3(dcg, dxg, B, S, H, 1)
                    dx.add_(dxg.index_select(0, pk.sel))
                    del dcg, dxg
                stage_done("conv")
            else:
                dx, _ = self._layer_bwd(run, sv, dx)
            if 1 <= sv.li < D:
                prompt_rows(sv.li, dx)
            stage_done(f"layer{sv.li}")
        if cfg.conv_kernel_size and runs("conv") and not runs("layer0"):
            # the conv stage is the lowest that runs (layer 0 was not saved): only its LayerNorm's gamma / beta are wanted
            g = self._hid_grad(run, ghid, 1) if D < 2 else None  # (D >= 2: joined at layer 1's prompt rows)
            if g is not None:
                dx.add_(g)
            cn = run.conv_norm
            L.ln_bwd(dx, cn.t, cn.stats, cn.gamma, rowmask=cn.rowmask, dgamma=self.Gl.get("deberta.encoder.conv.LayerNorm.weight"),
                     dbeta=self.Gl.get("deberta.encoder.conv.LayerNorm.bias"), ws=self._ln_ws)
            stage_done("conv")
        if run.cb is not None:  # (no convolution: the compact rows end here)
            dx = to_grid(dx)
        return end(dx if runs("emb") else None)

    def _backward_bottom(self, run, red, ghid, dx):
        """The end of every backward: encoder.LayerNorm from the position-table chain (if it is live), the embedding stage
        (dx: the gradient of the embedding output, or None when that stage does not run), the end of the gradient exchange.
        Returns the gradients of the inputs named in run.grad_in."""
        H, dev = self.H, self.dev
        B, S, T, N, pk = run.B, run.S, run.T, run.N, run.pk
        # ---- relative-position LayerNorm (receives grads from every layer execution)
        rn = run.rel_norm
        if run.pos_chain is not None and run.pos_extra is not None:
            run.pos_chain.add(*run.pos_extra)
        run.pos_extra = None
        if run.pos_chain is not None:
            dR = pos_table_grads_batched(self, run, run.pos_chain)
            run.pos_chain = None
            if any(REL_LN + k in self.Gl for k in ("weight", "bias")):  # (the chain also runs for LoRA on query / key alone)
                L.ln_bwd(dR, rn.t, rn.stats, rn.gamma, dgamma=self.Gl.get("deberta.encoder.LayerNorm.weight"),
                         dbeta=self.Gl.get("deberta.encoder.LayerNorm.bias"), ws=self._ln_ws)
        if red:
            red.ready("relln")
        if dx is None:  # nothing live in the embedding stage and no input takes a gradient: the backward ends here
            if red:
                red.finish()  # (the buckets of the stages that did not run leave now, as zeros)
            return {}
        # ---- embeddings: dropout -> *mask -> LN ; linear_video
        g = self._hid_grad(run, ghid, 0)  # hidden_states[0]: the embedding output, behind its dropout
        if g is not None:
            dx.add_(g)
        if run.p_hid > 0:
            L.dropout_f32(dx, run.p_hid, run.seed_emb, out_f32=dx)
        en = run.emb_norm
        dt0 = torch.empty(N, H, dtype=F32, device=dev)
        L.ln_bwd(dx, en.t, en.stats, en.gamma, rowmask=en.rowmask, out_dt=dt0,
                 dgamma=self.Gl.get("deberta.embeddings.LayerNorm.weight"), dbeta=self.Gl.get("deberta.embeddings.LayerNorm.bias"),
                 ws=self._ln_ws)
        gvw, gvb = (self.Gl.get("deberta.embeddings.linear_video." + k) for k in ("weight", "bias"))
        if T and (gvw is not None or gvb is not None or "video" in run.grad_in):
            if pk is None:
                dv = dt0.view(B, S, H)[:, :T].reshape(B * T, H).contiguous()
            else:  # the video slots are the first T rows of every sample
                dv = dt0.index_select(0, (pk.row0[:-1].long()[:, None] + torch.arange(T, device=dev)[None]).reshape(-1))
            if gvw is not None:  # (dead: its weight-gradient product is not formed)
                Kp = _ru(B * T, 64)
                dvT = torch.empty(H, Kp, dtype=BF16, device=dev)
                vT = torch.empty(self.Fp, Kp, dtype=BF16, device=dev)
                L.transpose_to_bf16(dv, dvT)
                L.transpose_to_bf16(run.video_bf16, vT)
                L.gemm(dvT, vT, aux=gvw, aux_kind=L.AUX_ADD_F32, out_f32=gvw, N=self.F)
            if gvb is not None:
                L.colsum(dv, gvb, self._cs_ws)
        gp = self.Gl.get(PROMPT_NAME)
        if gp is not None:  # prompt tuning, the prompt live: its gradient = the prompt slots' rows of dt0 summed over the batch in
            # ascending b (fbl_prompt_grad: ordered fp32 adds onto what the buffer holds, reproducible bit for bit)
            L.prompt_grad(dt0, None if pk is None else pk.row0, B, S, T, gp)
        if red:
            red.ready("emb")
            red.finish()
        # ---- inputs that take a gradient of their own (run.grad_in): dt0 is the gradient of the embedding rows in front of the
        # LayerNorm -- the video slots' rows through linear_video, the text rows as they are.  Rows whose mask is 0 are exactly
        # zero in dt0 (the LayerNorm backward multiplies by the row mask, model/deberta.py:1045-1052), hence in both gradients.
        gin = {}
        if "video" in run.grad_in and T:
            # dvideo = dt0[video rows] . W_video: bf16 operands, fp32 accumulation, against the K-contiguous (transposed) copy of
            # linear_video.weight, which only a step with this gradient builds
            wname = "deberta.embeddings.linear_video.weight"
            WvT = torch.empty(self.F, H, dtype=BF16, device=dev)
            L.transpose_to_bf16(self.Pb[wname], WvT)
            dvb = torch.empty(B * T, H, dtype=BF16, device=dev)
            L.cast_bf16(dv, dvb)
            dvid = torch.empty(B * T, self.Fp, dtype=F32, device=dev)
            L.gemm(dvb, WvT, out_f32=dvid, N=self.F)
            gin["video"] = dvid[:, : self.F].reshape(B, T, self.F).to(run.video_dtype)
        if "embeds" in run.grad_in:
            if pk is None:
                grid = dt0
            else:  # positions without a row: exactly zero
                grid = L.zeros(B * S, H, dtype=F32, device=dev).index_copy_(0, pk.sel, dt0)
            gin["embeds"] = grid.view(B, S, H)[:, T + run.P:].to(run.embeds.dtype).contiguous()
        return gin

    def _conv_bwd(self, run, dout):
        """Backward of _conv_fwd: returns (grad of the layer-0 output, grad of the im2col matrix)."""
        B, S, H, dev = run.B, run.S, self.H, self.dev
        N = run.N
        cn = run.conv_norm
        dt = torch.empty(N, H, dtype=F32, device=dev)
        L.ln_bwd(dout, cn.t, cn.stats, cn.gamma, rowmask=cn.rowmask, out_dt=dt,
                 dgamma=self.Gl.get("deberta.encoder.conv.LayerNorm.weight"),
                 dbeta=self.Gl.get("deberta.encoder.conv.LayerNorm.bias"), ws=self._ln_ws)
        dc = torch.empty(N, H, dtype=BF16, device=dev)
        L.dropout_gelu_bwd(dt, run.conv_c, run.p_hid, run.seed_conv, out_bf16=dc)
        dcol = torch.empty(N, 3 * H, dtype=F32, device=dev)
        L.gemm(dc, self.WcT, rowscale=run.mask_f, out_f32=dcol)
        return dt, dcol


class _Ready:
    """Reducer front end used by Engine.backward: a bucket may only leave once the side-stream dW kernels that fill it
    have finished.  (Module level on purpose: a class created per call is only reclaimed by the cyclic GC, and its
    closure would keep the whole `run` -- gigabytes of saved activations -- alive until then.)"""

    __slots__ = ("eng", "run", "reducer")

    def __init__(self, eng, run, reducer):
        self.eng, self.run, self.reducer = eng, run, reducer

    def ready(self, key):
        if self.run.dw_event is not None:
            torch.cuda.current_stream().wait_event(self.run.dw_event)
        self.reducer.ready(key)

    def finish(self):
        self.reducer.finish()


@dataclass
class LayerSave:
    li: int = 0
    emd: bool = False
    extra: bool = False  # the last encoder layer's own execution (its output is hs[nL] only), saved for differentiable hidden states
    qkv: torch.Tensor = None
    pqk: torch.Tensor = None
    ctx: torch.Tensor = None
    lse: torch.Tensor = None
    ob: torch.Tensor = None
    z1: torch.Tensor = None
    ln1: NormRef = None
    hpre: torch.Tensor = None
    fb: torch.Tensor = None
    z2: torch.Tensor = None
    ln2: NormRef = None
    seed_pos: int = 0
    seed_att: int = 0
    seed_ad1: int = 0
    seed_ad2: int = 0
    seed_ln1: int = 0
    seed_ln2: int = 0
    psave: torch.Tensor = None
    msave: torch.Tensor = None
    # decoder on selected rows (_decoder_rows_fwd) in place of qkv; pqk, ctx and lse above are then those of its R compact rows
    # LoRA (engine.lora_r > 0): the bf16 inputs of the projections -- the key/value stream (the layer input) and, in the decoder
    # passes, the query stream
    xkv: Optional[torch.Tensor] = None
    xq: Optional[torch.Tensor] = None
    qc: Optional[torch.Tensor] = None   # bf16 [R, H]: the projected query of the selected rows
    kvp: Optional[torch.Tensor] = None  # bf16 [N, 2H]: K|V of hs[-2], shared by both passes; set = a decoder-rows execution


@dataclass
class Run:
    """The state of one step (one forward and its backward), of either engine: everything a stage leaves for a later one."""
    B: int
    S: int
    T: int
    Lt: int
    train: bool
    save: bool
    seed_base: int
    p_hid: float
    p_att: float
    p_ad: float
    # ---- inputs (Engine.run / BertEngine.run / train_graph)
    mask: torch.Tensor = None                      # int32 [B*S]: video mask | attention mask
    labels: torch.Tensor = None                    # int64 [B*S] on the padded grid (-100: no label), or None
    rows: torch.Tensor = None                      # int64: the labelled activation rows
    label_rows: Optional[torch.Tensor] = None      # packed rows only: the same rows on the padded grid (where `labels` live)
    logit_rows: Optional[torch.Tensor] = None      # int32: the head (and, with gradients, its backward) on these activation rows only
    want_attn: bool = False                        # output_attentions=True
    seed_word: Optional[torch.Tensor] = None       # device word added to every dropout seed of this pass (see Engine.run)
    pk: Optional["Packing"] = None                 # packed-row layout of this pass (model.packed_rows) or None: the padded [B, S] grid
    bwd_rows: Optional["Packing"] = None           # the compact layout the BACKWARD may use next to a padded forward (Engine._backward_rows)
    cb: Optional["Packing"] = None                 # ... set while the backward is on it (_backward: from the head down to layer 0)
    bwd_compact: bool = False                      # ... whether this step's backward ran on it (set by _backward; tests, tools)
    N: int = 0                                     # activation rows: B*S, or pk.n
    embeds: Optional[torch.Tensor] = None          # inputs_embeds [B, L, H] given in place of input_ids
    P: int = 0                                     # prompt slots between the video slots and the text (S = T + P + Lt)
    grad_in: tuple = ()                            # inputs that take a gradient of their own, as _StepFn lists them: "video", "embeds"
    hid_grad: bool = False                         # the hidden states handed out are differentiable (outputs of the step's node)
    video_dtype: Optional[torch.dtype] = None      # the caller's dtype of `video` (its gradient is returned in it)
    _site: int = 0                                 # dropout sites drawn so far (next_seed)
    # ---- forward, before the layers
    mask_i32: torch.Tensor = None                  # [B*S]: the mask as the attention kernels index it (padded grid)
    rowmask: torch.Tensor = None                   # int32 [N]: the mask per activation row
    mask_f: torch.Tensor = None                    # fp32 [N]: rowmask as a GEMM row scale
    klen: torch.Tensor = None                      # int32 [B]: last valid position + 1
    border: torch.Tensor = None                    # int32 [B]: samples longest first (dispatch order of the attention kernels)
    video_bf16: torch.Tensor = None                # bf16 [B*T, Fp]: operand of linear_video, kept for its weight gradient
    emb_norm: NormRef = None                       # embedding LayerNorm
    seed_emb: int = 0                              # dropout behind it
    rel_norm: NormRef = None                       # encoder.LayerNorm over the relative-position table
    R32: Optional[torch.Tensor] = None             # fp32 [2*span, H]: that table, materialised for its dropout (training)
    Rb: Optional[torch.Tensor] = None              # bf16 [2*span, H]: the table as a GEMM operand, before any dropout
    # ---- layers
    layers: list = field(default_factory=list)     # LayerSave / BertLayerSave per execution that has a backward
    dec_grid: Optional[torch.Tensor] = None        # model.decoder_rows: the selected rows on the padded grid, caller's order
    dec_plan: Optional[object] = None              # ... their row_plan.QueryRowPlan
    emd_qkv: Optional[torch.Tensor] = None         # inference: Q|K|V of the first decoder pass, reused by the second
    attn_out: list = field(default_factory=list)   # want_attn: fp32 [B, nh, S, S] probabilities per encoder layer
    hidden_out: tuple = None                       # want_hidden: fp32 [B, S, H] per layer
    seed_conv: int = 0                             # ConvLayer: dropout seed, conv output c, LayerNorm
    conv_c: torch.Tensor = None
    conv_norm: NormRef = None
    # ---- head
    head_in_all: Optional[torch.Tensor] = None     # bf16 [N, H] head input when the forward ran the head on the labelled rows only
    head_pre: torch.Tensor = None                  # fp32: dense output in front of the GELU
    head_norm: NormRef = None                      # head LayerNorm
    head_ln_bf16: torch.Tensor = None              # ... its bf16 output: operand of the vocabulary GEMM
    head_table: torch.Tensor = None                # bf16 [Vout, H], fp32 [Vout]: vocabulary (or answer) table and bias
    head_bias: torch.Tensor = None
    Vout: int = 0                                  # logit columns; ldv: their padded leading dimension
    ldv: int = 0
    use_ans: bool = False                          # BertEngine: the answer table is the head's table
    rows_i32: torch.Tensor = None                  # `rows` as int32
    labels_c: torch.Tensor = None                  # int64 [R]: labels of the labelled rows
    logits_c: torch.Tensor = None                  # fp32 [R, ldv]: their logits, row_lse [R]: their log-sum-exp
    row_lse: torch.Tensor = None
    loss_acc: torch.Tensor = None                  # fp32 [2]: (sum of row losses, labelled rows)
    logits: torch.Tensor = None                    # fp32 [B*S or rows, ldv]: the tensor handed out
    logits_pending: bool = False                   # ... not filled yet (fill_logits does it on first access)
    # ---- backward
    dw_pending: list = field(default_factory=list)     # parked adapter-gradient products (_adapter_bwd / _dw_flush)
    dw_ready_keys: list = field(default_factory=list)  # finished stages whose buckets wait for a parked product
    dw_count: int = 0                              # products parked so far
    side_used: bool = False                        # the side stream holds weight-gradient work of this pass
    dw_event: Optional[torch.cuda.Event] = None    # ... recorded behind the latest of it (data-parallel buckets wait for it)
    _pos_keep: list = field(default_factory=list)  # captured steps: tensors the side stream reads, referenced for the step's life
    pos_chain: Optional["PosChain"] = None         # attn_bwd.PosChain: what the position-table gradients collect per execution
    pos_extra: Optional[tuple] = None              # ... of the LayerSave.extra execution, which joins the chain last
    lora_pos_wait: bool = False                    # LoRA on query / key is live: the chain adds to the layers' gradients at the end
    # ---- partial fine-tuning
    plan: Optional[object] = None                  # live_set.StagePlan: the stages whose backward runs (None: all of them)
    live_version: int = 0                          # the engine's live set this step was planned for
    low_layer: int = -1                            # BertEngine: the lowest layer whose backward runs (-1: the embeddings too)

    def __post_init__(self):
        if not self.N:
            self.N = self.B * self.S

    @property
    def row0(self) -> Optional[torch.Tensor]:
        """int32 [B+1] first activation row of every sample as the attention kernels take it: packed rows only, else None"""
        return self.pk.row0 if self.pk is not None else None

    def next_seed(self) -> int:
        self._site += 1
        # seed_base: the step's position in the mask stream (eager) or 0 (captured: the device word carries it; Run.seed_word)
        return (self.seed_base + self._site * 0x85EBCA77) & 0xFFFFFFFFFFFFFFFF


class _StepFn(torch.autograd.Function):
    """Single autograd node for the whole model: forward already ran; backward runs Engine.backward which writes the
    gradients straight into the flat grad buffer (p.grad views), so autograd itself accumulates nothing.  logits_t is the
    [B, S, Vout] grid or, for a `logit_rows` call, the [R, Vout] rows; glogits arrives in the same shape.  `rest` is the
    n_hid hidden states of an output_hidden_states=True call (outputs of the node too: a gradient handed in on one of them joins
    the backward where it crosses that boundary), then the inputs that take a gradient of their own (run.grad_in: video,
    inputs_embeds), then the trainable parameters.  Gradients are not materialised: an output nobody used arrives as None."""

    @staticmethod
    def forward(ctx, engine, run, loss_t, logits_t, n_hid, *rest):
        ctx.engine, ctx.run, ctx.n_hid = engine, run, n_hid
        ctx.set_materialize_grads(False)
        return (loss_t.detach().clone(), logits_t.detach()) + tuple(h.detach() for h in rest[:n_hid])

    @staticmethod
    def backward(ctx, gloss, glogits, *ghid):
        eng, run = ctx.engine, ctx.run
        gin = {}
        ghid = ghid if any(g is not None for g in ghid) else None
        if gloss is not None or glogits is not None or ghid is not None:
            gin = eng.backward(run, gloss, glogits, ghid=ghid) or {}
        return (None,) * (5 + ctx.n_hid) + tuple(gin.get(k) for k in run.grad_in) + tuple(None for _ in eng.order)
