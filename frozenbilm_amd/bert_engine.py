"""Explicit forward / backward pipeline of the BERT variant (``--model_name=bert-*``, reference model/bert.py) on MI355X.

Same contract as ``engine.py``: a fixed sequence of C-ABI kernel launches on the current HIP stream, torch only owns HBM
allocations, one autograd node for the whole model.  The stages (reference lines per stage):

  embeddings   cat(linear_video(video), E[ids]) + position rows 0..S-1 + token-type-0 row, LayerNorm, dropout  (:242-278)
  layer        QKV (one GEMM against [Wq;Wk;Wv]) -> fbl_mha_fwd (additive key mask, every query row computed)  (:138-191)
               -> Wo -> LN(x + dropout(.))  (:288-292) -> GELU(Wi .) -> Wd -> LN(a + dropout(.))  (:203-206, :356-360)
  head         LN(gelu(dense(x))) . E^T + cls bias, or the answer table t.A^T + answer_bias  (:67-95)

Only linear_video and the LayerNorms under ``bert.`` train (freeze rule :547-553), so the backward forms dX through the
transposed frozen weights (packed once) and accumulates dgamma / dbeta and the linear_video gradient into the flat buffer.

Packed rows (opt-in ``model.packed_rows``, as on the DeBERTa engine): a call with labels or ``logit_rows`` outside a stream
capture drops the trailing rows of every sample that nothing reads (``bert_packing``).  The embedding gather goes through
the padded grid once; every GEMM and LayerNorm after it sees ``N = pk.n`` rows, the attention becomes fbl_mha_fwd_rows /
fbl_mha_bwd_rows (``row0``; mask and lse stay on the grid), and the head maps its rows through ``pk.inv``.  Attention dropout
draws the padded call's decisions; the row-wise sites are keyed by the packed element index (another, equally distributed
mask stream).

Data parallelism: the flat gradient buffer is preceded by ``parallel.SCALAR_SLOT`` floats and cut into one bucket per
encoder layer plus one for the embeddings, in backward-completion order; ``backward`` tells an attached
``parallel.GradReducer`` when a bucket is final (``ready``), where collectives may start (``window``: in front of each
layer's attention backward) and when the step ends (``finish``).

No adapters and no launch graphs on this path.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional

import torch

from . import lib as L
from .engine import BF16, F32, Engine, NormRef, Packing, Run, Stream, _ru, _StepFn, check_logit_rows
from .live_set import LiveSetMixin
from .predict import check_topk, of_call as predictions_of_call


@dataclass
class BertLayerSave:
    qkv: torch.Tensor       # bf16 [N, 3H]
    ctx: torch.Tensor       # bf16 [N, H]
    lse: torch.Tensor       # fp32 [B, nh, S]
    gp: torch.Tensor        # bf16 [N, I]: gelu'(pre-activation) of the intermediate layer
    ln1: NormRef
    ln2: NormRef
    seed_att: int
    seed_ln1: int
    seed_ln2: int


def flat_order(nL: int, names: List[str]) -> List[str]:
    """trainable names in backward-completion order: layer nL-1 .. 0, then the embeddings"""
    out: List[str] = []
    for i in reversed(range(nL)):
        out += [n for n in names if n.startswith(f"bert.encoder.layer.{i}.")]
    out += [n for n in names if n not in set(out)]
    return out


def bert_packing(mask, labels, logit_rows, B: int, S: int, T: int) -> Optional[Packing]:
    """Packed-row layout of a BERT batch, or None when no row can be dropped.  mask: [B*S] (video mask | attention mask), labels:
    int64 [B*S] on the grid (-100: none) or None, logit_rows: flat grid rows or None; any device (one host read of B integers).
    plen[b] = max(last position with a valid token, a label or a requested logit row + 1, T, 1) -- and S for a sample whose
    mask has no valid key: the additive mask makes such a sample attend to all S keys (Engine._make_packing may drop those
    rows because XSoftmax zeroes them; BERT's mask does not)."""
    dev = mask.device
    valid = mask.reshape(B, S) != 0
    keep = valid
    if labels is not None:
        keep = keep | (labels.reshape(B, S) != -100)
    if logit_rows is not None:
        want = torch.zeros(B * S, dtype=torch.bool, device=dev)
        want[logit_rows.to(dev).long().reshape(-1)] = True
        keep = keep | want.view(B, S)
    pos1 = torch.arange(1, S + 1, device=dev, dtype=torch.int32)
    last = (keep.to(torch.int32) * pos1).amax(1)
    last = torch.where(valid.any(1), last, torch.full_like(last, S))
    plen_h = [max(int(v), T, 1) for v in last.tolist()]
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


def _hid_rows(run, ghid, i):
    """the gradient handed in on hidden_states[i] as fp32 activation rows [N, H] (packed rows: gathered), or None"""
    g = ghid[i] if ghid is not None and i < len(ghid) else None
    if g is None:
        return None
    g = g.reshape(run.B * run.S, g.shape[-1]).to(F32)
    return g.index_select(0, run.pk.sel) if run.pk is not None else g.contiguous()


class BertEngine(LiveSetMixin):
    # LayerNorm forward / backward and materialisation work on the same representation as the DeBERTa engine's
    _ln = Engine._ln
    _ln_bwd = Engine._ln_bwd
    _materialize = Engine._materialize
    attach_grads = Engine.attach_grads

    def __init__(self, model):
        self.m = model
        cfg = model.config
        self.cfg = cfg
        self.H, self.I, self.V = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size
        self.nh, self.nL = cfg.num_attention_heads, cfg.num_hidden_layers
        if self.H != 64 * self.nh or self.H % 64 or self.I % 64:
            raise NotImplementedError(f"the fused attention takes head_dim 64 (hidden {self.H}, {self.nh} heads) and the GEMMs "
                                      "need hidden / intermediate sizes that are multiples of 64")
        self.F = model.features_dim
        self.Fp = _ru(self.F, 64) if self.F else 0
        self.Vp = _ru(self.V, 64)
        dev = model.device
        if dev.type != "cuda":
            raise RuntimeError("frozenbilm_amd runs on MI355X only: move the model to a cuda (HIP) device; "
                               "there is no CPU fallback")
        L.load()
        self.dev = dev
        self.scale = 1.0 / math.sqrt(cfg.hidden_size // cfg.num_attention_heads)
        self.reducer = None
        self.params_version = 0  # bumped by FusedAdam.step
        self._ln_ws = L.ln_bwd_ws(self.H, dev)
        self._cs_ws = L.colsum_ws(self.H, dev)
        self.sk_ws = torch.empty(16 << 20, dtype=F32, device=dev)  # split-K partials (head backward, linear_video dW)
        self._pos: Dict[tuple, torch.Tensor] = {}
        self._build_flat()
        self._pack_frozen()

    # ------------------------------------------------------------------ parameters
    def _build_flat(self):
        m = self.m
        named = dict(m.named_parameters())
        # the trainable-BY-CONSTRUCTION set (the constructor flags), whatever requires_grad says now: see Engine._build_flat
        order = flat_order(self.nL, m.trainable_names())
        offs, total = {}, 0
        for n in order:
            offs[n] = total
            total += _ru(named[n].numel(), 8)
        self.flat = torch.zeros(max(total, 8), dtype=F32, device=self.dev)
        # in front of the gradients: the floats that travel with the first data-parallel bucket (the step's logged loss)
        from .parallel import SCALAR_SLOT

        self.flat_grad_full = torch.zeros(SCALAR_SLOT + max(total, 8), dtype=F32, device=self.dev)
        self.flat_grad = self.flat_grad_full[SCALAR_SLOT:]
        self.offsets, self.order, self.named = offs, order, named
        self.G: Dict[str, torch.Tensor] = {}
        for n in order:
            p = named[n]
            o, k = offs[n], p.numel()
            view = self.flat[o:o + k].view(p.shape)
            view.copy_(p.data)
            p.data = view
            self.G[n] = self.flat_grad[o:o + k].view(p.shape)
        self.P = {n: p.data for n, p in named.items()}
        # one data-parallel bucket per backward stage: the encoder layers nL-1 .. 0, then the embeddings
        self.bucket_ends: Dict[str, int] = {}
        for n in order:
            self.bucket_ends[self._bucket_key(n)] = offs[n] + _ru(named[n].numel(), 8)
        self._init_live()

    def lowest_layer(self, grad_in=()) -> int:
        """The lowest encoder layer whose backward a step with the current live set runs: -1 when the embedding stage runs too
        (linear_video or the embedding LayerNorm is live, or `video` takes a gradient), nL when no layer does."""
        if grad_in:
            return -1
        low = self.nL
        for n in self.live_order:
            low = min(low, int(n.split(".")[3]) if n.startswith("bert.encoder.layer.") else -1)
        return low

    @staticmethod
    def _bucket_key(name: str) -> str:
        if name.startswith("bert.encoder.layer."):
            return "layer" + name.split(".")[3]
        return "emb"

    def _pack_frozen(self):
        P, H = self.P, self.H
        bf = lambda t: t.to(BF16).contiguous()
        self.Lw = []
        for i in range(self.nL):
            p = f"bert.encoder.layer.{i}."
            s = p + "attention.self."
            Wqkv = torch.cat([P[s + "query.weight"], P[s + "key.weight"], P[s + "value.weight"]], 0)
            self.Lw.append(dict(
                Wqkv=bf(Wqkv), WqkvT=bf(Wqkv.t()),
                bqkv=torch.cat([P[s + "query.bias"], P[s + "key.bias"], P[s + "value.bias"]]).float().contiguous(),
                Wo=bf(P[p + "attention.output.dense.weight"]), WoT=bf(P[p + "attention.output.dense.weight"].t()),
                bo=P[p + "attention.output.dense.bias"].float().contiguous(),
                Wi=bf(P[p + "intermediate.dense.weight"]), WiT=bf(P[p + "intermediate.dense.weight"].t()),
                bi=P[p + "intermediate.dense.bias"].float().contiguous(),
                Wd=bf(P[p + "output.dense.weight"]), WdT=bf(P[p + "output.dense.weight"].t()),
                bd=P[p + "output.dense.bias"].float().contiguous(),
            ))
        c = "cls.predictions."
        self.Wh, self.WhT = bf(P[c + "transform.dense.weight"]), bf(P[c + "transform.dense.weight"].t())
        self.bh = P[c + "transform.dense.bias"].float().contiguous()
        E = P["bert.embeddings.word_embeddings.weight"]
        self.E32, self.Eb = E.float().contiguous(), bf(E)
        self.ETb = torch.zeros(H, self.Vp, dtype=BF16, device=self.dev)
        self.ETb[:, : self.V] = E.t().to(BF16)
        self.head_bias = P[c + "bias"].float().contiguous()
        e = "bert.embeddings."
        # position rows + the token-type-0 row: the plain residual of the embedding LayerNorm (frozen)
        self.pos_type = (P[e + "position_embeddings.weight"].float() + P[e + "token_type_embeddings.weight"][0].float()).contiguous()
        if self.m.n_ans:
            T = P["answer_embeddings.weight"]
            self.n_ans = T.shape[0]
            self.Ansb = bf(T)
            self.AnsTb = torch.zeros(H, _ru(self.n_ans, 64), dtype=BF16, device=self.dev)
            self.AnsTb[:, : self.n_ans] = T.t().to(BF16)
            self.ans_bias = P["answer_bias"].float().contiguous()

    def invalidate_operands(self):
        self.params_version += 1

    def _video_weight(self):
        """bf16 [H, Fp] operand of linear_video (trainable: cast every forward)"""
        w = torch.zeros(self.H, self.Fp, dtype=BF16, device=self.dev)
        w[:, : self.F] = self.P["bert.embeddings.linear_video.weight"]
        return w

    def _pos_rows(self, B, S):
        key = (B, S)
        if key not in self._pos:
            self._pos.clear()
            self._pos[key] = self.pos_type[:S].repeat(B, 1).contiguous()
        return self._pos[key]

    # ------------------------------------------------------------------ forward
    def run(self, input_ids, attention_mask, video, video_mask, labels, mlm, want_hidden, logit_rows=None):
        m = self.m
        train = m.training
        k_pred = check_topk(getattr(m, "predict_topk", 0))  # opt-in `model.predict_topk`, read per call (as Engine.run does)
        if input_ids.device != self.dev:
            raise RuntimeError(f"inputs must be on {self.dev}")
        if attention_mask is None:
            attention_mask = torch.ones_like(input_ids)
        B, Lt = input_ids.shape
        use_video = bool(self.F) and video is not None
        # a `video` that takes a gradient of its own becomes a tensor input of the step's autograd node (as Engine.run does it)
        grad_in = [("video", video)] if (torch.is_grad_enabled() and use_video and video.requires_grad) else []
        # the live set (as Engine.run reads it); nothing live and no input with a gradient: no bookkeeping, dropout stays live
        need_grad = torch.is_grad_enabled() and (self.update_live() or bool(grad_in))
        T = video.shape[1] if use_video else 0
        S = T + Lt
        if S > self.cfg.max_position_embeddings:
            raise RuntimeError(
                f"sequence of {S} positions (video {T} + text {Lt}) exceeds max_position_embeddings="
                f"{self.cfg.max_position_embeddings} (the reference fails the same way, model/bert.py:258-262)")
        if use_video:
            if video_mask is None:
                video_mask = torch.ones(video.shape[:2], device=self.dev, dtype=attention_mask.dtype)
            mask = torch.cat([video_mask.to(attention_mask.dtype), attention_mask], 1)
        else:
            mask = attention_mask
        mask = mask.to(torch.int32).contiguous()
        full_labels = rows_labelled = None
        if labels is not None:
            fl = torch.cat([torch.full((B, T), -100, dtype=torch.long, device=self.dev), labels], 1) if use_video else labels
            full_labels = fl.contiguous().view(-1)
            rows_labelled = torch.nonzero(full_labels != -100).view(-1)
        if logit_rows is not None:
            if labels is not None:
                raise RuntimeError("logit_rows cannot be combined with labels (the loss of a labelled call lives on its own rows)")
            if need_grad:  # duplicates would race in the backward's scatter-add; refused before anything is queued
                check_logit_rows(logit_rows, B * S)
        # packed rows (opt-in): only for calls whose outputs live on selected rows; the layout is a function of the input,
        # read back before anything is queued (as Engine.run does it)
        pk = None
        if (getattr(m, "packed_rows", False) and (full_labels is not None or logit_rows is not None)
                and not torch.cuda.is_current_stream_capturing()):
            pk = bert_packing(mask.view(-1), full_labels, logit_rows, B, S, T)
        if train:
            m.step_seed += 1
        run = Run(B=B, S=S, T=T, Lt=Lt, train=train, save=need_grad, seed_base=m.dropout_seed_base() * 0x9E3779B1 & 0x7FFFFFFFFFFFFFFF
                  if train else 0, p_hid=self.cfg.hidden_dropout_prob if train else 0.0,
                  p_att=self.cfg.attention_probs_dropout_prob if train else 0.0, p_ad=0.0, pk=pk,
                  N=pk.n if pk is not None else B * S)
        run.mask = mask.view(-1)
        pos1 = torch.arange(1, S + 1, device=self.dev, dtype=torch.int32)
        run.klen = (mask * pos1).amax(1).to(torch.int32).contiguous()
        run.border = torch.argsort(run.klen, descending=True, stable=True).to(torch.int32).contiguous()
        run.labels = full_labels
        if full_labels is not None:
            run.rows = rows_labelled
            if pk is not None:  # the head works on packed rows; the label values are looked up on the grid
                run.label_rows = rows_labelled
                run.rows = pk.inv[rows_labelled]
        use_ans = bool(m.n_ans) and not mlm
        if logit_rows is not None:  # the head runs on these rows only; with gradients its backward does too
            run.logit_rows = logit_rows.to(self.dev).to(torch.int32).contiguous().view(-1)
            if pk is not None:
                run.logit_rows = pk.inv[run.logit_rows.long()].to(torch.int32)
        run.grad_in = tuple(k for k, _ in grad_in)
        if need_grad:  # the backward stops below this layer, and the forward saves nothing below it
            run.low_layer, run.live_version = self.lowest_layer(run.grad_in), self.live_version
        run.video_dtype = video.dtype if use_video else None
        run.hid_grad = bool(want_hidden) and need_grad  # the hidden states handed out are outputs of the step's node
        with L.seed_word(None):
            logits, loss_t = self._forward(run, input_ids.contiguous(), video, use_ans, want_hidden)
        Vout = run.Vout
        if logit_rows is not None:
            res = {"logits": logits[:, :Vout], "loss": None, "run": run}
        else:
            res = {"logits": logits.view(B, S, -1)[:, :, :Vout], "loss": None, "run": run}
        if k_pred:
            res["predictions"] = predictions_of_call(run, logits, k_pred, rows_labelled, logit_rows)
        if want_hidden:
            res["hidden_states"] = run.hidden_out
        if need_grad:
            lt = loss_t if loss_t is not None else torch.zeros((), dtype=F32, device=self.dev)
            hid = res["hidden_states"] if run.hid_grad else ()
            outs = _StepFn.apply(self, run, lt, res["logits"], len(hid), *hid, *[t for _, t in grad_in],
                                 *[self.named[n] for n in self.order])
            loss_o, res["logits"] = outs[:2]
            res["loss"] = loss_o if run.labels is not None else None
            if hid:
                res["hidden_states"] = tuple(outs[2:])
        elif run.labels is not None:
            res["loss"] = loss_t
        return res

    def _forward(self, run, input_ids, video, use_ans, want_hidden):
        H, dev = self.H, self.dev
        B, S, T = run.B, run.S, run.T
        pk, N = run.pk, run.N
        # ---- embeddings
        vproj = None
        if T:
            vb = torch.zeros(B * T, self.Fp, dtype=BF16, device=dev)
            vb[:, : self.F] = video.detach().reshape(B * T, self.F)  # (detached: its gradient comes from the step's own backward)
            vproj = torch.empty(B * T, H, dtype=F32, device=dev)
            L.gemm(vb, self._video_weight(), bias=self.P["bert.embeddings.linear_video.bias"], out_f32=vproj)
            run.video_bf16 = vb
        t0 = torch.empty(B * S, H, dtype=F32, device=dev)
        L.embed_gather(input_ids, self.E32, vproj, T, t0)
        if pk is None:
            pos_rows = self._pos_rows(B, S)
        else:  # packed rows: the gather went through the padded grid; the position of a row is pk.pos
            t0 = t0.index_select(0, pk.sel)
            pos_rows = self.pos_type.index_select(0, pk.pos)
        emb, _ = self._ln(run, "bert.embeddings.LayerNorm", y=t0, resid=Stream(bf16=None, plain=pos_rows), N=N,
                          want_f32=run.p_hid > 0)
        run.emb_norm = emb.norm if run.low_layer < 0 else None
        if run.low_layer >= 0:
            run.video_bf16 = None
        if run.p_hid > 0:  # post-LN dropout (:277): the layers see the materialised, dropped-out rows
            run.seed_emb = run.next_seed()
            L.dropout_f32(emb.plain, run.p_hid, run.seed_emb, out_f32=emb.plain, out_bf16=emb.bf16)
            emb = Stream(bf16=emb.bf16, plain=emb.plain)
        hs = [emb]
        x = emb
        for i in range(self.nL):
            x = self._layer_fwd(run, i, x)
            hs.append(x)
        if want_hidden:
            if pk is None:
                run.hidden_out = tuple(self._materialize(s).view(B, S, H) for s in hs)
            else:  # (positions without a row read as zero)
                run.hidden_out = tuple(torch.zeros(B * S, H, dtype=F32, device=dev).index_copy_(0, pk.sel, self._materialize(s))
                                       .view(B, S, H) for s in hs)
        # ---- MLM / answer head
        if use_ans:
            Vout, table, bias = self.n_ans, self.Ansb, self.ans_bias
        else:
            Vout, table, bias = self.V, self.Eb, self.head_bias
        ldv = _ru(Vout, 64)
        run.Vout, run.head_table, run.head_bias, run.ldv, run.use_ans = Vout, table, bias, ldv, use_ans
        rows_only = run.logit_rows
        if rows_only is not None:
            hin = torch.empty(rows_only.numel(), H, dtype=BF16, device=dev)
            if rows_only.numel():
                L.gather_rows_bf16(x.bf16, rows_only, hin)
            hp, hl = self._head_stage(run, hin)
            if run.save:  # row-compact: what the head backward of exactly these rows reads
                run.head_pre, run.head_norm = hp, hl.norm
            logits = torch.empty(rows_only.numel(), ldv, dtype=F32, device=dev)
            L.gemm(hl.bf16, table, bias=bias, out_f32=logits, N=Vout)
            run.logits = logits
            return logits, None
        hp, hl = self._head_stage(run, x.bf16)
        run.head_pre, run.head_norm = hp, hl.norm
        logits = torch.empty(B * S, ldv, dtype=F32, device=dev)  # (on the grid in both layouts)
        run.logits = logits
        if run.labels is None:  # (never packed: packing needs labels or logit_rows)
            L.gemm(hl.bf16, table, bias=bias, out_f32=logits, N=Vout)
            return logits, None
        # a loss is asked for: CE on the labelled rows from a small GEMM; the full logits are filled on first access
        run.rows_i32 = run.rows.to(torch.int32)
        R = run.rows_i32.numel()
        run.loss_acc = L.zeros(2, dtype=F32, device=dev)
        if R:
            hrows = torch.empty(R, H, dtype=BF16, device=dev)
            L.gather_rows_bf16(hl.bf16, run.rows_i32, hrows)
            lc = torch.empty(R, ldv, dtype=F32, device=dev)
            L.gemm(hrows, table, bias=bias, out_f32=lc, N=Vout)
            run.labels_c = run.labels[run.rows if run.label_rows is None else run.label_rows].contiguous()
            run.row_lse = torch.empty(R, dtype=F32, device=dev)
            L.ce_fwd(lc, run.labels_c, Vout, run.row_lse, run.loss_acc)
            run.logits_c = lc
        run.head_ln_bf16 = hl.bf16
        run.logits_pending = True
        return logits, run.loss_acc[0] / run.loss_acc[1]

    def fill_logits(self, run):
        if run.logits_pending:
            run.logits_pending = False
            pk = run.pk
            if pk is None:
                L.gemm(run.head_ln_bf16, run.head_table, bias=run.head_bias, out_f32=run.logits, N=run.Vout)
                return
            # packed rows: grid positions without a row read as zero; the others arrive in slabs of 1024 rows
            run.logits.zero_()
            for r0 in range(0, pk.n, 1024):
                r1 = min(pk.n, r0 + 1024)
                slab = torch.empty(r1 - r0, run.logits.shape[1], dtype=F32, device=self.dev)
                L.gemm(run.head_ln_bf16[r0:r1], run.head_table, bias=run.head_bias, out_f32=slab, N=run.Vout)
                run.logits.index_copy_(0, pk.sel[r0:r1], slab)

    def _head_stage(self, run, hin):
        """BertPredictionHeadTransform (:67-71): LayerNorm(gelu(dense(x)))"""
        N = hin.shape[0]
        hp = torch.empty(N, self.H, dtype=F32, device=self.dev)
        L.gemm(hin, self.Wh, bias=self.bh, out_f32=hp)
        hg = torch.empty(N, self.H, dtype=F32, device=self.dev)
        L.dropout_gelu_fwd(hp, 0.0, 0, hg)
        hl, _ = self._ln(run, "cls.predictions.transform.LayerNorm", y=hg, resid=None, N=N)
        return hp, hl

    def _layer_fwd(self, run, li: int, x: Stream) -> Stream:
        w, H, I, dev = self.Lw[li], self.H, self.I, self.dev
        B, S, nh = run.B, run.S, self.nh
        N = run.N
        p = f"bert.encoder.layer.{li}."
        qkv = torch.empty(N, 3 * H, dtype=BF16, device=dev)
        L.gemm(x.bf16, w["Wqkv"], bias=w["bqkv"], out_bf16=qkv)
        ctx = torch.empty(N, H, dtype=BF16, device=dev)
        lse = torch.empty(B, nh, S, dtype=F32, device=dev)
        seed_att = run.next_seed() if run.p_att > 0 else 0
        if run.pk is None:
            L.mha_fwd(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], run.mask, self.scale, ctx, lse, B, S, nh, p_drop=run.p_att,
                      seed=seed_att, klen=run.klen, border=run.border)
        else:
            L.mha_fwd_rows(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], run.mask, run.klen, run.pk.row0, self.scale, ctx, lse, B, S,
                           nh, p_drop=run.p_att, seed=seed_att, border=run.border)
        y1 = torch.empty(N, H, dtype=F32, device=dev)
        L.gemm(ctx, w["Wo"], bias=w["bo"], out_f32=y1)
        a, seed1 = self._ln(run, p + "attention.output.LayerNorm", y=y1, resid=x, N=N, p_drop=run.p_hid)
        hmid = torch.empty(N, I, dtype=BF16, device=dev)
        save = run.save and li >= run.low_layer  # (below the lowest layer with a live leaf nothing is kept for a backward)
        gp = torch.empty(N, I, dtype=BF16, device=dev) if save else None
        L.gemm(a.bf16, w["Wi"], bias=w["bi"], act=L.ACT_GELU_GRAD if save else L.ACT_GELU, out_bf16=hmid, out_pre=gp)
        y2 = torch.empty(N, H, dtype=F32, device=dev)
        L.gemm(hmid, w["Wd"], bias=w["bd"], out_f32=y2)
        out, seed2 = self._ln(run, p + "output.LayerNorm", y=y2, resid=a, N=N, p_drop=run.p_hid)
        run.layers.append(BertLayerSave(qkv=qkv if save else None, ctx=ctx if save else None, lse=lse if save else None, gp=gp,
                                        ln1=a.norm if save else None, ln2=out.norm if save else None, seed_att=seed_att,
                                        seed_ln1=seed1, seed_ln2=seed2))
        return out

    # ------------------------------------------------------------------ backward
    def backward(self, run, gloss: Optional[torch.Tensor], glogits: Optional[torch.Tensor] = None, attach: bool = True,
                 ghid=None):
        """ghid: gradients handed in on the hidden states of an output_hidden_states=True call ([B, S, H] or None each); each is
        added to the running dx where the backward crosses that boundary.  Returns the gradients of the inputs named in
        run.grad_in as a dict ("video": [B, T, F] in the caller's dtype)."""
        if not run.save:
            raise RuntimeError("forward was run without gradient bookkeeping")
        H, dev = self.H, self.dev
        B, S, T = run.B, run.S, run.T
        pk, N = run.pk, run.N
        if attach:
            self.attach_grads()
        red = self.reducer  # data parallel: told when a stage's bucket is final, where collectives may start, when the step ends
        if ghid is not None and all(g is None for g in ghid):
            ghid = None
        if run.logit_rows is not None and run.logit_rows.numel() == 0 and red is None and ghid is None:
            return  # no row was asked for: every gradient is exactly zero, nothing is launched (a reducer still needs its buckets)
        dx = L.zeros(N, H, dtype=F32, device=dev)
        Vout = run.Vout
        Vp = _ru(Vout, 64)
        if gloss is not None and run.labels is not None and run.rows_i32.numel():
            R = run.rows_i32.numel()
            dlog = torch.empty(R, Vp, dtype=BF16, device=dev)
            gs = gloss.detach().to(F32) if (isinstance(gloss, torch.Tensor) and gloss.is_cuda) else float(gloss)
            ar = torch.arange(R, dtype=torch.int32, device=dev)
            L.ce_bwd_rows(run.logits_c, run.labels_c, ar, Vout, Vp, run.row_lse, run.loss_acc, gs, dlog)
            dx = self._head_bwd(run, run.rows_i32, dlog, dx)
        if glogits is not None and run.logit_rows is not None:  # the requested rows only (distinct: check_logit_rows)
            R = run.logit_rows.numel()
            if R:
                dlog = torch.zeros(R, Vp, dtype=BF16, device=dev)
                dlog[:, :Vout].copy_(glogits.reshape(R, Vout))
                dx = self._head_bwd(run, run.logit_rows, dlog, dx, compact=True)
        elif glogits is not None:
            gl = glogits.reshape(B * S, Vout)
            if pk is not None:  # (gradients handed in at positions without a row have nothing to flow into)
                gl = gl.index_select(0, pk.sel)
            dlog = torch.zeros(N, Vp, dtype=BF16, device=dev)
            dlog[:, :Vout].copy_(gl)
            dx = self._head_bwd(run, None, dlog, dx)
        low = run.low_layer
        for li in reversed(range(max(low, 0), self.nL)):
            g = _hid_rows(run, ghid, li + 1)  # handed in on this layer's output
            if g is not None:
                dx.add_(g)
            dx = self._layer_bwd(run, li, run.layers[li], dx)
            if red is not None:
                red.ready(f"layer{li}")
        run.layers.clear()
        if low >= 0:  # nothing live below layer `low` and no input takes a gradient: the backward ends here
            if red is not None:
                red.finish()  # (the buckets of the stages that did not run leave now, as zeros)
            return {}
        # ---- embeddings: post-LN dropout, LayerNorm (dgamma / dbeta), linear_video on the video rows
        g = _hid_rows(run, ghid, 0)  # hidden_states[0]: the embedding output, behind its dropout
        if g is not None:
            dx.add_(g)
        if run.p_hid > 0:
            L.dropout_f32(dx, run.p_hid, run.seed_emb, out_f32=dx)
        dt, dyb = self._ln_bwd("bert.embeddings.LayerNorm", dx, run.emb_norm, 0.0, 0, want_dy_bf16=bool(T))
        want_dvideo = "video" in run.grad_in and T
        gvw, gvb = (self.Gl.get("bert.embeddings.linear_video." + k) for k in ("weight", "bias"))
        if T and (gvw is not None or gvb is not None or want_dvideo):
            # the video slots are the first T rows of every sample (packed rows: plen >= T)
            first = torch.arange(B, device=dev, dtype=torch.int32) * S if pk is None else pk.row0[:-1]
            vrows = (first[:, None] + torch.arange(T, device=dev, dtype=torch.int32)[None, :]).view(-1).contiguous()
            dv = torch.empty(B * T, H, dtype=BF16, device=dev)
            L.gather_rows_bf16(dyb, vrows, dv)
        if T and gvw is not None:
            L.gemm_tn_acc(dv, run.video_bf16, gvw, self.sk_ws, M=H, N=self.F)
        if T and gvb is not None:
            L.colsum(dv, gvb, self._cs_ws)
        if red is not None:
            red.ready("emb")
            red.finish()
        gin = {}
        if want_dvideo:
            # dvideo = d(embedding rows of the video slots) . W_video: bf16 operands, fp32 accumulation, against the K-contiguous
            # (transposed) copy of linear_video.weight, which only a step with this gradient builds
            WvT = torch.empty(self.F, H, dtype=BF16, device=dev)
            L.transpose_to_bf16(self.P["bert.embeddings.linear_video.weight"], WvT)
            dvid = torch.empty(B * T, self.Fp, dtype=F32, device=dev)
            L.gemm(dv, WvT, out_f32=dvid, N=self.F)
            gin["video"] = dvid[:, : self.F].reshape(B, T, self.F).to(run.video_dtype)
        return gin

    def _head_bwd(self, run, rows, dlog, dx, compact=False):
        """dx[rows] += d/d(head input) for the bf16 logit gradients dlog [R, Vp] of those rows (rows None: every row); returns dx.
        compact: the forward ran the head on exactly these rows (logit_rows), so what it saved is already [R, .]."""
        H, dev = self.H, self.dev
        R = dlog.shape[0]
        tableT = self.AnsTb if run.use_ans else self.ETb
        dhl = L.zeros(R, H, dtype=F32, device=dev)
        Vp = dlog.shape[1]
        if R >= 2048:
            L.gemm(dlog, tableT, out_f32=dhl, N=H)
        else:
            L.gemm(dlog, tableT, out_f32=dhl, N=H, splitk=max(2, min(16, Vp // 8192)), ws=self.sk_ws)
        hn = run.head_norm
        if rows is None or compact:
            sub, pre = hn, run.head_pre
        else:
            rl = rows.long()
            sub, pre = NormRef(hn.t[rl].contiguous(), hn.stats[rl].contiguous(), hn.gamma, hn.beta), run.head_pre[rl].contiguous()
        dt, _ = self._ln_bwd("cls.predictions.transform.LayerNorm", dhl, sub, 0.0, 0, want_dy_bf16=False)
        dpre = torch.empty(R, H, dtype=BF16, device=dev)
        L.dropout_gelu_bwd(dt, pre, 0.0, 0, out_bf16=dpre)
        if rows is None:  # every row: dx + dpre . Wh into a fresh buffer
            out = torch.empty(R, H, dtype=F32, device=dev)
            L.gemm(dpre, self.WhT, aux=dx, aux_kind=L.AUX_ADD_F32, out_f32=out)
            return out
        dxr = torch.empty(R, H, dtype=F32, device=dev)
        L.gemm(dpre, self.WhT, out_f32=dxr)
        L.scatter_rows_f32(dxr, rows, dx)  # (scatter-add)
        return dx

    def _layer_bwd(self, run, li: int, sv: BertLayerSave, dout: torch.Tensor) -> torch.Tensor:
        """dout: gradient of the layer's output (fp32 [N, H]); returns the gradient of its input"""
        w, H, I, dev = self.Lw[li], self.H, self.I, self.dev
        B, S, nh = run.B, run.S, self.nh
        N = run.N
        p = f"bert.encoder.layer.{li}."
        dt2, dy2 = self._ln_bwd(p + "output.LayerNorm", dout, sv.ln2, run.p_hid, sv.seed_ln2)
        dh = torch.empty(N, I, dtype=BF16, device=dev)
        L.gemm(dy2, w["WdT"], aux=sv.gp, aux_kind=L.AUX_MUL_BF16, out_bf16=dh)  # through Wd and the GELU
        da = torch.empty(N, H, dtype=F32, device=dev)
        L.gemm(dh, w["WiT"], aux=dt2, aux_kind=L.AUX_ADD_F32, out_f32=da)  # + the residual branch
        dt1, dy1 = self._ln_bwd(p + "attention.output.LayerNorm", da, sv.ln1, run.p_hid, sv.seed_ln1)
        dctx = torch.empty(N, H, dtype=BF16, device=dev)
        L.gemm(dy1, w["WoT"], out_bf16=dctx)
        Dv = torch.empty(B, nh, S, dtype=F32, device=dev)
        dqkv = torch.empty(N, 3 * H, dtype=BF16, device=dev)
        q = sv.qkv
        if self.reducer is not None:  # a stretch without one-workgroup-per-CU GEMM tiles: where gradient collectives may start
            self.reducer.window()
        if run.pk is None:
            L.attn_rowdot(dctx, sv.ctx, Dv, B, S, nh)
            L.mha_bwd(q[:, :H], q[:, H:2 * H], q[:, 2 * H:], dctx, run.mask, sv.lse, Dv, self.scale, dqkv[:, :H], dqkv[:, H:2 * H],
                      dqkv[:, 2 * H:], B, S, nh, p_drop=run.p_att, seed=sv.seed_att, klen=run.klen, border=run.border)
        else:
            L.mha_bwd_rows(q[:, :H], q[:, H:2 * H], q[:, 2 * H:], dctx, sv.ctx, run.mask, run.klen, run.pk.row0, sv.lse, Dv,
                           self.scale, dqkv[:, :H], dqkv[:, H:2 * H], dqkv[:, 2 * H:], B, S, nh, p_drop=run.p_att,
                           seed=sv.seed_att, border=run.border)
        dx = torch.empty(N, H, dtype=F32, device=dev)
        L.gemm(dqkv, w["WqkvT"], aux=dt1, aux_kind=L.AUX_ADD_F32, out_f32=dx)
        return dx
