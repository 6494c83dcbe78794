"""Host-side orchestration of the disentangled-attention backward (see csrc/attn_bwd.hip for the math).  Two routes, chosen
by whether the training forward saved its probabilities (sv.psave, engine option attn_save_p):

  saved P (shipped)  prep     : D = rowdot(dO, O) + the position tables expanded by the index map (PQX / PKX)     (one launch)
                     dspk     : dV, dK, dS, dS^T from the saved probabilities (fbl_disent_attn_bwd_dspk)
                     dq       : dQ = dS.K + the c2p term in Toeplitz form (fbl_disent_attn_bwd_dq)
  recompute          prep     : D, PKX and the transposed copies Q^T / PQ^T of the key-major shear pass
                     ds       : recomputes the probabilities; dV, dS, dS^T (fbl_disent_attn_bwd_ds)
                     dq       : as above
                     shear    : dK = dS^T.Q + the p2c term by the key-major shear pass (fbl_disent_attn_bwd_shear)
  both               pos_grad : dPK[h] = sum_b G1^T.Q , dPQ[h] = sum_b G2^T.K -- straight from dS / dS^T, all layer executions at
                                the end of backward (fbl_attn_pos_grad: the sheared operand G is formed on the fly out of LDS)
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Optional

import torch

from . import lib as L

BF16, F32 = torch.bfloat16, torch.float32
# softmax scale of the disentangled attention: head dimension 64, three score terms (content-content, content-position,
# position-content; model/deberta.py:769-776: 1 / sqrt(d * scale_factor))
ATTN_SCALE = 1.0 / math.sqrt(64 * 3)


_RANGE = {}


def _relidx_range(S, cfg):
    """(first, count) of the position-table rows the relative-index map of a length-S sequence can touch (host integers,
    computed once per sequence length)"""
    key = (S, cfg.position_buckets, cfg.max_rel, cfg.att_span)
    if key not in _RANGE:
        from .model.relpos import rel_index_vector

        rv = rel_index_vector(S, cfg.position_buckets, cfg.max_rel, cfg.att_span)
        _RANGE[key] = (int(rv[0]), int(rv[-1]) - int(rv[0]) + 1)
    return _RANGE[key]


_DRANGE = {}
POS_GRAD_MAX_DELTAS = 8  # deltas per table row the walking kernel of fbl_attn_pos_grad takes (beyond: its prefix-difference kernel)


def _delta_ranges(S, cfg, dev, limit=POS_GRAD_MAX_DELTAS):
    """(dlo, dcnt, max dcnt): int16 device tensors [rcnt]: table row rmin + r collects the deltas [dlo[r], dlo[r] + dcnt[r]) -- the inverse
    of the (monotone) relative-index vector, computed once per sequence length.  With a limit (default POS_GRAD_MAX_DELTAS: the
    maps the walking kernel takes), raises NotImplementedError for a bucket map that puts more than `limit` deltas on one table
    row (the FrozenBiLM map, 256 buckets / 512 positions, peaks at 6); limit=None takes every map -- fbl_attn_pos_grad picks
    its kernel from the max, as the position-table gradients do."""
    key = (S, cfg.position_buckets, cfg.max_rel, cfg.att_span, str(dev))
    if key not in _DRANGE:
        import numpy as np

        from .model.relpos import rel_index_vector

        rv = np.asarray(rel_index_vector(S, cfg.position_buckets, cfg.max_rel, cfg.att_span), dtype=np.int64)
        rmin, rcnt = int(rv[0]), int(rv[-1]) - int(rv[0]) + 1
        first = np.searchsorted(rv, np.arange(rmin, rmin + rcnt), side="left")
        last = np.searchsorted(rv, np.arange(rmin, rmin + rcnt), side="right")
        dlo = (first - (S - 1)).astype(np.int16)
        dcnt = (last - first).astype(np.int16)
        _DRANGE[key] = (torch.from_numpy(dlo).to(dev), torch.from_numpy(dcnt).to(dev), int(dcnt.max()))
    cmax = _DRANGE[key][2]
    if limit is not None and cmax > limit:
        raise NotImplementedError(
            f"position-table gradients (fbl_attn_pos_grad) take at most {limit} relative positions per table "
            f"row; position_buckets={cfg.position_buckets}, max_relative_positions={cfg.max_rel} at sequence length {S} "
            f"puts {cmax} on one row")
    return _DRANGE[key]


def disent_attn_bwd(eng, run, sv, dctx, dqkv, dpqk, defer_pos=False):
    """defer_pos=True: skip the position-table gradients and return the state they need (the engine runs them for ALL layer
    executions at once at the end of backward: pos_table_grads_batched); otherwise dpqk [span2, 2H] (bf16, [dPQ|dPK]) is filled
    here."""
    B, S, H, nh, span2 = run.B, run.S, eng.H, eng.nh, eng.span2
    Sp = (S + 63) // 64 * 64
    dev = eng.dev
    qkv = sv.qkv
    q, k, v = qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:]
    pq, pk = sv.pqk[:, :H], sv.pqk[:, H:]
    relidx = eng.relidx(S)
    # This is also the kernel-level entry that the kernel tests and tools/pmc_attn.py drive with bare stand-ins for `run` and
    # `sv` (B, S, p_att, mask_i32, klen / qkv, pqk, ctx, lse, seed_att): what only an engine step carries is optional here.
    klen, border = run.klen, getattr(run, "border", None)
    scale = ATTN_SCALE
    pk_ = getattr(run, "cb", None) or getattr(run, "pk", None)  # (cb: the compact backward next to a padded forward, Run.cb)
    row0 = pk_.row0 if pk_ is not None else None  # packed-row layout of q / k / v / dO and of the dQ / dK / dV outputs
    saved_p = getattr(sv, "psave", None) is not None

    # One launch prepares the backward: D_i = dO_i . O_i and the expanded tables PKX (dq) and PQX (dspk) -- the shipped,
    # saved-P route.  Only the recompute route also gets the transposed copies Q^T / PQ^T (its key-major shear pass reads
    # them); nothing prepares K^T / Q^T for the position-table gradients any more: fbl_attn_pos_grad reads the token rows of
    # q / k.  (Folding D into kernel A was measured: +43 us there for the O tiles on its critical path; five separate small
    # launches: 65 us in situ.)
    Dv = torch.empty(B, nh, S, dtype=F32, device=dev)
    PKX = torch.empty(nh, 2 * Sp, 64, dtype=BF16, device=dev)
    if saved_p:
        QT = PQT = None
        PQX = torch.empty(nh, 2 * Sp, 64, dtype=BF16, device=dev)
    else:
        QT = torch.empty(nh, 64, B, Sp, dtype=BF16, device=dev)
        PQT = torch.empty(nh, 64, span2, dtype=BF16, device=dev)
        PQX = None
    L.attn_bwd_prep(q, pq, pk, dctx, sv.ctx, QT, PQT, Dv, B, S, Sp, nh, span2, row0=row0, relidx=relidx, PQX=PQX, PKX=PKX)
    dS = torch.empty(B, nh, Sp, Sp, dtype=BF16, device=dev)
    dST = torch.empty(B, nh, Sp, Sp, dtype=BF16, device=dev)
    # |i-j| < lin: relidx injective -- identity buckets (model/deberta.py:578-589: mid = bucket_size // 2), or a clamped table
    # (position_buckets <= 0): clamp(delta + span, 0, 2 span - 1) puts delta = span - 1 AND every delta >= span on the top edge
    # row (every delta <= -span on the bottom one), so it is injective for |delta| < span - 1
    lin = eng.cfg.position_buckets // 2 if eng.cfg.position_buckets > 0 else eng.cfg.att_span - 1
    if saved_p:
        # kernel A from the probabilities the training forward saved, dK formed in place
        L.disent_attn_bwd_dspk(sv.psave, sv.msave, q, v, dctx, PQX, sv.lse, Dv, scale, dqkv[:, H:2 * H], dqkv[:, 2 * H:], dS, dST,
                               B, S, Sp, nh, p_drop=run.p_att, seed=sv.seed_att, klen=klen, border=border, row0=row0)
        sv.psave = sv.msave = None
    else:
        lin_a = min(lin, span2 // 2) if eng.cfg.position_buckets > 0 else 0  # affine addressing of kernel A: identity buckets only
        L.disent_attn_bwd_ds(q, k, v, dctx, pk, pq, relidx, run.mask_i32, sv.lse, Dv, scale, dqkv[:, 2 * H:], dS, dST,
                             B, S, Sp, nh, span2, p_drop=run.p_att, seed=sv.seed_att, klen=klen, border=border, lin=lin_a, row0=row0)
    L.disent_attn_bwd_dq(dS, k, PKX, dqkv[:, :H], B, S, Sp, nh, klen=klen, border=border, row0=row0)
    if not saved_p:
        L.disent_attn_bwd_shear(dST, QT, PQT, relidx, dqkv[:, H:2 * H], B, S, Sp, nh, span2, klen=klen, lin=lin, border=border,
                                row0=row0)
    # only the table rows inside the range of relidx can have a non-zero gradient; fbl_attn_pos_grad reads dS / dS^T and the
    # token rows of q / k themselves
    rmin, rcnt = _relidx_range(S, eng.cfg)
    state = dict(dS=dS, dST=dST, q=q, k=k, rmin=rmin, rcnt=rcnt, B=B, S=S, Sp=Sp, klen=klen, row0=row0)
    if defer_pos:
        return state
    dpqk.copy_(pos_table_grads(eng, state))  # fp32 -> bf16
    return None


def pos_table_grads(eng, st):
    """dPK[h] = sum_b G1^T[h] . Q[h],  dPQ[h] = sum_b G2^T[h] . K[h]  of one layer execution -> fp32 [span2, 2H] laid out
    [dPQ | dPK] (head h owns columns h*64 .. h*64+63)"""
    H, nh, span2 = eng.H, eng.nh, eng.span2
    rmin, rcnt, B, Sp = st["rmin"], st["rcnt"], st["B"], st["Sp"]
    dpos = torch.zeros(span2, 2 * H, dtype=F32, device=eng.dev)
    dlo, dcnt, cmax = _delta_ranges(st["S"], eng.cfg, eng.dev, limit=None)
    for neg, X, Y, col0 in ((0, st["dS"], st["q"], H), (1, st["dST"], st["k"], 0)):
        d = torch.empty(1, nh, rcnt, 64, dtype=F32, device=eng.dev)
        L.attn_pos_grad(neg, [X], [Y], dlo, dcnt, cmax, d, B, st["S"], Sp, nh, rcnt, klen=st["klen"], row0=st["row0"])
        dpos[rmin:rmin + rcnt, col0:col0 + H].view(rcnt, nh, 64).copy_(d[0].permute(1, 0, 2))
    return dpos


@dataclass
class PosChain:
    """What the position-table gradients of ALL layer executions need, collected execution by execution: dS / dS^T (2 x 157 MB
    per execution at the bench shape, kept until the end of backward) and the token rows of the saved q / k."""
    rmin: int
    rcnt: int
    B: int
    S: int
    Sp: int
    dS: list = field(default_factory=list)
    dST: list = field(default_factory=list)
    q: list = field(default_factory=list)
    k: list = field(default_factory=list)
    seeds: list = field(default_factory=list)   # seed of each execution's position dropout
    klen: Optional[torch.Tensor] = None         # the same for every execution of a step
    row0: Optional[torch.Tensor] = None
    # Executions that form their table gradients themselves (the decoder on selected rows, engine._attn_bwd_qrows) are the FIRST
    # of the chain; they write into dbuf = (dPK, dPQ) fp32 [n_exec, nh, rcnt, 64], the buffers fbl_attn_pos_grad fills for the rest
    n_formed: int = 0
    n_exec: int = 0
    nh: int = 0
    dev: Optional[torch.device] = None
    dbuf: Optional[tuple] = None

    def add(self, st, seed_pos):
        """st: the state disent_attn_bwd(defer_pos=True) returned for one execution"""
        self.dS.append(st["dS"]); self.dST.append(st["dST"]); self.q.append(st["q"]); self.k.append(st["k"])
        self.seeds.append(seed_pos)
        self.klen, self.row0 = st["klen"], st["row0"]

    def formed_slot(self):
        """(dPK, dPQ) fp32 [nh, rcnt, 64] of the next execution that forms its table gradients itself"""
        assert not self.dS and self.n_exec > self.n_formed, "executions with formed table gradients come first"
        if self.dbuf is None:
            self.dbuf = tuple(torch.empty(self.n_exec, self.nh, self.rcnt, 64, dtype=F32, device=self.dev) for _ in range(2))
        return self.dbuf[0][self.n_formed], self.dbuf[1][self.n_formed]

    def add_formed(self, seed_pos):
        self.n_formed += 1
        self.seeds.append(seed_pos)


def pos_chain_buffers(eng, run):
    """an empty PosChain for the backward of `run`"""
    rmin, rcnt = _relidx_range(run.S, eng.cfg)
    return PosChain(rmin=rmin, rcnt=rcnt, B=run.B, S=run.S, Sp=(run.S + 63) // 64 * 64, nh=eng.nh, dev=eng.dev)


def pos_table_grads_batched(eng, run, pc: PosChain):
    """The relative-position-table gradient of the whole backward pass in five launches at its END (it feeds only
    encoder.LayerNorm's gamma / beta, the last thing backward needs): until round 4 every layer execution ran its own chain
    (two split-K products, folds, cast, projection, dropout, accumulation) on a side stream next to the following layer's GEMMs
    -- 9.3 ms of side-queue kernel time per step whose long-lived workgroups cost the main stream 2.7 ms.  Now, over all E
    executions at once:
        dPK[e,h] = G1^T[e,h] . Q[e,h] ,  dPQ[e,h] = G2^T[e,h] . K[e,h]     (fbl_attn_pos_grad, straight from dS / dS^T)
        dR_e     = [dPQ | dPK]_e . [Wq ; Wk]_e                              (one batched GEMM against the packed weights)
        dR       = sum_e dropout_e(dR_e)                                    (fbl_dropout_sum_f32: each through its own mask)
    Returns dR [span2, H] fp32.  autograd of model/deberta.py:779, 847-853, 870-918 summed over the executions."""
    H, nh, span2 = eng.H, eng.nh, eng.span2
    E, rmin, rcnt, B, Sp = len(pc.seeds), pc.rmin, pc.rcnt, pc.B, pc.Sp
    dev = eng.dev
    # [dPQ | dPK] of every execution, rows rmin .. rmin + rcnt of the tables (the others cannot be touched: their gradient is
    # zero): bf16 operand of the projection, fully written by the two copies below
    dpb = torch.empty(E, rcnt, 2 * H, dtype=BF16, device=dev)
    dlo, dcnt, cmax = _delta_ranges(pc.S, eng.cfg, dev, limit=None)
    for neg, X, Y, col0 in ((0, pc.dS, pc.q, H), (1, pc.dST, pc.k, 0)):
        nf = pc.n_formed
        if pc.dbuf is not None:  # the first nf executions have written their tables already
            assert pc.n_exec == E, (pc.n_exec, E)
            d = pc.dbuf[neg]
        else:
            d = torch.empty(E, nh, rcnt, 64, dtype=F32, device=dev)
        if X:
            L.attn_pos_grad(neg, X, Y, dlo, dcnt, cmax, d[nf:], B, pc.S, Sp, nh, rcnt, klen=pc.klen, row0=pc.row0)
        # [e, h, r, 64] fp32 -> [e, r, h*64 + .] bf16, into this table's column block
        L.heads_to_rows_bf16(d, dpb[:, :, col0:col0 + H])
    if getattr(run, "lora_pos_wait", False):  # LoRA on query_proj / key_proj: their weights' gradient through PQ / PK
        eng._lora_pos_bwd(run, pc, dpb)
    tmp = torch.empty(E, rcnt, H, dtype=F32, device=dev)
    L.gemm(dpb, eng.WposT_exec[:E], out_f32=tmp)
    dR = L.zeros(span2, H, dtype=F32, device=dev)
    # (dropout keys of the [span2, H] table: element (r, c) <-> r*H + c)
    L.dropout_sum_f32(tmp, pc.seeds if run.p_hid > 0 else [0] * E, run.p_hid, dR[rmin:rmin + rcnt], key0=rmin * H)
    return dR
