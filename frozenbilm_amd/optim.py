"""Fused clip + Adam over the flat trainable buffer (two kernel launches per step instead of ~300 x k).

Drop-in for ``torch.optim.Adam(params_requiring_grad, lr, betas, weight_decay)`` as built by the reference
(main.py:182-188) followed by ``clip_grad_norm_(model.parameters(), max_norm)`` (main.py:82-84): pass
``clip_max_norm`` to ``step`` to fold the global-norm clip into the update.  ``param_groups[0]["lr"]`` is honoured so
``adjust_learning_rate`` (util/misc.py:59-78) keeps working.

One deliberate difference from ``torch.optim.Adam``: the update runs over the whole flat trainable buffer with ONE step
counter, so a parameter whose gradient is identically zero in a step (``linear_video`` on a batch without video -- no
loop of the reference produces one) still sees its moments decay and moves by ``lr * m_hat / (sqrt(v_hat) + eps)``,
whereas torch skips parameters whose ``.grad`` is None.  Exported states carry the common step count for every parameter.

Partial fine-tuning.  The optimizer's parameter list -- and with it the state schema of checkpoints -- is the model's
trainable-BY-CONSTRUCTION set (``model.trainable_names()``), whatever ``requires_grad`` says at the time; the step acts on the
LIVE set, the members whose ``requires_grad`` was true at the last grad-mode forward (``engine.update_live``).  A dead
parameter is left alone bit for bit -- value, first and second moment: no weight decay, no moment decay -- and the clip norm
is the norm over the live elements only, as ``clip_grad_norm_`` sees it when ``.grad`` is None.  The ONE step counter stays: a
parameter that goes live at step t starts from zero moments with the bias correction of step t (torch would start it at its
own step 1; with the reference's betas the two agree after a few dozen steps).  A step with nothing live does nothing and does
not count.  ``state_dict()`` exports states only for parameters that have been updated at least once, as torch does.  With
every flag untouched the step issues the two launches it always issued (fbl_sumsq, fbl_adam_flat); otherwise their live-set
twins (include/fbl_live.h) over a device table of ranges -- two launches too, however the set is cut up.

Parameter groups.  ``param_groups=[{"params": [...], "lr": .., "betas": .., "eps": .., "weight_decay": ..,
"decoupled_weight_decay": ..}, ...]`` as torch takes them: ``params`` holds parameter names, ``fnmatch`` patterns over the names
or the tensors themselves; a key a group leaves out inherits the constructor's value; every trainable-by-construction parameter
lands in exactly one group and what no group names joins group 0 (frozenbilm_amd/param_groups.py).  ``decoupled_weight_decay``
(torch >= 2.7's own key; also a constructor keyword, the default of every group) makes a group's decay AdamW's:
``p <- p * (1 - lr * wd)``, then Adam with no decay term in the gradient.  ``lr_scale`` gives a group the rate
``param_groups[0]["lr"] * lr_scale``, read at every ``step()`` (and written back to the group's ``lr``), so ``adjust_learning_rate``,
which writes ``param_groups[0]["lr"]`` only, moves every group; a group with both ``lr`` and ``lr_scale`` is refused, and so is
``lr_scale`` on group 0.  ``layerwise_param_groups(model, decay)`` builds the groups of layer-wise rate decay with no weight decay
on LayerNorms and biases.  The hyper-parameters are read from the group dicts at every step.  Everything above holds per group:
ONE step counter, ONE clip norm over the live elements of all groups, a dead parameter untouched in whatever group it sits.
With one group and coupled decay the step is the path described above, launch for launch; otherwise it is the norm (fbl_sumsq or
fbl_sumsq_live) plus ONE fbl_adam_flat_groups (include/fbl_groups.h) over a device table of (live run, group) segments, cached per
live set.  Checkpoints speak torch's multi-group schema: the parameter indices run through the groups in order.
"""
from __future__ import annotations

import torch

from . import lib as L
from . import param_groups as PG


def layerwise_param_groups(model, decay: float, no_decay=("LayerNorm", "bias")):
    """``param_groups`` for layer-wise learning-rate decay (param_groups.layerwise_groups): a stage i steps below the top trains
    at ``decay**i`` of group 0's rate; names holding a ``no_decay`` substring get ``weight_decay = 0``."""
    return PG.layerwise_groups(model.trainable_names(), model.config.num_hidden_layers, decay, no_decay)


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, model, lr=3e-4, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.0, *, param_groups=None,
                 decoupled_weight_decay=False):
        self.model = model
        names = model.trainable_names()
        cons = set(names)
        named = {n: p for n, p in model.named_parameters() if n in cons}
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        if param_groups is None and not decoupled_weight_decay:
            super().__init__([named[n] for n in names], defaults)
        else:
            spec = [dict(g) for g in (param_groups or [])] or [dict(params=[])]
            PG.check_groups(spec)
            members = PG.resolve(spec, names, {id(p): n for n, p in named.items()})
            for g, mem in zip(spec, members):
                g["params"] = [named[n] for n in mem]
            defaults["decoupled_weight_decay"] = bool(decoupled_weight_decay)
            super().__init__(spec, defaults)
            self._sync_lr()
        self._ever = set()  # names of the parameters that a step has updated (or whose state a checkpoint brought)
        self._m = self._v = None
        self._step = 0
        self._ss = None
        self._ss_ws = None
        self._seg_tables = {}  # "engine" -> the engine the tables belong to; (device, live_version) -> table of include/fbl_groups.h

    def _sync_lr(self):
        """a group with lr_scale follows group 0: its `lr` is what the next step uses"""
        for g, lr in zip(self.param_groups, PG.learning_rates(self.param_groups)):
            g["lr"] = lr

    def _plain(self) -> bool:
        """one group with coupled decay: the step of fbl_adam_flat / fbl_adam_flat_live"""
        return len(self.param_groups) == 1 and not self.param_groups[0].get("decoupled_weight_decay", False)

    def _segment_table(self, eng):
        if self._seg_tables.get("engine") is not eng:  # (live_version numbers the live sets of ONE engine)
            self._seg_tables = {"engine": eng}
        key = (str(eng.flat.device), eng.live_version)
        t = self._seg_tables.get(key)
        if t is None:
            gof = {}
            name_of = {id(eng.named[n]): n for n in eng.order}
            for k, g in enumerate(self.param_groups):
                for p in g["params"]:
                    gof[name_of[id(p)]] = k
            numel = {n: eng.named[n].numel() for n in eng.order}
            segs = PG.segments(eng.order, eng.offsets, numel, eng.live_order, gof)
            t = self._seg_tables[key] = L.group_table(segs, eng.flat.numel(), eng.flat.device, len(self.param_groups))
        return t

    def zero_grad(self, set_to_none: bool = True):
        eng = self.model._engine
        if eng is not None and not set_to_none:
            from . import lib as L

            L.zero_(eng.flat_grad)
            return
        super().zero_grad(set_to_none=set_to_none)

    @torch.no_grad()
    def step(self, closure=None, clip_max_norm: float = 0.0, grad_scale: float = 1.0):
        eng = self.model.engine()
        flat, g = eng.flat, eng.flat_grad
        if self._m is None:
            self._m = torch.zeros_like(flat)
            self._v = torch.zeros_like(flat)
            self._ss = torch.zeros(1, dtype=torch.float32, device=flat.device)
            self._ss_ws = torch.empty(L.load().fbl_sumsq_ws_floats(), dtype=torch.float32, device=flat.device)
        elif self._m.numel() != flat.numel():
            raise RuntimeError("the trainable set changed size under a live optimizer state")
        elif self._m.device != flat.device:  # the model moved: the moments follow it
            self._m, self._v = self._m.to(flat.device), self._v.to(flat.device)
            self._ss = torch.zeros(1, dtype=torch.float32, device=flat.device)
            self._ss_ws = torch.empty(L.load().fbl_sumsq_ws_floats(), dtype=torch.float32, device=flat.device)
        grp = self.param_groups[0]
        if not eng.live_any:  # nothing trains: nothing moves, the step does not count
            return
        table = None if eng.all_live else eng.live_table()  # (device ranges of the live set; None: the whole buffer)
        self._step += 1
        self._ever.update(eng.live_order)
        ss = None
        if clip_max_norm and clip_max_norm > 0:
            self._ss.zero_()
            if self._ss_ws is None or self._ss_ws.device != g.device:
                self._ss_ws = torch.empty(L.load().fbl_sumsq_ws_floats(), dtype=torch.float32, device=g.device)
            if table is None:
                L.sumsq(g, self._ss, ws=self._ss_ws)
            else:
                L.sumsq_live(g, table, self._ss, self._ss_ws)
            ss = self._ss
        if not self._plain():  # parameter groups: ONE launch over the (live run, group) segments
            self._sync_lr()
            hyper = [(q["lr"], q["betas"][0], q["betas"][1], q["eps"], q["weight_decay"], q.get("decoupled_weight_decay", False))
                     for q in self.param_groups]
            L.adam_flat_groups(flat, g, self._m, self._v, self._segment_table(eng), hyper, self._step, sumsq_t=ss,
                               max_norm=clip_max_norm or 0.0, grad_scale=grad_scale)
            eng.params_version += 1
            return
        b1, b2 = grp["betas"]
        if table is None:
            L.adam_flat(flat, g, self._m, self._v, grp["lr"], b1, b2, grp["eps"], grp["weight_decay"], self._step, sumsq_t=ss,
                        max_norm=clip_max_norm or 0.0, grad_scale=grad_scale)
        else:
            L.adam_flat_live(flat, g, self._m, self._v, table, grp["lr"], b1, b2, grp["eps"], grp["weight_decay"], self._step,
                             sumsq_t=ss, max_norm=clip_max_norm or 0.0, grad_scale=grad_scale)
        eng.params_version += 1  # the bf16 operand copies of the engine are stale now

    def grad_norm(self) -> torch.Tensor:
        """global L2 norm of the last clipped step's gradients (device scalar)"""
        return self._ss.sqrt() if self._ss is not None else torch.zeros(())

    # ---- checkpoints: torch.optim.Adam's schema, so files written by the reference (main.py:290-300 saves
    # optimizer.state_dict() of torch.optim.Adam over [p for p in model.parameters() if p.requires_grad], main.py:182-188)
    # resume here and files written here resume there.  Parameter i of the schema is the i-th trainable parameter in
    # model.parameters() order; its moments are the slice of the flat m / v buffers at that parameter's offset.
    def _slices(self, eng):
        by_id = {id(eng.named[n]): (eng.offsets[n], eng.named[n].numel(), tuple(eng.named[n].shape), n) for n in eng.order}
        return [by_id[id(p)] for g in self.param_groups for p in g["params"]]  # (the indices run through the groups in order)

    def state_dict(self):
        eng = self.model.engine()
        state = {}
        if self._m is not None and self._step > 0:
            for i, (o, k, shape, name) in enumerate(self._slices(eng)):
                if name not in self._ever:  # never updated: no state, as torch keeps none for a parameter it never stepped
                    continue
                state[i] = {"step": torch.tensor(float(self._step)), "exp_avg": self._m[o:o + k].view(shape).clone(),
                            "exp_avg_sq": self._v[o:o + k].view(shape).clone()}
        groups = []
        index = PG.index_lists([g["params"] for g in self.param_groups])
        for g, idx in zip(self.param_groups, index):
            d = {k: v for k, v in g.items() if k != "params"}
            d["params"] = idx
            groups.append(d)
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd):
        eng = self.model.engine()
        flat = eng.flat
        m = torch.zeros_like(flat)
        v = torch.zeros_like(flat)
        self._ever = set()
        if "state" in sd:  # torch.optim.Adam schema (reference-written or ours)
            if len(self.param_groups) > 1 or len(sd["param_groups"]) > 1:  # several groups: the same index lists, as torch asks
                mine = PG.index_lists([g["params"] for g in self.param_groups])
                theirs = [[int(i) for i in g["params"]] for g in sd["param_groups"]]
                if mine != theirs:
                    raise ValueError("loaded state dict has other parameter groups than the optimizer: "
                                     f"{[len(t) for t in theirs]} parameters per group against {[len(t) for t in mine]}")
            sl = self._slices(eng)
            steps = set()
            for i, st in sd["state"].items():
                i = int(i)
                if i >= len(sl):
                    raise ValueError(f"optimizer state for parameter {i}, but only {len(sl)} trainable parameters")
                o, k, shape, name = sl[i]
                self._ever.add(name)
                if st["exp_avg"].numel() != k or st["exp_avg_sq"].numel() != k:
                    raise ValueError(f"optimizer state {i}: {tuple(st['exp_avg'].shape)} does not match parameter {shape}")
                m[o:o + k].copy_(st["exp_avg"].reshape(-1).to(flat.device, flat.dtype))
                v[o:o + k].copy_(st["exp_avg_sq"].reshape(-1).to(flat.device, flat.dtype))
                steps.add(int(float(st["step"])))
            if len(steps) > 1:
                raise ValueError(f"per-parameter step counts differ ({sorted(steps)}): the fused update keeps one")
            self._step = steps.pop() if steps else 0
        else:  # flat schema of earlier builds: {"step", "m", "v"}
            if sd["m"] is not None:
                if sd["m"].numel() != flat.numel() or sd["v"].numel() != flat.numel():
                    raise ValueError("flat optimizer state does not match the trainable buffer")
                m.copy_(sd["m"].to(flat.device, flat.dtype))
                v.copy_(sd["v"].to(flat.device, flat.dtype))
            self._step = int(sd["step"])
            if sd["m"] is not None:
                self._ever.update(eng.order)
        self._m, self._v = m, v
        self._ss = torch.zeros(1, dtype=torch.float32, device=flat.device)
        for g, s_ in zip(self.param_groups, sd["param_groups"]):
            g.update({k: v_ for k, v_ in s_.items() if k != "params"})
