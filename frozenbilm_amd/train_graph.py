"""Training steps (model forward + backward) as two replayable launch graphs each (opt-in): the MLM step of main.py:59-84
(`model.training_graphs`) and the fine-tuning step of videoqa.py:62-101 / mc.py:94-113 (`model.finetune_graphs`).

One training step of the engine is ~1450 kernel launches; issued one by one they cost the host ~19 ms (bench.py `host`).  At
one GPU that hides behind ~47 ms of GPU work; with eight processes per node, or once the kernels get faster, it does not.
`model.training_graphs = True` makes `model(**batch)` -- training mode, `labels` given, nothing else requested -- capture the
launch sequence of the forward and of the backward once per batch shape (hipGraph through `torch.cuda.CUDAGraph`, both graphs in
ONE private memory pool: the backward reads the activations the forward left in it) and replay them afterwards:

    out = model(**batch)        # copies the batch into the graph's static inputs, replays the forward graph
    out.loss.backward()         # replays the backward graph: gradients land in p.grad (views of the flat buffer)
    optimizer.step(...)         # stays eager: two launches whose arguments (lr, Adam step) change every step

What had to move for this:
  * dropout seeds are per-site constants + the step's position in the mask stream; eager launches add the two on the host,
    captured launches keep the constants as (frozen) kernel arguments and read the position from a device word that is
    rewritten before every replay (include/fbl.h "Dropout seeds"): the same sums, hence the same masks;
  * the list of labelled rows has a fixed capacity per graph (next multiple of 256): the host still counts the labels at the
    start of the step -- on an input, as the eager path does -- and pads the list with an unlabelled row, whose loss term and
    gradient are exactly zero (fbl_ce_fwd / fbl_ce_bwd_rows ignore labels < 0);
  * the gradient exchange of data-parallel runs leaves after the backward replay (`GradReducer.finish`: the "after"
    placement), not from inside it.
Replayed and eager steps run the same kernels on the same inputs with the same seeds: they agree bit for bit
(tests/test_gpu_model.py::test_graphed_training_step_equals_the_eager_step).

The fine-tuning step (`model.finetune_graphs = True`: training mode, `logit_rows` given, no `labels`) is the same pair of
graphs around another hand-over: the forward graph ends at the [R, Vout] logits of the requested rows, the caller computes its
loss on a copy of them, and the gradient autograd hands back on that copy is written into a static buffer that the backward
graph starts from (Engine.backward's `glogits` entry).

    logits = model(logit_rows=rows, **feed)["logits"]   # text padded to a length bucket; forward graph replayed; a copy
    loss_fn(logits, answers).backward()                 # the loss stays eager; its gradient is copied in, backward graph replayed

The text is padded to the next multiple of `model.GRAPH_L_BUCKET` (the inference graphs' bucket) with masked pad tokens, so a loop
whose batches are padded to their longest sample needs a handful of graphs; the row count (one [MASK] per sample) is a
constant of the batch shape.  A replayed step equals the eager step ON THE PADDED BATCH bit for bit
(tests/test_gpu_finetune_graphs.py); against the eager step on the unpadded batch the rows that exist get the padded grid's
values (tile shapes differ: 2e-3 on logits, as for `inference_graphs`) and training-mode dropout draws another, equally
distributed, mask stream (the element keys contain b*S + s), as with `packed_rows`.
"""
from __future__ import annotations

from typing import Callable, Dict, NamedTuple, Optional

import torch

from . import lib as L
from .engine import Run, check_logit_rows

F32 = torch.float32
ROW_BUCKET = 256  # capacity granularity of the labelled-row list
MAX_GRAPHS = 4    # captured (batch shape, row capacity, live set) configurations kept per model (each owns one step's activations)
MAX_CAPTURES = 12  # captures per model before the feature switches itself off with a warning (a shape-static loop needs 1-3)


def bucket_length(Lt: int, T: int, max_positions: int, bucket: int) -> Optional[int]:
    """Text length a length-bucketed graph runs `Lt` tokens at: the next multiple of `bucket`, capped at what the position table
    leaves behind T video slots; None when that cap cuts below Lt (the caller takes the eager path, which raises the
    reference's error)."""
    Lp = min(-(-Lt // bucket) * bucket, max_positions - T)
    return Lp if Lp >= Lt else None


def remap_rows(rows: torch.Tensor, S_old: int, S_new: int) -> torch.Tensor:
    """flat rows b*S_old + s of the [B, S_old] token grid as rows b*S_new + s of the grid padded to S_new positions"""
    return (rows // S_old) * S_new + rows % S_old


class _Replay(torch.autograd.Function):
    """autograd node of a graphed step: hands out a copy of the forward graph's static output (the loss, or the logits of the
    requested rows); backward gives the incoming gradient to the step, which replays the backward graph"""

    @staticmethod
    def forward(ctx, step, out_t, *params):
        ctx.step = step
        ctx.set_materialize_grads(False)
        return out_t.detach().clone()

    @staticmethod
    def backward(ctx, gout):
        step = ctx.step
        if gout is not None:
            step.run_backward(gout)
        return (None, None) + tuple(None for _ in step.eng.order)


class _GraphedPair:
    """What the graphed steps share: the static copies of the batch, the device word of the step's mask-stream position, a
    forward and a backward graph in one private pool, and the replay of the two.  A subclass says what the forward launches
    (`_forward_launches`, which leaves `self.run` behind) and where the backward starts (`_backward_launches`)."""

    def __init__(self, model, eng, feed: Dict[str, torch.Tensor]):
        self.model, self.eng = model, eng
        self.static = {k: v.clone() for k, v in feed.items()}
        self.seed_word = torch.zeros(1, dtype=torch.int64, device=eng.dev)
        self.pool = torch.cuda.graph_pool_handle()
        self.g_fwd, self.g_bwd = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        self.run: Optional[Run] = None
        self.pending_backward = False

    def _new_run(self):
        """the Run of the static batch (mask set, seeds read from the device word), its token ids and its video"""
        eng, m, st = self.eng, self.model, self.static
        cfg = eng.cfg
        input_ids = st["input_ids"]
        B, Lt = input_ids.shape
        video = st.get("video")
        T = video.shape[1] if video is not None else 0
        run = Run(B=B, S=T + Lt, T=T, Lt=Lt, train=True, save=True, seed_base=0, p_hid=cfg.hidden_dropout_prob,
                  p_att=cfg.attention_probs_dropout_prob, p_ad=m.adapter_dropout)
        run.seed_word = self.seed_word
        # the stages this capture saves for and back-propagates through: those of the live set it was captured under (the live
        # set's version is part of the cache key, so another set gets a capture of its own)
        run.plan, run.live_version = eng.plan(()), eng.live_version
        am = st["attention_mask"]
        if T:
            vm = st.get("video_mask")
            if vm is None:
                vm = torch.ones(video.shape[:2], device=eng.dev, dtype=am.dtype)
            mask = torch.cat([vm.to(am.dtype), am], 1)
        else:
            mask = am
        run.mask = mask.to(torch.int32).contiguous().view(-1)
        return run, input_ids, video

    def capture(self):
        eng = self.eng
        red, eng.reducer = eng.reducer, None  # the gradient exchange stays outside the graphs (_replay_backward)
        # The cyclic garbage collector must not run while a stream is capturing: an object it frees may own a HIP event (the
        # events of an earlier pass's side-stream joins, a dropped engine's) and destroying an event during a capture aborts
        # the process -- seen twice in round 6 as "Fatal Python error: Aborted ... Garbage-collecting" inside this function,
        # with whatever allocation happened to cross the collector's threshold.  torch.cuda.graph collects on entry; nothing
        # may collect until the capture has ended.
        import gc

        gc_was_on = gc.isenabled()
        try:
            gc.collect()
            gc.disable()
            with torch.cuda.graph(self.g_fwd, pool=self.pool):
                self._forward_launches()
            eng.attach_grads()
            with torch.cuda.graph(self.g_bwd, pool=self.pool):
                self._backward_launches()
        finally:
            if gc_was_on:
                gc.enable()
            eng.reducer = red
        return self

    # ------------------------------------------------------------------ per step
    def _replay_forward(self, feed, seed_word_value: int):
        for k, v in feed.items():
            self.static[k].copy_(v, non_blocking=True)
        self.seed_word.fill_(seed_word_value)
        self.g_fwd.replay()
        self.pending_backward = True

    def _replay_backward(self):
        eng = self.eng
        named, G = eng.named, eng.G
        if not all(named[n].grad is not None and named[n].grad.data_ptr() == G[n].data_ptr() for n in eng.live_order):
            eng.attach_grads()  # (skipped while every p.grad still is its view of the flat buffer -- zero_grad(set_to_none=True)
            #                      or a foreign / dropped .grad on ANY parameter brings the full pass back; ~300 pointer compares)
        self.g_bwd.replay()
        self.pending_backward = False
        if eng.reducer is not None:
            eng.reducer.finish()


class GraphedStep(_GraphedPair):
    """the MLM step: the loss of the labelled rows out of the forward graph, its gradient (a scalar) into the backward graph"""

    def __init__(self, model, eng, feed: Dict[str, torch.Tensor], r_cap: int):
        super().__init__(model, eng, feed)
        self.r_cap = r_cap
        dev = eng.dev
        self.rows = torch.zeros(r_cap, dtype=torch.int64, device=dev)
        self.gloss = torch.ones((), dtype=F32, device=dev)
        self.loss_t = None

    # ------------------------------------------------------------------ the two launch sequences
    def _forward_launches(self):
        eng, st = self.eng, self.static
        run, input_ids, video = self._new_run()
        if run.T:
            labels = torch.cat([torch.full((run.B, run.T), -100, dtype=torch.long, device=eng.dev), st["labels"]], 1)
        else:
            labels = st["labels"]
        run.labels = labels.contiguous().view(-1)
        run.rows = self.rows
        eng._refresh_if_stale(True)
        with L.seed_word(self.seed_word):
            _, loss_t = eng._forward(run, input_ids, video, False, False)
        self.run, self.loss_t = run, loss_t

    def _backward_launches(self):
        self.eng.backward(self.run, self.gloss, attach=False)

    # ------------------------------------------------------------------ per step
    def run_forward(self, feed, rows_padded, seed_word_value: int):
        self.rows.copy_(rows_padded, non_blocking=True)
        self._replay_forward(feed, seed_word_value)
        self.run.logits_pending = True  # (the [N, V] logits of THIS replay are filled on access, by an eager launch)
        return _Replay.apply(self, self.loss_t, *[self.eng.named[n] for n in self.eng.order])

    def run_backward(self, gloss):
        self.gloss.copy_(gloss.detach().to(F32).reshape(()))
        self._replay_backward()


class FinetuneStep(_GraphedPair):
    """the fine-tuning step: the [R, Vout] logits of the requested rows (`feed["rows"]`, int32, on the padded grid) out of the
    forward graph, the caller's gradient on them into the backward graph"""

    def __init__(self, model, eng, feed: Dict[str, torch.Tensor], use_ans: bool):
        super().__init__(model, eng, feed)
        self.use_ans = use_ans
        self.logits = None   # [R, Vout] view of the forward graph's output
        # [R, Vout]: where the backward graph reads the gradient handed in on the logits
        self.glogits = torch.zeros(feed["rows"].numel(), eng.n_ans if use_ans else eng.V, dtype=F32, device=eng.dev)

    def _forward_launches(self):
        eng = self.eng
        run, input_ids, video = self._new_run()
        run.logit_rows = self.static["rows"]
        eng._refresh_if_stale(True)
        with L.seed_word(self.seed_word):
            logits, _ = eng._forward(run, input_ids, video, self.use_ans, False)
        self.run, self.logits = run, logits[:, : run.Vout]

    def _backward_launches(self):
        self.eng.backward(self.run, None, glogits=self.glogits, attach=False)

    def run_forward(self, feed, seed_word_value: int):
        self._replay_forward(feed, seed_word_value)
        return _Replay.apply(self, self.logits, *[self.eng.named[n] for n in self.eng.order])

    def run_backward(self, glogits):
        self.glogits.copy_(glogits.detach())
        self._replay_backward()


# ---------------------------------------------------------------------- what the two routes keep on the model
class _Route(NamedTuple):
    switch: str    # the public attribute that turns the route on
    cache: str     # model.__dict__ keys: the captured steps (LRU, most recently used last) ...
    keys: str      # ... (engine id, the distinct configurations seen on it) ...
    captures: str  # ... their count ...
    auto_off: str  # ... and whether the route switched ITSELF off (capture budget)
    what: str      # a configuration, for the warning


MLM = _Route("training_graphs", "_train_graphs", "_train_graph_keys", "_train_graph_captures", "_train_graphs_auto_off",
             "(batch shape, label capacity)")
FINETUNE = _Route("finetune_graphs", "_finetune_graph_cache", "_finetune_graph_keys", "_finetune_graph_captures",
                  "_finetune_graphs_auto_off", "(batch shape, length bucket)")
ROUTES = (MLM, FINETUNE)


def restore_reducer_overlap(eng):
    """The CALLER switched the graph routes (`model.training_graphs`, `model.finetune_graphs`) off again (on every rank, like
    any other change of the training loop): the reducer goes back to the overlap placement it had before the graphs forced
    "after" mode -- otherwise the data-parallel overlap stays lost for the rest of the run.  Not used when a route switched
    ITSELF off on this rank (capture budget)."""
    red = getattr(eng, "reducer", None)
    prev = None if red is None else red.__dict__.pop("_overlap_before_graphs", None)
    if prev is not None:
        red.overlap = prev


def drop_pending_backward(model):
    """A graphed step's output was dropped without `backward()` (a skipped batch, an exception between forward and backward):
    tell the graphs that no backward is outstanding, so the next forward is served again.  An output handed out BEFORE this
    call must not be back-propagated afterwards: the activations it belongs to are overwritten by the next replay."""
    for route in ROUTES:
        for step in model.__dict__.get(route.cache, {}).values():
            step.pending_backward = False


def _hold_reducer_after(eng):
    """Data parallel: a rank served by a graph exchanges ONE [0, n) collective after the replay (_replay_backward); a rank that
    falls back to the eager step (no labelled row in its shard, a failed capture, a used-up budget) must issue the same
    pattern, or the ranks' collectives no longer match in count and size.  While a graph route is on the reducer therefore
    runs in "after" mode."""
    if eng.reducer is not None and eng.reducer.overlap != "after":
        eng.reducer.__dict__.setdefault("_overlap_before_graphs", eng.reducer.overlap)  # restored by restore_reducer_overlap()
        eng.reducer.overlap = "after"


def _eager_step_without_a_trace(model, eng, step: Callable[[], None]):
    """One eager step of a shape in front of its capture: lazy initialisations (kernel attributes, workspaces, allocator
    warm-up) happen outside the capture.  It leaves no trace: the caller's accumulated gradients, the STATE of every p.grad
    (None stays None: the next attach_grads then zero-fills as it would have; a view of the flat buffer gets its old contents
    back) and the mask-stream position are restored."""
    seed0 = model.step_seed
    saved = eng.flat_grad.clone()
    grads_before = [eng.named[n].grad for n in eng.order]
    red, eng.reducer = eng.reducer, None  # (no collectives: ranks may capture at different steps -- their row capacities differ)
    try:
        step()
    finally:
        eng.reducer = red
    eng.flat_grad.copy_(saved)
    for n, g in zip(eng.order, grads_before):
        eng.named[n].grad = g
    del saved, grads_before
    torch.cuda.synchronize(eng.dev)
    model.step_seed = seed0


def _graphed_step(model, eng, route: _Route, key, warm_up: Callable[[], None], build: Callable[[], _GraphedPair]):
    """The captured step of configuration `key` (key[0] = id(eng)) from the route's cache -- an LRU of MAX_GRAPHS entries --
    captured now if need be: one eager warm-up step, then the two graphs.  None when the call has to take the eager path: the
    budget of MAX_CAPTURES distinct configurations is used up or the capture failed; both switch the route off."""
    import warnings

    cache = model.__dict__.setdefault(route.cache, {})
    step = cache.pop(key, None)
    if step is None:
        for k in [k for k in cache if k[0] != id(eng)]:
            del cache[k]
        while len(cache) >= MAX_GRAPHS:
            del cache[next(iter(cache))]
        # a loop whose batch shapes keep changing (text padded to the longest sample, label counts crossing a row bucket) would
        # capture -- one eager warm-up step plus two captures, ~10 GB of pooled activations each -- and evict continuously
        # (counted: DISTINCT configurations of the current engine -- a rebuilt engine (load_state_dict, .to(), new answer
        #  embeddings) or a cache the caller cleared starts over, and re-capturing a configuration seen before does not count)
        seen = model.__dict__.setdefault(route.keys, (id(eng), set()))
        if seen[0] != id(eng):
            seen = model.__dict__[route.keys] = (id(eng), set())
        seen[1].add(key[1:])
        n_cap = len(seen[1])
        model.__dict__[route.captures] = n_cap
        if n_cap > MAX_CAPTURES:
            warnings.warn(f"model.{route.switch}: {n_cap} distinct {route.what} configurations seen -- the loop "
                          "is not shape-static (pad the text to a fixed length / bucket it); staying on the eager path")
            setattr(model, route.switch, False)
            # (the reducer STAYS in "after" mode: the other ranks may still be served by their graphs -- row capacities differ per
            #  rank, so the budgets run out at different steps -- and every rank must keep issuing the same one collective)
            model.__dict__[route.auto_off] = True
            cache.clear()
            return None
        _eager_step_without_a_trace(model, eng, warm_up)
        step = build()
        try:
            step.capture()
        except Exception as e:  # noqa: BLE001
            torch.cuda.synchronize(eng.dev)
            warnings.warn(f"{route.switch}: graph capture failed ({type(e).__name__}: {e}); staying on the eager path")
            setattr(model, route.switch, False)
            return None
    cache[key] = step
    if step.pending_backward:  # the graph owns ONE set of activations
        raise RuntimeError("graphed training step: forward called again before backward() of the previous output; "
                           f"set model.{route.switch} = False for loops that keep several forwards alive")
    return step


def _dtypes(feed) -> tuple:
    return tuple(sorted((k, str(v.dtype)) for k, v in feed.items()))


def graphed_forward(model, eng, input_ids, attention_mask, video, video_mask, labels):
    """`model.forward` of a training step through the captured graphs (captured on first use of a shape).  Returns the loss
    (connected to the trainable parameters for `.backward()`) and the Run (for `logits` on demand), or None when this call
    cannot be served from a graph (the caller takes the eager path)."""
    if labels is None or input_ids is None or not torch.is_grad_enabled():
        return None
    if video is not None and video.requires_grad:
        return None  # a captured step has no edge to its inputs: the eager path forms the gradient of `video`
    if not eng.update_live():
        return None  # nothing is live: the eager path runs the call without gradient bookkeeping
    _hold_reducer_after(eng)
    dev = eng.dev
    if attention_mask is None:
        attention_mask = torch.ones_like(input_ids)
    feed = {"input_ids": input_ids.contiguous(), "attention_mask": attention_mask.contiguous(), "labels": labels.contiguous()}
    use_video = bool(eng.F) and video is not None
    B, Lt = input_ids.shape
    T = video.shape[1] if use_video else 0
    if T + Lt > eng.cfg.max_position_embeddings:
        return None  # (the eager path raises the reference's error)
    if use_video:
        feed["video"] = video.contiguous()
        if video_mask is not None:
            feed["video_mask"] = video_mask.contiguous()
    # labelled rows: a function of the input, counted before anything is queued (the eager path does the same)
    full = labels if not T else torch.cat([torch.full((B, T), -100, dtype=torch.long, device=dev), labels], 1)
    flat = full.reshape(-1)
    rows = torch.nonzero(flat != -100).view(-1)
    R = rows.numel()
    N = flat.numel()
    if R == 0:
        return None
    r_cap = min(N, -(-R // ROW_BUCKET) * ROW_BUCKET)
    if r_cap > R:  # pad with the first unlabelled row (found on the device: no second synchronisation; R < N: one exists)
        free = torch.argmax((flat == -100).to(torch.int8)).view(1)
        rows = torch.cat([rows, free.expand(r_cap - R)])
    key = (id(eng), B, Lt, T, "video_mask" in feed, r_cap, _dtypes(feed), eng.live_version)

    def warm_up():
        eng.run(feed["input_ids"], feed["attention_mask"], feed.get("video"), feed.get("video_mask"), feed["labels"],
                False, False)["loss"].backward()

    step = _graphed_step(model, eng, MLM, key, warm_up, lambda: GraphedStep(model, eng, feed, r_cap))
    if step is None:
        return None
    model.step_seed += 1
    loss = step.run_forward(feed, rows, eng.seed_word_value())
    return loss, step.run


def finetune_forward(model, eng, input_ids, attention_mask, video, video_mask, mlm, logit_rows):
    """`model.forward` of a fine-tuning step (`logit_rows` under autograd, no `labels`) through the captured graphs.  Returns
    the [R, Vout] logits (a copy; connected to the trainable parameters, so the caller's loss back-propagates into the backward
    graph) and the Run, or None when this call cannot be served from a graph (the caller takes the eager path)."""
    import torch.nn.functional as F_

    if input_ids is None or (video is not None and video.requires_grad):
        return None  # inputs_embeds, or a `video` that takes a gradient: the static feeds hold ids and carry no edge to an input
    if not eng.update_live():
        return None  # nothing is live: the eager path runs the call without gradient bookkeeping
    _hold_reducer_after(eng)
    cfg = eng.cfg
    use_video = bool(eng.F) and video is not None
    B, Lt = input_ids.shape
    T = video.shape[1] if use_video else 0
    if T + Lt > cfg.max_position_embeddings:
        return None  # (the eager path raises the reference's error)
    # the rows are checked on the host before anything is queued, as on the eager path (one read of an input)
    check_logit_rows(logit_rows, B * (T + Lt))
    Lp = bucket_length(Lt, T, cfg.max_position_embeddings, model.GRAPH_L_BUCKET)
    if Lp is None:
        return None
    if attention_mask is None:
        attention_mask = torch.ones_like(input_ids)
    rows = logit_rows.to(eng.dev).view(-1)
    if Lp != Lt:  # (a text that fills its bucket goes in as it is)
        rows = remap_rows(rows.long(), T + Lt, T + Lp)
        input_ids = F_.pad(input_ids, (0, Lp - Lt), value=cfg.pad_token_id)
        attention_mask = F_.pad(attention_mask, (0, Lp - Lt), value=0)
    feed = {"input_ids": input_ids.contiguous(), "attention_mask": attention_mask.contiguous(), "rows": rows.to(torch.int32)}
    if use_video:
        feed["video"] = video.contiguous()
        if video_mask is not None:
            feed["video_mask"] = video_mask.contiguous()
    use_ans = bool(model.n_ans) and not mlm
    key = (id(eng), B, Lp, T, "video_mask" in feed, rows.numel(), bool(mlm), _dtypes(feed), eng.live_version)

    def warm_up():
        lg = eng.run(feed["input_ids"], feed["attention_mask"], feed.get("video"), feed.get("video_mask"), None, mlm, False,
                     logit_rows=feed["rows"])["logits"]
        lg.backward(torch.ones_like(lg))

    step = _graphed_step(model, eng, FINETUNE, key, warm_up, lambda: FinetuneStep(model, eng, feed, use_ans))
    if step is None:
        return None
    model.step_seed += 1
    logits = step.run_forward(feed, eng.seed_word_value())
    model.__dict__["_finetune_graph_replays"] = model.__dict__.get("_finetune_graph_replays", 0) + 1
    return logits, step.run
