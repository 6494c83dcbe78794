"""The launch graphs (hipGraphs through `torch.cuda.CUDAGraph`): which calls of `model.forward` a captured graph serves
(`route_for`), the captured graphs, and what the model keeps of them.  Three routes, each an opt-in attribute of the model:
  * `model.inference_graphs`: the `logit_rows` inference forward (what `videoqa.evaluate` / `mc.evaluate` run per batch,
    videoqa.py:157-168, mc.py:160-172) as ONE graph: ~700 launches cost the host ~10 ms per batch when issued one by one;
  * `model.training_graphs`: the MLM step of main.py:59-84 (training mode, `labels` given, nothing else requested) as a forward
    and a backward graph in ONE private memory pool (the backward reads the activations the forward left in it): ~1450
    launches, ~19 ms of host time (bench.py `host`), which ~47 ms of GPU work hide at one GPU but not at eight processes per
    node.  `model(**batch)` copies the batch into the static inputs and replays the forward graph, `out.loss.backward()`
    replays the backward graph (gradients land in p.grad, views of the flat buffer), `optimizer.step(...)` stays eager;
  * `model.finetune_graphs`: the fine-tuning step of videoqa.py:62-101 / mc.py:94-113 (training mode, `logit_rows`, no
    `labels`) as the same pair around another hand-over: the forward graph ends at the [R, Vout] logits of the requested rows,
    the caller computes its loss on a copy of them, and the gradient autograd hands back on that copy is written into a static
    buffer that the backward graph starts from (Engine.backward's `glogits` entry).
What had to move for the training steps:
  * dropout seeds are per-site constants + the step's position in the mask stream; eager launches add the two on the host,
    captured launches keep the constants as (frozen) kernel arguments and read the position from a device word that is
    rewritten before every replay (include/fbl.h "Dropout seeds"): the same sums, hence the same masks;
  * the list of labelled rows has a fixed capacity per graph (next multiple of 256): the host still counts the labels at the
    start of the step -- on an input, as the eager path does -- and pads the list with an unlabelled row, whose loss term and
    gradient are exactly zero (fbl_ce_fwd / fbl_ce_bwd_rows ignore labels < 0);
  * the gradient exchange of data-parallel runs leaves after the backward replay (`GradReducer.finish`: "after" placement).
Replayed and eager steps run the same kernels on the same inputs with the same seeds: they agree bit for bit
(tests/test_gpu_model.py::test_graphed_training_step_equals_the_eager_step).  The two `logit_rows` routes pad the text to the
next multiple of `model.GRAPH_L_BUCKET` with masked pad tokens (a sample's logits do not depend on padding), so a loop whose
batches are padded to their longest sample needs a handful of graphs: there a replayed step equals the eager step ON THE PADDED
BATCH bit for bit (tests/test_gpu_finetune_graphs.py); against the eager step on the unpadded batch the rows that exist get the
padded grid's values (tile shapes differ: 2e-3 on logits) and training-mode dropout draws another, equally distributed, mask
stream (the element keys contain b*S + s), as with `packed_rows`.
"""
from __future__ import annotations

import contextlib
import gc
import warnings
from collections import namedtuple
from dataclasses import dataclass, field
from typing import Callable, Dict, NamedTuple, Optional

import torch
import torch.nn.functional as F_

from . import lib as L
from .engine import Run, check_logit_rows

F32 = torch.float32
ROW_BUCKET = 256  # capacity granularity of the labelled-row list
MAX_GRAPHS = 4    # captured (batch shape, row capacity, live set) configurations kept per model (each owns one step's activations)
MAX_CAPTURES = 12  # captures per model before the feature switches itself off with a warning (a shape-static loop needs 1-3)


# ---------------------------------------------------------------------- the routes and what the model keeps of them
class Route(NamedTuple):
    switch: str     # the public attribute of the model that turns the route on
    cache: str      # name in model.__dict__ of its graphs: a dict, most recently used last; popping it releases them
    capacity: int   # entries the cache keeps (least recently used dropped first)
    budgeted: bool  # MAX_CAPTURES distinct configurations, then the route switches itself off
    what: str       # a configuration, for the budget's warning
    failed: str     # opening words of the failed-capture warning


INFERENCE = Route("inference_graphs", "_graph_cache", 6, False, "(batch shape, length bucket, rows)", "inference graph")
MLM = Route("training_graphs", "_train_graphs", MAX_GRAPHS, True, "(batch shape, label capacity)", "training_graphs: graph")
FINETUNE = Route("finetune_graphs", "_finetune_graph_cache", MAX_GRAPHS, True, "(batch shape, length bucket)",
                 "finetune_graphs: graph")
ROUTES = (INFERENCE, MLM, FINETUNE)


@dataclass
class RouteState:
    """what a model remembers of one route besides its cache"""
    seen_engine: Optional[int] = None        # id of the engine `seen` was counted on
    seen: set = field(default_factory=set)   # distinct configurations captured on it (budgeted routes)
    auto_off: bool = False                   # the route switched ITSELF off (capture budget)
    replays: int = 0                         # calls served by a graph

    @property
    def captures(self) -> int:
        return len(self.seen)


def new_states() -> Dict[str, RouteState]:  # (the model's constructor declares `_graph_routes` with it)
    return {route.switch: RouteState() for route in ROUTES}


def stats(model, route: Route) -> RouteState:
    return model._graph_routes[route.switch]


def reset(model, route: Route) -> None:  # release the route's graphs and start its counters over
    model.__dict__.pop(route.cache, None)
    model._graph_routes[route.switch] = RouteState()


def drop_pending_backward(model):
    """A graphed step's output was dropped without `backward()` (a skipped batch, an exception between forward and backward):
    tell the graphs that no backward is outstanding, so the next forward is served again.  An output handed out BEFORE this
    call must not be back-propagated afterwards: the activations it belongs to are overwritten by the next replay."""
    for route in ROUTES:
        for step in model.__dict__.get(route.cache, {}).values():
            step.pending_backward = False


# ---------------------------------------------------------------------- which call takes which route
# what `model.forward` was called with, as far as the routes care: which arguments were given (`rows`: logit_rows.numel(), None
# when not given; `video_grad`: a video that requires grad), the output flags and torch.is_grad_enabled()
Call = namedtuple("Call", "ids embeds labels rows video_grad mlm hidden_states attentions grad")


def route_for(model, call: Call) -> Optional[Route]:
    """The route that serves this call, None for the eager path; host logic over the model's switches and mode alone.  The
    graphs feed token ids into static buffers and carry no edge to an input (no inputs_embeds, no `video` that takes a
    gradient); they are shape-static and end at the loss or the requested rows (no packed_rows / decoder_rows, no hidden
    states or attentions, no predict_topk: the predictions are formed by the eager route).  A model with LoRA on its attention
    projections (lora_rank > 0) is served eagerly: no graph route has been checked against it; so is a model with prompt slots
    (n_prompt > 0): the graphs' static feeds know the [video | text] sequence only."""
    if (not call.ids or call.embeds or call.hidden_states or call.attentions or model.packed_rows or model.decoder_rows
            or getattr(model, "predict_topk", 0) or (call.grad and call.video_grad) or getattr(model, "lora_rank", 0)
            or getattr(model, "n_prompt", 0)):
        return None
    if not model.training and not call.grad:
        return INFERENCE if model.inference_graphs and call.rows is not None and not call.labels else None
    if not (model.training and call.grad):
        return None
    if call.labels:  # (with an answer head the loss needs mlm=True: the head's own logits are not what the labels index)
        return MLM if model.training_graphs and call.rows is None and not (model.n_ans and not call.mlm) else None
    return FINETUNE if model.finetune_graphs and call.rows else None


# ---------------------------------------------------------------------- the batch of a call as a graph's inputs
def bucket_length(Lt: int, T: int, max_positions: int, bucket: int) -> Optional[int]:
    """Text length a length-bucketed graph runs `Lt` tokens at: the next multiple of `bucket`, capped at what the position table
    leaves behind T video slots; None when that cap cuts below Lt (the caller takes the eager path, which raises the
    reference's error)."""
    Lp = min(-(-Lt // bucket) * bucket, max_positions - T)
    return Lp if Lp >= Lt else None


def remap_rows(rows: torch.Tensor, S_old: int, S_new: int) -> torch.Tensor:
    """flat rows b*S_old + s of the [B, S_old] token grid as rows b*S_new + s of the grid padded to S_new positions"""
    return (rows // S_old) * S_new + rows % S_old


def _video_slots(eng, video) -> int:
    return video.shape[1] if (eng.F and video is not None) else 0


def build_feed(eng, input_ids, attention_mask, video, video_mask, labels=None, rows=None, bucket: int = 0):
    """The static inputs of a graph, contiguous: `input_ids`, `attention_mask` (all ones by default), `labels` / flat int32
    `rows` when given, `video` when the engine projects one, `video_mask` when given.  With a `bucket` the text is padded to it
    (pad tokens, mask 0; a text that fills its bucket goes in as it is) and the rows move along; None when none fits."""
    cfg = eng.cfg
    Lt, T = input_ids.shape[1], _video_slots(eng, video)
    if attention_mask is None:
        attention_mask = torch.ones_like(input_ids)
    if rows is not None:
        rows = rows.to(eng.dev).view(-1)
    if bucket:
        Lp = bucket_length(Lt, T, cfg.max_position_embeddings, bucket)
        if Lp is None:
            return None
        if Lp != Lt:
            rows = remap_rows(rows.long(), T + Lt, T + Lp)
            input_ids = F_.pad(input_ids, (0, Lp - Lt), value=cfg.pad_token_id)
            attention_mask = F_.pad(attention_mask, (0, Lp - Lt), value=0)
    feed = dict(input_ids=input_ids, attention_mask=attention_mask, labels=labels,
                rows=None if rows is None else rows.to(torch.int32))
    if eng.F and video is not None:
        feed.update(video=video, video_mask=video_mask)
    return {k: v.contiguous() for k, v in feed.items() if v is not None}


def _eager_run(eng, feed, mlm):  # the eager forward of a feed: the loss of its `labels` or the [R, Vout] logits of its `rows`
    return eng.run(feed["input_ids"], feed["attention_mask"], feed.get("video"), feed.get("video_mask"), feed.get("labels"), mlm,
                   False, logit_rows=feed.get("rows"))


# ---------------------------------------------------------------------- the captured graphs
@contextlib.contextmanager
def no_gc_during_capture():
    """The cyclic garbage collector must not run while a stream is capturing: an object it frees may own a HIP event (the
    events of an earlier pass's side-stream joins, a dropped engine's) and destroying an event during a capture aborts the
    process -- seen twice in round 6 as "Fatal Python error: Aborted ... Garbage-collecting" inside a capture, with whatever
    allocation happened to cross the collector's threshold.  torch.cuda.graph collects on entry; nothing may collect until the
    capture has ended.  The collector's previous state comes back however the body ends."""
    was_on = gc.isenabled()
    gc.collect()
    gc.disable()
    try:
        yield
    finally:
        if was_on:
            gc.enable()


class _StaticFeed:
    """the static copies of a batch that captured launches read, and the copy of a call's batch into them"""
    pending_backward = False  # (a training pair: its forward was replayed, its backward not yet)

    def __init__(self, eng, feed: Dict[str, torch.Tensor]):
        self.eng = eng
        self.static = {k: v.to(eng.dev).clone() for k, v in feed.items()}

    def _copy_in(self, feed):
        for k, v in feed.items():
            self.static[k].copy_(v, non_blocking=True)


class InferenceGraph(_StaticFeed):
    """the `logit_rows` inference forward as one graph that ends at the [R, Vout] logits of the requested rows"""

    def __init__(self, eng, feed: Dict[str, torch.Tensor], mlm: bool):
        super().__init__(eng, feed)
        self.mlm, self.graph, self.logits = mlm, torch.cuda.CUDAGraph(), None

    def capture(self):
        with no_gc_during_capture(), torch.cuda.graph(self.graph):
            self.logits = _eager_run(self.eng, self.static, self.mlm)["logits"]

    def replay(self, feed):
        self._copy_in(feed)
        self.graph.replay()
        return self.logits.clone()


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


class _GraphedPair(_StaticFeed):
    """What the graphed steps share: the static copies of the batch, the device word of the step's mask-stream position, a
    forward and a backward graph in one private pool, and the replay of the two.  A subclass says what the forward launches
    (`_forward_launches`, which leaves `self.run` behind) and where the backward starts (`_backward_launches`)."""

    def __init__(self, model, eng, feed: Dict[str, torch.Tensor]):
        super().__init__(eng, feed)
        self.model = model
        self.seed_word = torch.zeros(1, dtype=torch.int64, device=eng.dev)
        self.pool = torch.cuda.graph_pool_handle()
        self.g_fwd, self.g_bwd = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        self.run: Optional[Run] = None

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
        try:
            with no_gc_during_capture():
                with torch.cuda.graph(self.g_fwd, pool=self.pool):
                    self._forward_launches()
                eng.attach_grads()
                with torch.cuda.graph(self.g_bwd, pool=self.pool):
                    self._backward_launches()
        finally:
            eng.reducer = red

    # ------------------------------------------------------------------ per step
    def _replay_forward(self, feed, seed_word_value: int):
        self._copy_in(feed)
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


def _hold_reducer_after(eng):
    """Data parallel: a rank served by a graph exchanges ONE [0, n) collective after the replay (_replay_backward); a rank that
    falls back to the eager step (no labelled row in its shard, a failed capture, a used-up budget) must issue the same pattern,
    or the ranks' collectives no longer match in count and size: while a training route is on, the reducer runs in "after" mode."""
    red = eng.reducer
    if red is not None and red.overlap != "after":
        red._overlap_before_graphs = red._overlap_before_graphs or red.overlap  # restored by restore_reducer_overlap()
        red.overlap = "after"


def restore_reducer_overlap(eng):
    """the reducer goes back to the overlap placement it had before the graphs forced "after" mode"""
    red = getattr(eng, "reducer", None)
    if red is not None and red._overlap_before_graphs is not None:
        red.overlap, red._overlap_before_graphs = red._overlap_before_graphs, None


def restore_reducer_overlap_if_routes_off(model, eng):
    """The CALLER switched both training routes off again (on every rank, like any other change of the training loop): the
    reducer gets its placement back -- otherwise the data-parallel overlap stays lost for the rest of the run.  Not when a
    route switched ITSELF off on this rank (capture budget): the other ranks may still be served by their graphs."""
    if not (model.training_graphs or model.finetune_graphs or stats(model, MLM).auto_off or stats(model, FINETUNE).auto_off):
        restore_reducer_overlap(eng)


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
    model.step_seed = seed0


def _graphed_step(model, eng, route: Route, key, warm_up: Callable[[], None], build: Callable[[], _StaticFeed]):
    """The captured graph(s) of configuration `key` (key[0] = id(eng)) from the route's cache -- an LRU of `route.capacity`
    entries -- captured now if need be: `warm_up()` outside the capture, then `build().capture()`.  None (eager path, route
    switched off) when the route's budget of MAX_CAPTURES distinct configurations is used up or the capture failed."""
    cache = model.__dict__.setdefault(route.cache, {})
    step = cache.pop(key, None)
    if step is None:
        for k in [k for k in cache if k[0] != id(eng)]:
            del cache[k]
        while len(cache) >= route.capacity:
            del cache[next(iter(cache))]
        if route.budgeted:
            # a loop whose batch shapes keep changing (text padded to the longest sample, label counts crossing a row bucket)
            # would capture -- one eager warm-up step plus two captures, ~10 GB of pooled activations each -- and evict
            # continuously (counted: DISTINCT configurations of the current engine -- a rebuilt engine (load_state_dict, .to(),
            # new answer embeddings) starts over, and re-capturing a configuration seen before does not count)
            state = stats(model, route)
            if state.seen_engine != id(eng):
                state.seen_engine, state.seen = id(eng), set()
            state.seen.add(key[1:])
            if state.captures > MAX_CAPTURES:
                warnings.warn(f"model.{route.switch}: {state.captures} distinct {route.what} configurations seen -- the loop "
                              "is not shape-static (pad the text to a fixed length / bucket it); staying on the eager path")
                setattr(model, route.switch, False)
                # (the reducer STAYS in "after" mode: the other ranks may still be served by their graphs -- row capacities differ
                #  per rank, so the budgets run out at different steps -- and every rank must keep issuing the same one collective)
                state.auto_off = True
                cache.clear()
                return None
        warm_up()
        torch.cuda.synchronize(eng.dev)  # (lazy initialisation and the allocator's warm-up have ended before the capture begins)
        step = build()
        try:
            step.capture()
        except Exception as e:  # noqa: BLE001
            torch.cuda.synchronize(eng.dev)
            warnings.warn(f"{route.failed} capture failed ({type(e).__name__}: {e}); staying on the eager path")
            setattr(model, route.switch, False)
            return None
    cache[key] = step
    if step.pending_backward:  # the graph owns ONE set of activations
        raise RuntimeError("graphed training step: forward called again before backward() of the previous output; "
                           f"set model.{route.switch} = False for loops that keep several forwards alive")
    return step


def _dtypes(feed) -> tuple:
    return tuple(sorted((k, str(v.dtype)) for k, v in feed.items()))


# ---------------------------------------------------------------------- the three routes
def serve(model, eng, route: Route, input_ids, attention_mask, video, video_mask, labels, mlm, logit_rows):
    """A call that `route_for` gave to `route`, served from its graphs: `loss`, `logits` and `run` as `Engine.run` returns
    them, or None when the engine or the batch say no after all (the caller takes the eager path)."""
    if route is INFERENCE:
        return _inference_forward(model, eng, input_ids, attention_mask, video, video_mask, mlm, logit_rows)
    if not eng.update_live():
        return None  # nothing is live: the eager path runs the call without gradient bookkeeping
    _hold_reducer_after(eng)
    if _video_slots(eng, video) + input_ids.shape[1] > eng.cfg.max_position_embeddings:
        return None  # (the eager path raises the reference's error)
    if route is MLM:
        return _mlm_forward(model, eng, input_ids, attention_mask, video, video_mask, labels)
    return _finetune_forward(model, eng, input_ids, attention_mask, video, video_mask, mlm, logit_rows)


def _inference_forward(model, eng, input_ids, attention_mask, video, video_mask, mlm, logit_rows):
    # operands of the trainable weights / composed adapter rows are rebuilt (in place) outside the graph: on every call,
    # or -- inside weights_frozen(), where the evaluate loops run -- only when something wrote to the parameters
    eng.prepare_inference()
    feed = build_feed(eng, input_ids, attention_mask, video, video_mask, rows=logit_rows, bucket=model.GRAPH_L_BUCKET)
    if feed is None:
        return None
    B, Lp = feed["input_ids"].shape
    key = (id(eng), B, Lp, _video_slots(eng, video), video_mask is not None, feed["rows"].numel(), bool(mlm))
    eng._no_pos_cache = True  # the captured forward recomputes the position projections: it reads nothing that a later
    try:                      # rebuild of the trainable operands would re-allocate behind its back
        graph = _graphed_step(model, eng, INFERENCE, key, lambda: _eager_run(eng, feed, mlm),
                              lambda: InferenceGraph(eng, feed, mlm))
    finally:
        eng._no_pos_cache = False
    if graph is None:
        return None
    stats(model, INFERENCE).replays += 1
    return {"loss": None, "logits": graph.replay(feed)}


def _mlm_forward(model, eng, input_ids, attention_mask, video, video_mask, labels):
    """the loss connected to the trainable parameters; the [B, S, Vout] logits carry no autograd edge and are filled on access"""
    feed = build_feed(eng, input_ids, attention_mask, video, video_mask, labels=labels)
    B, Lt = input_ids.shape
    T = _video_slots(eng, video)
    # labelled rows: a function of the input, counted before anything is queued (the eager path does the same)
    full = labels if not T else torch.cat([torch.full((B, T), -100, dtype=torch.long, device=eng.dev), labels], 1)
    flat = full.reshape(-1)
    rows = torch.nonzero(flat != -100).view(-1)
    R, N = rows.numel(), flat.numel()
    if R == 0:
        return None
    r_cap = min(N, -(-R // ROW_BUCKET) * ROW_BUCKET)
    if r_cap > R:  # pad with the first unlabelled row (found on the device: no second synchronisation; R < N: one exists)
        free = torch.argmax((flat == -100).to(torch.int8)).view(1)
        rows = torch.cat([rows, free.expand(r_cap - R)])
    key = (id(eng), B, Lt, T, "video_mask" in feed, r_cap, _dtypes(feed), eng.live_version)

    step = _graphed_step(model, eng, MLM, key,
                         lambda: _eager_step_without_a_trace(model, eng, lambda: _eager_run(eng, feed, False)["loss"].backward()),
                         lambda: GraphedStep(model, eng, feed, r_cap))
    if step is None:
        return None
    model.step_seed += 1
    loss = step.run_forward(feed, rows, eng.seed_word_value())
    stats(model, MLM).replays += 1
    run = step.run
    return {"loss": loss, "logits": run.logits.view(run.B, run.S, -1)[:, :, : run.Vout], "run": run}


def _finetune_forward(model, eng, input_ids, attention_mask, video, video_mask, mlm, logit_rows):
    """the [R, Vout] logits as a copy connected to the trainable parameters: the caller's loss reaches the backward graph"""
    # the rows are checked on the host before anything is queued, as on the eager path (one read of an input)
    check_logit_rows(logit_rows, input_ids.shape[0] * (_video_slots(eng, video) + input_ids.shape[1]))
    feed = build_feed(eng, input_ids, attention_mask, video, video_mask, rows=logit_rows, bucket=model.GRAPH_L_BUCKET)
    if feed is None:
        return None
    B, Lp = feed["input_ids"].shape
    key = (id(eng), B, Lp, _video_slots(eng, video), "video_mask" in feed, feed["rows"].numel(), bool(mlm), _dtypes(feed),
           eng.live_version)

    def eager_step():
        lg = _eager_run(eng, feed, mlm)["logits"]
        lg.backward(torch.ones_like(lg))

    step = _graphed_step(model, eng, FINETUNE, key, lambda: _eager_step_without_a_trace(model, eng, eager_step),
                         lambda: FinetuneStep(model, eng, feed, bool(model.n_ans) and not mlm))
    if step is None:
        return None
    model.step_seed += 1
    logits = step.run_forward(feed, eng.seed_word_value())
    stats(model, FINETUNE).replays += 1
    return {"loss": None, "logits": logits, "run": step.run}
