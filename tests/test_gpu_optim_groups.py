"""GPU: FusedAdam with parameter groups, decoupled weight decay and layer-wise rates, at model level.

Models: the tiny 3-layer DeBERTa at S = 17 and the 2-layer one at the xlarge row width, as tests/test_gpu_input_grads.py builds
them (its build / _cfg / _params / _batch are imported), and the tiny BERT of tests/test_gpu_bert.py.  The reference is
tests/group_cases.ref_adam_groups in float64, fed the flat gradients each step produced; the bound per element is the one
tests/test_gpu_rowops.py applies to fbl_adam_flat, U (|p0| + k LR) C_ADAM after k steps (imported; every rate here is at most
LR).  Bit equalities are conditions.

Seen on the parent commit: the module does not import -- ImportError: cannot import name 'param_groups' from 'frozenbilm_amd'
(and frozenbilm_amd.optim has no layerwise_param_groups, FusedAdam no `param_groups` keyword) -- so every test here fails."""
import math
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

from frozenbilm_amd import lib as L  # noqa: E402
from frozenbilm_amd import param_groups as PG  # noqa: E402
from frozenbilm_amd.optim import FusedAdam, layerwise_param_groups  # noqa: E402
from frozenbilm_amd.util.misc import adjust_learning_rate  # noqa: E402
from tests import group_cases as GC  # noqa: E402
from tests.test_gpu_input_grads import _batch, _cfg, _params, build  # noqa: E402
from tests.test_gpu_rowops import C_ADAM, LR, U, judge  # noqa: E402

DEV = "cuda"
BETAS, EPS, WD = (0.9, 0.95), 1e-8, 0.01
SIZES = {"S17": (4, 13, False), "xl": (10, 64, True)}


def bits(t):
    return t.detach().view(torch.int32)


class Model:
    """a model in train mode, its batch, and what a test needs of its engine"""

    def __init__(self, size, seed=92):
        if size == "bert":
            from tests import test_gpu_bert as TB

            torch.manual_seed(913)
            self.m = TB._model(TB._params(TB._ocfg()), train=True)
            self.db = TB._to(TB._batch())
            self.prefix = "bert"
        else:
            T, Lt, xl = SIZES[size]
            cfg = _cfg(T, xl=xl)
            batch = _batch(cfg, T, Lt, seed=32, B=2 if xl else 3)
            torch.manual_seed(912)
            self.m = build(cfg, _params(cfg, seed), train=True)
            self.db = {k: v.to(DEV) for k, v in batch.items()}
            self.prefix = "deberta"
        self.named = dict(self.m.named_parameters())
        self.names = self.m.trainable_names()
        self.nL = self.m.config.num_hidden_layers

    def backward(self, seed):
        """one forward / backward from mask-stream position `seed`; returns the engine (its flat_grad holds the gradients)"""
        for p in self.m.parameters():
            p.grad = None
        self.m.step_seed = seed
        self.m(**self.db).loss.backward()
        return self.m.engine()

    def span(self, name):
        eng = self.m.engine()
        return eng.offsets[name], eng.offsets[name] + eng.named[name].numel()

    def top_ln(self):
        return f"{self.prefix}.encoder.layer.{self.nL - 1}.output.LayerNorm.weight"


def hyper_of(opt):
    """the records the step must use, worked out here from the group dicts (lr_scale relative to group 0)"""
    g0 = opt.param_groups[0]
    return [(g0["lr"] * g["lr_scale"] if "lr_scale" in g else g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"],
             bool(g.get("decoupled_weight_decay", False))) for g in opt.param_groups]


def segments_of(opt, eng):
    name_of = {id(eng.named[n]): n for n in eng.order}
    gof = {name_of[id(p)]: k for k, g in enumerate(opt.param_groups) for p in g["params"]}
    numel = {n: eng.named[n].numel() for n in eng.order}
    return PG.segments(eng.order, eng.offsets, numel, eng.live_order, gof)


def live_mask(segs, n):
    mk = torch.zeros(n, dtype=torch.bool, device=DEV)
    for b, e, _ in segs:
        mk[b:e] = True
    return mk


def ref_step(opt, eng, ref, step, max_norm):
    """one float64 step of (p, m, v) = ref on the gradients in eng.flat_grad; returns the clip factor"""
    segs = segments_of(opt, eng)
    g = eng.flat_grad.double()
    norm = math.sqrt(float((g[live_mask(segs, g.numel())] ** 2).sum()))
    clip = min(1.0, max_norm / (norm + 1e-6)) if max_norm > 0 else 1.0
    GC.ref_adam_groups(ref[0], g, ref[1], ref[2], segs, hyper_of(opt), step=step, clip=clip)
    return clip


def start(eng):
    n = eng.flat.numel()
    return [eng.flat.double(), torch.zeros(n, dtype=torch.float64, device=DEV), torch.zeros(n, dtype=torch.float64, device=DEV)]


def first_norm(M):
    eng = M.backward(0)
    return math.sqrt(float((eng.flat_grad.double() ** 2).sum()))


# ------------------------------------------------------------------------------------------------ 1. layer-wise AdamW
@pytest.mark.parametrize("size", ["S17", "xl", "bert"])
def test_layerwise_adamw_three_steps(size):
    """layerwise_param_groups(decay=0.5), AdamW, no decay on LayerNorm / bias; the clip bites on the first step; a LayerNorm
    weight whose gradient is zeroed by hand keeps its bits under weight_decay > 0 (it sits in an undecayed group)"""
    M = Model(size)
    groups = layerwise_param_groups(M.m, 0.5)
    opt = FusedAdam(M.m, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, param_groups=groups, decoupled_weight_decay=True)
    assert len(opt.param_groups) == len(groups) > 2
    assert all(g["decoupled_weight_decay"] for g in opt.param_groups) and opt.param_groups[0]["weight_decay"] == WD
    scales = sorted({g.get("lr_scale", 1.0) for g in opt.param_groups}, reverse=True)
    assert scales == [0.5 ** i for i in range(M.nL + 1)]
    max_norm = 0.5 * first_norm(M)
    eng = M.m.engine()
    ln = M.top_ln()
    b, e = M.span(ln)
    k_ln = [k for k, g in enumerate(opt.param_groups) if any(p is M.named[ln] for p in g["params"])]
    assert len(k_ln) == 1 and opt.param_groups[k_ln[0]]["weight_decay"] == 0.0
    p0 = eng.flat.clone()
    ref = start(eng)
    for step in (1, 2, 3):
        M.backward(step - 1)
        eng.flat_grad[b:e].zero_()
        clip = ref_step(opt, eng, ref, step, max_norm)
        assert step > 1 or clip < 1.0, "the clip must bite on the first step"
        opt.step(clip_max_norm=max_norm)
    torch.cuda.synchronize()
    assert opt._step == 3
    for k, g in enumerate(opt.param_groups):  # lr_scale is written back to the group's lr
        assert g["lr"] == LR * g.get("lr_scale", 1.0), k
    live = live_mask(segments_of(opt, eng), p0.numel())
    assert bool(live.any())
    judge(f"{size}: parameters after three layer-wise AdamW steps", eng.flat[live], ref[0][live],
          U * (p0.double().abs()[live] + 3 * LR), C_ADAM)
    moved = eng.flat != p0
    assert torch.equal(bits(eng.flat[b:e]), bits(p0[b:e])), "a LayerNorm weight with zero gradient moved in an undecayed group"
    for k, g in enumerate(opt.param_groups):  # every group with members moved
        for p in g["params"]:
            if p is not M.named[ln]:
                bb, ee = M.span([n for n in M.names if M.named[n] is p][0])
                assert bool(moved[bb:ee].any()), f"group {k}: a member did not move"
    assert abs(float(opt.grad_norm()) - math.sqrt(float((eng.flat_grad.double() ** 2).sum()))) <= 1e-5 * float(opt.grad_norm())


def test_a_zero_gradient_layernorm_moves_in_a_decayed_group():
    M = Model("S17")
    groups = layerwise_param_groups(M.m, 0.5, no_decay=("bias",))
    opt = FusedAdam(M.m, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, param_groups=groups, decoupled_weight_decay=True)
    eng = M.backward(0)
    b, e = M.span(M.top_ln())
    eng.flat_grad[b:e].zero_()
    w0 = eng.flat[b:e].clone()
    opt.step(clip_max_norm=1.0)
    w1 = eng.flat[b:e]
    assert bool((w1 != w0).all()) and bool((w0 != 0).all())
    want = w0.double() * (1.0 - LR * WD)  # decay only: m = v = 0 and a zero gradient leave Adam's own term at exactly zero
    assert float((w1.double() - want).abs().max()) <= 2 * U * float(w0.abs().max())


# ------------------------------------------------------------------------------------------------ 2. one group: the parent's path
def test_one_group_is_the_plain_path_bit_for_bit(monkeypatch):
    """new keywords at their defaults (and one explicit coupled group): fbl_sumsq + fbl_adam_flat, never fbl_adam_flat_groups;
    the bits of direct lib.adam_flat calls on clones; the state dict's group has the keys it always had"""
    calls = dict(flat=0, live=0, groups=0)
    real = dict(flat=L.adam_flat, live=L.adam_flat_live, groups=L.adam_flat_groups)

    def counted(which):
        def f(*a, **kw):
            calls[which] += 1
            return real[which](*a, **kw)
        return f

    monkeypatch.setattr(L, "adam_flat", counted("flat"))
    monkeypatch.setattr(L, "adam_flat_live", counted("live"))
    monkeypatch.setattr(L, "adam_flat_groups", counted("groups"))
    for explicit in (False, True):
        M = Model("S17")
        if explicit:
            opt = FusedAdam(M.m, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, param_groups=[dict(params=["*"])])
        else:
            opt = FusedAdam(M.m, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD)
        assert len(opt.param_groups) == 1 and len(opt.param_groups[0]["params"]) == len(M.names)
        calls.update(flat=0, live=0, groups=0)
        m_ = v_ = None
        for step in (1, 2):
            eng = M.backward(step - 1)
            p_, g_ = eng.flat.clone(), eng.flat_grad.clone()
            if m_ is None:
                m_, v_ = torch.zeros_like(p_), torch.zeros_like(p_)
            ss = torch.zeros(1, device=DEV)
            L.sumsq(g_, ss)
            real["flat"](p_, g_, m_, v_, LR, BETAS[0], BETAS[1], EPS, WD, step, sumsq_t=ss, max_norm=1.0)
            opt.step(clip_max_norm=1.0)
            assert torch.equal(bits(eng.flat), bits(p_)) and torch.equal(bits(opt._m), bits(m_)) and torch.equal(bits(opt._v), bits(v_))
        assert calls == dict(flat=2, live=0, groups=0), calls
        # a frozen parameter: the live twin, still not the groups kernel
        M.named[M.top_ln()].requires_grad_(False)
        M.backward(2)
        opt.step(clip_max_norm=1.0)
        assert calls == dict(flat=2, live=1, groups=0), calls
        sd = opt.state_dict()
        want_keys = {"lr", "betas", "eps", "weight_decay", "params"} | ({"decoupled_weight_decay"} if explicit else set())
        assert set(sd["param_groups"][0]) == want_keys and sd["param_groups"][0]["params"] == list(range(len(M.names)))
    # ... and anything else is ONE fbl_adam_flat_groups
    M = Model("S17")
    opt = FusedAdam(M.m, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, decoupled_weight_decay=True)
    calls.update(flat=0, live=0, groups=0)
    M.backward(0)
    opt.step(clip_max_norm=1.0)
    M.named[M.top_ln()].requires_grad_(False)
    M.backward(1)
    opt.step(clip_max_norm=1.0)
    assert calls == dict(flat=0, live=0, groups=2), calls


# ------------------------------------------------------------------------------------------------ 3. the schedule reaches every group
def test_adjust_learning_rate_moves_a_group_with_lr_scale():
    M = Model("S17")
    opt = FusedAdam(M.m, lr=LR, betas=BETAS, eps=EPS, weight_decay=0.0,
                    param_groups=[dict(params=[]), dict(params=["*adapter*"], lr_scale=0.25)])
    args = SimpleNamespace(lr=LR, schedule="linear_with_warmup", fraction_warmup_steps=0.1)
    adjust_learning_rate(opt, curr_step=5, num_training_steps=100, args=args)  # half way through the warm-up
    assert opt.param_groups[0]["lr"] == 0.5 * LR
    eng = M.backward(0)
    p0 = eng.flat.clone()
    ref = start(eng)
    ref_step(opt, eng, ref, 1, 0.0)
    opt.step()
    assert opt.param_groups[1]["lr"] == 0.25 * 0.5 * LR and opt.param_groups[0]["lr"] == 0.5 * LR
    segs = segments_of(opt, eng)
    live = live_mask(segs, p0.numel())
    judge("parameters after a step on the schedule's rate", eng.flat[live], ref[0][live], U * (p0.double().abs()[live] + LR), C_ADAM)
    # the first Adam step moves an element by its rate (|m_hat / sqrt(v_hat)| = 1 where |g| >> eps): a quarter of group 0's
    d = (eng.flat.double() - p0.double()).abs()
    big = eng.flat_grad.abs() > 1e-5
    for k, want in ((0, 0.5 * LR), (1, 0.125 * LR)):
        mk = torch.zeros_like(live)
        for b, e, kk in segs:
            if kk == k:
                mk[b:e] = True
        mk &= big
        assert bool(mk.any())
        assert abs(float(d[mk].median()) - want) <= 0.02 * want, (k, float(d[mk].median()), want)
    with pytest.raises(ValueError, match="both"):
        FusedAdam(M.m, lr=LR, param_groups=[dict(params=[]), dict(params=["*adapter*"], lr=1e-4, lr_scale=0.25)])
    with pytest.raises(ValueError, match="group 0"):
        FusedAdam(M.m, lr=LR, param_groups=[dict(params=["*adapter*"], lr_scale=0.25)])
    with pytest.raises(ValueError, match="twice"):
        FusedAdam(M.m, lr=LR, param_groups=[dict(params=["*adapter*"]), dict(params=[M.named[[n for n in M.names if "adapter" in n][0]]])])


# ------------------------------------------------------------------------------------------------ 4. freezing in a multi-group run
def test_a_parameter_frozen_mid_run_keeps_value_and_moments():
    M = Model("S17")
    opt = FusedAdam(M.m, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, param_groups=layerwise_param_groups(M.m, 0.5),
                    decoupled_weight_decay=True)
    M.backward(0)
    opt.step(clip_max_norm=1.0)
    eng = M.m.engine()
    name = f"deberta.encoder.layer.{M.nL - 1}.attention.output.adapter.down.weight"
    k = [k for k, g in enumerate(opt.param_groups) if any(p is M.named[name] for p in g["params"])][0]
    others = [n for n in M.names if n != name and any(p is M.named[n] for p in opt.param_groups[k]["params"])]
    assert others, "the frozen parameter shares its group"
    b, e = M.span(name)
    p1, m1, v1 = eng.flat.clone(), opt._m.clone(), opt._v.clone()
    assert bool(m1[b:e].any()) and bool(v1[b:e].any())
    M.named[name].requires_grad_(False)
    M.backward(1)
    ref = [p1.double(), m1.double(), v1.double()]
    ref_step(opt, eng, ref, 2, 1.0)
    opt.step(clip_max_norm=1.0)
    assert opt._step == 2
    for t, t1, what in ((eng.flat, p1, "value"), (opt._m, m1, "first moment"), (opt._v, v1, "second moment")):
        assert torch.equal(bits(t[b:e]), bits(t1[b:e])), f"the frozen parameter's {what} moved"
    for n in others:
        bb, ee = M.span(n)
        assert bool((eng.flat[bb:ee] != p1[bb:ee]).any()) and bool((opt._m[bb:ee] != m1[bb:ee]).any()), n
    live = live_mask(segments_of(opt, eng), p1.numel())
    assert not bool(live[b:e].any())
    judge("the live parameters after the frozen step", eng.flat[live], ref[0][live], U * (p1.double().abs()[live] + LR), C_ADAM)
    # nothing live: the step does nothing and does not count
    for n in M.names:
        M.named[n].requires_grad_(False)
    eng.update_live()
    opt.step(clip_max_norm=1.0)
    assert opt._step == 2


# ------------------------------------------------------------------------------------------------ 5. checkpoints
def _torch_twin(M, opt):
    """torch.optim.Adam over CPU float32 clones of the parameters, in the optimizer's groups with its values"""
    clones, groups = {}, []
    for g, h in zip(opt.param_groups, hyper_of(opt)):
        mine = []
        for p in g["params"]:
            n = [n for n in M.names if M.named[n] is p][0]
            clones[n] = torch.nn.Parameter(p.detach().cpu().clone())
            mine.append(clones[n])
        groups.append(dict(params=mine, lr=h[0], betas=(h[1], h[2]), eps=h[3], weight_decay=h[4], decoupled_weight_decay=h[5]))
    return clones, torch.optim.Adam(groups, lr=1.0, foreach=False)


def test_checkpoints_speak_torchs_multi_group_schema():
    M = Model("S17")
    mk_groups = lambda: [dict(params=[]), dict(params=["*LayerNorm*"], weight_decay=0.0, lr_scale=0.5),  # noqa: E731
                         dict(params=["*adapter*bias"], betas=(0.8, 0.9), eps=1e-6, decoupled_weight_decay=False)]
    new_opt = lambda: FusedAdam(M.m, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, param_groups=mk_groups(),  # noqa: E731
                                decoupled_weight_decay=True)
    opt = new_opt()
    for step in (1, 2):
        M.backward(step - 1)
        opt.step(clip_max_norm=1.0)
    eng = M.m.engine()
    sd = opt.state_dict()
    # the schema: indices run through the groups in order; every parameter has a state with the common step
    sizes = [len(g["params"]) for g in opt.param_groups]
    assert all(sizes) and sum(sizes) == len(M.names)
    flat_idx = [i for g in sd["param_groups"] for i in g["params"]]
    assert flat_idx == list(range(len(M.names))) and [len(g["params"]) for g in sd["param_groups"]] == sizes
    assert sorted(sd["state"]) == flat_idx and all(float(s["step"]) == 2.0 for s in sd["state"].values())
    assert sd["param_groups"][1]["lr_scale"] == 0.5 and sd["param_groups"][1]["lr"] == 0.5 * LR
    assert [g["decoupled_weight_decay"] for g in sd["param_groups"]] == [True, True, False]
    i = 0
    for g in opt.param_groups:
        for p in g["params"]:
            b, e = M.span([n for n in M.names if M.named[n] is p][0])
            assert torch.equal(sd["state"][i]["exp_avg"].reshape(-1), opt._m[b:e]) and sd["state"][i]["exp_avg"].shape == p.shape
            i += 1
    # ---- continue here: a fresh optimizer that loaded the file equals the uninterrupted run bit for bit
    M.backward(2)
    p2, g2 = eng.flat.clone(), eng.flat_grad.clone()
    opt.step(clip_max_norm=1.0)
    p3, m3, v3 = eng.flat.clone(), opt._m.clone(), opt._v.clone()
    eng.flat.copy_(p2)
    eng.params_version += 1
    opt2 = new_opt()
    opt2.load_state_dict(sd)
    assert opt2._step == 2
    opt2.step(clip_max_norm=1.0)  # (the gradients of the third backward are still in the flat buffer)
    assert torch.equal(bits(eng.flat), bits(p3)) and torch.equal(bits(opt2._m), bits(m3)) and torch.equal(bits(opt2._v), bits(v3))
    # ---- continue in torch: the same file, the same gradients, within the Adam bound
    eng.flat.copy_(p2)
    eng.params_version += 1
    clones, topt = _torch_twin(M, opt)
    topt.load_state_dict(sd)
    assert [len(g["params"]) for g in topt.param_groups] == sizes
    for n, c in clones.items():
        b, e = M.span(n)
        c.grad = g2[b:e].view(c.shape).cpu().clone()
    torch.nn.utils.clip_grad_norm_(list(clones.values()), 1.0)
    topt.step()
    for n, c in clones.items():
        b, e = M.span(n)
        judge(f"torch.optim.Adam from our file: {n}", p3[b:e].cpu(), c.detach().reshape(-1),
              U * (p2[b:e].double().abs().cpu() + LR), C_ADAM)
    # ---- and back: a state dict written by that torch optimizer loads here
    tsd = topt.state_dict()
    opt3 = new_opt()
    opt3.load_state_dict(tsd)
    assert opt3._step == 3
    for n, c in clones.items():
        b, e = M.span(n)
        assert torch.equal(opt3._m[b:e].cpu(), topt.state[c]["exp_avg"].reshape(-1))
        assert torch.equal(opt3._v[b:e].cpu(), topt.state[c]["exp_avg_sq"].reshape(-1))
    assert opt3.param_groups[2]["betas"] == (0.8, 0.9) and opt3.param_groups[1]["lr_scale"] == 0.5
    # ---- a file with other group index lists is refused
    bad = {"state": sd["state"], "param_groups": [dict(g) for g in sd["param_groups"]]}
    bad["param_groups"][0]["params"] = sd["param_groups"][0]["params"] + sd["param_groups"][1]["params"][:1]
    bad["param_groups"][1]["params"] = sd["param_groups"][1]["params"][1:]
    with pytest.raises(ValueError, match="groups"):
        new_opt().load_state_dict(bad)
    with pytest.raises(ValueError, match="groups"):
        new_opt().load_state_dict({"state": sd["state"], "param_groups": sd["param_groups"][:2]})
    with pytest.raises(ValueError, match="groups"):
        FusedAdam(M.m, lr=LR).load_state_dict(sd)


# ------------------------------------------------------------------------------------------------ 6. the group dicts are read every step
def test_writing_a_groups_weight_decay_between_steps_takes_effect():
    M = Model("S17")
    wd = 0.1
    opt = FusedAdam(M.m, lr=LR, betas=BETAS, eps=EPS, weight_decay=wd, decoupled_weight_decay=True,
                    param_groups=[dict(params=[]), dict(params=["*adapter*weight"])])
    eng = M.backward(0)
    p0 = eng.flat.clone()
    ref = start(eng)
    ref_step(opt, eng, ref, 1, 1.0)
    opt.step(clip_max_norm=1.0)
    M.backward(1)
    old = [t.clone() for t in ref]
    ref_step(opt, eng, old, 2, 1.0)  # what the step would do had nothing been written
    opt.param_groups[1]["weight_decay"] = 0.0
    ref_step(opt, eng, ref, 2, 1.0)
    opt.step(clip_max_norm=1.0)
    segs = segments_of(opt, eng)
    live = live_mask(segs, p0.numel())
    form = U * (p0.double().abs() + 2 * LR)
    judge("parameters after weight_decay was written", eng.flat[live], ref[0][live], form[live], C_ADAM)
    g1 = torch.zeros_like(live)
    for b, e, k in segs:
        if k == 1:
            g1[b:e] = True
    # (the check tells the two apart: on group 1 the old value of weight_decay lies far outside the bound somewhere)
    assert float(((old[0] - ref[0]).abs() / form)[g1].max()) > 4 * C_ADAM
    assert torch.equal(old[0][live & ~g1], ref[0][live & ~g1])
